// cvr_internal.h — context state and kernel launch parameters shared by the C-ABI
// implementation (cvr_*.cpp; host-only helpers: cvr_host.h) and the gfx950 kernels (*.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>
#include <functional>
#include <string>
#include <vector>

#include "../../include/cvr.h"

namespace cvr {

// Padded-cell volume layout ("cell8"): cell (a,b,c), a in [0, N], holds the 8
// corner values that GL trilinear filtering reads for texel coordinate
// x in [a-1, a): corners clamp(a-1) and clamp(a) per axis (CLAMP_TO_EDGE).
// One sample = one 16-byte (fp16 corners) load.  Cells are x-fastest (a 4x4x4
// bricked order measured 6-18 % slower on the headline frame and was dropped).
struct CellGrid {
  int cx, cy, cz;           // cells per axis = N + 1
  int pitch_y, pitch_z;     // cx, cx*cy
  long long linear_origin;  // index of cell (1,1,1) = texel (0,0,0)
  int bpitch_y, bpitch_z;   // the pitches in bytes (16 B per cell)
  uint32_t borigin;         // linear_origin * 16, mod 2^32 (byte offsets of buffer loads)
};

// Screen-tile split: which TxT tile is rank r's k-th.  Tiles
// are numbered in a virtual row-major order in which tile row ty is rotated by
// s*ty tiles, and virtual tile v belongs to rank v mod N.  When N divides the
// tiles per row, rank(tx, ty) = (tx + s*ty) mod N: a diagonal lattice instead
// of the columns plain t mod N gives (tools/split_balance.py, samples max/mean
// over ranks on four reference camera views at 1024^2, 16^2 tiles, N = 8:
// columns up to 1.21, s = 3 at most 1.014).  Any s keeps the per-rank counts of
// t mod N (cvr_tiles_for_rank).
__host__ __device__ inline int split_shift(int nranks) { return nranks >= 4 ? 3 : 1; }
__host__ __device__ inline void split_tile(int rank, int nranks, int k, int ntx, int& tx, int& ty) {
  const int v = rank + k * nranks;
  ty = v / ntx;
  const int xv = v - ty * ntx;
  tx = xv - (int)(((long long)split_shift(nranks) * ty) % ntx);
  if (tx < 0) tx += ntx;
}

// Per-frame constants of the rc1pass kernel (passed by value).
struct Rc1passArgs {
  // ray generation (ray_marching_1p.comp:87-99)
  float eye[3];
  float col0[3], col1[3], col2[3];   // columns of mat3(View)
  float tan_half_fovy, aspect;
  float inv_w, inv_h;                // unused: exact division by W/H is used
  int W, H;
  // volume grid (rc1prenderer.cpp:233-258)
  float half_grid[3];                // VolumeGridSize / 2
  float n_over_g[3];                 // N / VolumeGridSize  (texel space)
  float nm1[3];                      // N - 1 (float)
  int N[3];
  CellGrid cells;
  float step;
  int tf_n;
  int exp_fast;                      // 1: every -(alpha*h) lies in [-86, 0] (no exp range checks)
  int exp_native;                    // tolerance mode (option native_exp): v_exp_f32, not CVR-SPEC
  // Blinn-Phong (ray_marching_1p.comp:48-81)
  float ka, kd, ks, shininess;
  float ispec[3];
  float light[3];
  // screen-tile split (cvr_frame)
  int tile, rank, nranks, ntx, my_tiles;
  int packed;
  int interleave;                    // no launch order: tile t on block t (XCD t % 8) instead of XCD bands
  int out_half;                      // 1: store RGBA16F (uint2 per pixel), 0: float4
  int ntiles;                        // 8x8 wave tiles of this launch
  unsigned long long* tile_stats;    // diagnostics (tile_stats option) or null
  unsigned long long* shade_ctr;     // measurement (shade_counters): [0] += shaded samples (Phong),
                                     // [1] += samples the cell skip stepped over without a load
  int cost_time;                     // LPT cost = measured tile time (1) or longest ray (0)
  // empty-space skipping: occupancy byte per macro cell (null = off)
  const uint8_t* occ;
  int mdim[3];                       // macro cells per axis
  int mshift;                        // macro cell = 2^mshift texels a side
  // GL texture-unit filter mode (option "filter_bits"): 0 = exact float weights
  // (CVR-SPEC), 8 = every GL_LINEAR weight (volume, gradient, TF) rounded to 8
  // fraction bits, as GPU texture units filter (CVR-SPEC-8)
  int filter_bits;
  // per-cell skip (march_common.h cell_empty): 0 off, 1 empty-sample flags,
  // 2 flags + distance skip; inv_step = 1 / step (the full-step bound)
  int cell_skip;
  float inv_step;
};

constexpr int kMaxTfLds = 4096;          // TF entries a kernel stages into LDS
constexpr int kMaxExtLevels = 16;        // extinction mip levels (up to 32768^3)

// One level of the extinction pyramid as the cone fetches address it.
struct ExtLevel {
  int off;                           // first cell8 texel of the level
  int dx, dy, dz;                    // dimensions
  float sx, sy, sz;                  // d / G: texel coordinate = fma(p, d/G, -0.5)
  float mx, my, mz;                  // d - 1 (clamp-to-edge bound)
  int pad[2];
};

// Directional-occlusion shading (dos.hip): one cone's tables on the device.
// Early exit of a cone stage (dos.hip cone_stage): per stage, the sections where
// the border scale 2^-(2 floor(mip) + 1) changes ("runs": first section, its
// tap distance `track`, the scale) and the track after the stage's last section,
// all by the kernel's own float recurrence on the fp16-rounded table.
constexpr int kMaxConeRuns = 12;
struct ConeStageExit {
  int nruns;                         // 0: no exit test for this stage
  int end_s;                         // first section after the stage
  float end_track;                   // track after the stage's last section
  int run_first[kMaxConeRuns];
  float run_t[kMaxConeRuns], run_inv[kMaxConeRuns];
};

struct DosCone {
  int counts[3];                     // sections of 1, 3, 7 rays
  float initial_step, ray7w, ui_weight;
  float axes[30];                    // 3-ray then 7-ray axes (x, y, z)
  const float4* sections;            // (interval, mip, d_integral, amplitude), fp16-rounded
  ConeStageExit exit[3];
};

struct DosArgs {
  Rc1passArgs a;                     // ray, volume, TF, Blinn-Phong constants, tiles
  float G[3];                        // VolumeScaledSizes
  int ext_levels;
  const struct ExtLevel* levels;     // per level, device memory (read by scalar loads)
  int apply_occlusion, apply_shadow, shadow_type, phong;
  float ka, kd, ks;                  // Kambient if occlusion, Kdiffuse/Kspecular if shadow, else 0
  float lfwd[3], lup[3], lright[3];  // light camera vectors (RenderingParameters)
  float spot_cos;                    // SpotLightMaxAngle uniform
  int zero_skip;                     // every pyramid value finite: taps with a 0 border factor are 0
  int count_taps;                    // shade_counters: count the taps fetched (measurement)
  DosCone occ, sdw;
};

// Pre-illumination (lightcache.hip): the light cache is an RG16F 3D image, one
// uint32 per voxel (Idao in the low half, Idcs in the high half), x-fastest.
// Its producers are the DOS cone kernel (lightcache.hip) and the EBS SAT kernel
// (ebs_lightcache.hip); any producer that fills the same image
// (cvr_set_light_cache) feeds the same march.
constexpr int kMaxLightCacheDim = 512;
struct LightCacheArgs {              // the computation's own uniforms (DosArgs holds the rest)
  int dims[3];                       // LightCacheDimensions
  int nb[3];                         // 4x4x4 voxel blocks per axis (set by the launcher)
  float vs[3];                       // VolumeScales * (VolumeDimensions / LightCacheDimensions)
  float cam_up[3];                   // EyeCamUp (Camera::GetCameraVectors' cup; the DOS producer only)
};
struct LightCacheView {              // what the cached march's fetch reads
  const uint32_t* rg;
  int d[3];
  float s[3];                        // L / G: texel coordinate = fma(p, L / G, -0.5)
  float m[3];                        // L - 1 (clamp-to-edge bound)
};

// Extinction-based shading (ebs.hip): the SAT and the shader's uniforms.
struct EbsArgs {
  Rc1passArgs a;                     // ray, volume, TF, Blinn-Phong constants, tiles
  float S[3], G[3];                  // VolumeScales, VolumeScaledSizes
  float inv_vs[3];                   // 1 / (G + 2 S)
  float nsat[3], nsat_m1[3];         // SAT dims as float, and dims - 1
  int sat_dims[3];
  uint32_t sat_pz;                   // texels per SAT plane (the cell4 layout's z + 1 plane offset)
  float min_sat[3], max_sat[3];      // S / 2, G + 1.5 S
  int apply_occlusion, occ_shells;
  float occ_radius;
  // 1 / r^2 of shell i (r = R*(i+1)) and W_A = 1 / (R*shells)^2, computed on the host
  // with the shader's float expressions (the divisions are the same for every sample)
  static constexpr int kMaxAoShells = 64;
  float ao_w[kMaxAoShells];
  float ao_wa;
  int apply_shadow, shadow_type, phong;
  float p_cs, p_sn, n_cs, n_sn;      // cos / sin of +-DirSdwConeAngle
  int recip_cone;                    // cone angle <= 44 deg: cone-edge divisions by reciprocal (ebs.hip cone_div)
  float interval, initial_step, ui_weight, max_distance;
  float lfwd[3];
  float ka, kd, ks;                  // Kambient if occlusion, Kdiffuse/Kspecular if shadow, else 0
};

// Ground-truth cone ray-caster (crtgt.hip): the shader's uniforms, and the
// progressive frame's device state.  A launch round marches at most
// kCrtgtRoundSamples iterations per pixel, so the round's job storage is bounded.
constexpr int kCrtgtRoundSamples = 4;
struct CrtgtArgs {
  Rc1passArgs a;                     // ray, volume, TF, eye, light position, shininess
  float G[3];                        // VolumeGridSize
  float light_gap, light_step;
  int apply_occlusion, apply_shadow, shadow_type, phong;
  float ka, kd, ks;                  // Ka if occlusion, Kd / Ks if shadow, else 0
  float occ_distance, sdw_distance;
  int n_occ, n_sdw;
  const float* occ_rays;             // n x (r, g, b), binary16-rounded (device)
  const float* sdw_rays;
  float lzaxs[3], lup[3], lright[3]; // LightCamForward (= -light.forward), Up, Right
};
struct CrtgtState {
  float4* dst = nullptr;             // per pixel: the composite so far
  float* s = nullptr;                // the ray parameter of the next iteration
  uint32_t* cnt = nullptr;           // loop iterations so far
  uint32_t* done = nullptr;          // 1: the pixel's loop has ended
  uint32_t* nj = nullptr;            // jobs of the current round
  float4* jobs = nullptr;            // slot = pixel * kCrtgtRoundSamples + j: 2 float4 (+1 with Phong)
  uint32_t* list = nullptr;          // the round's occupied slots, compacted
  unsigned long long* ctr = nullptr; // [0] jobs of the round, [1] unfinished pixels, [2] iterations so far
};

// Voxel cone tracing (vct.hip, vct_precompute.hip).  The pyramid is RG16F, one
// uint32 per texel (mean in the low half, standard deviation in the high half),
// x fastest, the levels concatenated.
constexpr int kMaxVctLevels = CVR_VCT_MAX_LEVELS;
struct VctLevel {                    // one level as the cone fetches address it
  int off;                           // first texel of the level
  int d[3];                          // dimensions
  float s[3];                        // d / G: texel coordinate = fma(p, d / G, -0.5)
  float m[3];                        // d - 1 (clamp-to-edge bound)
};
// One sample of the cone schedule (wave-uniform: it depends on the cone parameters
// only, so one thread computes all of it once, vct.hip vct_schedule_kernel)
struct VctStep {
  float xl;                          // apex_distance + step_size / 2
  float expo;                        // step_size * corr_fact
  float frac;                        // the level fraction (filter_weight applied); 0 with one level
  int nlev;                          // 1: lv[0] only, 2: lerp(lv[0], lv[1], frac)
  VctLevel lv[2];
};
struct VctArgs {
  Rc1passArgs a;                     // ray, volume, TF, Blinn-Phong constants, tiles
  float G[3];                        // VolumeScaledSizes
  int apply_shadow, phong;
  float ka, kd, ks;                  // Kambient if occlusion, Kdiffuse / Kspecular if shadow, else 0
  int samples;                       // ConeNumberOfSamples
  float tab_w, tab_h;                // table dimensions as float (texel coordinate = fma(u, n, -0.5))
  float max_density, max_stddev;     // VolumeMaxDensity (255), (float)VolumeMaxStandardDeviation
  int tab_wi, tab_hi;
};
struct VctData {
  const uint32_t* pyr;               // the pyramid
  const uint16_t* table;             // R16F, tab_hi rows of tab_wi
  const VctStep* steps;              // [samples]
};

// Slice-based directional occlusion (sbtm.hip).  One slice as its pass reads it:
// everything here is the host's float arithmetic (cvr_sbtm.cpp, DESIGN.md 5d''').
constexpr int kSbtmMaxBatch = 16;        // slices one launch advances (option sbtm_slices_per_launch)
constexpr int kSbtmTile = 64;            // the blocked form's screen tile, pixels a side
constexpr int kSbtmHalo = 16;            // most halo pixels per side its LDS region holds
constexpr int kSbtmRegion = kSbtmTile + 2 * kSbtmHalo;
constexpr int kSbtmThreads = 512;
struct SbtmSlice {
  float depth;                       // view depth of the slice's quad
  float c[3];                        // the quad's centre
  float cvx, cvy;                    // CVector (equation 12)
  int rx, ry;                        // tap radius in pixels (the proven bound)
  int plane;                         // the occlusion plane this slice writes (it reads the other)
};
struct SbtmBatch {
  int n;                             // slices of this launch
  int ex, ey;                        // the summed radii: the halo loaded around the tile
  SbtmSlice s[kSbtmMaxBatch];
};
struct SbtmArgs {
  Rc1passArgs a;                     // ray generation, volume, TF size, filter_bits
  float right[3], up[3];             // cam_right, cam_up
  float half_diag;                   // volume_diagonal / 2 (voxels, unscaled)
  float att;                         // UITransparencyScale
  int gx, gy;
  float gxy;                         // GridSize.x * GridSize.y
  float tapx[CVR_SBTM_MAX_GRID];     // the grid's p.x per xpos_sample, p.y per ypos_sample
  float tapy[CVR_SBTM_MAX_GRID];
};
struct SbtmPlanes {
  uint2* eye;                        // RGBA16F
  uint16_t* occ;                     // two R16F planes, plane p at occ + p * W * H
  uint16_t* occ_out;                 // the blocked form stores its tiles' planes here, never into occ:
                                     // another workgroup of the launch may still load its halo from occ
  uint32_t* samples;                 // per-pixel fragments kept, or null
  unsigned long long* total;         // their sum is added here, or null
};

// Isosurface ray-casters with block skipping (iso.hip): the shaders' uniforms.
struct IsoArgs {
  Rc1passArgs a;                     // ray, volume, Blinn-Phong constants, tiles
  float G[3];                        // VolumeGridSize
  float nb[3];                       // numBlocks (vec3 uniform)
  int nbi[3];                        // the same as int (table addressing, REPEAT wrap)
  float iso, step_small, step_large, step_range;
  float half_block_len;              // length(G / numBlocks) * 0.5 (variant 1)
  float bs[3];                       // G / numBlocks (getBlockBounds' blockSize)
  float nhg[3];                      // -G * 0.5
  float inv_g[3];                    // 1 / G (the block index fast path, verified)
  float color[4];
};

// Deferred isosurface shading (deferred.hip).  The G-buffer is two float4 planes of
// W x H, gPosition then gNormal.  gNormal.w always equals gPosition.w (hit: 1, in-box
// miss: 0, off the box: the clear value's w), so its slot holds the pixel's fetch
// count instead (uint32 bits; 0 exactly off the box) and readers take w from gPosition.
struct DeferredShadeArgs {           // lighting_pass.comp's and post_process.frag's uniforms
  int W, H;
  float eye[3];                      // CameraEye of the kept frame
  float light[3];                    // LightSourcePosition
  float light_color[3];
  float color[4];                    // objectColor
  float ka, kd, ks, shininess;
  float exposure, gamma;
};

// Advanced deferred shading (advdeferred.hip).  The curvature planes are one float4
// per pixel, (k1, k2, dir.x, dir.y): the lighting pass reads a neighbour in one 16-B fetch.
constexpr int kAdvColorMapSize = 256;  // curvatureColorMap: float4 texels (rgb, 1)
constexpr int kAdvRidgeMapSize = 256;  // ridgeValleyMap: 256 x 256 floats (its .r channel)
struct AdvShadeArgs {                // lighting_pass.comp's and post_process.frag's uniforms
  int W, H;
  float eye[3];                      // viewPos: CameraEye of the kept frame
  float light[3];                    // lightPos
  float light_color[3];
  float alpha;                       // objectColor.a
  float ka, kd, ks, shininess;
  float flow_speed, flow_scale, time;
  int show_ridges, show_valleys;
  float accessibility;               // accessibilityStrength
  float screen[2];                   // screenSize, resolved (> 0)
  float exposure, gamma;
};

// Several frames in one ray-march launch (cvr_render_rc1pass_frames): frame f
// takes workgroups [f * grid, (f + 1) * grid) and differs from frame 0 only in
// its view (camera) and its outputs.  grid is a multiple of 8 whenever the
// single-frame grid is, so workgroup b keeps XCD b % 8's share of the frame.
// interleave (under a launch order, grid a multiple of 8): workgroup
// 8 (n e + f) + x runs entry e of XCD band x of frame f, so the dispatcher hands
// out entry e of every frame before entry e + 1 of any -- each band's longest
// tiles of ALL frames start first (LPT over the launch, not per frame).
constexpr int kMaxLaunchFrames = 16;
struct FrameView {
  float eye[3];
  float col0[3], col1[3], col2[3];   // columns of mat3(View)
  float tan_half_fovy, aspect;
};
struct LaunchFrames {
  int n;                             // frames in the launch (1: a plain launch, the rest unused)
  int grid;                          // workgroups per frame
  int interleave;                    // 1: the frames' entries interleaved by launch-order entry (below)
  FrameView view[kMaxLaunchFrames];
  float4* out[kMaxLaunchFrames];
  uint32_t* samples[kMaxLaunchFrames];
};

// How one frame is cut into work: one 8x8 wave tile per workgroup.
struct RenderPlan {
  int ntiles;                        // 8x8 wave tiles (one workgroup each)
  int order_slots;                   // grid size under an LPT order (8 x entries per band)
  int boost;                         // per band, the first `boost` entries run at priority 2
  int quad_pct;                      // per band, this % of the longest tiles march 4 lanes/ray
  int keep;                          // diagnostics: >0 keeps only the first `keep` entries per band
  int max_seg;                       // most tiles one (work-balanced) band may take
  int epi_stop;                      // diagnostics: the epilogue stops after phase k (0 = full)
  const LaunchFrames* frames;        // null: one frame; else frames->n frames in one launch
};

constexpr int kMaxBandTiles = 8192;


// Flat shading of the DOS/EBS renderers (option "shade_flat", shaded_march.h):
// one frame's shading jobs in a single global list, shaded by a grid of their own
// and folded into the pixels afterwards.  Buffers grow on demand, one set per context.
// One set of flat-shading buffers (shaded_march.h launch_shaded_flat).  Each
// render stream gets its own set (Ctx::flat), so DOS/EBS frames on different
// streams pipeline; a set is sized from the totals of its earlier frames, read
// back without blocking (ev_read), and a frame whose list would not fit renders
// through the per-wave kernel instead, decided on the device (flag).
struct FlatJobs {
  uint32_t* tile_off = nullptr;             // jobs per 8x8 tile, scanned in place to offsets [tiles + 1]
  uint32_t* tile_roff = nullptr;            // march rounds with a job per tile, scanned likewise
  unsigned long long* masks = nullptr;      // per such round: the lanes that made a job (ballot)
  unsigned long long* total = nullptr;      // [3]: the frame's jobs, rounds, overflow flag (device)
  unsigned long long* h_total = nullptr;    // pinned host copy of an earlier frame's [3]
  float4* cam = nullptr;                    // the ray's camera direction per pixel slot
  float4* jobs = nullptr;                   // 2 float4 per job (+1 with Phong)
  float4* res = nullptr;                    // shaded rgb * alpha, alpha, per job
  int tiles = 0;                            // allocated 8x8 tiles
  size_t cap = 0;                           // allocated jobs (float4 units: cap * 3)
  size_t rcap = 0;                          // allocated round masks
  // host side of the set
  hipEvent_t ev_read = nullptr;             // h_total holds the totals of the frame recorded last
  hipEvent_t ev_done = nullptr;             // the set's last frame is done with its buffers
  bool pending_read = false;
  size_t want_jobs = 0, want_rounds = 0;    // the largest totals read back so far
  hipStream_t stream = nullptr;             // the render stream the set serves
  bool owned = false;
  long long last_use = -1;
};    // the epilogue sorts a band in LDS (32 KiB + group prefixes)

struct Ctx {
  int device = 0;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  std::string err;
  // volume
  int N[3] = {0, 0, 0};
  float scale[3] = {1, 1, 1};
  int bpv = 0;
  void* d_vox = nullptr;          // raw voxels (u8/u16), kept for gradient/precompute
  size_t vox_bytes = 0;
  void* d_cells = nullptr;        // cell8 fp16 layout
  size_t cells_bytes = 0;
  CellGrid cells{};
  uint16_t* d_lut = nullptr;      // raw value -> R16F bits (GetNormalizedSample)
  // empty-space skipping (option "macro": log2 of the macro cell, 0 = off)
  int macro_shift = 3;
  int skip_min_pct = 15;          // skipping is compiled in when >= this % of cells are empty
  // per-cell skip flags in the cells' sign bits (march_common.h cell_empty /
  // cell_skip_q; option "cell_skip": 0 off, 1 empty-sample flags, 2 flags + the
  // distance skip per lane, 3 (default) when every marching lane can, 4 by the
  // lanes that can; raymarch.hip march_ray)
  int cell_skip = 3;
  int debug_flags_oom = 0;        // tests (option "debug_cell_flags_oom"): the flag build reports OOM
  // transfer function (RGBA16F values as float)
  float* d_tf = nullptr;
  int tf_n = 0;
  float tf_max_alpha = 0.0f;         // largest (fp16-rounded) TF opacity; NaN if any is not finite
  // gradient (4 x fp16 per voxel, x-fastest)
  void* d_grad = nullptr;          // gradient cell8: 3 uint4 (x, y, z fp16 pairs) per volume cell
  size_t grad_bytes = 0;
  int grad_mode = 0;
  // march tuning: samples fetched per batch (2, 4; 0 = auto: 4, or 2 with Phong
  // shading, whose extra registers make occupancy worth more than a deeper batch)
  int batch = 0;
  int cost_time = 0;               // option "tile_cost": 0 longest ray, 1 measured time (worse)
  int max_waves_cu = 0;            // experiment (option "max_waves_cu"): cap residency via LDS
  int epi_stop = 0;                // diagnostics (option "debug_epi_stop")
  int debug_keep = 0;              // diagnostics (option "debug_keep"): render only the longest entries
  int band_cap_pct = 130;           // option "band_cap": most tiles a work-balanced XCD band may take, % of 1/8
  int boost_pct = 5;               // % of every band's longest entries run at raised priority
  int filter_bits = 0;             // GL_LINEAR weights at this many fraction bits (0 = exact; rc1pass)
  int quad_pct = 0;                // % of every band's longest tiles marched 4 lanes per ray
  int shade_counters = 0;          // DOS/EBS: count shaded and shadow-lit samples
  int shade_flat = 1;              // DOS/EBS: 1 = flat job list (FlatJobs), 0 = per-wave batches
  int flat_group = 8;              // flat shading: 64-job chunks per XCD turn (XCD-aware order)
  int debug_flat_limit = 0;        // tests: a frame with more jobs takes the per-wave fallback
  static constexpr int kFlatSets = 16;    // flat-shading buffer sets, one per render stream
  mutable FlatJobs flat[kFlatSets];
  mutable long long flat_clock = 0;
  unsigned long long* d_shade = nullptr;   // [3]: shaded, lit, secondary fetches (last frame)
  int tile_stats = 0;              // record per-tile timing (diagnostics)
  unsigned long long* d_tile_stats = nullptr;
  int tile_stats_n = 0;
  // kernel_timing option: HIP events around every frame's ray-march launch (ring)
  std::vector<hipEvent_t> ev_start, ev_stop;
  long long timed_frames = 0;
  int use_order = 1;               // 1: longest-first (LPT) from an earlier frame's costs;
                                   // 0: screen order in XCD bands; 2: screen order interleaved over XCDs
  // The LPT order is built off the critical path: frame i's costs are sorted
  // on a side stream while frames i+1, i+2 render, and frame i+3 uses the
  // result (kOrderSlots slots in rotation; frame i uses and refills slot
  // i % kOrderSlots).  With two slots the sort, which only gets CUs in the
  // next frame's tail, still held up the frame after (~11 us per frame).
  struct OrderSlot {
    int* d_order = nullptr;        // launch order (8 x slots per band)
    uint32_t* d_cost = nullptr;    // per-wave-tile critical path, written by the frame
    int units = 0;                 // order entries allocated
    int ntiles = 0;                // cost entries allocated
    int key = -1;                  // plan signature of the order in d_order
    int valid = 0;
    hipEvent_t done = nullptr;     // the side-stream sort of this slot has finished
    bool pending = false;
    hipStream_t stream = nullptr;  // render stream that owns the slot (async_order 0)
    bool owned = false;
    long long frames = 0;          // frames rendered with this slot
    float view[7] = {0};           // eye, unit forward, tan(fovy/2) of the frame the order came from
    bool has_view = false;
    float last_view[7] = {0};      // the previous frame's view on this slot
    bool has_last = false;
  };
  int stale_deg = 5;               // option "stale_deg": an order learned on a view more than this
                                   // far away (degrees / 1/12 of the eye distance) is not used
  static constexpr int kOrderSlots = 32;  // one per render stream (async_order uses the first 3)
  int async_order = 0;             // option "async_order": 1 = sort on a side stream (lag 3)
  int order_interval = 8;          // option "order_interval": rebuild the order every n-th frame
  OrderSlot oslot[kOrderSlots];
  int slot_rr = 0;                 // next slot handed to a new render stream
  long long frame_no = 0;
  int rc1pass_variant = -1;        // option "rc1pass_variant": the last rc1pass_tile_kernel launched (-1: none)
  hipStream_t side = nullptr;      // high-priority stream for the order builds
  hipEvent_t ev_frame = nullptr;   // end of a frame's ray-march (the side stream waits on it)
  int num_cus = 0;
  // options of the EBS SAT build: z planes per work item; the frame reads 0 = the cell4
  // copy, 1 = the plain SAT; 1 keeps the double build grid for rebuilds
  int sat_chunk = 32, sat_layout = 0, sat_keep_scratch = 0;
  // State derived from (volume, TF): one struct per technique, each with one drop
  // function (cvr_host.h); cvr_api.cpp derived_drop says who drops which.
  // Empty-space skipping (cvr_rc1pass.cpp), from (volume, TF, option "macro"): the
  // macro cells' min/max (of the volume, for mm_shift), the TF's prefix counts of
  // entries with alpha > 0, the occupancy built of both (occ_empty: the empty
  // fraction), and whether the density cells' sign bits carry skip flags (set), of
  // the current TF (valid), or their build ran out of memory (oom: retried after a
  // volume / TF change).  Occupancy and flags are rebuilt lazily by the frames.
  struct Skip {
    uint32_t* d_macro_minmax = nullptr;
    uint8_t* d_occ = nullptr;
    int* d_tf_prefix = nullptr;
    int mm_shift = -1, mdim[3] = {0, 0, 0}, occ_valid = 0;
    float occ_empty = 0.0f;
    int flags_valid = 0, flags_set = 0, flags_oom = 0;
  } skip;
  // Directional occlusion (cvr_dos.cpp), from (volume, the RGBA TF and sigma0 of
  // cvr_set_extinction_volume): the extinction pyramid as fp16 levels (x fastest,
  // concatenated at `off`) and as cell8 texels, its level table [kMaxExtLevels]
  // for the cone fetches, finite (every TF opacity < 1: no infinite extinction),
  // and the cone tables (occlusion, shadow) of cone_key on the host and the
  // device, rebuilt when a frame's cone parameters differ.
  struct Ext {
    uint16_t* d_ext = nullptr;
    uint4* d_cells = nullptr;
    ExtLevel* d_levels = nullptr;
    int res[3] = {0, 0, 0}, levels = 0, finite = 0;
    long long off[kMaxExtLevels + 1] = {};
    float sigma0 = 1.0f;
    float4* d_cones = nullptr;
    cvr_cone_params cone_key[2] = {};
    int cone_valid = 0;
    cvr_cone_tables cone_tab[2] = {};
  } ext;
  // Extinction-based shading (cvr_ebs.cpp), from (volume, the extinction LUT of
  // cvr_set_extinction_sat): the float SAT of (N + 2) cells per axis, its cell4
  // copy (4 float corners of a plane per texel, sat.hip; only while sat_layout 0
  // reads it), the double grid of the build (only with sat_keep_scratch) and the
  // GPU time of the last build.
  struct Sat {
    float* d_sat = nullptr;
    float4* d_cells = nullptr;
    void* d_scratch = nullptr;
    int dims[3] = {0, 0, 0}, build_us = 0;
  } sat;
  // What a light cache was computed from (cvr_render_dosct_preillum and
  // cvr_render_extbsd_preillum skip the compute when nothing of it changed);
  // invalid after cvr_set_light_cache.  Compared as bytes: 4-byte members only.
  // kind: the producer, 0 DOS cones, 1 EBS SAT; the other producer's part and the
  // parameters of a term that is switched off stay zero.
  struct LightCacheKey {
    int valid = 0, kind = 0, dims[3] = {0, 0, 0};
    int apply_occlusion = 0, apply_shadow = 0, shadow_type = 0, filter_bits = 0;
    struct Dos {
      cvr_cone_params cone[2] = {};
      cvr_light light = {};
      float eye[3] = {0, 0, 0}, cam_up[3] = {0, 0, 0};   // with occlusion on
    } dos;
    struct Ebs {
      int shells = 0;
      float radius = 0, angle = 0, interval = 0, initial = 0, weight = 0, max_distance = 0;
      float light[3] = {0, 0, 0};      // the position (shadow type 0) or the forward vector (1)
    } ebs;
  };
  // Pre-illumination (cvr_lightcache.cpp), from `key` plus the volume, the TF and
  // the producer's pyramid or SAT: the RG16F cache (4 B per voxel), and who reads
  // and wrote it.  readers: frames that read the cache since it was last written,
  // 0 none, 1 on `reader` only (a later write on that stream is ordered behind
  // them), 2 on several streams (the write drains the device first).  written: the
  // last compute ran on `writer` and ended at `ev` (a frame on another stream
  // waits for it).  builds: computes so far.
  struct LightCache {
    uint32_t* d_cache = nullptr;
    int dims[3] = {0, 0, 0};
    size_t bytes = 0;
    LightCacheKey key;
    hipStream_t reader = nullptr, writer = nullptr;
    hipEvent_t ev = nullptr;
    int readers = 0, builds = 0;
    bool written = false;
  } lc;
  // Isosurface block table (cvr_iso.cpp), from (volume, nb): float2 min/max per block.
  struct Iso {
    float2* d_mm = nullptr;
    int nb[3] = {0, 0, 0}, valid = 0;
  } iso;
  // ground-truth cone ray-caster (cvr_crtgt.cpp): the progressive frame between
  // cvr_crtgt_begin and its cvr_crtgt_advance calls
  struct Crtgt {
    bool valid = false;                // begun, and the volume, TF and gradient are still those
    CrtgtArgs q{};
    CrtgtState st;
    float* d_rays = nullptr;           // both tables, occlusion first
    size_t npix = 0;                   // pixels the state is allocated for
    int job_f4 = 0;                    // float4 per job the storage is allocated for
    size_t ray_cap = 0;                // rays d_rays holds
    size_t bytes = 0;                  // all of the above (cvr_device_bytes)
    int ntiles = 0;
    unsigned long long unfinished = 0;
  } gt;
  // voxel cone tracing (cvr_vct.cpp): the supervoxel pyramid of the volume, the
  // pre-integration table of (volume, opacities) and the cone schedule of the
  // last frame's parameters
  struct Vct {
    uint32_t* d_pyr = nullptr;
    VctLevel* d_levels = nullptr;      // [kMaxVctLevels]
    VctLevel levels[kMaxVctLevels] = {};
    int nl = 0;                        // 0: no pyramid
    size_t texels = 0;
    double max_stddev = 0.0;
    int builds = 0;                    // option "vct_pyramid_builds" (read-only)
    std::vector<float> opacity;        // GetOpc(i, 255), i < 255; empty: not set
    uint16_t* d_table = nullptr;
    int tab_h = 0;                     // 0: no table
    VctStep* d_steps = nullptr;
    int steps_cap = 0;
    float steps_key[8] = {};           // what d_steps was computed from
    int steps_valid = 0;
    size_t bytes = 0;                  // all of the above (cvr_device_bytes)
  } vct;
  // slice-based directional occlusion (cvr_sbtm.cpp): the eye buffer and two sets of
  // the two occlusion planes of the last frame's viewport (16 B per pixel; set `cur`
  // holds the planes, a blocked launch reads it and writes the other), and what the
  // read-only options sbtm_slices / sbtm_launches report
  struct Sbtm {
    uint2* d_eye = nullptr;
    uint16_t* d_occ = nullptr;         // set k at d_occ + k * 2 * npix
    int cur = 0;
    size_t npix = 0;
    size_t bytes = 0;                  // all of the above (cvr_device_bytes)
    int slices = 0, launches = 0;
  } sbtm;
  int sbtm_slices_per_launch = 1;    // option "sbtm_slices_per_launch" (default: by measurement, DESIGN.md 5d''')
  // deferred isosurface shading (cvr_deferred.cpp): the G-buffer of the last geometry
  // pass (DeferredShadeArgs above: 32 B per pixel), the viewport and camera eye of that
  // pass, its hit counter on the device (option "deferred_hits") and the geometry
  // launches so far (option "deferred_launches")
  struct Deferred {
    float4* d_gbuf = nullptr;          // gPosition at [0, npix), gNormal at [npix, 2 npix)
    unsigned long long* d_hits = nullptr;
    int W = 0, H = 0;
    bool valid = false;                // a geometry pass has filled it
    float eye[3] = {0, 0, 0};
    size_t bytes = 0;                  // the planes (cvr_device_bytes)
    int launches = 0;
  } deferred;
  // advanced deferred shading (cvr_advdeferred.cpp): the curvature planes of the kept
  // G-buffer (16 B per pixel; valid for that G-buffer and the projection scales p00 /
  // p11: every geometry pass clears `valid`, deferred_drop frees them), the two tables
  // of the lighting pass (built once; the colour map again when s or v change), the
  // feature-pixel counter of the last lighting pass, and the curvature launches so far
  struct AdvDeferred {
    float4* d_curv = nullptr;
    float4* d_cmap = nullptr;
    float* d_ridge = nullptr;
    unsigned long long* d_features = nullptr;
    bool valid = false;
    bool shaded = false;               // a lighting pass has written d_features
    float p00 = 0, p11 = 0;
    float cmap_s = 0, cmap_v = 0;      // what d_cmap was built from
    size_t bytes = 0;                  // the planes (cvr_device_bytes)
    size_t table_bytes = 0;            // the tables
    int launches = 0;
  } adv;
  unsigned long long* d_tile_samples = nullptr;   // per-wave-tile sample counts (zeroed)
  int tile_samples_n = 0;
  // d_tile_samples and d_shade are one set per context: a frame that uses them on
  // another stream than the previous user waits for that frame (counters_guard)
  hipStream_t counters_stream = nullptr;
  hipEvent_t ev_counters = nullptr;
  // multi-GPU gather (cvr_comm.cpp): RCCL communicator, its stream and events
  void* comm = nullptr;
  int split_streams = 1;           // option "split_streams": render streams the caller rotates
  int gather_sets = 0;             // option "gather_sets": buffer sets the caller rotates (>= split_streams)
  int launch_interleave = 1;       // option "launch_interleave": multi-frame launches deal the frames'
                                   // launch-order entries interleaved (LaunchFrames::interleave)
  int gather_root_idle = 0;        // option "gather_root_idle": rank 0 only gathers (renders nothing)
  int exchange_code = 1;           // option "exchange_code": RGBA16F exchanges move the per-tile code
  int native_exp = 0;               // option "native_exp": tolerance mode (v_exp_f32 in the EA composite)
  int encode_onepass = 0;          // option "encode_onepass": cvr_encode_tiles uses the exchange's
                                   // one-launch encode (tiles in claim order)
  int exchange_lag = -1;           // option "exchange_lag": data phase trails by this many exchanges
                                   // (-1 = split_streams - 1, bounded by the buffer sets)
  // single-process group (cvr_create_group, cvr_group.cpp): the members this context fans out to
  struct Group* group = nullptr;
  // scratch
  unsigned long long* d_total = nullptr;
  void* d_scratch = nullptr;      // host-output staging
  size_t scratch_bytes = 0;
};

void comm_release(Ctx* c);   // cvr_comm.cpp
// cvr_group.cpp: a group context's members
struct Group;
using MemberRender = std::function<cvr_status(cvr_ctx*, const cvr_frame*, int, const cvr_output*)>;
void group_release(Ctx* g);
cvr_status group_each(Ctx* g, const std::function<cvr_status(cvr_ctx*)>& fn);
cvr_status group_call_root(Ctx* g, const std::function<cvr_status(cvr_ctx*)>& fn);
Ctx* group_root(Ctx* g);
cvr_status group_render(Ctx* g, const cvr_frame* frames, int nf, const cvr_output* outs,
                        const MemberRender& render);
void flat_release(FlatJobs& J);   // flat.hip

// postpass.hip: multiscaling filters (mode 1-3, kernel 0-5) and the screenshot
hipError_t launch_multiscale(int mode, int kernel, void* frame, int fw, int fh, void* screen, int sw,
                             int sh, hipStream_t s);
hipError_t launch_screenshot(const void* frame, int half, int w, int h, uint8_t* rgb,
                             hipStream_t s);

// kernels / launchers (raymarch.hip)
hipError_t launch_build_cells_impl(const void* vox, int bpv, const uint16_t* lut, const int N[3],
                                   const CellGrid& g, void* cells, hipStream_t s);
hipError_t launch_gradient(const Ctx& c, int mode, uint2* tmp, hipStream_t s);
hipError_t launch_selftest_arith(int e_rcp_lo, int e_rcp_n, int e_sqrt_lo, int e_sqrt_n,
                                 unsigned long long* bad, hipStream_t s);
// plan.frames: null for one frame, else plan.frames->n frames in one launch
// (out / samples: frame 0's).  variant: the packed template arguments of the
// rc1pass_tile_kernel it launched (Rc1Variant::packed, option "rc1pass_variant");
// left alone when nothing was launched
hipError_t launch_rc1pass(const Ctx& c, const Rc1passArgs& a, bool phong, float4* out,
                          uint32_t* samples, unsigned long long* tile_samples, const int* order,
                          uint32_t* tile_cost, const RenderPlan& plan, hipStream_t s, int& variant);
// after a frame: sums tile_samples into *total and/or builds the next LPT order
hipError_t launch_tile_epilogue(uint32_t* tile_cost, unsigned long long* tile_samples,
                                unsigned long long* total, const RenderPlan& plan, int* order,
                                hipStream_t s);
hipError_t launch_macro_minmax(const Ctx& c, int shift, const int mdim[3], uint32_t* out,
                               hipStream_t s);
hipError_t launch_occupancy(const uint32_t* minmax, int n_macro, const uint16_t* lut,
                            const int* prefix, int tf_n, uint8_t* occ, unsigned int* n_empty,
                            hipStream_t s);
// skip flags of the density cells for the current TF (clear: strip them); t0, t1
// are two scratch bytes per cell
hipError_t launch_cell_flags(const Ctx& c, bool clear, uint8_t* t0, uint8_t* t1, hipStream_t s);
hipError_t launch_ext_volume(const Ctx& c, const float4* d_tf_rgba, int tf_n, const int res[3],
                             float sigma0, int nlevels, const long long* off, uint16_t* d_ext,
                             uint4* d_ext_cells,
                             hipStream_t s);
hipError_t launch_sat_build(const Ctx& c, const float* d_lut, double* d_sd, float* d_sf,
                            hipStream_t s);
hipError_t launch_sat_cells(const Ctx& c, const float* d_sf, float4* d_cells, hipStream_t s);
size_t sat_cells_float4s(int w, int h, int d);   // the size of that layout, in float4
hipError_t launch_ebs(const Ctx& c, const EbsArgs& q, float4* out, uint32_t* samples,
                      unsigned long long* shade, unsigned long long* tile_samples, hipStream_t s);
hipError_t launch_dos(const Ctx& c, const DosArgs& q, float4* out, uint32_t* samples,
                      unsigned long long* shade,
                      unsigned long long* tile_samples, hipStream_t s);
// lightcache.hip: the light cache of the DOS cones, and the march that reads a cache
hipError_t launch_light_cache(const DosArgs& q, const LightCacheArgs& p, const uint4* ext,
                              uint32_t* out, hipStream_t s);
// ebs_lightcache.hip: the light cache of the EBS SAT terms (the context's SAT in its sat_layout)
hipError_t launch_ebs_light_cache(const Ctx& c, const EbsArgs& q, const LightCacheArgs& p, uint32_t* out,
                                  hipStream_t s);
hipError_t launch_preillum(const Ctx& c, const DosArgs& q, const LightCacheView& v, float4* out,
                           uint32_t* samples, unsigned long long* shade,
                           unsigned long long* tile_samples, hipStream_t s);
// crtgt.hip: the ground-truth frame's state reset, one launch round of at most k
// (<= kCrtgtRoundSamples) iterations per pixel (march, shade, fold), and the copy of
// the state into an output image
hipError_t launch_crtgt_init(const CrtgtArgs& q, const CrtgtState& st, hipStream_t s);
hipError_t launch_crtgt_round(const Ctx& c, const CrtgtArgs& q, const CrtgtState& st, int k, hipStream_t s);
hipError_t launch_crtgt_store(const CrtgtArgs& q, const CrtgtState& st, float4* out, uint32_t* samples,
                              unsigned long long* total, int half, hipStream_t s);
// vct_precompute.hip: the pyramid of the context's u8 volume (levels laid out by
// `lv`; scratch: doubles for the means of every level >= 1; max_bits: the largest
// standard deviation's double bits, zeroed by the caller)
hipError_t launch_vct_pyramid(const Ctx& c, const VctLevel* lv, int nl, uint32_t* pyr, double* scratch,
                              unsigned long long* max_bits, hipStream_t s);
// vct.hip: the cone schedule of a frame's parameters, and the frame
hipError_t launch_vct_schedule(const VctLevel* d_levels, int nl, float initial, float step, float rate,
                               float tan_apex, float corr, int n, int filter_bits, VctStep* out,
                               hipStream_t s);
hipError_t launch_vct(const Ctx& c, const VctArgs& q, const VctData& data, float4* out, uint32_t* samples,
                      unsigned long long* shade, unsigned long long* tile_samples, hipStream_t s);
// sbtm.hip: the frame's clear (eye 0, both occlusion planes 1, counts 0), one launch
// of b.n consecutive slices (b.n == 1: the plain form, occlusion read from global
// memory, in place; else the blocked form, b.ex / b.ey <= kSbtmHalo, which reads
// p.occ and leaves the planes in p.occ_out), and the eye buffer's copy into an
// output image
hipError_t launch_sbtm_clear(const SbtmPlanes& p, int W, int H, hipStream_t s);
hipError_t launch_sbtm_slices(const Ctx& c, const SbtmArgs& q, const SbtmBatch& b, const SbtmPlanes& p,
                              hipStream_t s);
hipError_t launch_sbtm_store(const SbtmPlanes& p, int W, int H, float4* out, int half, hipStream_t s);
// iso.hip: raw per-block extremes (uint2), and the isosurface march (variant 0/1)
hipError_t launch_block_minmax(const void* vox, int bpv, const int N[3], const int nb[3], uint2* out,
                               hipStream_t s);
hipError_t launch_iso(const Ctx& c, const IsoArgs& q, int variant, bool phong, const float2* mm,
                      float4* out, uint32_t* samples, unsigned long long* tile_samples,
                      hipStream_t s);
// deferred.hip: the geometry pass (q: the iso march's uniforms; clear: the G-buffer's
// clear value; hits: += pixels with a hit) and the shade pass over a G-buffer (lighting
// and tone map; samples / total: the geometry pass's counts, total is added to)
hipError_t launch_deferred_geometry(const Ctx& c, const IsoArgs& q, const float clear[4], const float2* mm,
                                    float4* gbuf, unsigned long long* hits, hipStream_t s);
hipError_t launch_deferred_shade(const DeferredShadeArgs& q, const float4* gbuf, float4* out, int half,
                                 uint32_t* samples, unsigned long long* total, hipStream_t s);
// advdeferred.hip: the curvature pass over a G-buffer's normal plane (p00, p11: the
// projection's x and y scales) and the feature-lighting pass with the tone map
// (features: += pixels whose feature colour has red or green set)
hipError_t launch_adv_curvature(int W, int H, float p00, float p11, const float4* gbuf, float4* curv,
                                hipStream_t s);
hipError_t launch_adv_shade(const AdvShadeArgs& q, const float4* gbuf, const float4* curv, const float4* cmap,
                            const float* ridge, float4* out, int half, uint32_t* samples,
                            unsigned long long* total, unsigned long long* features, hipStream_t s);
// codec.hip: the lossless per-tile code of RGBA16F tiles (cvr_encode_tiles)
size_t tile_code_bound_bytes(int tile, int ntiles);
hipError_t launch_tile_encode(const void* d_tiles, int tile, int ntiles, void* d_stream,
                              unsigned long long* d_bytes, hipStream_t s);
hipError_t launch_tile_decode(const void* d_stream, int tile, int ntiles, void* d_tiles, hipStream_t s);
hipError_t launch_unpack_tiles(const void* packed, void* out, int half, int W, int H, int tile,
                               int nranks, int tpr_max, hipStream_t s, size_t rank_stride = 0);
hipError_t launch_unpack_tiles_u32(const uint32_t* packed, uint32_t* out, int W, int H, int tile,
                                   int nranks, int tpr_max, hipStream_t s, size_t rank_stride);
// the exchange's one-launch encode of a group (nframes x k tiles at slot stride tpr)
// into d_dst; ctr: a zeroed 64-bit counter on this device that no other launch in
// flight uses, left zero (it may be d_bytes itself); h_bytes (may be null): the same
// length into mapped host memory (its device pointer)
hipError_t launch_exchange_encode(const void* d_packed, int tile, int k, int tpr, int nframes, void* d_dst,
                                  unsigned long long* ctr, unsigned long long* d_bytes, unsigned long long* h_bytes,
                                  hipStream_t s);
// rank 0: every source's stream (or raw tiles) of a group decoded into the frames' images
struct ExchangeDecode {
  const uint32_t* src;               // source r's stream at src + r * slot_words
  size_t slot_words;
  const uint2* raw0;                 // source 0 as raw packed tiles (a rendering root), or null
  size_t raw0_fstride;               // tiles between frames of raw0
  int nsrc;                          // sources = the split's ranks
  int nsplit;                        // the split's nranks (split_tile)
  int nframes, tpr;                  // frames of the group, tile slots per frame and source
  int tile, W, H, ntx, tile_grid_n;  // tile size, image, tiles per row, tiles per frame
  uint2* img[kMaxLaunchFrames];      // frame f's RGBA16F image (null: skipped)
};
hipError_t launch_exchange_decode(const ExchangeDecode& a, hipStream_t s);

inline CellGrid make_cell_grid(const int N[3]) {
  CellGrid g;
  g.cx = N[0] + 1; g.cy = N[1] + 1; g.cz = N[2] + 1;
  g.pitch_y = g.cx;
  g.pitch_z = g.cx * g.cy;
  g.linear_origin = 1 + (long long)g.pitch_y + (long long)g.pitch_z;
  g.bpitch_y = (int)((long long)g.pitch_y * 16 < (1ll << 31) ? g.pitch_y * 16 : 0);
  g.bpitch_z = (int)((long long)g.pitch_z * 16 < (1ll << 31) ? (long long)g.pitch_z * 16 : 0);
  g.borigin = (uint32_t)((unsigned long long)g.linear_origin * 16ull);
  return g;
}

inline size_t cell_count(const CellGrid& g) { return (size_t)g.cx * g.cy * g.cz; }

// ---------------------------------------------------------------------------
// Addressing of a SAT fetch (ebs.hip), shared by the kernels and the host check
// cvr_sat_layout_check.  The texel (tx, ty, tz) is clamped to [0, dims - 1]; its
// element index (tz * h + ty) * w + tx is formed with 24-bit products (both
// operands < 2^24, the result < 2^32: checked on the host).  A fetch reads:
//  * layout 0 (cell4, float4 per texel): elements idx and idx + w*h;
//  * layout 1 (plain float SAT): the float pairs at idx, idx + w, idx + w*h and
//    idx + w*h + w (x, x + 1 of rows y, y + 1 of planes z, z + 1).  A clamped
//    texel's +1 neighbours have weight 0 but are still read; at the far corner
//    (w-1, h-1, d-1) the last one is element w*h*d + w*h + w, so the buffer
//    carries kSatPlainPadPlanes planes of zeros after the SAT.  (Round 3's
//    variant padded one plane: that read ran w + 1 floats past its allocation,
//    4108 B at 1026^3 — always into the next 4 KiB page — and faulted there.)
// ---------------------------------------------------------------------------
constexpr int kSatPlainPadPlanes = 2;

__host__ __device__ inline uint32_t sat_texel_index(uint32_t tx, uint32_t ty, uint32_t tz, uint32_t w,
                                                    uint32_t h) {
#ifdef __HIP_DEVICE_COMPILE__
  return __umul24(__umul24(tz, h) + ty, w) + tx;
#else
  return ((tz * h + ty) & 0xffffffu) * w + tx;   // the 24-bit product's operand, as the device
#endif
}

// floats the plain layout allocates for a w x h x d SAT
inline size_t sat_plain_floats(int w, int h, int d) {
  return (size_t)w * h * (size_t)(d + kSatPlainPadPlanes);
}

}  // namespace cvr
