// sbtm.hip — slice-based directional occlusion (cppvolrend s_sbtm_dos,
// SBTMDirectionalOcclusionShading: evaluationslice.vert / .frag) on gfx950.
//
// The reference rasterises one view-aligned quad per slice; every fragment of it is
// the point of its pixel's view ray at the slice's depth, so a slice is a 2-D pass
// over the screen (sbtm_fragment): the box and quad tests, one volume sample and TF
// fetch, the front-to-back composite into the RGBA16F eye buffer weighted by a
// bilinear fetch of the previous occlusion plane, and the next occlusion plane as the
// mean of GridSize.x x GridSize.y bilinear taps of the previous one (Algorithm3).
// A pixel therefore reads its neighbours' values of the slice before, which no ray
// march here does.  Two forms of the pass, the same bits:
//
//  * plain (one slice per launch): the planes are read from and written to global
//    memory; slices are ordered by the stream.  Correct by construction.
//  * blocked (n <= 16 slices per launch): a workgroup owns a 64 x 64 screen tile plus
//    a halo of the batch's summed tap radii (at most 16 pixels a side), holds both
//    occlusion planes of that region in LDS as halves (36 KiB: four workgroups fit
//    a CU's LDS) and its tile's eye pixels in registers, and advances the slices with
//    a __syncthreads() between them.  After slice j only the tile grown by the radii
//    of the slices still to come is valid, which is all those slices read; ring
//    pixels compute the occlusion only.  Only the tile is written back, and into
//    a second set of planes: a neighbour's halo is this tile, and nothing orders
//    that workgroup's load against this one's store, so a launch reads one set
//    and writes the other (every pixel belongs to one tile: the set written is
//    complete).
//
// A slice's radius is a proven bound (cvr_sbtm.cpp, DESIGN.md 5d'''), so a tap never
// leaves the region; the screen border clamps as CLAMP_TO_EDGE does, toward the
// pixel, hence also inside the region.  No grid-wide barrier, no spinning.
//
// Arithmetic follows CVR-SPEC (DESIGN.md 5d''') as tests/support/sbtm_ref.cpp does,
// op for op.  Compiled -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "cvr_device.h"
#include "march_common.h"

namespace cvr {

namespace {

constexpr int T = kSbtmTile;
constexpr int NT = kSbtmThreads;
constexpr int kPix = T * T / NT;             // tile pixels per thread

__device__ __forceinline__ float h2f(uint16_t b) { return (float)__builtin_bit_cast(_Float16, b); }

__device__ __forceinline__ float4 eye_widen(uint2 e) {
  float4 v;
  h2f2(e.x, v.x, v.y);
  h2f2(e.y, v.z, v.w);
  return v;
}
__device__ __forceinline__ uint2 eye_pack(float4 v) {
  return make_uint2(f32_to_h16(v.x) | (f32_to_h16(v.y) << 16), f32_to_h16(v.z) | (f32_to_h16(v.w) << 16));
}

// texture(TexTransferFunc, density) from the table in global memory (a slice takes
// one sample per pixel: staging the table per workgroup would cost more than it saves)
template <int FB>
__device__ __forceinline__ float4 classify_global(const float4* __restrict__ tf, int n, float dens) {
  const float fn = (float)n;
  const float x = fminf(fmaxf(fmaf(dens, fn, -0.5f), -1.0f), fn - 1.0f);
  const float fl = floorf(x);
  const float a = filter_weight<FB>(x - fl);
  const int i = (int)fl;
  const float4 t0 = tf[max(i, 0)], t1 = tf[min(i + 1, n - 1)];
  return make_float4(lerpf(t0.x, t1.x, a), lerpf(t0.y, t1.y, a), lerpf(t0.z, t1.z, a), lerpf(t0.w, t1.w, a));
}

// texture(OcclusionBufferPrev, (u, v)).r: GL_LINEAR, CLAMP_TO_EDGE, x then y.
// at(x, y): the stored half of texel (x, y), widened.
template <int FB, class At>
__device__ __forceinline__ float occ_fetch(const Rc1passArgs& A, float u, float v, const At& at) {
  const float wf = (float)A.W, hf = (float)A.H;
  const float x = fminf(fmaxf(fmaf(u, wf, -0.5f), 0.0f), wf - 1.0f);
  const float y = fminf(fmaxf(fmaf(v, hf, -0.5f), 0.0f), hf - 1.0f);
  const float flx = floorf(x), fly = floorf(y);
  const float ax = filter_weight<FB>(x - flx), ay = filter_weight<FB>(y - fly);
  const int x0 = (int)flx, y0 = (int)fly;
  const int x1 = min(x0 + 1, A.W - 1), y1 = min(y0 + 1, A.H - 1);
  return lerpf(lerpf(at(x0, y0), at(x1, y0), ax), lerpf(at(x0, y1), at(x1, y1), ax), ay);
}

// One fragment of slice S at pixel (px, py) (evaluationslice.frag main).  Returns
// false for a discarded fragment, which writes nothing.  EYE: composite into dst
// (the pixel's eye value, halves widened; returned rounded to half again); without
// it only the new occlusion value is computed (the blocked form's ring).
template <int FB, bool EYE, class At>
__device__ __forceinline__ bool sbtm_fragment(const SbtmArgs& Q, const SbtmSlice& S,
                                              const uint4* __restrict__ cells, const float4* __restrict__ tf,
                                              int px, int py, const At& at, float4& dst, float& occ_new) {
  const Rc1passArgs& A = Q.a;
  // xy_d, and the pixel's view ray with view-space z = -1 (the ray generation's arithmetic)
  const float u = ((float)px + 0.5f) / (float)A.W, v = ((float)py + 0.5f) / (float)A.H;
  const float vx = fmaf(u, 2.0f, -1.0f), vy = fmaf(v, 2.0f, -1.0f);
  const f3 c{(vx * A.tan_half_fovy) * A.aspect, vy * A.tan_half_fovy, -1.0f};
  const f3 d{dot3(c, f3{A.col0[0], A.col0[1], A.col0[2]}), dot3(c, f3{A.col1[0], A.col1[1], A.col1[2]}),
             dot3(c, f3{A.col2[0], A.col2[1], A.col2[2]})};
  const f3 P{fmaf(d.x, S.depth, A.eye[0]), fmaf(d.y, S.depth, A.eye[1]), fmaf(d.z, S.depth, A.eye[2])};
  // outside the slice quad (a NaN fails both tests)
  const f3 rel{P.x - S.c[0], P.y - S.c[1], P.z - S.c[2]};
  const float qa = dot3(rel, f3{Q.right[0], Q.right[1], Q.right[2]});
  const float qb = dot3(rel, f3{Q.up[0], Q.up[1], Q.up[2]});
  if (!(fabsf(qa) <= Q.half_diag && fabsf(qb) <= Q.half_diag)) return false;
  // outside the scaled box (.frag:88-92)
  const f3 hg{A.half_grid[0], A.half_grid[1], A.half_grid[2]};
  if (P.x > hg.x || P.x < -hg.x || P.y > hg.y || P.y < -hg.y || P.z > hg.z || P.z < -hg.z) return false;
  // GetFromTransferFunction(world_pos + aabb)
  SamplePos sp = sample_pos_clamped(fmaf(P.x + hg.x, A.n_over_g[0], -0.5f), fmaf(P.y + hg.y, A.n_over_g[1], -0.5f),
                                    fmaf(P.z + hg.z, A.n_over_g[2], -0.5f), A);
  if (FB) quantise_weights<FB>(sp);
  const float dens = trilerp_cell(cells[sp.idx], sp.ax, sp.ay, sp.az);
  const float4 src = classify_global<FB>(tf, A.tf_n, dens);
  const float e1 = -(src.w * A.step);                    // -st * StepSize
  if (EYE) {
    const float occ = occ_fetch<FB>(A, u, v, at);        // gl_FragCoord.st / ScreenSize
    const float al = 1.0f - cvr_expf_nb(e1);
    const float om = 1.0f - dst.w;
    dst.x = fmaf(om, (src.x * occ) * al, dst.x);
    dst.y = fmaf(om, (src.y * occ) * al, dst.y);
    dst.z = fmaf(om, (src.z * occ) * al, dst.z);
    dst.w = fmaf(om, al, dst.w);
    dst = eye_widen(eye_pack(dst));
  }
  // Algorithm3 (.frag:35-83)
  float sum = 0.0f;
  for (int ix = 0; ix < Q.gx; ix++) {
    const float ptx = fmaf(0.5f, fmaf(S.cvx, Q.tapx[ix], vx), 0.5f);
    for (int iy = 0; iy < Q.gy; iy++) {
      const float pty = fmaf(0.5f, fmaf(S.cvy, Q.tapy[iy], vy), 0.5f);
      sum = sum + occ_fetch<FB>(A, ptx, pty, at);
    }
  }
  occ_new = (sum / Q.gxy) * cvr_expf_nb(e1 * Q.att);
  return true;
}

// The fragments this wave kept, added to *total by one lane.
__device__ __forceinline__ void add_total(unsigned long long* total, uint32_t n) {
  const unsigned long long v = wave_sum((unsigned long long)n);
  if ((threadIdx.x & 63) == 0 && v) atomicAdd(total, v);
}

__global__ void __launch_bounds__(256) sbtm_clear_kernel(SbtmPlanes P, long long npix) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= npix) return;
  P.eye[i] = make_uint2(0u, 0u);
  P.occ[i] = 0x3c00u;              // 1.0
  P.occ[npix + i] = 0x3c00u;
  if (P.samples) P.samples[i] = 0u;
}

__global__ void __launch_bounds__(256)
sbtm_store_kernel(const uint2* __restrict__ eye, long long npix, float4* __restrict__ out, int half) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= npix) return;
  const uint2 e = eye[i];
  if (half) reinterpret_cast<uint2*>(out)[i] = e;
  else out[i] = eye_widen(e);
}

// Plain form: 32 x 8 pixels per workgroup, the planes in global memory.
template <int FB>
__global__ void __launch_bounds__(256)
sbtm_plain_kernel(SbtmArgs Q, SbtmSlice S, const uint4* __restrict__ cells, const float4* __restrict__ tf,
                  SbtmPlanes P) {
  const int W = Q.a.W, H = Q.a.H;
  const size_t npix = (size_t)W * H;
  const int px = blockIdx.x * 32 + (threadIdx.x & 31), py = blockIdx.y * 8 + (threadIdx.x >> 5);
  bool kept = false;
  if (px < W && py < H) {
    const size_t pix = (size_t)py * W + px;
    const uint16_t* prev = P.occ + (size_t)(S.plane ^ 1) * npix;
    float4 dst = eye_widen(P.eye[pix]);
    float occ_new;
    kept = sbtm_fragment<FB, true>(Q, S, cells, tf, px, py,
                                   [&](int x, int y) { return h2f(prev[(size_t)y * W + x]); }, dst, occ_new);
    if (kept) {
      P.eye[pix] = eye_pack(dst);
      P.occ[(size_t)S.plane * npix + pix] = (uint16_t)f32_to_h16(occ_new);
      if (P.samples) P.samples[pix] += 1u;
    }
  }
  if (P.total) add_total(P.total, kept ? 1u : 0u);
}

// Blocked form.  Region pixel (gx, gy) lives at lds[(gy - oy) * RW + (gx - ox)];
// only pixels inside the screen are loaded, computed or read.
template <int FB>
__global__ void __launch_bounds__(NT)
sbtm_blocked_kernel(SbtmArgs Q, SbtmBatch B, const uint4* __restrict__ cells, const float4* __restrict__ tf,
                    SbtmPlanes P) {
  __shared__ uint16_t lds[2][kSbtmRegion * kSbtmRegion];
  const int W = Q.a.W, H = Q.a.H;
  const size_t npix = (size_t)W * H;
  const int tid = threadIdx.x;
  const int tx0 = blockIdx.x * T, ty0 = blockIdx.y * T;
  const int ox = tx0 - B.ex, oy = ty0 - B.ey;
  const int RW = T + 2 * B.ex, RH = T + 2 * B.ey;
  for (int i = tid; i < RW * RH; i += NT) {
    const int ly = i / RW, lx = i - ly * RW;
    const int gx = ox + lx, gy = oy + ly;
    if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
      const size_t pix = (size_t)gy * W + gx;
      lds[0][i] = P.occ[pix];
      lds[1][i] = P.occ[npix + pix];
    }
  }
  uint2 eye[kPix];
  uint32_t cnt[kPix];
#pragma unroll
  for (int k = 0; k < kPix; k++) {
    const int idx = tid + k * NT;
    const int gx = tx0 + (idx & (T - 1)), gy = ty0 + idx / T;
    eye[k] = (gx < W && gy < H) ? P.eye[(size_t)gy * W + gx] : make_uint2(0u, 0u);
    cnt[k] = 0u;
  }
  __syncthreads();
  int ex = B.ex, ey = B.ey;
  for (int j = 0; j < B.n; j++) {          // workgroup-uniform
    const SbtmSlice& S = B.s[j];
    ex -= S.rx;                            // the radii of the slices still to come
    ey -= S.ry;
    const uint16_t* prev = lds[S.plane ^ 1];
    uint16_t* next = lds[S.plane];
    const auto at = [&](int x, int y) { return h2f(prev[(y - oy) * RW + (x - ox)]); };
#pragma unroll
    for (int k = 0; k < kPix; k++) {       // the tile: eye and occlusion
      const int idx = tid + k * NT;
      const int gx = tx0 + (idx & (T - 1)), gy = ty0 + idx / T;
      if (gx < W && gy < H) {
        float4 dst = eye_widen(eye[k]);
        float occ_new;
        if (sbtm_fragment<FB, true>(Q, S, cells, tf, gx, gy, at, dst, occ_new)) {
          eye[k] = eye_pack(dst);
          next[(gy - oy) * RW + (gx - ox)] = (uint16_t)f32_to_h16(occ_new);
          cnt[k]++;
        }
      }
    }
    // the ring of width (ex, ey) around the tile: occlusion only.  ey rows above, ey
    // rows below (both RV wide), then ex columns left and right of the tile's rows.
    const int RV = T + 2 * ex, top = ey * RV;
    const int nring = 2 * top + 2 * ex * T;
    for (int i = tid; i < nring; i += NT) {
      int rx, ry;
      if (i < 2 * top) {
        const int i2 = i < top ? i : i - top;
        const int row = i2 / RV;
        rx = i2 - row * RV - ex;
        ry = i < top ? row - ey : T + row;
      } else {
        const int i3 = i - 2 * top;
        ry = i3 / (2 * ex);
        const int col = i3 - ry * (2 * ex);
        rx = col < ex ? col - ex : T + (col - ex);
      }
      const int gx = tx0 + rx, gy = ty0 + ry;
      if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
        float4 none;
        float occ_new;
        if (sbtm_fragment<FB, false>(Q, S, cells, tf, gx, gy, at, none, occ_new))
          next[(gy - oy) * RW + (gx - ox)] = (uint16_t)f32_to_h16(occ_new);
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < kPix; k++) {
    const int idx = tid + k * NT;
    const int lx = idx & (T - 1), ly = idx / T;
    const int gx = tx0 + lx, gy = ty0 + ly;
    if (gx < W && gy < H) {
      const size_t pix = (size_t)gy * W + gx;
      const int li = (ly + B.ey) * RW + (lx + B.ex);
      P.eye[pix] = eye[k];
      P.occ_out[pix] = lds[0][li];
      P.occ_out[npix + pix] = lds[1][li];
      if (P.samples) P.samples[pix] += cnt[k];
    }
  }
  uint32_t kept = 0;
#pragma unroll
  for (int k = 0; k < kPix; k++) kept += cnt[k];
  if (P.total) add_total(P.total, kept);
}

}  // namespace

hipError_t launch_sbtm_clear(const SbtmPlanes& p, int W, int H, hipStream_t s) {
  const long long npix = (long long)W * H;
  hipLaunchKernelGGL(sbtm_clear_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, s, p, npix);
  return hipGetLastError();
}

hipError_t launch_sbtm_store(const SbtmPlanes& p, int W, int H, float4* out, int half, hipStream_t s) {
  const long long npix = (long long)W * H;
  hipLaunchKernelGGL(sbtm_store_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, s, p.eye, npix, out,
                     half);
  return hipGetLastError();
}

hipError_t launch_sbtm_slices(const Ctx& c, const SbtmArgs& q, const SbtmBatch& b, const SbtmPlanes& p,
                              hipStream_t s) {
  const int W = q.a.W, H = q.a.H;
  if (b.n < 1 || b.n > kSbtmMaxBatch || q.gx < 1 || q.gx > CVR_SBTM_MAX_GRID || q.gy < 1 ||
      q.gy > CVR_SBTM_MAX_GRID)
    return hipErrorInvalidValue;
  const uint4* cells = (const uint4*)c.d_cells;
  const float4* tf = (const float4*)c.d_tf;
  const bool fb8 = q.a.filter_bits == 8;
  if (b.n == 1) {
    const dim3 grid((W + 31) / 32, (H + 7) / 8);
    if (fb8) hipLaunchKernelGGL(sbtm_plain_kernel<8>, grid, dim3(256), 0, s, q, b.s[0], cells, tf, p);
    else hipLaunchKernelGGL(sbtm_plain_kernel<0>, grid, dim3(256), 0, s, q, b.s[0], cells, tf, p);
    return hipGetLastError();
  }
  // the region must hold the halo, and every slice's radius must be part of it
  int sx = 0, sy = 0;
  for (int j = 0; j < b.n; j++) {
    if (b.s[j].rx < 1 || b.s[j].ry < 1) return hipErrorInvalidValue;
    sx += b.s[j].rx;
    sy += b.s[j].ry;
  }
  if (sx != b.ex || sy != b.ey || b.ex > kSbtmHalo || b.ey > kSbtmHalo) return hipErrorInvalidValue;
  const dim3 grid((W + T - 1) / T, (H + T - 1) / T);
  if (fb8) hipLaunchKernelGGL(sbtm_blocked_kernel<8>, grid, dim3(NT), 0, s, q, b, cells, tf, p);
  else hipLaunchKernelGGL(sbtm_blocked_kernel<0>, grid, dim3(NT), 0, s, q, b, cells, tf, p);
  return hipGetLastError();
}

}  // namespace cvr
