// cvr_rc1pass.cpp — the single-pass ray-caster (rc1pass): the frame constants and
// per-context resources every renderer shares (cvr_host.h), the launch-order
// state of cvr_render_rc1pass, and its counters' read-back.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>

#include "cvr_host.h"

using namespace cvr;

namespace cvr {

// The per-tile sample counts and shade counters are shared by every render
// stream.  A frame that uses them on stream s first waits for the last frame
// that used them on another stream (frames in flight on rotated streams), and
// records the event after its own epilogue (counters_release).
cvr_status counters_acquire(Ctx* c, hipStream_t s) {
  if (!c->ev_counters) HIP_TRY(c, hipEventCreateWithFlags(&c->ev_counters, hipEventDisableTiming));
  if (c->counters_stream && c->counters_stream != s)
    HIP_TRY(c, hipStreamWaitEvent(s, c->ev_counters, 0));
  return CVR_OK;
}

cvr_status counters_release(Ctx* c, hipStream_t s) {
  HIP_TRY(c, hipEventRecord(c->ev_counters, s));
  c->counters_stream = s;
  return CVR_OK;
}

cvr_status ensure_scratch(Ctx* c, size_t bytes) {
  if (c->scratch_bytes >= bytes) return CVR_OK;
  free_dev(c->d_scratch);
  c->scratch_bytes = 0;
  HIP_TRY(c, hipMalloc(&c->d_scratch, bytes));
  c->scratch_bytes = bytes;
  return CVR_OK;
}

cvr_status bind_frame_output(Ctx* c, const cvr_output* o, size_t npix, FrameOut& fo) {
  fo.half = o->format == CVR_FORMAT_RGBA16F;
  fo.rgba_bytes = npix * (fo.half ? 8 : 16);
  fo.smp_bytes = npix * 4;
  if (o->on_device) {
    fo.d_out = (float4*)o->rgba;
    fo.d_samples = (uint32_t*)o->samples;
    fo.d_total = (unsigned long long*)o->total;
    return CVR_OK;
  }
  const cvr_status st = ensure_scratch(c, fo.rgba_bytes + (o->samples ? fo.smp_bytes : 0));
  if (st != CVR_OK) return st;
  fo.d_out = (float4*)c->d_scratch;
  fo.d_samples = o->samples ? (uint32_t*)((char*)c->d_scratch + fo.rgba_bytes) : nullptr;
  fo.d_total = o->total ? c->d_total : nullptr;
  return CVR_OK;
}

cvr_status frame_counters_begin(Ctx* c, const cvr_output* o, int ntiles, hipStream_t s, FrameOut& fo) {
  fo.counters = fo.d_total || c->shade_counters;
  if (fo.counters) {
    const cvr_status st = counters_acquire(c, s);
    if (st != CVR_OK) return st;
  }
  // device outputs: the kernel ADDS to *total (the caller zeroes it); host
  // outputs: the context's own counter is reset here.
  if (fo.d_total && !o->on_device) HIP_TRY(c, hipMemsetAsync(fo.d_total, 0, sizeof(unsigned long long), s));
  // Sample total: every wave tile stores its count, a sum epilogue adds them up
  // (one atomic per band; a per-wave atomic on one word serialises the frame).
  if (fo.d_total) {
    if (c->tile_samples_n < ntiles) {
      free_dev(c->d_tile_samples); c->tile_samples_n = 0;
      HIP_TRY(c, hipMalloc((void**)&c->d_tile_samples, (size_t)ntiles * 8));
      HIP_TRY(c, hipMemsetAsync(c->d_tile_samples, 0, (size_t)ntiles * 8, s));
      c->tile_samples_n = ntiles;
    }
    fo.tile_samples = c->d_tile_samples;
  }
  if (c->shade_counters) {   // measurement: shaded samples (gradient fetches), skipped samples
    if (!c->d_shade) HIP_TRY(c, hipMalloc((void**)&c->d_shade, 3 * sizeof(unsigned long long)));
    HIP_TRY(c, hipMemsetAsync(c->d_shade, 0, 3 * sizeof(unsigned long long), s));
    fo.shade = c->d_shade;
  }
  return CVR_OK;
}

cvr_status frame_output_finish(Ctx* c, const cvr_output* o, const FrameOut& fo, hipStream_t s) {
  if (fo.counters) {
    const cvr_status st = counters_release(c, s);
    if (st != CVR_OK) return st;
  }
  if (o->on_device) return CVR_OK;
  HIP_TRY(c, hipMemcpyAsync(o->rgba, fo.d_out, fo.rgba_bytes, hipMemcpyDeviceToHost, s));
  if (o->samples) HIP_TRY(c, hipMemcpyAsync(o->samples, fo.d_samples, fo.smp_bytes, hipMemcpyDeviceToHost, s));
  if (o->total) HIP_TRY(c, hipMemcpyAsync(o->total, fo.d_total, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  return CVR_OK;
}

// The macro cells were built for one volume and one macro size.
static void skip_drop_macro(Ctx::Skip& k) {
  free_dev(k.d_macro_minmax);
  free_dev(k.d_occ);
  k.mm_shift = -1;
  k.occ_valid = 0;
}

void skip_drop(Ctx* c, bool volume_gone, bool tf_gone) {
  Ctx::Skip& k = c->skip;
  k.occ_valid = 0;
  k.flags_valid = 0;
  k.flags_oom = 0;
  if (volume_gone) {
    skip_drop_macro(k);
    k.flags_set = 0;   // the cells are rebuilt without flags
  }
  if (tf_gone) free_dev(k.d_tf_prefix);
}

// Occupancy support for the TF just set (RGBA16F-rounded, n entries): prefix[k] =
// #{padded entries j < k with alpha > 0}, where padded entry j is
// T[clamp(j - 1, 0, n - 1)] (j = 0 .. n + 1).  The old TF's went with skip_drop.
cvr_status skip_set_tf(Ctx* c, const float* rgbt, int n) {
  std::vector<int> prefix((size_t)n + 3, 0);
  for (int j = 0; j < n + 2; j++) {
    const float a = rgbt[(size_t)std::min(std::max(j - 1, 0), n - 1) * 4 + 3];
    prefix[(size_t)j + 1] = prefix[(size_t)j] + (a > 0.0f || a != a ? 1 : 0);
  }
  HIP_TRY(c, hipMalloc((void**)&c->skip.d_tf_prefix, prefix.size() * sizeof(int)));
  HIP_TRY(c, hipMemcpy(c->skip.d_tf_prefix, prefix.data(), prefix.size() * sizeof(int),
                       hipMemcpyHostToDevice));
  return CVR_OK;
}

// Occupancy of the macro cells for the current volume, TF and macro size
// (rebuilt lazily after any of them changes; on the context stream).
cvr_status ensure_occupancy(Ctx* c) {
  Ctx::Skip& k = c->skip;
  if (k.occ_valid) return CVR_OK;
  if (!c->d_lut || !k.d_tf_prefix) return fail(c, CVR_ERR_STATE, "occupancy: no volume or TF");
  QUIESCE(c);   // frames in flight on other streams may still read d_occ
  const int sh = c->macro_shift;
  if (k.mm_shift != sh) {
    skip_drop_macro(k);
    for (int i = 0; i < 3; i++) k.mdim[i] = ((c->N[i] - 1) >> sh) + 1;
    const size_t nm = (size_t)k.mdim[0] * k.mdim[1] * k.mdim[2];
    HIP_TRY(c, hipMalloc((void**)&k.d_macro_minmax, nm * sizeof(uint32_t)));
    HIP_TRY(c, hipMalloc((void**)&k.d_occ, nm));
    HIP_TRY(c, cvr::launch_macro_minmax(*c, sh, k.mdim, k.d_macro_minmax, c->stream));
    k.mm_shift = sh;
  }
  const int nm = k.mdim[0] * k.mdim[1] * k.mdim[2];
  if (!c->d_total) HIP_TRY(c, hipMalloc((void**)&c->d_total, sizeof(unsigned long long)));
  unsigned int* d_n = reinterpret_cast<unsigned int*>(c->d_total);
  HIP_TRY(c, hipMemsetAsync(d_n, 0, sizeof(unsigned int), c->stream));
  HIP_TRY(c, cvr::launch_occupancy(k.d_macro_minmax, nm, c->d_lut, k.d_tf_prefix, c->tf_n,
                                   k.d_occ, d_n, c->stream));
  unsigned int n_empty = 0;
  HIP_TRY(c, hipMemcpyAsync(&n_empty, d_n, sizeof(n_empty), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  k.occ_empty = (float)n_empty / (float)nm;
  k.occ_valid = 1;
  return CVR_OK;
}

// Skip flags of the density cells for the current volume and TF (rebuilt lazily
// after either changes; on the context stream).  Frames in flight on other
// streams may still read the cells' old flags, so the device drains first (a
// TF change is rare); the two scratch bytes per cell are freed after the build.
cvr_status ensure_cell_flags(Ctx* c) {
  if (c->skip.flags_valid) return CVR_OK;
  if (!c->d_cells || !c->skip.d_tf_prefix) return fail(c, CVR_ERR_STATE, "cell flags: no volume or TF");
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipDeviceSynchronize());
  const size_t n = cvr::cell_count(c->cells);
  if (c->debug_flags_oom)   // tests: the scratch allocation fails
    return fail(c, CVR_ERR_OOM, "cell flags: scratch allocation failed (debug_cell_flags_oom)");
  uint8_t* t = nullptr;
  HIP_TRY(c, hipMalloc((void**)&t, 2 * n));
  hipError_t e = cvr::launch_cell_flags(*c, false, t, t + n, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  (void)hipFree(t);
  if (e != hipSuccess)
    return fail_hip(c, "cell flags", e);
  c->skip.flags_valid = 1;
  c->skip.flags_set = 1;
  return CVR_OK;
}

// The per-cell skip is a bit-exact optimisation, so a frame must not fail for
// want of its 2 bytes of scratch per cell (2.1 GB at 1024^3, next to the EBS
// SAT): on OOM the frame renders without it (every density read takes |corner|,
// so stale flags in the sign bits are ignored) until the next volume or TF
// change, which clears cell_flags_oom and retries the build.  The frame itself
// succeeds, so the OOM message is not left in cvr_last_error.  Any other error is
// returned.
cvr_status cell_flags_or_off(Ctx* c) {
  if (c->skip.flags_oom && !c->skip.flags_valid) return CVR_ERR_OOM;
  const cvr_status st = ensure_cell_flags(c);
  if (st == CVR_ERR_OOM) {
    (void)hipGetLastError();   // clear the failed allocation's error
    c->skip.flags_oom = 1;
    c->err.clear();
  }
  return st;
}

cvr_status enable_cell_skip(Ctx* c, Rc1passArgs& A, int level) {
  if (c->cell_skip <= 0) return CVR_OK;
  const cvr_status st = cell_flags_or_off(c);
  if (st == CVR_OK) {
    A.cell_skip = level;
    A.inv_step = 1.0f / A.step;
  }
  return st == CVR_ERR_OOM ? CVR_OK : st;
}

cvr_status check_frame_output(Ctx* c, const char* who, const cvr_frame* f, const cvr_output* o,
                              bool tiling) {
  if (!o->rgba) return fail(c, CVR_ERR_ARG, "%s: null argument", who);
  if (o->format != CVR_FORMAT_RGBA32F && o->format != CVR_FORMAT_RGBA16F)
    return fail(c, CVR_ERR_ARG, "%s: unknown output format %d", who, o->format);
  if (f->width < 1 || f->height < 1 || f->width > 32768 || f->height > 32768)
    return fail(c, CVR_ERR_ARG, "%s: bad viewport %dx%d", who, f->width, f->height);
  if (tiling && f->nranks > 1 &&
      (f->tile_size < 16 || f->tile_size % 16 != 0 || f->rank < 0 || f->rank >= f->nranks))
    return fail(c, CVR_ERR_ARG, "%s: bad tiling", who);
  return CVR_OK;
}

void set_phong_constants(Rc1passArgs& A, float ka, float kd, float ks, float shininess,
                         const float ispec[3], const float light[3]) {
  A.ka = ka;
  A.kd = kd;
  A.ks = ks;
  A.shininess = shininess;
  for (int i = 0; i < 3; i++) { A.ispec[i] = ispec[i]; A.light[i] = light[i]; }
}

// Camera, volume and tiling constants of one frame (shared by every renderer):
// ray generation (glm lookAt + tan(fovy/2)), VolumeGridSize, step, TF size, and
// the 8x8 wave tiles of the whole image or of this rank's packed tiles.
void fill_frame_args(Ctx* c, const cvr_frame* f, float step, cvr::Rc1passArgs& A,
                     int& ntiles, size_t& npix) {
  float V[16], tanh;
  cvr_camera_lookat(&f->camera, V, &tanh);
  if (f->use_view)
    for (int i = 0; i < 16; i++) V[i] = f->view[i];
  for (int i = 0; i < 3; i++) {
    A.eye[i] = f->camera.eye[i];
    A.col0[i] = V[0 * 4 + i];
    A.col1[i] = V[1 * 4 + i];
    A.col2[i] = V[2 * 4 + i];
  }
  A.tan_half_fovy = tanh;
  A.aspect = f->camera.aspect > 0 ? f->camera.aspect : (float)f->width / (float)f->height;
  A.W = f->width;
  A.H = f->height;
  for (int i = 0; i < 3; i++) {
    float G = (float)c->N[i] * c->scale[i];     // VolumeGridSize, rc1prenderer.cpp:241
    A.half_grid[i] = G * 0.5f;
    A.n_over_g[i] = (float)c->N[i] / G;
    A.nm1[i] = (float)(c->N[i] - 1);
    A.N[i] = c->N[i];
  }
  A.cells = c->cells;
  A.step = step > 0 ? step : cvr_default_step(c->scale);
  A.tf_n = c->tf_n;
  // Sample opacity: a TF lerp lies within [0, max alpha] up to an ulp, and h <= step.
  const double ext = (double)c->tf_max_alpha * (double)A.step * (1.0 + 1.0 / 1024.0);
  A.exp_fast = (ext >= 0.0 && ext <= 86.0) ? 1 : 0;
  A.exp_native = c->native_exp;
  if (f->nranks <= 1) {
    A.packed = 0;
    ntiles = ((f->width + 7) / 8) * ((f->height + 7) / 8);
    npix = (size_t)f->width * f->height;
  } else {
    A.packed = 1;
    A.tile = f->tile_size; A.rank = f->rank; A.nranks = f->nranks;
    A.ntx = (f->width + f->tile_size - 1) / f->tile_size;
    A.my_tiles = cvr_tiles_for_rank(f, f->rank);
    const int s8 = f->tile_size / 8;
    ntiles = A.my_tiles * s8 * s8;
    npix = (size_t)A.my_tiles * f->tile_size * f->tile_size;
  }
  A.ntiles = ntiles;
}

}  // namespace cvr

// The view a launch order was learned on: eye, unit forward direction (the
// centre pixel's ray, -(row 2 of mat3(View))), tan(fovy/2).
static void view_signature(const cvr::Rc1passArgs& A, float v[7]) {
  const float fx = -A.col0[2], fy = -A.col1[2], fz = -A.col2[2];
  const float n = std::sqrt(fx * fx + fy * fy + fz * fz);
  const float inv = n > 0.0f ? 1.0f / n : 0.0f;
  v[0] = A.eye[0]; v[1] = A.eye[1]; v[2] = A.eye[2];
  v[3] = fx * inv; v[4] = fy * inv; v[5] = fz * inv;
  v[6] = A.tan_half_fovy;
}

// Tile costs shift with the view: an order learned on a view more than `deg`
// degrees (direction, or an eye displacement of the matching chord of the eye's
// distance to the volume centre, or a zoom of that fraction) away is stale.
static bool view_close(const float a[7], const float b[7], int deg) {
  if (deg <= 0) return true;
  const double rad = deg * 3.14159265358979 / 180.0;
  const double c = (double)a[3] * b[3] + (double)a[4] * b[4] + (double)a[5] * b[5];
  if (c < std::cos(rad)) return false;
  const double dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
  const double r = std::sqrt((double)b[0] * b[0] + (double)b[1] * b[1] + (double)b[2] * b[2]);
  if (std::sqrt(dx * dx + dy * dy + dz * dz) > rad * std::max(r, 1e-6)) return false;
  return std::fabs((double)a[6] - b[6]) <= rad * std::fabs((double)b[6]);
}

// Every argument and state check of a launch of nf frames.
static cvr_status check_rc1pass_frames(Ctx* c, const cvr_frame* frames, int nf,
                                       const cvr_rc1pass_params* p, const cvr_output* outs) {
  const cvr_frame* f = frames;
  const cvr_output* o = outs;
  if (!f || !p || !o) return fail(c, CVR_ERR_ARG, "cvr_render_rc1pass: null argument");
  if (nf < 1 || nf > cvr::kMaxLaunchFrames)
    return fail(c, CVR_ERR_ARG, "cvr_render_rc1pass_frames: nframes %d not in 1..%d", nf,
                cvr::kMaxLaunchFrames);
  for (int i = 1; i < nf; i++) {
    const cvr_frame& g = frames[i];
    if (g.width != f->width || g.height != f->height || g.tile_size != f->tile_size ||
        g.rank != f->rank || g.nranks != f->nranks)
      return fail(c, CVR_ERR_ARG, "cvr_render_rc1pass_frames: frame %d differs from frame 0 in "
                                  "viewport or screen split", i);
    if (!outs[i].rgba || !outs[i].on_device || outs[i].format != o->format || outs[i].total)
      return fail(c, CVR_ERR_ARG, "cvr_render_rc1pass_frames: output %d must be a device buffer of "
                                  "frame 0's format, without a total", i);
  }
  if (nf > 1 && !o->on_device)
    return fail(c, CVR_ERR_ARG, "cvr_render_rc1pass_frames: the outputs must be device buffers");
  // (the tiling check, with its own message, follows the state checks)
  {
    const cvr_status st = check_frame_output(c, "cvr_render_rc1pass", f, o, false);
    if (st != CVR_OK) return st;
  }
  if (!c->d_cells) return fail(c, CVR_ERR_STATE, "cvr_render_rc1pass: no volume set");
  if (!c->d_tf) return fail(c, CVR_ERR_STATE, "cvr_render_rc1pass: no transfer function set");
  if (p->apply_gradient_shading != 0 && !c->d_grad)
    return fail(c, CVR_ERR_STATE, "cvr_render_rc1pass: gradient shading needs cvr_set_gradient");
  if (f->nranks > 1 && (f->tile_size < 16 || f->tile_size % 16 != 0 || f->rank < 0 || f->rank >= f->nranks))
    return fail(c, CVR_ERR_ARG, "cvr_render_rc1pass: bad tiling (tile %d, rank %d/%d)",
                f->tile_size, f->rank, f->nranks);
  return CVR_OK;
}

// Frame 0's kernel arguments but for the outputs and the launch order: the frame
// constants, the shading, and the empty-space skip (per-cell flags, else the
// macro cells' occupancy), which the state may have to build first.
static cvr_status fill_rc1pass_args(Ctx* c, const cvr_frame* f, const cvr_rc1pass_params* p,
                                    cvr::Rc1passArgs& A, int& ntiles, size_t& npix) {
  fill_frame_args(c, f, p->step, A, ntiles, npix);
  set_phong_constants(A, p->ka, p->kd, p->ks, p->shininess, p->ispecular, p->light_pos);
  A.filter_bits = c->filter_bits;
  A.cost_time = c->cost_time;
  {   // (the quad march ignores it)
    const cvr_status st = enable_cell_skip(c, A, c->cell_skip);
    if (st != CVR_OK) return st;
  }
  if (c->macro_shift > 0 && A.cell_skip == 0) {
    cvr_status st = ensure_occupancy(c);
    if (st != CVR_OK) return st;
    // the skip path costs the march registers and a probe: worth it only
    // with enough empty space (the Marschner-Lobb headline field has ~4 %)
    if (c->skip.occ_empty * 100.0f >= (float)c->skip_min_pct) {
      A.occ = c->skip.d_occ;
      for (int i = 0; i < 3; i++) A.mdim[i] = c->skip.mdim[i];
      A.mshift = c->macro_shift;
    }
  }
  if (c->tile_stats) {
    if (c->tile_stats_n < ntiles) {
      free_dev(c->d_tile_stats); c->tile_stats_n = 0;
      HIP_TRY(c, hipMalloc((void**)&c->d_tile_stats, (size_t)ntiles * 32));
      c->tile_stats_n = ntiles;
    }
    A.tile_stats = c->d_tile_stats;
  }
  return CVR_OK;
}

// How the frame's ntiles wave tiles are cut into work (options only).
static cvr::RenderPlan make_render_plan(const Ctx* c, int ntiles) {
  cvr::RenderPlan plan{};
  plan.ntiles = ntiles;
  plan.quad_pct = c->filter_bits ? 0 : c->quad_pct;   // the quad march has no filter_bits variant
  // Bands are cut by predicted work, so one may hold more than 1/8 of the
  // tiles: up to band_cap % of the even share (default 130;
  // tile_epilogue_kernel moves the band boundaries the least that fits the
  // cap); every band gets that many slots (+3 per quad-split tile), and the
  // slots past a band's entries are empty workgroups.
  const int seg_avg = (ntiles + 7) / 8;
  const int cap = (int)(((long long)seg_avg * c->band_cap_pct + 99) / 100);
  plan.max_seg = std::min(std::min(ntiles, cap), cvr::kMaxBandTiles);
  if (plan.max_seg < seg_avg) plan.max_seg = seg_avg;   // (too large to order; see render_rc1pass_frames)
  int per_band = plan.max_seg + 3 * (int)(((long long)plan.max_seg * plan.quad_pct) / 100);
  per_band = (per_band + 3) & ~3;   // whole groups of 4 waves per workgroup (raymarch.hip)
  plan.order_slots = 8 * per_band;
  plan.boost = (int)(((long long)seg_avg * c->boost_pct) / 100);
  plan.keep = c->debug_keep;
  plan.epi_stop = c->epi_stop;
  return plan;
}

// The views and outputs of a launch's frames (frames 1.. differ from frame 0,
// whose arguments are A, in nothing else).  Returns whether every frame is near
// frame 0's view vsig: one launch order serves them all.
static bool fill_launch_views(Ctx* c, const cvr_frame* frames, int nf, const cvr_rc1pass_params* p,
                              const cvr_output* outs, const cvr::Rc1passArgs& A, const float vsig[7],
                              cvr::LaunchFrames& lf) {
  lf.n = nf;
  lf.grid = 0;
  bool views_close = true;
  for (int i = 0; i < nf; i++) {
    cvr::Rc1passArgs Ai = A;
    if (i > 0) {
      int nti;
      size_t npi;
      fill_frame_args(c, &frames[i], p->step, Ai, nti, npi);
      float vi[7];
      view_signature(Ai, vi);
      if (!view_close(vi, vsig, c->stale_deg)) views_close = false;
    }
    cvr::FrameView& v = lf.view[i];
    for (int k = 0; k < 3; k++) {
      v.eye[k] = Ai.eye[k];
      v.col0[k] = Ai.col0[k];
      v.col1[k] = Ai.col1[k];
      v.col2[k] = Ai.col2[k];
    }
    v.tan_half_fovy = Ai.tan_half_fovy;
    v.aspect = Ai.aspect;
    lf.out[i] = (float4*)outs[i].rgba;
    lf.samples[i] = (uint32_t*)outs[i].samples;
  }
  return views_close;
}

// The launch order (Ctx::OrderSlot).  Longest-first (LPT) order learned on an
// earlier frame of the same plan: the kernel records each wave tile's critical
// path into the slot's costs, and the slot's order is rebuilt from them
// (tile_epilogue_kernel: work-balanced XCD bands + bucket LPT).
//
// One slot per render stream: frames issued on different streams may overlap
// on the device (the screen-tile split alternates two), and a slot's order,
// costs and rebuilds stay in its stream's order.  async_order: slots rotate.
static cvr_status order_slot_for_stream(Ctx* c, hipStream_t s, Ctx::OrderSlot*& os) {
  int si = -1;
  if (c->async_order) {
    si = (int)(c->frame_no % 3);
  } else {
    for (int i = 0; i < Ctx::kOrderSlots; i++)
      if (c->oslot[i].owned && c->oslot[i].stream == s) si = i;
    if (si < 0) {
      si = c->slot_rr++ % Ctx::kOrderSlots;
      Ctx::OrderSlot& o = c->oslot[si];
      if (o.owned) HIP_TRY(c, hipDeviceSynchronize());   // the slot's last frame is done
      o.stream = s;
      o.owned = true;
      o.valid = 0;
      o.frames = 0;
    }
  }
  os = &c->oslot[si];
  return CVR_OK;
}

// The slot's order and cost buffers for this plan; under async_order also the
// side stream and its events, and the wait for the slot's sort in flight.
static cvr_status order_slot_reserve(Ctx* c, Ctx::OrderSlot& os, const cvr::RenderPlan& plan, hipStream_t s) {
  if (c->async_order && !c->side) {   // side stream + events only for side-stream sorts
    int lo = 0, hi = 0;
    HIP_TRY(c, hipDeviceGetStreamPriorityRange(&lo, &hi));
    HIP_TRY(c, hipStreamCreateWithPriority(&c->side, hipStreamNonBlocking, hi));
    HIP_TRY(c, hipEventCreateWithFlags(&c->ev_frame, hipEventDisableTiming));
    for (auto& o : c->oslot) HIP_TRY(c, hipEventCreateWithFlags(&o.done, hipEventDisableTiming));
  }
  // the slot's previous sort must be done before this frame reads its order
  // and overwrites its costs (it ran alongside the previous frame)
  if (os.pending) HIP_TRY(c, hipStreamWaitEvent(s, os.done, 0));
  if (os.units >= plan.order_slots && os.ntiles >= plan.ntiles) return CVR_OK;
  if (c->side) HIP_TRY(c, hipStreamSynchronize(c->side));
  free_dev(os.d_order);
  free_dev(os.d_cost);
  os.units = os.ntiles = 0;
  os.valid = 0;
  HIP_TRY(c, hipMalloc((void**)&os.d_order, (size_t)plan.order_slots * sizeof(int)));
  HIP_TRY(c, hipMalloc((void**)&os.d_cost, (size_t)plan.ntiles * sizeof(uint32_t) + 64));
  HIP_TRY(c, hipMemsetAsync(os.d_cost, 0, (size_t)plan.ntiles * sizeof(uint32_t) + 64, s));
  os.units = plan.order_slots;
  os.ntiles = plan.ntiles;
  return CVR_OK;
}

// The order this frame launches under, or null: the slot's, if it was built for
// this plan (key) on a view near this one.
static const int* order_for_frame(const Ctx* c, const Ctx::OrderSlot& os, int key, const float vsig[7],
                                  bool views_close) {
  if (!os.valid || os.key != key) return nullptr;
  // an order learned on a distant view costs more than none (interleaved
  // screen order): measured +18 % mean over the 24 reference views
  if (os.has_view && !view_close(vsig, os.view, c->stale_deg)) return nullptr;
  return views_close ? os.d_order : nullptr;   // frames far apart in one launch: no shared order
}

// The slot's order is (being) built from this frame's costs.
static void order_commit(Ctx::OrderSlot& os, int key, const float vsig[7]) {
  os.valid = 1;
  os.key = key;
  std::memcpy(os.view, vsig, sizeof(os.view));
  os.has_view = true;
}

// Whether this frame's epilogue rebuilds the order; counts the frame on the slot.
// The order is rebuilt every order_interval-th frame (and whenever it is
// missing or stale for this plan): costs shift slowly between frames, and
// the rebuild (~15 us on the frame's stream) would otherwise cost ~10 %.
// ... and only while the camera holds still (or moves little) from frame to
// frame: when every frame jumps to a distant view, a new order would never be
// used and its rebuild (~15 us on the frame's stream) is skipped
static bool order_rebuild_due(const Ctx* c, Ctx::OrderSlot& os, const float vsig[7], bool views_close,
                              bool have_order) {
  const bool steady = views_close && (!os.has_last || view_close(vsig, os.last_view, c->stale_deg));
  std::memcpy(os.last_view, vsig, sizeof(os.last_view));
  os.has_last = true;
  const bool due = !have_order || os.frames % std::max(1, c->order_interval) == 0;
  os.frames++;
  return !c->async_order && steady && due;
}

// After the march: the sample total's sum and the order for a later frame, in
// one epilogue on the frame's stream, or (async_order) the order on the side stream.
static cvr_status launch_rc1pass_epilogue(Ctx* c, Ctx::OrderSlot& os, const cvr::RenderPlan& plan, int key,
                                          const float vsig[7], bool rebuild, uint32_t* tile_cost,
                                          const FrameOut& fo, hipStream_t s) {
  if (rebuild) {
    HIP_TRY(c, cvr::launch_tile_epilogue(tile_cost, fo.tile_samples, fo.d_total, plan, os.d_order, s));
    os.pending = false;
    order_commit(os, key, vsig);
  } else if (fo.tile_samples) {
    HIP_TRY(c, cvr::launch_tile_epilogue(nullptr, fo.tile_samples, fo.d_total, plan, nullptr, s));
  }
  if (tile_cost && c->async_order) {
    HIP_TRY(c, hipEventRecord(c->ev_frame, s));
    HIP_TRY(c, hipStreamWaitEvent(c->side, c->ev_frame, 0));
    HIP_TRY(c, cvr::launch_tile_epilogue(tile_cost, nullptr, nullptr, plan, os.d_order, c->side));
    HIP_TRY(c, hipEventRecord(os.done, c->side));
    os.pending = true;
    order_commit(os, key, vsig);
  }
  return CVR_OK;
}

// nf frames (1..kMaxLaunchFrames) in one ray-march launch; nf = 1 is cvr_render_rc1pass.
static cvr_status render_rc1pass_frames(Ctx* c, const cvr_frame* frames, int nf,
                                        const cvr_rc1pass_params* p, const cvr_output* outs) {
  cvr_status st = check_rc1pass_frames(c, frames, nf, p, outs);
  if (st != CVR_OK) return st;
  const cvr_frame* f = frames;
  const cvr_output* o = outs;
  cvr::Rc1passArgs A{};
  int ntiles;
  size_t npix;
  st = fill_rc1pass_args(c, f, p, A, ntiles, npix);
  if (st != CVR_OK) return st;
  cvr::RenderPlan plan = make_render_plan(c, ntiles);

  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  FrameOut fo;
  st = bind_frame_output(c, o, npix, fo);
  if (st == CVR_OK) st = frame_counters_begin(c, o, ntiles, s, fo);
  if (st != CVR_OK) return st;
  A.out_half = fo.half;
  A.shade_ctr = fo.shade;

  float vsig[7];
  view_signature(A, vsig);
  cvr::LaunchFrames lf;
  const bool views_close = fill_launch_views(c, frames, nf, p, outs, A, vsig, lf);
  if (nf > 1) plan.frames = &lf;
  const int key = (ntiles << 2) ^ (plan.quad_pct << 24) ^
                  (f->nranks > 1 ? (f->rank << 8) ^ (f->nranks << 12) ^ 1 : 0);
  Ctx::OrderSlot* os;
  st = order_slot_for_stream(c, s, os);
  if (st != CVR_OK) return st;
  const int* order = nullptr;
  uint32_t* tile_cost = nullptr;
  if (c->use_order == 1 && (ntiles + 7) / 8 <= cvr::kMaxBandTiles) {   // else too large to order
    st = order_slot_reserve(c, *os, plan, s);
    if (st != CVR_OK) return st;
    order = order_for_frame(c, *os, key, vsig, views_close);
    tile_cost = os->d_cost;
  }
  // without an order, tiles go to the XCDs interleaved (tile t on XCD t mod 8):
  // it balances any view, where contiguous bands need the learned costs
  A.interleave = c->use_order == 2 || (!order && c->use_order == 1);

  const bool phong = p->apply_gradient_shading != 0;
  st = timed_launch(c, s, [&] {
    return cvr::launch_rc1pass(*c, A, phong, fo.d_out, fo.d_samples, fo.tile_samples, order, tile_cost, plan, s,
                               c->rc1pass_variant);
  });
  if (st != CVR_OK) return st;
  const bool rebuild = order_rebuild_due(c, *os, vsig, views_close, order != nullptr) && tile_cost;
  st = launch_rc1pass_epilogue(c, *os, plan, key, vsig, rebuild, tile_cost, fo, s);
  if (st != CVR_OK) return st;
  c->frame_no++;
  return frame_output_finish(c, o, fo, s);
}

extern "C" {
#pragma GCC visibility push(default)

int cvr_tiles_for_rank(const cvr_frame* f, int rank) {
  if (!f || f->width < 1 || f->height < 1) return 0;
  if (f->nranks <= 1) return 1;
  if (f->tile_size < 16 || f->tile_size % 16 != 0 || rank < 0 || rank >= f->nranks) return 0;
  int ntx = (f->width + f->tile_size - 1) / f->tile_size;
  int nty = (f->height + f->tile_size - 1) / f->tile_size;
  int nt = ntx * nty;
  return nt > rank ? (nt - rank + f->nranks - 1) / f->nranks : 0;
}

cvr_status cvr_render_rc1pass(cvr_ctx* ctx, const cvr_frame* f, const cvr_rc1pass_params* p,
                              const cvr_output* o) {
  Ctx* c = reinterpret_cast<Ctx*>(ctx);
  if (c && c->group)
    return cvr::group_render(c, f, 1, o, [&](cvr_ctx* _m, const cvr_frame* mf, int, const cvr_output* mo) {
      return cvr_render_rc1pass(_m, mf, p, mo);
    });
  if (!c) return CVR_ERR_ARG;
  return render_rc1pass_frames(c, f, 1, p, o);
}

cvr_status cvr_render_rc1pass_frames(cvr_ctx* ctx, const cvr_frame* frames, int nframes,
                                     const cvr_rc1pass_params* p, const cvr_output* outs) {
  Ctx* c = reinterpret_cast<Ctx*>(ctx);
  if (c && c->group)
    return cvr::group_render(c, frames, nframes, outs, [&](cvr_ctx* _m, const cvr_frame* mf, int nf, const cvr_output* mo) {
      return cvr_render_rc1pass_frames(_m, mf, nf, p, mo);
    });
  if (!c) return CVR_ERR_ARG;
  return render_rc1pass_frames(c, frames, nframes, p, outs);
}

cvr_status cvr_copy_tile_stats(cvr_ctx* ctx, uint64_t* out, int max_tiles, int* out_tiles) {
  Ctx* c = reinterpret_cast<Ctx*>(ctx);
  if (c && c->group) return cvr::group_call_root(c, [&](cvr_ctx* _m) { return cvr_copy_tile_stats(_m, out, max_tiles, out_tiles); });
  if (!c || !out_tiles) return CVR_ERR_ARG;
  *out_tiles = c->tile_stats_n;
  if (!out) return CVR_OK;
  if (!c->d_tile_stats) return fail(c, CVR_ERR_STATE, "tile_stats option was not enabled");
  int n = max_tiles < c->tile_stats_n ? max_tiles : c->tile_stats_n;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipMemcpy(out, c->d_tile_stats, (size_t)n * 32, hipMemcpyDeviceToHost));
  return CVR_OK;
}

cvr_status cvr_read_shade_counters(cvr_ctx* ctx, uint64_t out[3]) {
  Ctx* c = reinterpret_cast<Ctx*>(ctx);
  if (!c || !out) return CVR_ERR_ARG;
  if (c->group) {
    uint64_t sum[3] = {0, 0, 0};
    cvr_status st = cvr::group_each(c, [&](cvr_ctx* _m) {
      uint64_t v[3];
      cvr_status e = cvr_read_shade_counters(_m, v);
      for (int i = 0; i < 3; i++) sum[i] += v[i];
      return e;
    });
    for (int i = 0; i < 3; i++) out[i] = sum[i];
    return st;
  }
  if (!c->d_shade) return fail(c, CVR_ERR_STATE, "shade_counters option was not enabled");
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipMemcpy(out, c->d_shade, 3 * sizeof(uint64_t), hipMemcpyDeviceToHost));
  return CVR_OK;
}

cvr_status cvr_read_kernel_times(cvr_ctx* ctx, float* ms, int max_frames, int* out_frames) {
  Ctx* c = reinterpret_cast<Ctx*>(ctx);
  if (c && c->group) return cvr::group_call_root(c, [&](cvr_ctx* _m) { return cvr_read_kernel_times(_m, ms, max_frames, out_frames); });
  if (!c || !out_frames || max_frames < 0 || (max_frames > 0 && !ms)) return CVR_ERR_ARG;
  const long long nev = (long long)c->ev_start.size();
  if (!nev) return fail(c, CVR_ERR_STATE, "kernel_timing option was not enabled");
  const long long have = c->timed_frames < nev ? c->timed_frames : nev;
  const int n = (int)(have < max_frames ? have : max_frames);
  HIP_TRY(c, hipSetDevice(c->device));
  // the most recent n frames, oldest first
  for (int i = 0; i < n; i++) {
    const size_t slot = (size_t)((c->timed_frames - n + i) % nev);
    HIP_TRY(c, hipEventSynchronize(c->ev_stop[slot]));
    HIP_TRY(c, hipEventElapsedTime(&ms[i], c->ev_start[slot], c->ev_stop[slot]));
  }
  *out_frames = n;
  c->timed_frames = 0;
  return CVR_OK;
}

#pragma GCC visibility pop
}  // extern "C"
