// cvr_host.h — what the C-ABI translation units (cvr_api.cpp, cvr_options.cpp,
// cvr_rc1pass.cpp, cvr_dos.cpp, cvr_ebs.cpp, cvr_lightcache.cpp, cvr_crtgt.cpp,
// cvr_vct.cpp, cvr_sbtm.cpp, cvr_deferred.cpp, cvr_advdeferred.cpp, cvr_iso.cpp) share:
// error reporting (fail, and fail_hip with the one mapping of a HIP error to a status,
// which cvr_comm.cpp and cvr_group.cpp take from here too), device-memory helpers, the
// half and vector helpers of the host arithmetic, the frame set-up and the frame-output
// path common to the renderers, and what the two deferred renderers share on the host.
// Host only: never included by a .hip file or a kernel header.
//
// Compiled with -ffp-contract=off: the arithmetic below feeds the kernels and
// must be bit-reproducible (CVR-SPEC).
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "cvr_internal.h"

namespace cvr {

// Stores the message in the context (cvr_last_error) and returns st.
cvr_status fail(Ctx* c, cvr_status st, const char* fmt, ...);

// A failed HIP call as a status and a message, "<who>: <HIP's text>" and, with `file`,
// " (<file>:<line>)": out of memory is CVR_ERR_OOM, everything else CVR_ERR_HIP.
inline cvr_status fail_hip(Ctx* c, const char* who, hipError_t e, const char* file = nullptr, int line = 0) {
  const cvr_status st = e == hipErrorOutOfMemory ? CVR_ERR_OOM : CVR_ERR_HIP;
  if (!file) return fail(c, st, "%s: %s", who, hipGetErrorString(e));
  return fail(c, st, "%s: %s (%s:%d)", who, hipGetErrorString(e), file, line);
}

#define HIP_TRY(ctx, expr)                                                     \
  do {                                                                         \
    hipError_t _e = (expr);                                                    \
    if (_e != hipSuccess) return ::cvr::fail_hip(ctx, #expr, _e, __FILE__, __LINE__); \
  } while (0)

// Before a state change writes or frees device state that frames read (volume
// cells, TF, gradient, occupancy, cone tables, extinction pyramid, SAT): frames
// may be in flight on any render stream the caller rotates (non-blocking
// streams do not wait for the null-stream copies below), so the whole device
// drains first.  The reference's equivalent is the GL pipeline's implicit
// ordering on Init after a TF change (renderingmanager.cpp:1050-1127).
#define QUIESCE(c)                             \
  do {                                         \
    HIP_TRY(c, hipSetDevice((c)->device));     \
    HIP_TRY(c, hipDeviceSynchronize());        \
  } while (0)

// The multi-device split of this path is not built: a group context refuses it.
#define NO_GROUP(c, who)                                                                       \
  do {                                                                                         \
    if ((c)->group)                                                                            \
      return ::cvr::fail(c, CVR_ERR_STATE,                                                     \
                         who ": not available on a group context (cvr_create_group)");         \
  } while (0)

template <class T>
void free_dev(T*& p) {
  if (p) (void)hipFree(p);
  p = nullptr;
}

// float -> binary16 bits, round to nearest even (the GL driver's conversion of
// GL_FLOAT client data to a 16F internal format).
inline uint16_t to_half_bits(float f) {
  _Float16 h = (_Float16)f;
  uint16_t b;
  std::memcpy(&b, &h, 2);
  return b;
}
inline float half_round(float f) {
  _Float16 h = (_Float16)f;
  return (float)h;
}
inline float half_to_float_host(uint16_t b) {
  _Float16 h;
  std::memcpy(&h, &b, 2);
  return (float)h;
}

struct V3 { float x, y, z; };
inline V3 sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
inline V3 cross(V3 x, V3 y) {
  return {x.y * y.z - y.y * x.z, x.z * y.x - y.z * x.x, x.x * y.y - y.x * x.y};
}
inline float gdot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
inline V3 gnormalize(V3 v) {
  float inv = 1.0f / std::sqrt(v.x * v.x + v.y * v.y + v.z * v.z);
  return {v.x * inv, v.y * inv, v.z * inv};
}

// cvr_rc1pass.cpp: per-context resources and the frame constants every renderer uses
cvr_status ensure_scratch(Ctx* c, size_t bytes);
cvr_status counters_acquire(Ctx* c, hipStream_t s);
cvr_status counters_release(Ctx* c, hipStream_t s);
cvr_status ensure_occupancy(Ctx* c);
cvr_status ensure_cell_flags(Ctx* c);
cvr_status cell_flags_or_off(Ctx* c);
void fill_frame_args(Ctx* c, const cvr_frame* f, float step, Rc1passArgs& A, int& ntiles,
                     size_t& npix);

// The checks of a frame and its output that every renderer makes, in this
// order: the output buffer, its format, the viewport, and (tiling) the screen
// split's tile size and rank.
cvr_status check_frame_output(Ctx* c, const char* who, const cvr_frame* f, const cvr_output* o,
                              bool tiling = true);

// The Blinn-Phong constants of the surface term (ray_marching_1p.comp:48-81).
void set_phong_constants(Rc1passArgs& A, float ka, float kd, float ks, float shininess,
                         const float ispec[3], const float light[3]);

// VolumeGridSize (= VolumeScaledSizes) of the context's volume (rc1prenderer.cpp:241).
inline void grid_size(const Ctx* c, float G[3]) {
  for (int i = 0; i < 3; i++) G[i] = (float)c->N[i] * c->scale[i];
}

// ShadeSample's weights in a shaded renderer's kernel arguments: Kambient only with
// occlusion, Kdiffuse / Kspecular only with shadows, else 0.
template <class Args>
void set_gated_weights(Args& Q, bool occlusion, bool shadow, float ka, float kd, float ks) {
  Q.ka = occlusion ? ka : 0.0f;
  Q.kd = shadow ? kd : 0.0f;
  Q.ks = shadow ? ks : 0.0f;
}

// cvr_api.cpp: light 0 of the reference's light list, the default light of the
// renderers that take a cvr_light
void default_light(cvr_light* l);

// With option "cell_skip" on: the march uses the cells' skip flags at `level`
// (built here when stale).  Without memory for the build the frame renders
// without them (cell_flags_or_off); any other error is returned.
cvr_status enable_cell_skip(Ctx* c, Rc1passArgs& A, int level);

// The drop functions of the context's derived state, one per struct of Ctx: each
// frees the struct's device memory and resets its bookkeeping, after the caller
// has drained the device (QUIESCE).  Who calls which: cvr_api.cpp derived_drop.
// cvr_rc1pass.cpp: without the volume the macro cells go and the cells carry no
// flags; without the TF its prefix counts go (skip_set_tf uploads the new TF's)
void skip_drop(Ctx* c, bool volume_gone, bool tf_gone);
cvr_status skip_set_tf(Ctx* c, const float* rgbt, int n);
void ext_drop(Ctx* c);   // cvr_dos.cpp: the pyramid, its level table, the cone tables
// cvr_ebs.cpp: the SAT, or only the parts of it that can go while it stays
enum SatPart { kSatScratch = 1, kSatCells = 2, kSatAll = 7 };
void sat_drop(Ctx* c, int parts = kSatAll);
// cvr_lightcache.cpp: a new volume, TF, extinction pyramid or SAT drops the cache;
// the context's end also destroys its event
void light_cache_drop(Ctx* c, bool destroy = false);
void iso_drop(Ctx* c);   // cvr_iso.cpp: the block table
// cvr_iso.cpp: the block min/max table of the context's volume for nb blocks per axis
// (ComputeBlocksFromVolume; the iso renderers' and DeferredShading's are one function),
// built when the volume or nb changed; blocks
cvr_status ensure_iso_blocks(Ctx* c, const int nb[3]);
// cvr_deferred.cpp: the G-buffer goes with the volume (and with another viewport);
// the context's end also frees its hit counter
void deferred_drop(Ctx* c, bool destroy = false);
// cvr_deferred.cpp, for the renderers over its G-buffer (cvr_advdeferred.cpp).
// cvr_advdeferred_params begins with the fields of cvr_deferred_params (include/cvr.h;
// deferred_prefix, checked at compile time), so what the two renderers have in common
// takes a cvr_deferred_params: the start of an entry (a context that is no group, no
// null argument), the common defaults (everything but ka .. shininess and
// gbuffer_clear), the lighting checks (`nan_what` names the parameters in the NaN
// message, `more_nan`: one of the caller's own is NaN), the checks of a call that
// marches `f`, the geometry pass into the context's G-buffer on the context stream,
// the check of an output's buffer and format, and the check of a call over the kept
// G-buffer (`kept`: it is there, else CVR_ERR_STATE with `missing`; another size than
// width x height is `mismatch`)
bool any_nan(const float* v, int n);
cvr_status deferred_entry(Ctx* c, const char* who, bool args_given);
void deferred_common_defaults(cvr_deferred_params* p);
cvr_status deferred_check_lighting(Ctx* c, const char* who, const cvr_deferred_params* p,
                                   const char* nan_what = "lighting or tone-map", bool more_nan = false);
cvr_status deferred_check_geometry_call(Ctx* c, const char* who, const cvr_frame* f, const cvr_deferred_params* p);
cvr_status deferred_geometry_pass(Ctx* c, const char* who, const cvr_frame* f, const cvr_deferred_params* p);
cvr_status deferred_check_output(Ctx* c, const char* who, const cvr_output* o);
cvr_status deferred_check_kept(Ctx* c, const char* who, bool kept, const char* missing, int width, int height,
                               cvr_status mismatch = CVR_ERR_ARG);
// cvr_advdeferred.cpp: the curvature planes go with the G-buffer (deferred_drop calls
// this); the context's end also frees the lighting pass's tables and its counter
void advdeferred_drop(Ctx* c, bool destroy = false);

// cvr_crtgt.cpp: a new volume, TF or gradient ends the ground-truth frame in
// progress; the context's end frees its state
void crtgt_invalidate(Ctx* c);
void crtgt_release(Ctx* c);

// cvr_vct.cpp: a new volume drops the pyramid and the table, a new TF the table
// and the opacities; the context's end frees everything
void vct_drop(Ctx* c, bool pyramid);

// cvr_sbtm.cpp: the eye buffer and the occlusion planes hold nothing between frames;
// a new volume or TF and the context's end free them
void sbtm_drop(Ctx* c);

// cvr_dos.cpp, cvr_ebs.cpp: a frame's kernel arguments (also for the light cache)
void resolve_cone_params(const Ctx* c, const cvr_dos_params* p, cvr_cone_params cp[2]);
cvr_status dos_prepare(Ctx* c, const char* who, const cvr_frame* f, const cvr_dos_params* p,
                       const cvr_output* o, bool need_cones, DosArgs& Q, int& ntiles, size_t& npix,
                       cvr_cone_params cp[2]);
float ebs_max_distance(const Ctx* c, const cvr_ebs_params* p);
cvr_status ebs_prepare(Ctx* c, const char* who, const cvr_frame* f, const cvr_ebs_params* p,
                       const cvr_output* o, EbsArgs& Q, int& ntiles, size_t& npix);

// One frame's output path, shared by every renderer: where the frame's kernels
// write (the caller's device buffers, or the context's scratch for a host
// output), the shared counters, the timing ring, and the read-back.  A frame
// calls, in this order on its stream s: bind_frame_output, frame_counters_begin,
// timed_launch, its own epilogue (launch_tile_epilogue when tile_samples is
// set), frame_output_finish.  Defined in cvr_rc1pass.cpp.
struct FrameOut {
  float4* d_out = nullptr;
  uint32_t* d_samples = nullptr;               // null: no per-pixel counts asked for
  unsigned long long* d_total = nullptr;       // null: no sample total asked for
  unsigned long long* tile_samples = nullptr;  // per-tile counts the sum epilogue adds into d_total
  unsigned long long* shade = nullptr;         // option "shade_counters": the [3] counters, cleared
  size_t rgba_bytes = 0, smp_bytes = 0;
  int half = 0;                                // RGBA16F output
  bool counters = false;                       // counters_acquire was called: release them
};

// Device outputs are bound as given; a host output renders into the context's
// scratch (grown here), its total into the context's own counter.
cvr_status bind_frame_output(Ctx* c, const cvr_output* o, size_t npix, FrameOut& fo);
// With a total or shade counters in use: waits for the counters' last user on
// another stream, clears a host output's total (a device total is the caller's:
// the kernels add to it), and reserves tile_samples and the cleared shade counters.
cvr_status frame_counters_begin(Ctx* c, const cvr_output* o, int ntiles, hipStream_t s, FrameOut& fo);
// After the frame's epilogue: releases the counters; a host output is then
// copied back and the stream drained.
cvr_status frame_output_finish(Ctx* c, const cvr_output* o, const FrameOut& fo, hipStream_t s);

// launch() between the events of option "kernel_timing" (cvr_read_kernel_times).
template <class Launch>
cvr_status timed_launch(Ctx* c, hipStream_t s, const Launch& launch) {
  const size_t nev = c->ev_start.size();
  const size_t slot = nev ? (size_t)(c->timed_frames % (long long)nev) : 0;
  if (nev) HIP_TRY(c, hipEventRecord(c->ev_start[slot], s));
  HIP_TRY(c, launch());
  if (nev) {
    HIP_TRY(c, hipEventRecord(c->ev_stop[slot], s));
    c->timed_frames++;
  }
  return CVR_OK;
}

// The lighting fields DeferredShadeArgs and AdvShadeArgs share, from the kept G-buffer
// and the parameters' common part.
template <class Args>
void fill_shade_lighting(Args& S, const Ctx::Deferred& D, const cvr_deferred_params* p) {
  S.W = D.W;
  S.H = D.H;
  for (int i = 0; i < 3; i++) {
    S.eye[i] = D.eye[i];
    S.light[i] = p->light_pos[i];
    S.light_color[i] = p->light_color[i];
  }
  S.ka = p->ka;
  S.kd = p->kd;
  S.ks = p->ks;
  S.shininess = p->shininess;
  S.exposure = p->exposure;
  S.gamma = p->gamma;
}

// A lighting pass over the kept G-buffer as a frame of that path (one "tile": the
// kernel adds its counts to the total itself): before(s) on the stream once the
// counters are ready, then launch(fo, s) between the timing events.
template <class Before, class Launch>
cvr_status shade_frame(Ctx* c, const cvr_output* o, const Before& before, const Launch& launch) {
  const size_t npix = (size_t)c->deferred.W * c->deferred.H;
  hipStream_t s = c->stream;
  FrameOut fo;
  cvr_status st = bind_frame_output(c, o, npix, fo);
  if (st == CVR_OK) st = frame_counters_begin(c, o, 1, s, fo);
  if (st == CVR_OK) st = before(s);
  if (st == CVR_OK) st = timed_launch(c, s, [&] { return launch(fo, s); });
  if (st != CVR_OK) return st;
  return frame_output_finish(c, o, fo, s);
}

// A shaded renderer's frame over that path: launch(out, samples, shade,
// tile_samples, stream), then the sum epilogue of the sample total.
template <class Launch>
cvr_status render_shaded(Ctx* c, const cvr_output* o, int ntiles, size_t npix, const Launch& launch) {
  hipStream_t s = c->stream;
  FrameOut fo;
  cvr_status st = bind_frame_output(c, o, npix, fo);
  if (st == CVR_OK) st = frame_counters_begin(c, o, ntiles, s, fo);
  if (st == CVR_OK)
    st = timed_launch(c, s, [&] { return launch(fo.d_out, fo.d_samples, fo.shade, fo.tile_samples, s); });
  if (st != CVR_OK) return st;
  if (fo.tile_samples) {
    RenderPlan plan{};
    plan.ntiles = ntiles;
    HIP_TRY(c, launch_tile_epilogue(nullptr, fo.tile_samples, fo.d_total, plan, nullptr, s));
  }
  return frame_output_finish(c, o, fo, s);
}

}  // namespace cvr
