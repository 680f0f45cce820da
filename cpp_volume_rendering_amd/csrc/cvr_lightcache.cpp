// cvr_lightcache.cpp — pre-illumination (PreIlluminationStructuredVolume): the
// light cache's state, its two producers (the DOS cones of lightcache.hip, the
// EBS SAT terms of ebs_lightcache.hip) and the march over it (lightcache.hip).
#include <hip/hip_runtime.h>

#include <cstring>

#include "cvr_host.h"

using namespace cvr;

namespace cvr {

// The pre-illumination light cache goes with the state it was computed from: a
// new volume, TF, extinction pyramid or SAT drops it (after the device has drained).
void light_cache_drop(Ctx* c, bool destroy) {
  Ctx::LightCache& l = c->lc;
  free_dev(l.d_cache);
  l.bytes = 0;
  l.dims[0] = l.dims[1] = l.dims[2] = 0;
  l.key.valid = 0;
  l.readers = 0;
  l.written = false;
  if (destroy && l.ev) (void)hipEventDestroy(l.ev);
}

}  // namespace cvr

static cvr_status light_cache_check_dims(Ctx* c, const char* who, const int dims[3]) {
  for (int i = 0; i < 3; i++)
    if (!dims || dims[i] < 2 || dims[i] > cvr::kMaxLightCacheDim)
      return fail(c, CVR_ERR_ARG, "%s: light cache dimensions must be in [2, %d]", who, cvr::kMaxLightCacheDim);
  return CVR_OK;
}

// Before the cache is written (or freed) on the context stream: frames that read
// it on this stream are ordered before the write; frames on other streams, or an
// earlier write on another stream, are not, so the device drains first.
static cvr_status light_cache_write_begin(Ctx* c) {
  const bool foreign_reader = c->lc.readers == 2 || (c->lc.readers == 1 && c->lc.reader != c->stream);
  const bool foreign_writer = c->lc.written && c->lc.writer != c->stream;
  if (foreign_reader || foreign_writer) QUIESCE(c);
  c->lc.readers = 0;
  c->lc.written = false;
  return CVR_OK;
}

// The cache buffer for `dims` (kept when the size is unchanged).
static cvr_status light_cache_reserve(Ctx* c, const int dims[3]) {
  const size_t bytes = (size_t)dims[0] * dims[1] * dims[2] * 4;
  if (!c->lc.d_cache || bytes != c->lc.bytes) {
    QUIESCE(c);   // frames in flight on any stream may read the buffer freed below
    light_cache_drop(c);
    HIP_TRY(c, hipMalloc((void**)&c->lc.d_cache, bytes));
    c->lc.bytes = bytes;
  }
  for (int i = 0; i < 3; i++) c->lc.dims[i] = dims[i];
  return CVR_OK;
}

// EyeCamUp: the cup of Camera::GetCameraVectors (camera.cpp:336-341), glm float
// arithmetic; with use_view the view matrix's own up row (the same vector of a
// lookAt matrix, which keeps its centre private)
static void eye_cam_up(const cvr_frame* f, float out[3]) {
  if (f->use_view) {
    out[0] = f->view[1]; out[1] = f->view[5]; out[2] = f->view[9];
    return;
  }
  const V3 eye{f->camera.eye[0], f->camera.eye[1], f->camera.eye[2]};
  const V3 center{f->camera.center[0], f->camera.center[1], f->camera.center[2]};
  const V3 up{f->camera.up[0], f->camera.up[1], f->camera.up[2]};
  const V3 dir = gnormalize(sub(center, eye));
  const V3 fwd{-dir.x, -dir.y, -dir.z};
  const V3 right = gnormalize(cross(up, fwd));
  const V3 cup = gnormalize(cross(fwd, right));
  out[0] = cup.x; out[1] = cup.y; out[2] = cup.z;
}

static void light_cache_key(const Ctx* c, const cvr_frame* f, const cvr_dos_params* p,
                            const cvr_cone_params cp[2], const int dims[3], Ctx::LightCacheKey& k) {
  k = Ctx::LightCacheKey{};
  k.valid = 1;
  for (int i = 0; i < 3; i++) k.dims[i] = dims[i];
  k.apply_occlusion = p->apply_occlusion != 0;
  k.apply_shadow = p->apply_shadow != 0;
  k.shadow_type = p->shadow_type;
  k.filter_bits = c->filter_bits;
  // a cone or a light that is switched off does not reach the cache
  if (k.apply_occlusion) k.dos.cone[0] = cp[0];
  if (k.apply_shadow) {
    k.dos.cone[1] = cp[1];
    k.dos.light = p->light;
  }
  if (k.apply_occlusion) {
    for (int i = 0; i < 3; i++) k.dos.eye[i] = f->camera.eye[i];
    eye_cam_up(f, k.dos.cam_up);
  }
}

static void ebs_light_cache_key(const Ctx* c, const cvr_ebs_params* p, const int dims[3],
                                Ctx::LightCacheKey& k) {
  k = Ctx::LightCacheKey{};
  k.valid = 1;
  k.kind = 1;
  for (int i = 0; i < 3; i++) k.dims[i] = dims[i];
  k.apply_occlusion = p->apply_occlusion != 0;
  k.apply_shadow = p->apply_shadow != 0;
  k.filter_bits = c->filter_bits;
  // a term that is switched off does not reach the cache; the camera never does
  if (k.apply_occlusion) {
    k.ebs.shells = p->occlusion_shells;
    k.ebs.radius = p->occlusion_radius;
  }
  if (k.apply_shadow) {
    k.shadow_type = p->shadow_type;
    k.ebs.angle = p->shadow_cone_angle_deg;
    k.ebs.interval = p->shadow_sample_interval;
    k.ebs.initial = p->shadow_initial_step;
    k.ebs.weight = p->shadow_ui_weight;
    k.ebs.max_distance = ebs_max_distance(c, p);
    for (int i = 0; i < 3; i++) k.ebs.light[i] = p->shadow_type == 0 ? p->light_pos[i] : p->light_forward[i];
  }
}

// The context's cache was computed from exactly `key`: the *_preillum renders skip
// the compute.
static bool light_cache_fresh(const Ctx* c, const Ctx::LightCacheKey& key) {
  return c->lc.d_cache && c->lc.key.valid && std::memcmp(&key, &c->lc.key, sizeof(key)) == 0;
}

// What the two PreComputeLightCache dispatches share, after the producer has
// prepared its kernel arguments: the cache is reserved for `dims` and
// launch(P) fills it on the context stream; `key` says what it was computed from.
template <class Launch>
static cvr_status light_cache_compute(Ctx* c, const char* who, const int dims[3], const Launch& launch,
                                      const Ctx::LightCacheKey& key) {
  if (c->native_exp)
    return fail(c, CVR_ERR_ARG, "%s: the light cache has no native_exp (tolerance) form", who);
  cvr_status st;
  if ((st = light_cache_write_begin(c)) != CVR_OK) return st;
  if ((st = light_cache_reserve(c, dims)) != CVR_OK) return st;
  cvr::LightCacheArgs P{};
  for (int i = 0; i < 3; i++) {
    P.dims[i] = dims[i];
    // VolumeScales * (VolumeDimensions / LightCacheDimensions), float (:537)
    P.vs[i] = c->scale[i] * ((float)c->N[i] / (float)dims[i]);
  }
  c->lc.key.valid = 0;
  HIP_TRY(c, launch(P));
  if (!c->lc.ev) HIP_TRY(c, hipEventCreateWithFlags(&c->lc.ev, hipEventDisableTiming));
  HIP_TRY(c, hipEventRecord(c->lc.ev, c->stream));
  c->lc.written = true;
  c->lc.writer = c->stream;
  c->lc.builds++;
  c->lc.key = key;
  return CVR_OK;
}

// PreComputeLightCache (dosrcrenderer.cpp:555-655), queued on the context stream.
static cvr_status dos_light_cache_compute(Ctx* c, const char* who, const cvr_frame* f,
                                          const cvr_dos_params* p, const int dims[3]) {
  cvr_status st = light_cache_check_dims(c, who, dims);
  if (st != CVR_OK) return st;
  cvr::DosArgs Q;
  int ntiles = 0;
  size_t npix = 0;
  cvr_cone_params cp[2];
  if ((st = dos_prepare(c, who, f, p, nullptr, true, Q, ntiles, npix, cp)) != CVR_OK) return st;
  Ctx::LightCacheKey key;
  light_cache_key(c, f, p, cp, dims, key);
  return light_cache_compute(c, who, dims, [&](cvr::LightCacheArgs& P) {
    eye_cam_up(f, P.cam_up);
    return cvr::launch_light_cache(Q, P, c->ext.d_cells, c->lc.d_cache, c->stream);
  }, key);
}

// RC1PExtinctionBasedShading's PreComputeLightCache (the dispatch of
// rc1pextbsd/lightcachecomputation.comp), queued on the context stream.
static cvr_status ebs_light_cache_compute(Ctx* c, const char* who, const cvr_ebs_params* p,
                                          const int dims[3]) {
  cvr_status st = light_cache_check_dims(c, who, dims);
  if (st != CVR_OK) return st;
  cvr::EbsArgs Q;
  int ntiles = 0;
  size_t npix = 0;
  if ((st = ebs_prepare(c, who, nullptr, p, nullptr, Q, ntiles, npix)) != CVR_OK) return st;
  Ctx::LightCacheKey key;
  ebs_light_cache_key(c, p, dims, key);
  return light_cache_compute(c, who, dims, [&](cvr::LightCacheArgs& P) {
    return cvr::launch_ebs_light_cache(*c, Q, P, c->lc.d_cache, c->stream);
  }, key);
}

// The cached march over the context's cache (cvr_render_preillum, and the second
// half of cvr_render_extbsd_preillum).
static cvr_status preillum_march(Ctx* c, const char* who, const cvr_frame* f, const cvr_dos_params* p,
                                 const cvr_output* o) {
  if (!o) return fail(c, CVR_ERR_ARG, "%s: null argument", who);
  cvr::DosArgs Q;
  int ntiles = 0;
  size_t npix = 0;
  cvr_cone_params cp[2];
  const cvr_status st = dos_prepare(c, who, f, p, o, false, Q, ntiles, npix, cp);
  if (st != CVR_OK) return st;
  if (!c->lc.d_cache)
    return fail(c, CVR_ERR_STATE, "%s: no light cache (cvr_compute_light_cache_dosct / "
                                  "cvr_compute_light_cache_extbsd / cvr_set_light_cache)", who);
  cvr::LightCacheView V{};
  V.rg = c->lc.d_cache;
  for (int i = 0; i < 3; i++) {
    V.d[i] = c->lc.dims[i];
    V.s[i] = (float)c->lc.dims[i] / Q.G[i];   // L / G, rounded once
    V.m[i] = (float)(c->lc.dims[i] - 1);
  }
  // a cache written on another stream: this frame waits for that write
  if (c->lc.written && c->lc.writer != c->stream) HIP_TRY(c, hipStreamWaitEvent(c->stream, c->lc.ev, 0));
  if (c->lc.readers == 0) {
    c->lc.readers = 1;
    c->lc.reader = c->stream;
  } else if (c->lc.reader != c->stream) {
    c->lc.readers = 2;
  }
  return render_shaded(c, o, ntiles, npix, [&](float4* out, uint32_t* smp, unsigned long long* shade,
                                                unsigned long long* ts, hipStream_t st) {
    return cvr::launch_preillum(*c, Q, V, out, smp, shade, ts, st);
  });
}

extern "C" {
#pragma GCC visibility push(default)

cvr_status cvr_compute_light_cache_dosct(cvr_ctx* ctx, const cvr_frame* f, const cvr_dos_params* p,
                                         const int dims[3]) {
  Ctx* c = reinterpret_cast<Ctx*>(ctx);
  if (!c) return CVR_ERR_ARG;
  NO_GROUP(c, "cvr_compute_light_cache_dosct");
  return dos_light_cache_compute(c, "cvr_compute_light_cache_dosct", f, p, dims);
}

cvr_status cvr_compute_light_cache_extbsd(cvr_ctx* ctx, const cvr_ebs_params* p, const int dims[3]) {
  Ctx* c = reinterpret_cast<Ctx*>(ctx);
  if (!c) return CVR_ERR_ARG;
  NO_GROUP(c, "cvr_compute_light_cache_extbsd");
  return ebs_light_cache_compute(c, "cvr_compute_light_cache_extbsd", p, dims);
}

cvr_status cvr_set_light_cache(cvr_ctx* ctx, const uint16_t* rg_half, const int dims[3]) {
  Ctx* c = reinterpret_cast<Ctx*>(ctx);
  if (!c) return CVR_ERR_ARG;
  NO_GROUP(c, "cvr_set_light_cache");
  if (!rg_half) return fail(c, CVR_ERR_ARG, "cvr_set_light_cache: null argument");
  cvr_status st = light_cache_check_dims(c, "cvr_set_light_cache", dims);
  if (st != CVR_OK) return st;
  QUIESCE(c);   // frames in flight on any stream read the cache replaced below
  c->lc.readers = 0;
  c->lc.written = false;
  if ((st = light_cache_reserve(c, dims)) != CVR_OK) return st;
  c->lc.key.valid = 0;   // not this library's compute: cvr_render_*_preillum recompute
  HIP_TRY(c, hipMemcpy(c->lc.d_cache, rg_half, c->lc.bytes, hipMemcpyHostToDevice));
  return CVR_OK;
}

cvr_status cvr_copy_light_cache(cvr_ctx* ctx, uint16_t* out, size_t capacity, int dims[3]) {
  Ctx* c = reinterpret_cast<Ctx*>(ctx);
  if (!c) return CVR_ERR_ARG;
  NO_GROUP(c, "cvr_copy_light_cache");
  if (!c->lc.d_cache) return fail(c, CVR_ERR_STATE, "cvr_copy_light_cache: no light cache");
  if (dims)
    for (int i = 0; i < 3; i++) dims[i] = c->lc.dims[i];
  if (!out) return CVR_OK;
  if (capacity < c->lc.bytes / 2)
    return fail(c, CVR_ERR_ARG, "cvr_copy_light_cache: need %zu halfs", c->lc.bytes / 2);
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (c->lc.written && c->lc.writer != c->stream) HIP_TRY(c, hipEventSynchronize(c->lc.ev));
  HIP_TRY(c, hipMemcpy(out, c->lc.d_cache, c->lc.bytes, hipMemcpyDeviceToHost));
  return CVR_OK;
}

cvr_status cvr_render_preillum(cvr_ctx* ctx, const cvr_frame* f, const cvr_dos_params* p,
                               const cvr_output* o) {
  Ctx* c = reinterpret_cast<Ctx*>(ctx);
  if (!c) return CVR_ERR_ARG;
  NO_GROUP(c, "cvr_render_preillum");
  return preillum_march(c, "cvr_render_preillum", f, p, o);
}

// RC1PConeTracingDirOcclusionShading::Update with pre-illumination on
// (dosrcrenderer.cpp:134-143): PreComputeLightCache, then the cached march.  The
// reference recomputes on every Update; here the compute is skipped while nothing
// the cache depends on has changed.
cvr_status cvr_render_dosct_preillum(cvr_ctx* ctx, const cvr_frame* f, const cvr_dos_params* p,
                                     const int dims[3], const cvr_output* o) {
  Ctx* c = reinterpret_cast<Ctx*>(ctx);
  if (!c) return CVR_ERR_ARG;
  NO_GROUP(c, "cvr_render_dosct_preillum");
  if (!f || !p || !o || !o->rgba) return fail(c, CVR_ERR_ARG, "cvr_render_dosct_preillum: null argument");
  cvr_status st = light_cache_check_dims(c, "cvr_render_dosct_preillum", dims);
  if (st != CVR_OK) return st;
  if (p->shadow_type < 0 || p->shadow_type > 2)
    return fail(c, CVR_ERR_ARG, "cvr_render_dosct_preillum: bad shadow type");
  cvr_cone_params cp[2];
  resolve_cone_params(c, p, cp);
  Ctx::LightCacheKey k;
  light_cache_key(c, f, p, cp, dims, k);
  if (!light_cache_fresh(c, k) &&
      (st = dos_light_cache_compute(c, "cvr_render_dosct_preillum", f, p, dims)) != CVR_OK)
    return st;
  return cvr_render_preillum(ctx, f, p, o);
}

// RC1PExtinctionBasedShading::Update with pre-illumination on: PreComputeLightCache,
// then the cached march (obj_ray_marching.comp, the DOS renderer's too).  The
// reference recomputes on every Update; here the compute is skipped while nothing
// the cache depends on has changed, and the camera is nothing it depends on.
cvr_status cvr_render_extbsd_preillum(cvr_ctx* ctx, const cvr_frame* f, const cvr_ebs_params* p,
                                      const int dims[3], const cvr_output* o) {
  Ctx* c = reinterpret_cast<Ctx*>(ctx);
  if (!c) return CVR_ERR_ARG;
  NO_GROUP(c, "cvr_render_extbsd_preillum");
  if (!f || !p || !o || !o->rgba) return fail(c, CVR_ERR_ARG, "cvr_render_extbsd_preillum: null argument");
  cvr_status st = light_cache_check_dims(c, "cvr_render_extbsd_preillum", dims);
  if (st != CVR_OK) return st;
  Ctx::LightCacheKey k;
  ebs_light_cache_key(c, p, dims, k);
  if (!light_cache_fresh(c, k) &&
      (st = ebs_light_cache_compute(c, "cvr_render_extbsd_preillum", p, dims)) != CVR_OK)
    return st;
  // the march reads the step, the Phong switch and constants, the light position
  // and the two switches: cvr_render_preillum's own inputs
  cvr_dos_params dp{};
  dp.step = p->step;
  dp.apply_gradient_shading = p->apply_gradient_shading;
  dp.ka = p->ka; dp.kd = p->kd; dp.ks = p->ks;
  dp.shininess = p->shininess;
  for (int i = 0; i < 3; i++) {
    dp.ispecular[i] = p->ispecular[i];
    dp.light.position[i] = p->light_pos[i];
  }
  dp.apply_occlusion = p->apply_occlusion;
  dp.apply_shadow = p->apply_shadow;
  return preillum_march(c, "cvr_render_extbsd_preillum", f, &dp, o);
}

#pragma GCC visibility pop
}  // extern "C"
