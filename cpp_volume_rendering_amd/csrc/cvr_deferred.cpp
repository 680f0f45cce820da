// cvr_deferred.cpp — deferred isosurface shading (DeferredShading; deferred.hip): the
// argument checks, the context's G-buffer, and the geometry / shade passes of a frame;
// and what AdvancedDeferredShading (cvr_advdeferred.cpp) has in common with it: the
// start of an entry, the common defaults, the lighting checks, the check of a call over
// the kept G-buffer (declared in cvr_host.h, next to the shade passes' shared frame).
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "cvr_host.h"

using namespace cvr;

namespace cvr {

void deferred_drop(Ctx* c, bool destroy) {
  Ctx::Deferred& D = c->deferred;
  free_dev(D.d_gbuf);
  D.W = D.H = 0;
  D.valid = false;
  D.bytes = 0;
  if (destroy) free_dev(D.d_hits);
  advdeferred_drop(c, destroy);   // the curvature planes are that G-buffer's
}

bool any_nan(const float* v, int n) {
  for (int i = 0; i < n; i++)
    if (v[i] != v[i]) return true;
  return false;
}
static bool any_negative(const float* v, int n) {
  for (int i = 0; i < n; i++)
    if (v[i] < 0.0f) return true;
  return false;
}

cvr_status deferred_entry(Ctx* c, const char* who, bool args_given) {
  if (!c) return CVR_ERR_ARG;
  if (c->group) return fail(c, CVR_ERR_ARG, "%s: not available on a group context (cvr_create_group)", who);
  if (!args_given) return fail(c, CVR_ERR_ARG, "%s: null argument", who);
  return CVR_OK;
}

// What a shade pass reads of the parameters (cvr_powf is specified for x >= 0).
cvr_status deferred_check_lighting(Ctx* c, const char* who, const cvr_deferred_params* p, const char* nan_what,
                                   bool more_nan) {
  const float scalars[] = {p->ka, p->kd, p->ks, p->shininess, p->exposure, p->gamma};
  if (more_nan || any_nan(scalars, 6) || any_nan(p->color, 4) || any_nan(p->light_color, 3) ||
      any_nan(p->light_pos, 3))
    return fail(c, CVR_ERR_ARG, "%s: a %s parameter is NaN", who, nan_what);
  if (p->ka < 0.0f || p->kd < 0.0f || p->ks < 0.0f)
    return fail(c, CVR_ERR_ARG, "%s: ka, kd and ks must be >= 0", who);
  if (any_negative(p->color, 4) || any_negative(p->light_color, 3))
    return fail(c, CVR_ERR_ARG, "%s: the colour and the light colour must be >= 0", who);
  return CVR_OK;
}

cvr_status deferred_check_kept(Ctx* c, const char* who, bool kept, const char* missing, int width, int height,
                               cvr_status mismatch) {
  if (!kept) return fail(c, CVR_ERR_STATE, "%s: %s", who, missing);
  if (width != c->deferred.W || height != c->deferred.H)
    return fail(c, mismatch, "%s: the G-buffer is %dx%d", who, c->deferred.W, c->deferred.H);
  return CVR_OK;
}

// The constructor's march (DeferredShading.cpp:123-127, AdvancedDeferredShading.cpp:124-128),
// Init's blocks (:348, :561), LightingPass's light (:216, :372-380), Redraw's tone map
// (:538-539, :752-753)
void deferred_common_defaults(cvr_deferred_params* p) {
  p->isovalue = 0.5f;
  p->step_small = 0.05f;
  p->step_large = 1.0f;
  p->step_range = 0.1f;
  for (int i = 0; i < 3; i++) p->num_blocks[i] = 4;
  p->color[0] = 0.66f; p->color[1] = 0.6f; p->color[2] = 0.05f; p->color[3] = 1.0f;
  for (int i = 0; i < 3; i++) p->light_color[i] = 1.0f;
  cvr_light l;
  default_light(&l);
  for (int i = 0; i < 3; i++) p->light_pos[i] = l.position[i];
  p->exposure = 1.0f;
  p->gamma = 2.2f;
}

}  // namespace cvr

namespace {

// What the geometry pass reads of them.
cvr_status check_geometry_params(Ctx* c, const char* who, const cvr_deferred_params* p) {
  const float scalars[] = {p->isovalue, p->step_small, p->step_large, p->step_range};
  if (any_nan(scalars, 4) || any_nan(p->gbuffer_clear, 4))
    return fail(c, CVR_ERR_ARG, "%s: a march parameter is NaN", who);
  if (!(p->step_small > 0.0f) || !(p->step_large > 0.0f) || !(p->step_range > 0.0f))
    return fail(c, CVR_ERR_ARG, "%s: the step sizes and the step range must be > 0", who);
  for (int i = 0; i < 3; i++)
    if (p->num_blocks[i] < 1 || p->num_blocks[i] > 1024)
      return fail(c, CVR_ERR_ARG, "%s: bad block count %d", who, p->num_blocks[i]);
  return CVR_OK;
}

}  // namespace

namespace cvr {

// The checks of a call that marches `f`, before anything is launched or allocated.
cvr_status deferred_check_geometry_call(Ctx* c, const char* who, const cvr_frame* f, const cvr_deferred_params* p) {
  if (f->width < 1 || f->height < 1 || f->width > 32768 || f->height > 32768)
    return fail(c, CVR_ERR_ARG, "%s: bad viewport %dx%d", who, f->width, f->height);
  if (f->nranks > 1)
    return fail(c, CVR_ERR_ARG, "%s: the lighting pass reads neighbouring pixels: whole frames only (nranks <= 1)",
                who);
  const cvr_status st = check_geometry_params(c, who, p);
  if (st != CVR_OK) return st;
  if (!c->d_cells || !c->d_vox) return fail(c, CVR_ERR_STATE, "%s: no volume set", who);
  return CVR_OK;
}

// The geometry pass of `f` into the context's G-buffer, on the context stream.
cvr_status deferred_geometry_pass(Ctx* c, const char* who, const cvr_frame* f, const cvr_deferred_params* p) {
  HIP_TRY(c, hipSetDevice(c->device));
  cvr_status st = ensure_iso_blocks(c, p->num_blocks);
  if (st != CVR_OK) return st;

  IsoArgs Q{};
  int ntiles = 0;
  size_t npix = 0;
  fill_frame_args(c, f, 1.0f, Q.a, ntiles, npix);
  grid_size(c, Q.G);
  for (int i = 0; i < 3; i++) {
    Q.nb[i] = (float)p->num_blocks[i];
    Q.nbi[i] = p->num_blocks[i];
  }
  Q.iso = p->isovalue;
  Q.step_small = p->step_small;
  Q.step_large = p->step_large;
  Q.step_range = p->step_range;
  {   // length(VolumeGridSize / numBlocks) * 0.5 (geometry_pass.comp:201-202)
    const float b0 = Q.G[0] / Q.nb[0], b1 = Q.G[1] / Q.nb[1], b2 = Q.G[2] / Q.nb[2];
    Q.half_block_len = std::sqrt(std::fmaf(b2, b2, std::fmaf(b1, b1, b0 * b0))) * 0.5f;
  }
  for (int i = 0; i < 3; i++) {
    Q.bs[i] = Q.G[i] / Q.nb[i];
    Q.nhg[i] = -Q.G[i] * 0.5f;
    Q.inv_g[i] = 1.0f / Q.G[i];
  }

  Ctx::Deferred& D = c->deferred;
  if (!D.d_hits) HIP_TRY(c, hipMalloc((void**)&D.d_hits, sizeof(unsigned long long)));
  if (!D.d_gbuf || D.W != f->width || D.H != f->height) {
    QUIESCE(c);   // an earlier frame may still read the planes
    deferred_drop(c);
    hipError_t e = hipMalloc((void**)&D.d_gbuf, npix * 32);
    if (e != hipSuccess) return fail_hip(c, who, e);
    D.W = f->width;
    D.H = f->height;
    D.bytes = npix * 32;
  }
  hipStream_t s = c->stream;
  D.valid = false;
  c->adv.valid = false;   // the curvature planes were another G-buffer's
  HIP_TRY(c, hipMemsetAsync(D.d_hits, 0, sizeof(unsigned long long), s));
  HIP_TRY(c, launch_deferred_geometry(*c, Q, p->gbuffer_clear, c->iso.d_mm, D.d_gbuf, D.d_hits, s));
  for (int i = 0; i < 3; i++) D.eye[i] = Q.a.eye[i];
  D.valid = true;
  D.launches++;
  return CVR_OK;
}

cvr_status deferred_check_output(Ctx* c, const char* who, const cvr_output* o) {
  if (!o->rgba) return fail(c, CVR_ERR_ARG, "%s: null argument", who);
  if (o->format != CVR_FORMAT_RGBA32F && o->format != CVR_FORMAT_RGBA16F)
    return fail(c, CVR_ERR_ARG, "%s: unknown output format %d", who, o->format);
  return CVR_OK;
}

}  // namespace cvr

namespace {

// The shade pass over the kept G-buffer into `o`, through the shared frame-output path.
cvr_status shade_pass(Ctx* c, const cvr_deferred_params* p, const cvr_output* o) {
  const Ctx::Deferred& D = c->deferred;
  DeferredShadeArgs S{};
  fill_shade_lighting(S, D, p);
  for (int i = 0; i < 4; i++) S.color[i] = p->color[i];
  HIP_TRY(c, hipSetDevice(c->device));
  return shade_frame(c, o, [](hipStream_t) { return CVR_OK; }, [&](const FrameOut& fo, hipStream_t s) {
    return launch_deferred_shade(S, D.d_gbuf, fo.d_out, fo.half, fo.d_samples, fo.d_total, s);
  });
}

}  // namespace

extern "C" {
#pragma GCC visibility push(default)

void cvr_deferred_params_default(cvr_deferred_params* p) {
  if (!p) return;
  *p = cvr_deferred_params{};
  deferred_common_defaults(p);
  // Update's uniforms (:477-480) are the ones BindUniforms binds; renderingparameters.cpp:23-26
  p->ka = 0.5f; p->kd = 0.5f; p->ks = 0.8f; p->shininess = 30.0f;
  p->gbuffer_clear[0] = p->gbuffer_clear[1] = p->gbuffer_clear[2] = 1.0f;   // WHITE_BACKGROUND
  p->gbuffer_clear[3] = 0.0f;
}

cvr_status cvr_deferred_geometry(cvr_ctx* ctx, const cvr_frame* f, const cvr_deferred_params* p) {
  Ctx* c = reinterpret_cast<Ctx*>(ctx);
  const char* who = "cvr_deferred_geometry";
  cvr_status st = deferred_entry(c, who, f && p);
  if (st == CVR_OK) st = deferred_check_geometry_call(c, who, f, p);
  if (st != CVR_OK) return st;
  return deferred_geometry_pass(c, who, f, p);
}

cvr_status cvr_deferred_shade(cvr_ctx* ctx, int width, int height, const cvr_deferred_params* p,
                              const cvr_output* o) {
  Ctx* c = reinterpret_cast<Ctx*>(ctx);
  const char* who = "cvr_deferred_shade";
  cvr_status st = deferred_entry(c, who, p && o);
  if (st == CVR_OK) st = deferred_check_output(c, who, o);
  if (st == CVR_OK) st = deferred_check_lighting(c, who, p);
  if (st == CVR_OK)
    st = deferred_check_kept(c, who, c->deferred.valid, "no G-buffer (cvr_deferred_geometry)", width, height);
  if (st != CVR_OK) return st;
  return shade_pass(c, p, o);
}

cvr_status cvr_render_deferred(cvr_ctx* ctx, const cvr_frame* f, const cvr_deferred_params* p,
                               const cvr_output* o) {
  Ctx* c = reinterpret_cast<Ctx*>(ctx);
  const char* who = "cvr_render_deferred";
  cvr_status st = deferred_entry(c, who, f && p && o);
  if (st == CVR_OK) st = deferred_check_output(c, who, o);
  if (st == CVR_OK) st = deferred_check_lighting(c, who, p);
  if (st == CVR_OK) st = deferred_check_geometry_call(c, who, f, p);
  if (st != CVR_OK) return st;
  st = deferred_geometry_pass(c, who, f, p);
  if (st != CVR_OK) return st;
  return shade_pass(c, p, o);
}

cvr_status cvr_deferred_read_gbuffer(cvr_ctx* ctx, int width, int height, float* out_position,
                                     float* out_normal) {
  Ctx* c = reinterpret_cast<Ctx*>(ctx);
  if (!c) return CVR_ERR_ARG;
  const char* who = "cvr_deferred_read_gbuffer";
  if (!out_position || !out_normal) return fail(c, CVR_ERR_ARG, "%s: null argument", who);
  if (c->group) return fail(c, CVR_ERR_ARG, "%s: not available on a group context", who);
  const Ctx::Deferred& D = c->deferred;
  const cvr_status st = deferred_check_kept(c, who, D.valid, "no G-buffer (cvr_deferred_geometry)", width, height);
  if (st != CVR_OK) return st;
  const size_t npix = (size_t)D.W * D.H;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipMemcpy(out_position, D.d_gbuf, npix * 16, hipMemcpyDeviceToHost));
  HIP_TRY(c, hipMemcpy(out_normal, D.d_gbuf + npix, npix * 16, hipMemcpyDeviceToHost));
  // gNormal.w's slot holds the fetch count; its value is gPosition.w's
  for (size_t i = 0; i < npix; i++) out_normal[i * 4 + 3] = out_position[i * 4 + 3];
  return CVR_OK;
}

#pragma GCC visibility pop
}  // extern "C"
