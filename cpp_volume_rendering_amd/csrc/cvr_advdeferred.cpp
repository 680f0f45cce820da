// cvr_advdeferred.cpp — advanced deferred isosurface shading (AdvancedDeferredShading;
// advdeferred.hip): the argument checks, the curvature planes kept next to the context's
// G-buffer, the lighting pass's two tables, and the three passes of a frame.  The
// geometry pass, the G-buffer and everything the parameters and the lighting pass have
// in common with DeferredShading's are cvr_deferred.cpp's and cvr_host.h's: this file
// keeps the feature parameters, the curvature pass and the tables.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstring>
#include <vector>

#include "cvr_host.h"

using namespace cvr;

namespace cvr {

void advdeferred_drop(Ctx* c, bool destroy) {
  Ctx::AdvDeferred& A = c->adv;
  free_dev(A.d_curv);
  A.valid = false;
  A.bytes = 0;
  if (destroy) {
    free_dev(A.d_cmap);
    free_dev(A.d_ridge);
    free_dev(A.d_features);
    A.table_bytes = 0;
    A.shaded = false;
  }
}

}  // namespace cvr

namespace {

// The parameters' common part: cvr_advdeferred_params begins with cvr_deferred_params'
// fields, in its order (include/cvr.h), so the geometry pass, the lighting checks and
// the shade arguments' filler take that prefix, and a field added to both is in it.
static_assert(offsetof(cvr_advdeferred_params, flow_speed) == sizeof(cvr_deferred_params) &&
                  offsetof(cvr_advdeferred_params, gbuffer_clear) == offsetof(cvr_deferred_params, gbuffer_clear),
              "cvr_advdeferred_params must begin with cvr_deferred_params' fields");
cvr_deferred_params deferred_prefix(const cvr_advdeferred_params* p) {
  cvr_deferred_params d;
  std::memcpy(&d, p, sizeof(d));
  return d;
}

// What the lighting pass reads of the parameters: the common checks, and its own scalars'
cvr_status check_shade_params(Ctx* c, const char* who, const cvr_advdeferred_params* p) {
  const float scalars[] = {p->flow_speed, p->flow_scale, p->time,           p->accessibility_strength,
                           p->colormap_s, p->colormap_v, p->screen_size[0], p->screen_size[1]};
  const cvr_deferred_params d = deferred_prefix(p);
  return deferred_check_lighting(c, who, &d, "lighting, feature or tone-map", any_nan(scalars, 8));
}

// Result[0][0] and Result[1][1] of Camera::Projection (camera.cpp:286-293): it hands
// field_of_view_y, degrees, to glm::perspective, which without GLM_FORCE_RADIANS converts
// it (glm/gtc/matrix_transform.inl:233-240), all in float.
void projection_scales(const cvr_frame* f, float& p00, float& p11) {
  const float aspect = f->camera.aspect > 0 ? f->camera.aspect : (float)f->width / (float)f->height;
  const float rad = f->camera.fovy_deg * 0.01745329251994329576923690768489f;
  const float tan_half = std::tan(rad / 2.0f);
  p00 = 1.0f / (aspect * tan_half);
  p11 = 1.0f / tan_half;
}

// CreateTransferFunctions' rainbow (AdvancedDeferredShading.cpp:241-264): texel i as
// (rgb, 1), in float as written
void build_color_map(float s, float v, std::vector<float>& map) {
  map.resize((size_t)kAdvColorMapSize * 4);
  for (int i = 0; i < kAdvColorMapSize; i++) {
    const float t = (float)i / (float)(kAdvColorMapSize - 1);
    const float h = t * 6.0f;
    const float ch = v * s;
    const float x = ch * (1.0f - std::fabs(std::fmod(h, 2.0f) - 1.0f));
    const float m = v - ch;
    float r, g, b;
    if (h < 1.0f) { r = ch; g = x; b = 0.0f; }
    else if (h < 2.0f) { r = x; g = ch; b = 0.0f; }
    else if (h < 3.0f) { r = 0.0f; g = ch; b = x; }
    else if (h < 4.0f) { r = 0.0f; g = x; b = ch; }
    else { r = x; g = 0.0f; b = ch; }
    map[(size_t)i * 4 + 0] = r + m;
    map[(size_t)i * 4 + 1] = g + m;
    map[(size_t)i * 4 + 2] = b + m;
    map[(size_t)i * 4 + 3] = 1.0f;
  }
}

// The .r channel of its ridge map (:274-293), the only one the shader reads
void build_ridge_map(std::vector<float>& map) {
  const int n = kAdvRidgeMapSize;
  map.resize((size_t)n * n);
  for (int y = 0; y < n; y++)
    for (int x = 0; x < n; x++) {
      const float k1 = ((float)x / (float)(n - 1)) * 2.0f - 1.0f;
      const float k2 = ((float)y / (float)(n - 1)) * 2.0f - 1.0f;
      map[(size_t)y * n + x] = std::fmax(0.0f, k1) * (k1 > k2 ? 1.0f : 0.0f);
    }
}

// The tables on the device: built once per context, the colour map again when s or v
// changed (an earlier lighting pass may still read it: the stream drains first).
cvr_status ensure_tables(Ctx* c, const cvr_advdeferred_params* p) {
  Ctx::AdvDeferred& A = c->adv;
  const size_t cmap_bytes = (size_t)kAdvColorMapSize * 16;
  const size_t ridge_bytes = (size_t)kAdvRidgeMapSize * kAdvRidgeMapSize * 4;
  if (!A.d_features) HIP_TRY(c, hipMalloc((void**)&A.d_features, sizeof(unsigned long long)));
  if (!A.d_ridge) {
    std::vector<float> ridge;
    build_ridge_map(ridge);
    HIP_TRY(c, hipMalloc((void**)&A.d_ridge, ridge_bytes));
    HIP_TRY(c, hipMemcpy(A.d_ridge, ridge.data(), ridge_bytes, hipMemcpyHostToDevice));
    A.table_bytes += ridge_bytes;
  }
  const bool fresh = !A.d_cmap;
  if (fresh) {
    HIP_TRY(c, hipMalloc((void**)&A.d_cmap, cmap_bytes));
    A.table_bytes += cmap_bytes;
  }
  if (fresh || A.cmap_s != p->colormap_s || A.cmap_v != p->colormap_v) {
    std::vector<float> cmap;
    build_color_map(p->colormap_s, p->colormap_v, cmap);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpy(A.d_cmap, cmap.data(), cmap_bytes, hipMemcpyHostToDevice));
    A.cmap_s = p->colormap_s;
    A.cmap_v = p->colormap_v;
  }
  return CVR_OK;
}

// The curvature pass over the kept G-buffer for `f`'s projection, on the context stream.
cvr_status curvature_pass(Ctx* c, const char* who, const cvr_frame* f) {
  const Ctx::Deferred& D = c->deferred;
  Ctx::AdvDeferred& A = c->adv;
  const size_t npix = (size_t)D.W * D.H;
  HIP_TRY(c, hipSetDevice(c->device));
  if (!A.d_curv) {   // deferred_drop frees the planes with a G-buffer of another size
    hipError_t e = hipMalloc((void**)&A.d_curv, npix * 16);
    if (e != hipSuccess) return fail_hip(c, who, e);
    A.bytes = npix * 16;
  }
  float p00, p11;
  projection_scales(f, p00, p11);
  A.valid = false;
  HIP_TRY(c, launch_adv_curvature(D.W, D.H, p00, p11, D.d_gbuf, A.d_curv, c->stream));
  A.p00 = p00;
  A.p11 = p11;
  A.valid = true;
  A.launches++;
  return CVR_OK;
}

// The lighting pass over the kept planes into `o`, through the shared frame-output path.
cvr_status shade_pass(Ctx* c, const cvr_advdeferred_params* p, const cvr_output* o) {
  const Ctx::Deferred& D = c->deferred;
  Ctx::AdvDeferred& A = c->adv;
  const cvr_deferred_params d = deferred_prefix(p);
  AdvShadeArgs S{};
  fill_shade_lighting(S, D, &d);
  S.alpha = p->color[3];
  S.flow_speed = p->flow_speed;
  S.flow_scale = p->flow_scale;
  S.time = p->time;
  S.show_ridges = p->show_ridges != 0;
  S.show_valleys = p->show_valleys != 0;
  S.accessibility = p->accessibility_strength;
  S.screen[0] = p->screen_size[0] > 0.0f ? p->screen_size[0] : (float)D.W;
  S.screen[1] = p->screen_size[1] > 0.0f ? p->screen_size[1] : (float)D.H;
  HIP_TRY(c, hipSetDevice(c->device));
  const cvr_status st = ensure_tables(c, p);
  if (st != CVR_OK) return st;
  return shade_frame(
      c, o,
      [&](hipStream_t s) {
        HIP_TRY(c, hipMemsetAsync(A.d_features, 0, sizeof(unsigned long long), s));
        return CVR_OK;
      },
      [&](const FrameOut& fo, hipStream_t s) {
        const hipError_t e = launch_adv_shade(S, D.d_gbuf, A.d_curv, A.d_cmap, A.d_ridge, fo.d_out, fo.half,
                                              fo.d_samples, fo.d_total, A.d_features, s);
        if (e == hipSuccess) A.shaded = true;
        return e;
      });
}

}  // namespace

extern "C" {
#pragma GCC visibility push(default)

void cvr_advdeferred_params_default(cvr_advdeferred_params* p) {
  if (!p) return;
  cvr_deferred_params d{};
  deferred_common_defaults(&d);
  *p = cvr_advdeferred_params{};
  std::memcpy(p, &d, sizeof(d));
  // lighting_pass.comp:200-207: constants of the shader, no uniforms
  p->ka = 0.1f; p->kd = 0.7f; p->ks = 0.2f; p->shininess = 32.0f;
  for (int i = 0; i < 4; i++) p->gbuffer_clear[i] = 1.0f;   // Redraw's glClearColor (:724)
  p->flow_speed = 1.0f;                          // AdvancedDeferredShading.h:129-133
  p->flow_scale = 10.0f;
  p->time = 0.0f;                                // m_current_time (constructor :130; :662 is a comment)
  p->show_ridges = 1;
  p->show_valleys = 1;
  p->accessibility_strength = 0.5f;
  p->screen_size[0] = p->screen_size[1] = 0.0f;  // never set (:379 is a comment): the frame's size
  p->colormap_s = 0.6f;                          // Init (:536-537)
  p->colormap_v = 0.2f;
}

cvr_status cvr_render_advdeferred(cvr_ctx* ctx, const cvr_frame* f, const cvr_advdeferred_params* p,
                                  const cvr_output* o) {
  Ctx* c = reinterpret_cast<Ctx*>(ctx);
  const char* who = "cvr_render_advdeferred";
  cvr_status st = deferred_entry(c, who, f && p && o);
  if (st != CVR_OK) return st;
  const cvr_deferred_params g = deferred_prefix(p);
  st = deferred_check_output(c, who, o);
  if (st == CVR_OK) st = check_shade_params(c, who, p);
  if (st == CVR_OK) st = deferred_check_geometry_call(c, who, f, &g);
  if (st != CVR_OK) return st;
  st = deferred_geometry_pass(c, who, f, &g);
  if (st == CVR_OK) st = curvature_pass(c, who, f);
  if (st != CVR_OK) return st;
  return shade_pass(c, p, o);
}

cvr_status cvr_advdeferred_curvature(cvr_ctx* ctx, const cvr_frame* f, const cvr_advdeferred_params* p) {
  Ctx* c = reinterpret_cast<Ctx*>(ctx);
  const char* who = "cvr_advdeferred_curvature";
  cvr_status st = deferred_entry(c, who, f && p);
  if (st != CVR_OK) return st;
  if (f->nranks > 1)
    return fail(c, CVR_ERR_ARG, "%s: the pass reads neighbouring pixels: whole frames only (nranks <= 1)", who);
  if (f->camera.fovy_deg != f->camera.fovy_deg || f->camera.aspect != f->camera.aspect)
    return fail(c, CVR_ERR_ARG, "%s: the camera's field of view or aspect is NaN", who);
  st = check_shade_params(c, who, p);
  if (st == CVR_OK)
    st = deferred_check_kept(c, who, c->deferred.valid, "no G-buffer (cvr_deferred_geometry)", f->width, f->height,
                             CVR_ERR_STATE);
  if (st != CVR_OK) return st;
  return curvature_pass(c, who, f);
}

cvr_status cvr_advdeferred_shade(cvr_ctx* ctx, int width, int height, const cvr_advdeferred_params* p,
                                 const cvr_output* o) {
  Ctx* c = reinterpret_cast<Ctx*>(ctx);
  const char* who = "cvr_advdeferred_shade";
  cvr_status st = deferred_entry(c, who, p && o);
  if (st == CVR_OK) st = deferred_check_output(c, who, o);
  if (st == CVR_OK) st = check_shade_params(c, who, p);
  if (st == CVR_OK)
    st = deferred_check_kept(c, who, c->deferred.valid && c->adv.valid,
                             "no curvature planes of the kept G-buffer (cvr_advdeferred_curvature)", width, height);
  if (st != CVR_OK) return st;
  return shade_pass(c, p, o);
}

cvr_status cvr_advdeferred_read_curvature(cvr_ctx* ctx, int width, int height, float* out_k1, float* out_k2,
                                          float* out_dir) {
  Ctx* c = reinterpret_cast<Ctx*>(ctx);
  if (!c) return CVR_ERR_ARG;
  const char* who = "cvr_advdeferred_read_curvature";
  if (!out_k1 || !out_k2 || !out_dir) return fail(c, CVR_ERR_ARG, "%s: null argument", who);
  if (c->group) return fail(c, CVR_ERR_ARG, "%s: not available on a group context", who);
  const cvr_status st = deferred_check_kept(c, who, c->deferred.valid && c->adv.valid,
                                            "no curvature planes (cvr_advdeferred_curvature)", width, height);
  if (st != CVR_OK) return st;
  const size_t npix = (size_t)width * height;
  std::vector<float> packed(npix * 4);
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipMemcpy(packed.data(), c->adv.d_curv, npix * 16, hipMemcpyDeviceToHost));
  for (size_t i = 0; i < npix; i++) {
    out_k1[i] = packed[i * 4 + 0];
    out_k2[i] = packed[i * 4 + 1];
    out_dir[i * 2 + 0] = packed[i * 4 + 2];
    out_dir[i * 2 + 1] = packed[i * 4 + 3];
  }
  return CVR_OK;
}

#pragma GCC visibility pop
}  // extern "C"
