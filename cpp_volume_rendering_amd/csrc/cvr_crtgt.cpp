// cvr_crtgt.cpp — the ground-truth cone ray-caster (RC1PConeLightGroundTruthSteps,
// rc1pcrtgt): the progressive frame's state, its launch rounds (crtgt.hip) and the
// three entry points over them.  The ray tables' builder is host arithmetic next to
// the other cone tables (cvr_cones.cpp).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <vector>

#include "cvr_host.h"

using namespace cvr;

namespace cvr {

// A new volume, TF or gradient: the frame in progress was marched through the old one.
void crtgt_invalidate(Ctx* c) { c->gt.valid = false; }

void crtgt_release(Ctx* c) {
  Ctx::Crtgt& g = c->gt;
  free_dev(g.st.dst); free_dev(g.st.s); free_dev(g.st.cnt); free_dev(g.st.done); free_dev(g.st.nj);
  free_dev(g.st.jobs); free_dev(g.st.list); free_dev(g.st.ctr);
  free_dev(g.d_rays);
  g = Ctx::Crtgt{};
}

}  // namespace cvr

// Bytes cvr_crtgt_begin holds for npix pixels, job_f4 float4 per job and nrays rays:
// 32 B of state per pixel, kCrtgtRoundSamples job slots and list entries per pixel,
// the round's three counters, the tables.
static size_t crtgt_bytes(size_t npix, int job_f4, size_t nrays) {
  return npix * 32 + npix * kCrtgtRoundSamples * ((size_t)job_f4 * 16 + 4) + 3 * sizeof(unsigned long long) +
         nrays * 12;
}

static cvr_status crtgt_reserve(Ctx* c, size_t npix, int job_f4, size_t nrays) {
  Ctx::Crtgt& g = c->gt;
  if (g.npix == npix && g.job_f4 == job_f4 && g.ray_cap >= nrays && g.st.dst) return CVR_OK;
  const size_t ray_cap = std::max(nrays, g.ray_cap);
  crtgt_release(c);
  CrtgtState& S = g.st;
  const size_t slots = npix * kCrtgtRoundSamples;
  hipError_t e = hipMalloc((void**)&S.dst, npix * 16);
  if (e == hipSuccess) e = hipMalloc((void**)&S.s, npix * 4);
  if (e == hipSuccess) e = hipMalloc((void**)&S.cnt, npix * 4);
  if (e == hipSuccess) e = hipMalloc((void**)&S.done, npix * 4);
  if (e == hipSuccess) e = hipMalloc((void**)&S.nj, npix * 4);
  if (e == hipSuccess) e = hipMalloc((void**)&S.jobs, slots * job_f4 * 16);
  if (e == hipSuccess) e = hipMalloc((void**)&S.list, slots * 4);
  if (e == hipSuccess) e = hipMalloc((void**)&S.ctr, 3 * sizeof(unsigned long long));
  if (e == hipSuccess) e = hipMalloc((void**)&g.d_rays, std::max<size_t>(ray_cap, 1) * 12);
  if (e != hipSuccess) {
    crtgt_release(c);
    return fail_hip(c, "cvr_crtgt_begin", e);
  }
  g.npix = npix;
  g.job_f4 = job_f4;
  g.ray_cap = ray_cap;
  g.bytes = crtgt_bytes(npix, job_f4, std::max<size_t>(ray_cap, 1));
  return CVR_OK;
}

// One secondary ray's loop `while (s < distance) { h = min(step, distance - s); s += h; }`
// must end: the step has to move a float of the largest |s|, and the step count is bounded.
static bool ray_loop_ok(float gap, float step, float dist) {
  if (!(step > 0.0f) || !std::isfinite(gap) || !std::isfinite(dist) || !std::isfinite(step)) return false;
  const float m = std::fmax(std::fabs(gap), std::fabs(dist));
  if (!(m + step > m)) return false;
  return !(((double)dist - (double)gap) / (double)step > (double)CVR_CRTGT_MAX_RAY_STEPS);
}

static cvr_status crtgt_begin(Ctx* c, const char* who, const cvr_frame* f, const cvr_crtgt_params* p,
                              const float* occ_rays, int n_occ, const float* sdw_rays, int n_sdw) {
  if (!f || !p) return fail(c, CVR_ERR_ARG, "%s: null argument", who);
  if (c->native_exp) return fail(c, CVR_ERR_ARG, "%s: the ground truth has no native_exp (tolerance) form", who);
  if (f->width < 1 || f->height < 1 || f->width > 32768 || f->height > 32768)
    return fail(c, CVR_ERR_ARG, "%s: bad viewport %dx%d", who, f->width, f->height);
  if (f->nranks > 1) return fail(c, CVR_ERR_ARG, "%s: whole frames only (nranks <= 1)", who);
  if ((size_t)f->width * f->height * kCrtgtRoundSamples >= ((size_t)1 << 32))
    return fail(c, CVR_ERR_ARG, "%s: viewport too large for 32-bit job slots", who);
  if (p->shadow_type < 0 || p->shadow_type > 2) return fail(c, CVR_ERR_ARG, "%s: bad shadow type", who);
  const bool occ = p->apply_occlusion != 0, sdw = p->apply_shadow != 0;
  if ((occ && (!occ_rays || n_occ < 1 || n_occ > CVR_CRTGT_MAX_RAYS)) ||
      (sdw && (!sdw_rays || n_sdw < 1 || n_sdw > CVR_CRTGT_MAX_RAYS)))
    return fail(c, CVR_ERR_ARG, "%s: a term that is on needs 1..%d rays", who, CVR_CRTGT_MAX_RAYS);
  if (!c->d_cells || !c->d_tf) return fail(c, CVR_ERR_STATE, "%s: no volume or TF", who);
  const bool phong = p->apply_gradient_shading != 0;
  if (phong && !c->d_grad) return fail(c, CVR_ERR_STATE, "%s: Phong needs cvr_set_gradient", who);
  if (c->tf_n > kMaxTfLds) return fail(c, CVR_ERR_ARG, "%s: TF too large", who);

  CrtgtArgs Q{};
  int ntiles = 0;
  size_t npix = 0;
  fill_frame_args(c, f, p->step, Q.a, ntiles, npix);
  Q.a.filter_bits = c->filter_bits;
  const float ispec[3] = {1.0f, 1.0f, 1.0f};   // `vec3(1) * (IShadow * ks * pow(...))`
  set_phong_constants(Q.a, p->ka, p->kd, p->ks, p->shininess, ispec, p->light.position);
  grid_size(c, Q.G);
  Q.light_gap = p->light_gap;
  Q.light_step = p->light_step;
  Q.apply_occlusion = occ;
  Q.apply_shadow = sdw;
  Q.shadow_type = p->shadow_type;
  Q.phong = phong;
  set_gated_weights(Q, occ, sdw, p->ka, p->kd, p->ks);
  // GetDiagonal() * 0.50f / 0.75f (crtgtrenderer.cpp:112-113), as the DOS cones' default
  const double vw = c->N[0] * (double)c->scale[0], vh = c->N[1] * (double)c->scale[1],
               vd = c->N[2] * (double)c->scale[2];
  const double diag = std::sqrt(vw * vw + vh * vh + vd * vd);
  Q.occ_distance = p->occ_distance > 0.0f ? p->occ_distance : (float)(diag * 0.50f);
  Q.sdw_distance = p->sdw_distance > 0.0f ? p->sdw_distance : (float)(diag * 0.75f);
  if ((occ && !ray_loop_ok(Q.light_gap, Q.light_step, Q.occ_distance)) ||
      (sdw && !ray_loop_ok(Q.light_gap, Q.light_step, Q.sdw_distance)))
    return fail(c, CVR_ERR_ARG, "%s: light_step must be > 0, advance a ray at its distance and take at "
                                "most %d steps", who, CVR_CRTGT_MAX_RAY_STEPS);
  Q.n_occ = occ ? n_occ : 0;
  Q.n_sdw = sdw ? n_sdw : 0;
  for (int i = 0; i < 3; i++) {
    Q.lzaxs[i] = -p->light.forward[i];   // zaxs = -GetBlinnPhongLightSourceCameraForward() (:227)
    Q.lup[i] = p->light.up[i];
    Q.lright[i] = p->light.right[i];
  }

  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamSynchronize(c->stream));   // an earlier frame's store may still read the state
  c->gt.valid = false;
  const cvr_status st = crtgt_reserve(c, npix, phong ? 3 : 2, (size_t)Q.n_occ + Q.n_sdw);
  if (st != CVR_OK) return st;
  Ctx::Crtgt& g = c->gt;
  // SetData(..., GL_RGB16F, GL_RGB, GL_FLOAT): every coefficient rounded to binary16
  std::vector<float> rays(((size_t)Q.n_occ + Q.n_sdw) * 3);
  for (size_t i = 0; i < (size_t)Q.n_occ * 3; i++) rays[i] = half_round(occ_rays[i]);
  for (size_t i = 0; i < (size_t)Q.n_sdw * 3; i++) rays[(size_t)Q.n_occ * 3 + i] = half_round(sdw_rays[i]);
  if (!rays.empty()) HIP_TRY(c, hipMemcpy(g.d_rays, rays.data(), rays.size() * 4, hipMemcpyHostToDevice));
  Q.occ_rays = g.d_rays;
  Q.sdw_rays = g.d_rays + (size_t)Q.n_occ * 3;
  g.q = Q;
  g.ntiles = ntiles;
  HIP_TRY(c, hipMemsetAsync(g.st.ctr, 0, 3 * sizeof(unsigned long long), c->stream));
  HIP_TRY(c, launch_crtgt_init(Q, g.st, c->stream));
  HIP_TRY(c, hipMemcpyAsync(&g.unfinished, g.st.ctr + 1, sizeof(unsigned long long), hipMemcpyDeviceToHost,
                            c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  g.valid = true;
  return CVR_OK;
}

static cvr_status crtgt_advance(Ctx* c, const char* who, int max_samples, const cvr_output* o,
                                unsigned long long* unfinished) {
  Ctx::Crtgt& g = c->gt;
  if (!g.valid)
    return fail(c, CVR_ERR_STATE, "%s: no frame in progress (cvr_crtgt_begin; a new volume, transfer "
                                  "function or gradient ends it)", who);
  if (c->native_exp) return fail(c, CVR_ERR_ARG, "%s: the ground truth has no native_exp (tolerance) form", who);
  if (max_samples < 1) return fail(c, CVR_ERR_ARG, "%s: max_samples must be >= 1", who);
  if (o) {
    if (!o->rgba) return fail(c, CVR_ERR_ARG, "%s: null argument", who);
    if (o->format != CVR_FORMAT_RGBA32F && o->format != CVR_FORMAT_RGBA16F)
      return fail(c, CVR_ERR_ARG, "%s: unknown output format %d", who, o->format);
  }
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  // rounds of at most kCrtgtRoundSamples iterations per pixel; the count of pixels
  // still unfinished comes back after each (a round's shading takes milliseconds)
  for (int left = max_samples; left > 0 && g.unfinished > 0;) {
    const int k = std::min(left, kCrtgtRoundSamples);
    HIP_TRY(c, hipMemsetAsync(g.st.ctr, 0, 2 * sizeof(unsigned long long), s));
    HIP_TRY(c, launch_crtgt_round(*c, g.q, g.st, k, s));
    HIP_TRY(c, hipMemcpyAsync(&g.unfinished, g.st.ctr + 1, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    left -= k;
  }
  if (unfinished) *unfinished = g.unfinished;
  if (!o) return CVR_OK;
  FrameOut fo;
  const cvr_status st = bind_frame_output(c, o, g.npix, fo);
  if (st != CVR_OK) return st;
  // the store adds the total up into a device output only: a host output's is
  // read back from the rounds' own counter
  if (!o->on_device) fo.d_total = nullptr;
  HIP_TRY(c, launch_crtgt_store(g.q, g.st, fo.d_out, fo.d_samples, fo.d_total, fo.half, s));
  if (!o->on_device) fo.d_total = g.st.ctr + 2;
  return frame_output_finish(c, o, fo, s);
}

extern "C" {
#pragma GCC visibility push(default)

void cvr_crtgt_params_default(cvr_crtgt_params* p) {
  if (!p) return;
  *p = cvr_crtgt_params{};
  p->ka = 0.5f; p->kd = 0.5f; p->ks = 0.8f; p->shininess = 30.0f;   // renderingparameters.cpp:23-26
  default_light(&p->light);
  p->light_gap = 1.0f;    // m_u_light_ray_initial_step (:35)
  p->light_step = 0.5f;   // m_u_light_ray_step_size (:36)
}

cvr_status cvr_crtgt_begin(cvr_ctx* ctx, const cvr_frame* f, const cvr_crtgt_params* p, const float* occ_rays,
                           int n_occ, const float* sdw_rays, int n_sdw) {
  Ctx* c = reinterpret_cast<Ctx*>(ctx);
  if (!c) return CVR_ERR_ARG;
  NO_GROUP(c, "cvr_crtgt_begin");
  return crtgt_begin(c, "cvr_crtgt_begin", f, p, occ_rays, n_occ, sdw_rays, n_sdw);
}

cvr_status cvr_crtgt_advance(cvr_ctx* ctx, int max_samples, const cvr_output* out,
                             unsigned long long* unfinished_pixels) {
  Ctx* c = reinterpret_cast<Ctx*>(ctx);
  if (!c) return CVR_ERR_ARG;
  NO_GROUP(c, "cvr_crtgt_advance");
  return crtgt_advance(c, "cvr_crtgt_advance", max_samples, out, unfinished_pixels);
}

// RC1PConeLightGroundTruthSteps::Update, then RedrawFrameTexture until no pixel's
// state says "unfinished" (crtgtrenderer.cpp:272-320).
cvr_status cvr_render_crtgt(cvr_ctx* ctx, const cvr_frame* f, const cvr_crtgt_params* p, const float* occ_rays,
                            int n_occ, const float* sdw_rays, int n_sdw, const cvr_output* out) {
  Ctx* c = reinterpret_cast<Ctx*>(ctx);
  if (!c) return CVR_ERR_ARG;
  NO_GROUP(c, "cvr_render_crtgt");
  if (!out || !out->rgba) return fail(c, CVR_ERR_ARG, "cvr_render_crtgt: null argument");
  if (out->format != CVR_FORMAT_RGBA32F && out->format != CVR_FORMAT_RGBA16F)
    return fail(c, CVR_ERR_ARG, "cvr_render_crtgt: unknown output format %d", out->format);
  const cvr_status st = crtgt_begin(c, "cvr_render_crtgt", f, p, occ_rays, n_occ, sdw_rays, n_sdw);
  if (st != CVR_OK) return st;
  return crtgt_advance(c, "cvr_render_crtgt", INT_MAX, out, nullptr);
}

#pragma GCC visibility pop
}  // extern "C"
