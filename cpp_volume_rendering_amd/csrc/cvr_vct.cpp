// cvr_vct.cpp — voxel cone tracing (rc1pvctsg): the supervoxel pyramid
// (vct_precompute.hip), the pre-integration table, the cone schedule and the
// VctArgs of a frame (vct.hip).
//
// The table (VCTPreProcessing::PreProcessPreIntegrationTable,
// preprocessingstages.cpp:147-202) is built here on the host, in double with
// libm's exp, as the reference builds it: a kernel would have to use another
// double exp than the CPU restatement it is compared with (DESIGN.md 5d'').
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "cvr_host.h"

using namespace cvr;

namespace cvr {

void vct_drop(Ctx* c, bool pyramid) {
  Ctx::Vct& v = c->vct;
  free_dev(v.d_table);
  v.tab_h = 0;
  v.opacity.clear();
  if (pyramid) {
    free_dev(v.d_pyr);
    free_dev(v.d_levels);
    free_dev(v.d_steps);
    v.nl = 0;
    v.texels = 0;
    v.max_stddev = 0.0;
    v.steps_cap = 0;
    v.steps_valid = 0;
  }
  v.bytes = v.texels * 4 + (v.d_levels ? sizeof(v.levels) : 0) + (size_t)v.steps_cap * sizeof(VctStep);
}

// OpacityGaussianEvaluation(iw, ih) for one row ih >= 1 (:153-173): the weights
// W(i, mean) = nf * exp(-((i - mean) * (i - mean)) / (2 sd sd)) depend on the
// integer i - mean alone, so the row computes each of them once; the operands of
// every operation are those of the reference's loop, hence its bits.
void vct_table_row(const float* opc, int w, int ih, float* row) {
  if (!(std::fabs((double)ih) > 0.0001)) {
    for (int iw = 0; iw < w; iw++) row[iw] = (float)(double)opc[iw];   // GetOpc(mean, 255)
    return;
  }
  const double sd = (double)ih;
  const double nf = 1.0 / (sd * std::sqrt(2.0 * 3.14159265358979323846264338327950288));
  // `for (int i = 0; i < dens_val; i++)` with int dens_val = GetMaxDensity() = 255 (:155-161):
  // i = 0 .. 254, so the TF's last entry (density 255) is never integrated
  const int n = w;
  std::vector<double> W((size_t)2 * w);
  for (int dlt = -(w - 1); dlt <= n - 1; dlt++) {
    const double x = (double)dlt;
    W[(size_t)(dlt + w)] = nf * std::exp(-(x * x) / (2.0 * sd * sd));
  }
  for (int iw = 0; iw < w; iw++) {
    double sg = 0.0, sw = 0.0;
    for (int i = 0; i < n; i++) {
      const double wt = W[(size_t)(i - iw + w)];
      sg += wt * (double)opc[i];
      sw += wt;
    }
    row[iw] = (float)(sg / sw);
  }
}

static cvr_status build_pyramid(Ctx* c, const char* who) {
  Ctx::Vct& v = c->vct;
  if (!c->d_vox) return fail(c, CVR_ERR_STATE, "%s: no volume", who);
  if (c->bpv != 1)
    return fail(c, CVR_ERR_ARG, "%s: voxel cone tracing supports 1-byte volumes only (the reference scales "
                                "the mean by 255 whatever the data's range)", who);
  if (v.nl) return CVR_OK;
  // the level chain (:62-69, 113-119): halve until a dimension reaches 0
  VctLevel lv[kMaxVctLevels] = {};
  int nl = 0;
  size_t texels = 0, upper = 0;
  for (int w = c->N[0], h = c->N[1], d = c->N[2]; w >= 1 && h >= 1 && d >= 1 && nl < kMaxVctLevels;
       w /= 2, h /= 2, d /= 2, nl++) {
    VctLevel& L = lv[nl];
    L.off = (int)texels;
    L.d[0] = w; L.d[1] = h; L.d[2] = d;
    for (int i = 0; i < 3; i++) {
      L.s[i] = (float)L.d[i] / ((float)c->N[i] * c->scale[i]);   // d / G, as the extinction pyramid
      L.m[i] = (float)(L.d[i] - 1);
    }
    const size_t n = (size_t)w * h * d;
    texels += n;
    if (nl) upper += n;
    if (texels >= ((size_t)1 << 31)) return fail(c, CVR_ERR_ARG, "%s: volume too large for the pyramid", who);
  }
  QUIESCE(c);
  HIP_TRY(c, hipMalloc((void**)&v.d_pyr, texels * 4));
  double* scratch = nullptr;
  unsigned long long* d_max = nullptr;
  hipError_t e = hipMalloc((void**)&v.d_levels, sizeof(lv));
  if (e == hipSuccess) e = hipMalloc((void**)&scratch, std::max<size_t>(upper, 1) * sizeof(double));
  if (e == hipSuccess) e = hipMalloc((void**)&d_max, sizeof(unsigned long long));
  if (e == hipSuccess) e = hipMemcpyAsync(v.d_levels, lv, sizeof(lv), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipMemsetAsync(d_max, 0, sizeof(unsigned long long), c->stream);
  if (e == hipSuccess) e = launch_vct_pyramid(*c, lv, nl, v.d_pyr, scratch, d_max, c->stream);
  unsigned long long bits = 0;
  if (e == hipSuccess) e = hipMemcpyAsync(&bits, d_max, sizeof(bits), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  (void)hipFree(scratch);
  (void)hipFree(d_max);
  if (e != hipSuccess) {
    free_dev(v.d_pyr);
    free_dev(v.d_levels);
    char what[64];
    std::snprintf(what, sizeof(what), "%s: pyramid", who);
    return fail_hip(c, what, e);
  }
  std::memcpy(v.levels, lv, sizeof(lv));
  v.nl = nl;
  v.texels = texels;
  std::memcpy(&v.max_stddev, &bits, sizeof(double));
  v.builds++;
  v.steps_valid = 0;
  v.bytes = texels * 4 + sizeof(lv) + (size_t)v.steps_cap * sizeof(VctStep);
  return CVR_OK;
}

static cvr_status build_table(Ctx* c, const char* who) {
  Ctx::Vct& v = c->vct;
  if (v.d_table) return CVR_OK;
  const int w = CVR_VCT_TABLE_WIDTH;
  const int h = (int)std::ceil(v.max_stddev);   // :184
  if (h < 1)
    return fail(c, CVR_ERR_ARG, "%s: the volume's maximum standard deviation is 0 (a pre-integration "
                                "table of height 0)", who);
  std::vector<uint16_t> tab((size_t)w * h);
  std::vector<float> row((size_t)w);
  for (int ih = 0; ih < h; ih++) {
    vct_table_row(v.opacity.data(), w, ih, row.data());
    for (int iw = 0; iw < w; iw++) tab[(size_t)ih * w + iw] = to_half_bits(row[iw]);   // GL_R16F
  }
  QUIESCE(c);
  HIP_TRY(c, hipMalloc((void**)&v.d_table, tab.size() * 2));
  const hipError_t e = hipMemcpy(v.d_table, tab.data(), tab.size() * 2, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    free_dev(v.d_table);
    return fail(c, CVR_ERR_HIP, "%s: table: %s", who, hipGetErrorString(e));
  }
  v.tab_h = h;
  v.bytes += tab.size() * 2;
  return CVR_OK;
}

}  // namespace cvr

extern "C" {
#pragma GCC visibility push(default)

void cvr_vct_params_default(cvr_vct_params* p) {
  if (!p) return;
  *p = cvr_vct_params{};
  p->ka = 0.5f; p->kd = 0.5f; p->ks = 0.8f; p->shininess = 30.0f;   // renderingparameters.cpp:23-26
  for (int i = 0; i < 3; i++) p->ispecular[i] = 1.0f;
  default_light(&p->light);
  // vctrenderer.cpp:33-43
  p->apply_occlusion = 1;
  p->apply_shadow = 1;
  p->cone_step = 2.0f;
  p->cone_step_increase_rate = 1.0f;
  p->cone_initial_step = 2.0f;
  p->cone_apex_angle_deg = 2.0f;
  p->apply_correction = 1;
  p->correction_factor = 2.0f;
  p->samples = 50;
}

cvr_status cvr_vct_set_opacity(cvr_ctx* ctx, const float* opacity, int n) {
  Ctx* c = reinterpret_cast<Ctx*>(ctx);
  if (c && c->group) return cvr::group_each(c, [&](cvr_ctx* _m) { return cvr_vct_set_opacity(_m, opacity, n); });
  if (!c) return CVR_ERR_ARG;
  if (!opacity || n != CVR_VCT_TABLE_WIDTH)
    return fail(c, CVR_ERR_ARG, "cvr_vct_set_opacity: need %d opacities", CVR_VCT_TABLE_WIDTH);
  for (int i = 0; i < n; i++)
    if (!std::isfinite(opacity[i])) return fail(c, CVR_ERR_ARG, "cvr_vct_set_opacity: opacity %d is not finite", i);
  QUIESCE(c);   // frames in flight read the table dropped below
  vct_drop(c, false);
  c->vct.opacity.assign(opacity, opacity + n);
  return CVR_OK;
}

cvr_status cvr_vct_precompute(cvr_ctx* ctx) {
  Ctx* c = reinterpret_cast<Ctx*>(ctx);
  if (c && c->group) return cvr::group_each(c, [&](cvr_ctx* _m) { return cvr_vct_precompute(_m); });
  if (!c) return CVR_ERR_ARG;
  HIP_TRY(c, hipSetDevice(c->device));
  cvr_status st = build_pyramid(c, "cvr_vct_precompute");
  if (st != CVR_OK || c->vct.opacity.empty()) return st;
  return build_table(c, "cvr_vct_precompute");
}

cvr_status cvr_vct_info(cvr_ctx* ctx, cvr_vct_pyramid_info* out) {
  Ctx* c = reinterpret_cast<Ctx*>(ctx);
  if (c && c->group) return cvr::group_call_root(c, [&](cvr_ctx* _m) { return cvr_vct_info(_m, out); });
  if (!c || !out) return CVR_ERR_ARG;
  *out = cvr_vct_pyramid_info{};
  out->levels = c->vct.nl;
  for (int l = 0; l < c->vct.nl; l++)
    for (int i = 0; i < 3; i++) out->dims[l][i] = c->vct.levels[l].d[i];
  out->max_stddev = c->vct.max_stddev;
  out->table_width = c->vct.tab_h ? CVR_VCT_TABLE_WIDTH : 0;
  out->table_height = c->vct.tab_h;
  return CVR_OK;
}

cvr_status cvr_vct_read_pyramid(cvr_ctx* ctx, int level, float* out_rg) {
  Ctx* c = reinterpret_cast<Ctx*>(ctx);
  if (c && c->group) return cvr::group_call_root(c, [&](cvr_ctx* _m) { return cvr_vct_read_pyramid(_m, level, out_rg); });
  if (!c || !out_rg) return CVR_ERR_ARG;
  if (!c->vct.nl) return fail(c, CVR_ERR_STATE, "cvr_vct_read_pyramid: no pyramid built");
  if (level < 0 || level >= c->vct.nl) return fail(c, CVR_ERR_ARG, "cvr_vct_read_pyramid: no level %d", level);
  const VctLevel& L = c->vct.levels[level];
  const size_t n = (size_t)L.d[0] * L.d[1] * L.d[2];
  std::vector<uint32_t> raw(n);
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipMemcpy(raw.data(), c->vct.d_pyr + L.off, n * 4, hipMemcpyDeviceToHost));
  for (size_t i = 0; i < n; i++) {
    out_rg[2 * i] = half_to_float_host((uint16_t)(raw[i] & 0xffffu));
    out_rg[2 * i + 1] = half_to_float_host((uint16_t)(raw[i] >> 16));
  }
  return CVR_OK;
}

cvr_status cvr_vct_read_table(cvr_ctx* ctx, float* out) {
  Ctx* c = reinterpret_cast<Ctx*>(ctx);
  if (c && c->group) return cvr::group_call_root(c, [&](cvr_ctx* _m) { return cvr_vct_read_table(_m, out); });
  if (!c || !out) return CVR_ERR_ARG;
  if (!c->vct.d_table) return fail(c, CVR_ERR_STATE, "cvr_vct_read_table: no table built");
  const size_t n = (size_t)CVR_VCT_TABLE_WIDTH * c->vct.tab_h;
  std::vector<uint16_t> raw(n);
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipMemcpy(raw.data(), c->vct.d_table, n * 2, hipMemcpyDeviceToHost));
  for (size_t i = 0; i < n; i++) out[i] = half_to_float_host(raw[i]);
  return CVR_OK;
}

cvr_status cvr_render_vct(cvr_ctx* ctx, const cvr_frame* f, const cvr_vct_params* p, const cvr_output* o) {
  Ctx* c = reinterpret_cast<Ctx*>(ctx);
  if (c && c->group)
    return cvr::group_render(c, f, 1, o, [&](cvr_ctx* _m, const cvr_frame* mf, int, const cvr_output* mo) {
      return cvr_render_vct(_m, mf, p, mo);
    });
  if (!c) return CVR_ERR_ARG;
  const char* who = "cvr_render_vct";
  if (!f || !p || !o || !o->rgba) return fail(c, CVR_ERR_ARG, "%s: null argument", who);
  cvr_status st = check_frame_output(c, who, f, o);
  if (st != CVR_OK) return st;
  if (c->native_exp) return fail(c, CVR_ERR_ARG, "%s: not available with option native_exp", who);
  if (p->samples < 0 || p->samples > CVR_VCT_MAX_SAMPLES)
    return fail(c, CVR_ERR_ARG, "%s: samples must be in [0, %d]", who, CVR_VCT_MAX_SAMPLES);
  if (!(p->cone_step > 0.0f)) return fail(c, CVR_ERR_ARG, "%s: the cone step must be positive", who);
  if (!(p->cone_step_increase_rate >= 1.0f))
    return fail(c, CVR_ERR_ARG, "%s: the cone step increase rate must be >= 1", who);
  if (!(p->cone_apex_angle_deg > 0.0f && p->cone_apex_angle_deg < 90.0f))
    return fail(c, CVR_ERR_ARG, "%s: the cone apex angle must lie in (0, 90) degrees", who);
  if (!c->d_cells || !c->d_tf) return fail(c, CVR_ERR_STATE, "%s: no volume or TF", who);
  if (c->bpv == 1 && c->vct.opacity.empty())
    return fail(c, CVR_ERR_STATE, "%s: no TF opacities (cvr_vct_set_opacity after cvr_set_transfer_function)", who);
  const bool phong = p->apply_gradient_shading != 0;
  if (phong && !c->d_grad) return fail(c, CVR_ERR_STATE, "%s: Phong needs cvr_set_gradient", who);
  HIP_TRY(c, hipSetDevice(c->device));
  if ((st = build_pyramid(c, who)) != CVR_OK) return st;
  if ((st = build_table(c, who)) != CVR_OK) return st;
  Ctx::Vct& v = c->vct;

  // the cone schedule of these parameters (vct.hip); the uniforms of Update
  // (vctrenderer.cpp:145-170) in float
  const float tan_apex = std::tan(p->cone_apex_angle_deg * 3.14159265358979323846f / 180.0f);
  const float corr = (float)(p->apply_correction ? 1 : 0) * p->correction_factor;   // corr_fact (:97)
  const float key[8] = {p->cone_initial_step, p->cone_step, p->cone_step_increase_rate, tan_apex, corr,
                        (float)p->samples, (float)c->filter_bits, (float)v.builds};
  if (!v.steps_valid || std::memcmp(key, v.steps_key, sizeof(key)) != 0) {
    QUIESCE(c);   // frames in flight on any stream read the schedule replaced below
    const int need = std::max(p->samples, 1);
    if (need > v.steps_cap) {
      free_dev(v.d_steps);
      v.bytes -= (size_t)v.steps_cap * sizeof(VctStep);
      v.steps_cap = 0;
      HIP_TRY(c, hipMalloc((void**)&v.d_steps, (size_t)need * sizeof(VctStep)));
      v.steps_cap = need;
      v.bytes += (size_t)need * sizeof(VctStep);
    }
    v.steps_valid = 0;
    HIP_TRY(c, launch_vct_schedule(v.d_levels, v.nl, p->cone_initial_step, p->cone_step,
                                   p->cone_step_increase_rate, tan_apex, corr, p->samples, c->filter_bits,
                                   v.d_steps, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    std::memcpy(v.steps_key, key, sizeof(key));
    v.steps_valid = 1;
  }

  cvr::VctArgs Q{};
  int ntiles = 0;
  size_t npix = 0;
  fill_frame_args(c, f, p->step, Q.a, ntiles, npix);
  Q.a.filter_bits = c->filter_bits;
  if ((st = enable_cell_skip(c, Q.a, 1)) != CVR_OK) return st;   // the per-cell skip flags in the count / emit march
  Q.a.out_half = o->format == CVR_FORMAT_RGBA16F;
  set_phong_constants(Q.a, p->ka, p->kd, p->ks, p->shininess, p->ispecular, p->light.position);
  grid_size(c, Q.G);
  Q.apply_shadow = p->apply_shadow != 0;
  Q.phong = phong;
  set_gated_weights(Q, p->apply_occlusion != 0, Q.apply_shadow != 0, p->ka, p->kd, p->ks);   // ShadeSample (:150-161)
  Q.samples = p->samples;
  Q.tab_wi = CVR_VCT_TABLE_WIDTH;
  Q.tab_hi = v.tab_h;
  Q.tab_w = (float)Q.tab_wi;
  Q.tab_h = (float)Q.tab_hi;
  Q.max_density = 255.0f;                  // (float)GetMaxDensity() (:166)
  Q.max_stddev = (float)v.max_stddev;      // (:169)
  const cvr::VctData data{v.d_pyr, v.d_table, v.d_steps};
  return render_shaded(c, o, ntiles, npix, [&](float4* out, uint32_t* smp, unsigned long long* shade,
                                                unsigned long long* ts, hipStream_t s) {
    return cvr::launch_vct(*c, Q, data, out, smp, shade, ts, s);
  });
}

#pragma GCC visibility pop
}  // extern "C"
