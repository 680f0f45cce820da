// cvr_dos.cpp — directional-occlusion shading (rc1pdosct): the extinction
// pyramid, the cone tables and the DosArgs of a frame (dos.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "cvr_host.h"

using namespace cvr;

static bool same_cone(const cvr_cone_params& a, const cvr_cone_params& b) {
  return std::memcmp(&a, &b, sizeof(a)) == 0;
}

namespace cvr {

// The pyramid goes with the volume or the table it was built from, and with it
// what was sized or computed for it: the level table and the cone tables (whose
// sections depend on sigma0).  All of them are built again on the next use.
void ext_drop(Ctx* c) {
  Ctx::Ext& x = c->ext;
  free_dev(x.d_ext);
  free_dev(x.d_cells);
  free_dev(x.d_levels);
  free_dev(x.d_cones);
  x.levels = 0;
  x.cone_valid = 0;
}

// The cone parameters a frame traces with: covered distance <= 0 -> the volume
// diagonal * 0.50 / 0.75 (GetDiagonal in double, dosrcrenderer.cpp:112-113)
void resolve_cone_params(const Ctx* c, const cvr_dos_params* p, cvr_cone_params cp[2]) {
  cp[0] = p->occlusion;
  cp[1] = p->shadow;
  double vw = c->N[0] * (double)c->scale[0], vh = c->N[1] * (double)c->scale[1],
         vd = c->N[2] * (double)c->scale[2];
  const double diag = std::sqrt(vw * vw + vh * vh + vd * vd);
  if (!(cp[0].covered_distance > 0.0f)) cp[0].covered_distance = (float)(diag * 0.50f);
  if (!(cp[1].covered_distance > 0.0f)) cp[1].covered_distance = (float)(diag * 0.75f);
}

// The DosArgs of a frame: the checks every DOS entry point shares, the cone tables
// (rebuilt and uploaded when the cone parameters changed) and the shaders' uniforms.
// o == null: no frame is rendered (cvr_compute_light_cache), so the output and
// viewport checks and the gradient requirement do not apply.  need_cones: the
// entry point traces cones (needs the extinction pyramid and the tables).
cvr_status dos_prepare(Ctx* c, const char* who, const cvr_frame* f, const cvr_dos_params* p,
                       const cvr_output* o, bool need_cones, cvr::DosArgs& Q, int& ntiles,
                       size_t& npix, cvr_cone_params cp[2]) {
  if (!f || !p) return fail(c, CVR_ERR_ARG, "%s: null argument", who);
  if (o) {
    const cvr_status st = check_frame_output(c, who, f, o);
    if (st != CVR_OK) return st;
  }
  if (!c->d_cells || !c->d_tf) return fail(c, CVR_ERR_STATE, "%s: no volume or TF", who);
  if (need_cones && !c->ext.d_ext) return fail(c, CVR_ERR_STATE, "%s: needs cvr_set_extinction_volume", who);
  const bool phong = o && p->apply_gradient_shading != 0;
  if (phong && !c->d_grad) return fail(c, CVR_ERR_STATE, "%s: Phong needs cvr_set_gradient", who);
  if (p->shadow_type < 0 || p->shadow_type > 2) return fail(c, CVR_ERR_ARG, "%s: bad shadow type", who);
  HIP_TRY(c, hipSetDevice(c->device));

  resolve_cone_params(c, p, cp);
  if (need_cones &&
      (!c->ext.cone_valid || !same_cone(cp[0], c->ext.cone_key[0]) || !same_cone(cp[1], c->ext.cone_key[1]))) {
    for (int k = 0; k < 2; k++) {
      cvr_status st = cvr_build_cone_tables(&cp[k], c->ext.sigma0, &c->ext.cone_tab[k]);
      if (st != CVR_OK) return fail(c, st, "%s: cone tables (%s)", who, k ? "shadow" : "occlusion");
    }
    std::vector<float> up(2 * CVR_MAX_CONE_SECTIONS * 4, 0.0f);
    for (int k = 0; k < 2; k++)
      for (int i = 0; i < c->ext.cone_tab[k].n_sections; i++)
        for (int j = 0; j < 4; j++)   // GetConeSectionsInfoTex uploads RGBA16F
          up[((size_t)k * CVR_MAX_CONE_SECTIONS + i) * 4 + j] = half_round(c->ext.cone_tab[k].sections[i][j]);
    if (!c->ext.d_cones) HIP_TRY(c, hipMalloc((void**)&c->ext.d_cones, up.size() * sizeof(float)));
    QUIESCE(c);   // DOS frames in flight on other streams read d_cones
    HIP_TRY(c, hipMemcpy(c->ext.d_cones, up.data(), up.size() * sizeof(float), hipMemcpyHostToDevice));
    c->ext.cone_key[0] = cp[0];
    c->ext.cone_key[1] = cp[1];
    c->ext.cone_valid = 1;
  }

  Q = cvr::DosArgs{};
  fill_frame_args(c, f, p->step, Q.a, ntiles, npix);
  Q.a.filter_bits = c->filter_bits;   // GL_LINEAR weights of every fetch (CVR-SPEC-8 at 8)
  if (o) {   // the per-cell skip flags in the count / emit march
    const cvr_status st = enable_cell_skip(c, Q.a, 1);
    if (st != CVR_OK) return st;
  }
  Q.a.out_half = o && o->format == CVR_FORMAT_RGBA16F;
  // Phong ambient/diffuse/specular weights of the surface term
  set_phong_constants(Q.a, p->ka, p->kd, p->ks, p->shininess, p->ispecular, p->light.position);
  grid_size(c, Q.G);
  Q.ext_levels = c->ext.levels;
  Q.levels = c->ext.d_levels;
  Q.apply_occlusion = p->apply_occlusion != 0;
  Q.apply_shadow = p->apply_shadow != 0;
  Q.shadow_type = p->shadow_type;
  Q.phong = phong;
  set_gated_weights(Q, Q.apply_occlusion != 0, Q.apply_shadow != 0, p->ka, p->kd, p->ks);   // ShadeSample (:607-656)
  for (int i = 0; i < 3; i++) {
    Q.lfwd[i] = p->light.forward[i];
    Q.lup[i] = p->light.up[i];
    Q.lright[i] = p->light.right[i];
  }
  // SpotLightMaxAngle: glm::cos(glm::pi<float>() * angle / 180.f) (dosrcrenderer.cpp:158)
  Q.spot_cos = std::cos(3.14159265358979323846f * p->light.spot_angle_deg / 180.0f);
  Q.zero_skip = c->ext.finite;
  Q.count_taps = c->shade_counters ? 1 : 0;
  for (int k = 0; need_cones && k < 2; k++) {
    cvr::DosCone& C = k ? Q.sdw : Q.occ;
    const cvr_cone_tables& T = c->ext.cone_tab[k];
    for (int i = 0; i < 3; i++) C.counts[i] = T.counts[i];
    C.initial_step = T.initial_step;
    C.ray7w = T.ray7_adj_weight;
    C.ui_weight = T.ui_weight;
    for (int i = 0; i < 10; i++)
      for (int j = 0; j < 3; j++) C.axes[3 * i + j] = T.axes[i][j];
    C.sections = c->ext.d_cones + (size_t)k * CVR_MAX_CONE_SECTIONS;
    // exit tables: the sections' track and border scale, replaying the kernel's
    // float recurrence (track += interval) on the RGBA16F-rounded table
    float track = T.initial_step;
    int s0 = 0;
    for (int st = 0; st < 3; st++) {
      cvr::ConeStageExit& X = C.exit[st];
      X.nruns = 0;
      bool ok = Q.zero_skip != 0;
      for (int i = s0; i < s0 + T.counts[st]; i++) {
        const float mip = half_round(T.sections[i][1]);
        const float inv = std::ldexp(1.0f, -(2 * (int)mip + 1));
        if (!(mip >= 0.0f)) ok = false;
        if (X.nruns == 0 || inv != X.run_inv[X.nruns - 1]) {
          if (X.nruns == cvr::kMaxConeRuns) ok = false;
          else {
            X.run_first[X.nruns] = i;
            X.run_t[X.nruns] = track;
            X.run_inv[X.nruns] = inv;
            X.nruns++;
          }
        }
        track = track + half_round(T.sections[i][0]);
      }
      s0 += T.counts[st];
      X.end_s = s0;
      X.end_track = track;
      if (!ok) X.nruns = 0;
    }
  }

  return CVR_OK;
}

}  // namespace cvr

extern "C" {
#pragma GCC visibility push(default)

cvr_status cvr_set_extinction_volume(cvr_ctx* ctx, const float* tf_rgba, int n, const int res_in[3],
                                     float sigma0) {
  Ctx* c = reinterpret_cast<Ctx*>(ctx);
  if (c && c->group) return cvr::group_each(c, [&](cvr_ctx* _m) { return cvr_set_extinction_volume(_m, tf_rgba, n, res_in, sigma0); });
  if (!c) return CVR_ERR_ARG;
  if (!tf_rgba || n < 2 || n > cvr::kMaxTfLds)
    return fail(c, CVR_ERR_ARG, "cvr_set_extinction_volume: need 2 <= n <= 4096 TF entries");
  if (!c->d_cells) return fail(c, CVR_ERR_STATE, "cvr_set_extinction_volume: no volume set");
  int res[3] = {128, 128, 128};   // ExtinctionCoefficientVolume defaults (:10-15)
  if (res_in)
    for (int i = 0; i < 3; i++) res[i] = res_in[i];
  for (int i = 0; i < 3; i++)
    if (res[i] < 1 || res[i] > 4096) return fail(c, CVR_ERR_ARG, "cvr_set_extinction_volume: bad resolution");
  if (!(sigma0 > 0.0f)) sigma0 = 1.0f;
  int nl = 1;
  for (int m = std::max(res[0], std::max(res[1], res[2])); m > 1; m >>= 1) nl++;
  if (nl > cvr::kMaxExtLevels) return fail(c, CVR_ERR_ARG, "cvr_set_extinction_volume: too many levels");
  long long off[cvr::kMaxExtLevels + 1] = {0};
  for (int L = 0; L < nl; L++) {
    long long v = 1;
    for (int i = 0; i < 3; i++) v *= std::max(1, res[i] >> L);
    off[L + 1] = off[L] + v;
  }
  // the RGBA16F opacity TF (GenerateTexture_1D_RGBA, transferfunction1d.cpp:58-87)
  std::vector<float> q((size_t)n * 4);
  for (size_t i = 0; i < q.size(); i++) q[i] = half_round(tf_rgba[i]);
  QUIESCE(c);   // frames in flight on any stream read the state replaced below
  ext_drop(c);
  light_cache_drop(c);
  // cell8 texels are addressed with 32-bit byte offsets (16 B each)
  if (off[nl] > (1LL << 28)) return fail(c, CVR_ERR_ARG, "cvr_set_extinction_volume: resolution too large");
  cvr::ExtLevel lv[cvr::kMaxExtLevels] = {};
  for (int L = 0; L < nl; L++) {
    int d[3];
    for (int i = 0; i < 3; i++) d[i] = std::max(1, res[i] >> L);
    lv[L].off = (int)off[L];
    lv[L].dx = d[0]; lv[L].dy = d[1]; lv[L].dz = d[2];
    float G[3];
    grid_size(c, G);
    lv[L].sx = (float)d[0] / G[0];   // d / G, rounded once
    lv[L].sy = (float)d[1] / G[1];
    lv[L].sz = (float)d[2] / G[2];
    lv[L].mx = (float)(d[0] - 1);
    lv[L].my = (float)(d[1] - 1);
    lv[L].mz = (float)(d[2] - 1);
  }
  float4* d_tf = nullptr;
  HIP_TRY(c, hipMalloc((void**)&d_tf, (size_t)n * 16));
  hipError_t e = hipMemcpy(d_tf, q.data(), (size_t)n * 16, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMalloc((void**)&c->ext.d_ext, (size_t)off[nl] * sizeof(uint16_t));
  if (e == hipSuccess) e = hipMalloc((void**)&c->ext.d_cells, (size_t)off[nl] * sizeof(uint4));
  if (e == hipSuccess) e = hipMalloc((void**)&c->ext.d_levels, sizeof(lv));
  if (e == hipSuccess) e = hipMemcpy(c->ext.d_levels, lv, sizeof(lv), hipMemcpyHostToDevice);
  if (e == hipSuccess)
    e = cvr::launch_ext_volume(*c, d_tf, n, res, sigma0, nl, off, c->ext.d_ext, c->ext.d_cells, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  (void)hipFree(d_tf);
  if (e != hipSuccess) {
    ext_drop(c);
    return fail_hip(c, "cvr_set_extinction_volume", e);
  }
  for (int i = 0; i < 3; i++) c->ext.res[i] = res[i];
  c->ext.levels = nl;
  {   // level values are Gaussian averages of these opacities: all < 1 -> finite tau
    bool fin = true;
    for (size_t i = 3; i < q.size(); i += 4) fin = fin && q[i] >= 0.0f && q[i] < 1.0f;
    c->ext.finite = fin ? 1 : 0;
  }
  for (int L = 0; L <= nl; L++) c->ext.off[L] = off[L];
  c->ext.sigma0 = sigma0;
  return CVR_OK;
}

cvr_status cvr_copy_extinction_level(cvr_ctx* ctx, int level, float* out, int dims[3],
                                     int* n_levels) {
  Ctx* c = reinterpret_cast<Ctx*>(ctx);
  if (c && c->group) return cvr::group_call_root(c, [&](cvr_ctx* _m) { return cvr_copy_extinction_level(_m, level, out, dims, n_levels); });
  if (!c) return CVR_ERR_ARG;
  if (n_levels) *n_levels = c->ext.levels;
  if (!c->ext.d_ext) return fail(c, CVR_ERR_STATE, "cvr_copy_extinction_level: no extinction volume");
  if (level < 0 || level >= c->ext.levels) return fail(c, CVR_ERR_ARG, "cvr_copy_extinction_level: bad level");
  int d[3];
  for (int i = 0; i < 3; i++) d[i] = std::max(1, c->ext.res[i] >> level);
  if (dims) for (int i = 0; i < 3; i++) dims[i] = d[i];
  if (!out) return CVR_OK;
  const size_t nv = (size_t)d[0] * d[1] * d[2];
  std::vector<uint16_t> h(nv);
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipMemcpy(h.data(), c->ext.d_ext + c->ext.off[level], nv * 2, hipMemcpyDeviceToHost));
  for (size_t i = 0; i < nv; i++) out[i] = half_to_float_host(h[i]);
  return CVR_OK;
}

cvr_status cvr_render_dosct(cvr_ctx* ctx, const cvr_frame* f, const cvr_dos_params* p,
                            const cvr_output* o) {
  Ctx* c = reinterpret_cast<Ctx*>(ctx);
  if (c && c->group)
    return cvr::group_render(c, f, 1, o, [&](cvr_ctx* _m, const cvr_frame* mf, int, const cvr_output* mo) {
      return cvr_render_dosct(_m, mf, p, mo);
    });
  if (!c) return CVR_ERR_ARG;
  if (!o) return fail(c, CVR_ERR_ARG, "cvr_render_dosct: null argument");
  cvr::DosArgs Q;
  int ntiles = 0;
  size_t npix = 0;
  cvr_cone_params cp[2];
  const cvr_status st = dos_prepare(c, "cvr_render_dosct", f, p, o, true, Q, ntiles, npix, cp);
  if (st != CVR_OK) return st;
  return render_shaded(c, o, ntiles, npix, [&](float4* out, uint32_t* smp, unsigned long long* shade,
                                                unsigned long long* ts, hipStream_t st) {
    return cvr::launch_dos(*c, Q, out, smp, shade, ts, st);
  });
}

#pragma GCC visibility pop
}  // extern "C"
