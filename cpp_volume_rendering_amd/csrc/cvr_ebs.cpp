// cvr_ebs.cpp — extinction-based shading (rc1pextbsd): the summed-area table of
// the extinction and the EbsArgs of a frame (sat.hip, ebs.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "cvr_host.h"

using namespace cvr;

namespace cvr {

// The whole SAT (a new volume, another grid, a failed build), or only the build's
// double grid and / or the cell4 copy, which go while the SAT stays.
void sat_drop(Ctx* c, int parts) {
  Ctx::Sat& t = c->sat;
  if (parts & kSatScratch) free_dev(t.d_scratch);
  if (parts & kSatCells) free_dev(t.d_cells);
  if (parts == kSatAll) {
    free_dev(t.d_sat);
    t.dims[0] = t.dims[1] = t.dims[2] = 0;
  }
}

// dir_cone_max_distance = 0.75f * Dv (ebsrenderer.cpp:98-105, float arithmetic)
// unless the caller gives one
float ebs_max_distance(const Ctx* c, const cvr_ebs_params* p) {
  if (p->shadow_max_distance > 0.0f) return p->shadow_max_distance;
  const float vw = (float)((double)c->N[0] * (double)c->scale[0]);
  const float vh = (float)((double)c->N[1] * (double)c->scale[1]);
  const float vd = (float)((double)c->N[2] * (double)c->scale[2]);
  return 0.75f * std::sqrt((vw * vw + vh * vh) + vd * vd);
}

// The EbsArgs of a frame: the checks the EBS entry points share and the shader's
// uniforms.  f == o == null: no frame is rendered (cvr_compute_light_cache_extbsd),
// so the frame, output and gradient checks do not apply and of Q.a only the
// volume box, the light and filter_bits are filled.
cvr_status ebs_prepare(Ctx* c, const char* who, const cvr_frame* f, const cvr_ebs_params* p,
                       const cvr_output* o, cvr::EbsArgs& Q, int& ntiles, size_t& npix) {
  if (!p || (o && !f)) return fail(c, CVR_ERR_ARG, "%s: null argument", who);
  if (o) {
    const cvr_status st = check_frame_output(c, who, f, o);
    if (st != CVR_OK) return st;
  }
  if (c->filter_bits && c->sat_layout != 0)
    return fail(c, CVR_ERR_ARG, "%s: filter_bits %d needs sat_layout 0 (the cell4 copy)", who,
                c->filter_bits);
  if (!c->d_cells || (o && !c->d_tf)) return fail(c, CVR_ERR_STATE, "%s: no volume or TF", who);
  if (!c->sat.d_sat) return fail(c, CVR_ERR_STATE, "%s: needs cvr_set_extinction_sat", who);
  if (c->sat_layout == 0 && !c->sat.d_cells) {   // switched back to the cell4 copy: build it
    const int w = c->sat.dims[0], h = c->sat.dims[1], d = c->sat.dims[2];
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMalloc((void**)&c->sat.d_cells, cvr::sat_cells_float4s(w, h, d) * sizeof(float4)));
    const hipError_t e = cvr::launch_sat_cells(*c, c->sat.d_sat, c->sat.d_cells, c->stream);
    if (e != hipSuccess) {   // never leave an unbuilt copy behind for the next frame to read
      sat_drop(c, kSatCells);
      return fail(c, CVR_ERR_HIP, "%s: cell4 SAT build: %s", who, hipGetErrorString(e));
    }
  }
  const bool phong = o && p->apply_gradient_shading != 0;
  if (phong && !c->d_grad) return fail(c, CVR_ERR_STATE, "%s: Phong needs cvr_set_gradient", who);
  if (p->shadow_type < 0 || p->shadow_type > 1) return fail(c, CVR_ERR_ARG, "%s: bad shadow type", who);
  if (p->apply_occlusion && p->occlusion_shells < 1)
    return fail(c, CVR_ERR_ARG, "%s: need >= 1 occlusion shell", who);
  if (p->apply_shadow && !(p->shadow_sample_interval > 0.0f))
    return fail(c, CVR_ERR_ARG, "%s: shadow sample interval must be positive", who);
  HIP_TRY(c, hipSetDevice(c->device));

  Q = cvr::EbsArgs{};
  ntiles = 0;
  npix = 0;
  if (o) {
    fill_frame_args(c, f, p->step, Q.a, ntiles, npix);
  } else {
    for (int i = 0; i < 3; i++) {
      Q.a.half_grid[i] = ((float)c->N[i] * c->scale[i]) * 0.5f;   // as fill_frame_args
      Q.a.N[i] = c->N[i];
    }
  }
  Q.a.filter_bits = c->filter_bits;   // GL_LINEAR weights of every fetch (CVR-SPEC-8 at 8)
  if (o) {   // the per-cell skip flags in the count / emit march
    const cvr_status st = enable_cell_skip(c, Q.a, 1);
    if (st != CVR_OK) return st;
  }
  Q.a.out_half = o && o->format == CVR_FORMAT_RGBA16F;
  set_phong_constants(Q.a, p->ka, p->kd, p->ks, p->shininess, p->ispecular, p->light_pos);
  grid_size(c, Q.G);
  for (int i = 0; i < 3; i++) {
    Q.S[i] = c->scale[i];
    Q.inv_vs[i] = 1.0f / (Q.G[i] + Q.S[i] * 2.0f);        // inv_vol_scaled (:75)
    Q.sat_dims[i] = c->sat.dims[i];
    Q.sat_pz = (uint32_t)c->sat.dims[0] * (uint32_t)c->sat.dims[1];
    Q.nsat[i] = (float)c->sat.dims[i];
    Q.nsat_m1[i] = (float)(c->sat.dims[i] - 1);
    Q.min_sat[i] = Q.S[i] * 0.5f;                        // MinSATPosition (:66)
    Q.max_sat[i] = Q.G[i] + Q.S[i] * 1.5f;               // MaxSATPosition (:67)
    Q.lfwd[i] = p->light_forward[i];
  }
  Q.apply_occlusion = p->apply_occlusion != 0;
  Q.occ_shells = p->occlusion_shells;
  Q.occ_radius = p->occlusion_radius;
  {   // ExtinctionAmbientOcclusion's per-shell weights (:117-144), float as the shader
    const float R = Q.occ_radius;
    for (int i = 0; i < cvr::EbsArgs::kMaxAoShells; i++) {
      const float r1 = i == 0 ? R : R * (float)(i + 1);
      Q.ao_w[i] = 1.0f / (r1 * r1);
    }
    const float rshi = R * (float)Q.occ_shells;
    Q.ao_wa = 1.0f / (rshi * rshi);
  }
  Q.apply_shadow = p->apply_shadow != 0;
  Q.shadow_type = p->shadow_type;
  Q.phong = phong;
  // DirSdwConeAngle = (float)(angle * pi / 180.0) (ebsrenderer.cpp:161); its cos / sin
  const float ang = (float)(p->shadow_cone_angle_deg * 3.14159265358979323846 / 180.0);
  Q.p_cs = std::cos(ang); Q.p_sn = std::sin(ang);
  Q.n_cs = std::cos(-ang); Q.n_sn = std::sin(-ang);
  Q.recip_cone = std::fabs(p->shadow_cone_angle_deg) <= 44.0f;
  Q.interval = p->shadow_sample_interval;
  Q.initial_step = p->shadow_initial_step;
  Q.ui_weight = p->shadow_ui_weight;
  Q.max_distance = ebs_max_distance(c, p);
  set_gated_weights(Q, Q.apply_occlusion != 0, Q.apply_shadow != 0, p->ka, p->kd, p->ks);   // ShadeSample (:502-518)
  return CVR_OK;
}

}  // namespace cvr

extern "C" {
#pragma GCC visibility push(default)

cvr_status cvr_set_extinction_sat(cvr_ctx* ctx, const float* ext_lut, int lut_n) {
  Ctx* c = reinterpret_cast<Ctx*>(ctx);
  if (c && c->group) return cvr::group_each(c, [&](cvr_ctx* _m) { return cvr_set_extinction_sat(_m, ext_lut, lut_n); });
  if (!c) return CVR_ERR_ARG;
  if (!c->d_vox) return fail(c, CVR_ERR_STATE, "cvr_set_extinction_sat: no volume set");
  const int nv = c->bpv == 1 ? 256 : 65536;
  if (!ext_lut || lut_n != nv)
    return fail(c, CVR_ERR_ARG, "cvr_set_extinction_sat: need one extinction per voxel value (%d)", nv);
  const int w = c->N[0] + 2, h = c->N[1] + 2, d = c->N[2] + 2;
  const size_t cells = (size_t)w * h * d;
  // the shader indexes texels (plus one cell4 plane) with 32-bit / 24-bit products
  if (w > 4096 || h > 4096 || d > 4096 || cells >= ((size_t)1 << 31))
    return fail(c, CVR_ERR_ARG, "cvr_set_extinction_sat: volume too large for the SAT");
  QUIESCE(c);   // frames in flight on any stream read the state replaced below
  light_cache_drop(c);   // an EBS light cache holds this SAT's occlusion and shadow
  // Same grid as the last build (a TF change): rebuild into the existing buffers.
  // Freeing and re-allocating the ~30 GB of a 1024^3 SAT costs seconds.
  const bool same = c->sat.d_sat && c->sat.dims[0] == w && c->sat.dims[1] == h && c->sat.dims[2] == d;
  if (!same) sat_drop(c);
  float* d_lut = nullptr;
  hipError_t e = hipMalloc((void**)&d_lut, (size_t)nv * sizeof(float));
  if (e == hipSuccess) e = hipMemcpy(d_lut, ext_lut, (size_t)nv * sizeof(float), hipMemcpyHostToDevice);
  // the double recurrence's grid: kept with the SAT for rebuilds (sat_keep_scratch,
  // 8.6 GB at 1024^3) or allocated for this build only
  if (e == hipSuccess && !c->sat.d_scratch) e = hipMalloc(&c->sat.d_scratch, cells * sizeof(double));
  double* d_sd = (double*)c->sat.d_scratch;
  // the float SAT plus kSatPlainPadPlanes zero planes (the plain layout's clamped
  // +1 neighbours: cvr_sat_layout_check)
  const size_t pad_floats = cvr::sat_plain_floats(w, h, d) - cells;
  if (e == hipSuccess && !same) e = hipMalloc((void**)&c->sat.d_sat, cvr::sat_plain_floats(w, h, d) * sizeof(float));
  if (e == hipSuccess && !same) e = hipMemsetAsync(c->sat.d_sat + cells, 0, pad_floats * sizeof(float), c->stream);
  // GPU time of the two compute phases (option "sat_build_us"): the wall time of
  // this call also holds the allocations of ~50 GB at 1024^3
  hipEvent_t ev[4] = {};
  for (hipEvent_t& x : ev)
    if (e == hipSuccess) e = hipEventCreate(&x);
  if (e == hipSuccess) e = hipEventRecord(ev[0], c->stream);
  if (e == hipSuccess) e = cvr::launch_sat_build(*c, d_lut, d_sd, c->sat.d_sat, c->stream);
  if (e == hipSuccess) e = hipEventRecord(ev[1], c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  (void)hipFree(d_lut);
  if (!c->sat_keep_scratch) sat_drop(c, kSatScratch);
  // the cell4 copy only for the layout that reads it
  if (e == hipSuccess && c->sat_layout == 0 && !c->sat.d_cells)
    e = hipMalloc((void**)&c->sat.d_cells, cvr::sat_cells_float4s(w, h, d) * sizeof(float4));
  if (e == hipSuccess) e = hipEventRecord(ev[2], c->stream);
  if (e == hipSuccess && c->sat_layout == 0) e = cvr::launch_sat_cells(*c, c->sat.d_sat, c->sat.d_cells, c->stream);
  if (e == hipSuccess) e = hipEventRecord(ev[3], c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e == hipSuccess) {
    float a = 0.f, b = 0.f;
    if (hipEventElapsedTime(&a, ev[0], ev[1]) == hipSuccess &&
        hipEventElapsedTime(&b, ev[2], ev[3]) == hipSuccess)
      c->sat.build_us = (int)((a + b) * 1000.0f);
  }
  if (e == hipSuccess && c->sat_layout == 1) sat_drop(c, kSatCells);   // a copy from an earlier layout is stale now
  for (hipEvent_t x : ev)
    if (x) (void)hipEventDestroy(x);
  if (e != hipSuccess) {
    sat_drop(c);
    return fail_hip(c, "cvr_set_extinction_sat", e);
  }
  c->sat.dims[0] = w; c->sat.dims[1] = h; c->sat.dims[2] = d;
  return CVR_OK;
}

cvr_status cvr_sat_layout_check(const int dims[3], int layout, int pad_planes, unsigned long long out[4]) {
  if (!dims || !out || (layout != 0 && layout != 1)) return CVR_ERR_ARG;
  const long long w = dims[0], h = dims[1], d = dims[2];
  if (w < 1 || h < 1 || d < 1) return CVR_ERR_ARG;
  const int pad = pad_planes >= 0 ? pad_planes : cvr::kSatPlainPadPlanes;
  // bytes allocated: cell4 = float4 per texel of d + 1 planes (sat_cells_float4s);
  // plain = floats of d + pad planes (sat_plain_floats)
  const unsigned long long alloc = layout == 0 ? (unsigned long long)cvr::sat_cells_float4s((int)w, (int)h, (int)d) * 16ull
                                               : (unsigned long long)(w * h * (d + pad)) * 4ull;
  bool wrap = (w * h) >= (1ll << 24) || h >= (1ll << 24) || w >= (1ll << 24) || (d - 1) * h + (h - 1) >= (1ll << 24);
  unsigned long long end = 0;
  const uint32_t pz = (uint32_t)(w * h);
  for (int c = 0; c < 8; c++) {   // the clamped extremes of every axis
    const uint32_t tx = (c & 1) ? (uint32_t)(w - 1) : 0u, ty = (c & 2) ? (uint32_t)(h - 1) : 0u,
                   tz = (c & 4) ? (uint32_t)(d - 1) : 0u;
    const uint32_t idx = cvr::sat_texel_index(tx, ty, tz, (uint32_t)w, (uint32_t)h);
    const unsigned long long exact = ((unsigned long long)tz * h + ty) * w + tx;
    if (idx != exact) wrap = true;
    if (layout == 0) {
      for (unsigned long long e : {exact, exact + pz}) {
        if (e + 1 > 0xffffffffull) wrap = true;
        end = std::max(end, (e + 1) * 16ull);
      }
    } else {
      for (unsigned long long e : {exact, exact + w, exact + pz, exact + pz + w}) {
        if (e + 2 > 0xffffffffull) wrap = true;   // the 32-bit element index of the pair
        end = std::max(end, (e + 2) * 4ull);      // a float pair: elements e, e + 1
      }
    }
  }
  out[0] = end;
  out[1] = alloc;
  out[2] = wrap ? 1ull : 0ull;
  out[3] = (!wrap && end <= alloc) ? 1ull : 0ull;
  return CVR_OK;
}

cvr_status cvr_copy_extinction_sat(cvr_ctx* ctx, float* out, size_t capacity, int dims[3]) {
  Ctx* c = reinterpret_cast<Ctx*>(ctx);
  if (c && c->group) return cvr::group_call_root(c, [&](cvr_ctx* _m) { return cvr_copy_extinction_sat(_m, out, capacity, dims); });
  if (!c) return CVR_ERR_ARG;
  if (!c->sat.d_sat) return fail(c, CVR_ERR_STATE, "cvr_copy_extinction_sat: no SAT built");
  if (dims) for (int i = 0; i < 3; i++) dims[i] = c->sat.dims[i];
  if (!out) return CVR_OK;
  const size_t n = (size_t)c->sat.dims[0] * c->sat.dims[1] * c->sat.dims[2];
  if (capacity < n) return fail(c, CVR_ERR_ARG, "cvr_copy_extinction_sat: buffer too small");
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipMemcpy(out, c->sat.d_sat, n * sizeof(float), hipMemcpyDeviceToHost));
  return CVR_OK;
}

cvr_status cvr_render_extbsd(cvr_ctx* ctx, const cvr_frame* f, const cvr_ebs_params* p,
                             const cvr_output* o) {
  Ctx* c = reinterpret_cast<Ctx*>(ctx);
  if (c && c->group)
    return cvr::group_render(c, f, 1, o, [&](cvr_ctx* _m, const cvr_frame* mf, int, const cvr_output* mo) {
      return cvr_render_extbsd(_m, mf, p, mo);
    });
  if (!c) return CVR_ERR_ARG;
  if (!f || !p || !o || !o->rgba) return fail(c, CVR_ERR_ARG, "cvr_render_extbsd: null argument");
  cvr::EbsArgs Q;
  int ntiles = 0;
  size_t npix = 0;
  const cvr_status st = ebs_prepare(c, "cvr_render_extbsd", f, p, o, Q, ntiles, npix);
  if (st != CVR_OK) return st;
  return render_shaded(c, o, ntiles, npix, [&](float4* out, uint32_t* smp, unsigned long long* shade,
                                                unsigned long long* ts, hipStream_t st) {
    return cvr::launch_ebs(*c, Q, out, smp, shade, ts, st);
  });
}

#pragma GCC visibility pop
}  // extern "C"
