// cvr_api.cpp — C-ABI implementation (include/cvr.h): the context, the volume,
// TF and gradient setters, the host-side camera / TF helpers, and the thin
// post-pass, codec and selftest wrappers.  The renderers live in files of their
// own (cvr_rc1pass.cpp, cvr_dos.cpp, cvr_ebs.cpp, cvr_lightcache.cpp,
// cvr_iso.cpp), the options in cvr_options.cpp.
//
// Compiled with -ffp-contract=off: the camera and TF arithmetic below feed the
// kernels and must be bit-reproducible (CVR-SPEC).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

#include "cvr_host.h"

using namespace cvr;

namespace cvr {

cvr_status fail(Ctx* c, cvr_status st, const char* fmt, ...) {
  if (c) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    c->err = buf;
  }
  return st;
}

void default_light(cvr_light* l) {
  const float pos[3] = {-206.873f, -51.0699f, 557.011f}, fwd[3] = {-0.346883f, -0.0856335f, 0.933991f},
              up[3] = {-0.0298143f, 0.996327f, 0.0802758f}, right[3] = {0.937434f, -0.0f, 0.348162f};
  for (int i = 0; i < 3; i++) {
    l->position[i] = pos[i];
    l->forward[i] = fwd[i];
    l->up[i] = up[i];
    l->right[i] = right[i];
  }
  l->spot_angle_deg = 20.0f;
}

}  // namespace cvr

// TransferFunction1D::BuildLinear + GenerateTexture_1D_RGBt
// (transferfunction1d.cpp:319-358, 89-118; transferfunction.h:79-82).
// TransferFunction1D::BuildLinear (transferfunction1d.cpp:319-358): the double
// table m_transferfunction of max_density + 1 entries.
static cvr_status build_tf_table(const double* rgb_cp, int n_rgb, const double* a_cp, int n_a,
                                 int max_density, std::vector<double>& tab) {
  if (max_density < 1 || n_rgb < 0 || n_a < 0) return CVR_ERR_ARG;
  if ((n_rgb > 0 && !rgb_cp) || (n_a > 0 && !a_cp)) return CVR_ERR_ARG;
  const int n = max_density + 1;
  tab.assign((size_t)n * 4, 0.0);   // glm 0.9.5 dvec4 zero-init
  for (int i = 0; i + 1 < n_rgb; i++) {
    // TransferControlPoint keeps its colour in a glm::vec4 (float)
    float c0[3], c1[3];
    for (int k = 0; k < 3; k++) {
      c0[k] = (float)rgb_cp[i * 4 + k];
      c1[k] = (float)rgb_cp[(i + 1) * 4 + k];
    }
    int i0 = (int)rgb_cp[i * 4 + 3], i1 = (int)rgb_cp[(i + 1) * 4 + 3];
    double diff[3] = {(double)(c1[0] - c0[0]), (double)(c1[1] - c0[1]), (double)(c1[2] - c0[2])};
    for (int x = i0; x <= i1; x++) {
      if (x < 0 || x >= n) return CVR_ERR_ARG;
      double k = (double)(x - i0) / (double)(i1 - i0);
      for (int ch = 0; ch < 3; ch++) tab[(size_t)x * 4 + ch] = (double)c0[ch] + diff[ch] * k;
    }
  }
  for (int i = 0; i + 1 < n_a; i++) {
    float a0 = (float)a_cp[i * 2], a1 = (float)a_cp[(i + 1) * 2];
    int i0 = (int)a_cp[i * 2 + 1], i1 = (int)a_cp[(i + 1) * 2 + 1];
    double diff = (double)(a1 - a0);
    for (int x = i0; x <= i1; x++) {
      if (x < 0 || x >= n) return CVR_ERR_ARG;
      double k = (double)(x - i0) / (double)(i1 - i0);
      tab[(size_t)x * 4 + 3] = (double)a0 + diff * k;
    }
  }
  return CVR_OK;
}

// What hangs off what: the state derived from (volume, TF) that a new volume, a
// new TF and the context's end drop, one line per struct of Ctx.  The pyramid and
// the SAT outlive a TF change: each was built from a table of its own
// (cvr_set_extinction_volume, cvr_set_extinction_sat, which also drop the light
// cache).  The device has drained (QUIESCE) before any of this is freed.
enum class Changed { kVolume, kTransferFunction, kDestroy };
static void derived_drop(Ctx* c, Changed what) {
  const bool volume_gone = what != Changed::kTransferFunction;
  const bool tf_gone = what != Changed::kVolume;
  const bool destroy = what == Changed::kDestroy;
  skip_drop(c, volume_gone, tf_gone);
  if (volume_gone) ext_drop(c);
  if (volume_gone) sat_drop(c);
  light_cache_drop(c, destroy);
  if (destroy) crtgt_release(c); else crtgt_invalidate(c);
  vct_drop(c, volume_gone);
  sbtm_drop(c);
  if (volume_gone) iso_drop(c);
  if (volume_gone) deferred_drop(c, destroy);
}

static cvr_status set_volume_common(Ctx* c, const void* src, bool src_device, int bpv, int w,
                                    int h, int d, const float scale[3]) {
  if (!src || (bpv != 1 && bpv != 2) || w < 1 || h < 1 || d < 1 || !scale)
    return fail(c, CVR_ERR_ARG, "cvr_set_volume: bad arguments");
  if (!(scale[0] > 0 && scale[1] > 0 && scale[2] > 0))
    return fail(c, CVR_ERR_ARG, "cvr_set_volume: scale must be positive");
  if ((size_t)(w + 4) * (h + 4) * (d + 4) >= (size_t)1 << 32)
    return fail(c, CVR_ERR_ARG, "cvr_set_volume: volume too large for 32-bit cell indexing");
  if ((size_t)(w + 1) * (h + 1) >= (size_t)1 << 23)
    return fail(c, CVR_ERR_ARG, "cvr_set_volume: slice too large for 24-bit cell addressing");
  QUIESCE(c);   // frames in flight on any stream read the state replaced below
  free_dev(c->d_vox); c->vox_bytes = 0;
  free_dev(c->d_cells); c->cells_bytes = 0;
  free_dev(c->d_grad); c->grad_bytes = 0; c->grad_mode = 0;
  c->N[0] = w; c->N[1] = h; c->N[2] = d;
  for (int i = 0; i < 3; i++) c->scale[i] = scale[i];
  c->bpv = bpv;
  c->vox_bytes = (size_t)w * h * d * bpv;
  HIP_TRY(c, hipMalloc(&c->d_vox, c->vox_bytes));
  HIP_TRY(c, hipMemcpyAsync(c->d_vox, src, c->vox_bytes,
                            src_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
  // GetNormalizedSample -> (GLfloat) -> GL_R16F, as a per-value table
  const int nv = bpv == 1 ? 256 : 65536;
  std::vector<uint16_t> lut(nv);
  for (int v = 0; v < nv; v++)
    lut[v] = to_half_bits((float)((double)v / (bpv == 1 ? (256.0 - 1.0) : (65536.0 - 1.0))));
  free_dev(c->d_lut);
  derived_drop(c, Changed::kVolume);
  HIP_TRY(c, hipMalloc((void**)&c->d_lut, nv * sizeof(uint16_t)));
  uint16_t* d_lut = c->d_lut;
  hipError_t e = hipMemcpyAsync(d_lut, lut.data(), nv * sizeof(uint16_t), hipMemcpyHostToDevice,
                                c->stream);
  c->cells = cvr::make_cell_grid(c->N);
  c->cells_bytes = cvr::cell_count(c->cells) * 16;
  if (e == hipSuccess) e = hipMalloc(&c->d_cells, c->cells_bytes);
  if (e == hipSuccess)
    e = cvr::launch_build_cells_impl(c->d_vox, bpv, d_lut, c->N, c->cells, c->d_cells, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) {
    free_dev(c->d_cells); c->cells_bytes = 0;
    return fail_hip(c, "cvr_set_volume", e);
  }
  return CVR_OK;
}

extern "C" {
#pragma GCC visibility push(default)

int cvr_abi_version(void) { return CVR_ABI_VERSION; }

const char* cvr_status_string(cvr_status s) {
  switch (s) {
    case CVR_OK: return "CVR_OK";
    case CVR_ERR_ARG: return "CVR_ERR_ARG";
    case CVR_ERR_HIP: return "CVR_ERR_HIP";
    case CVR_ERR_OOM: return "CVR_ERR_OOM";
    case CVR_ERR_STATE: return "CVR_ERR_STATE";
    case CVR_ERR_IO: return "CVR_ERR_IO";
  }
  return "CVR_ERR_UNKNOWN";
}

// glm::lookAt (glm 0.9.5, include/glm/gtc/matrix_transform.inl:403-428), float.
cvr_status cvr_camera_lookat(const cvr_camera* cam, float out_view[16], float* out_tan) {
  if (!cam || !out_view || !out_tan) return CVR_ERR_ARG;
  V3 eye{cam->eye[0], cam->eye[1], cam->eye[2]};
  V3 center{cam->center[0], cam->center[1], cam->center[2]};
  V3 up{cam->up[0], cam->up[1], cam->up[2]};
  V3 f = gnormalize(sub(center, eye));
  V3 s = gnormalize(cross(f, up));
  V3 u = cross(s, f);
  float* R = out_view;
  for (int i = 0; i < 16; i++) R[i] = (i % 5 == 0) ? 1.0f : 0.0f;
  R[0] = s.x; R[4] = s.y; R[8] = s.z;
  R[1] = u.x; R[5] = u.y; R[9] = u.z;
  R[2] = -f.x; R[6] = -f.y; R[10] = -f.z;
  R[12] = -gdot(s, eye);
  R[13] = -gdot(u, eye);
  R[14] = gdot(f, eye);
  // (float)tan(DEGREE_TO_RADIANS(fovy) / 2.0): rc1prenderer.cpp:97, math_utils/utils.h:13
  double rad = (double)cam->fovy_deg * (3.14159265358979323846 / 180.0);
  *out_tan = (float)std::tan(rad / 2.0);
  return CVR_OK;
}

// rc1prenderer.cpp:62-63
float cvr_default_step(const float scale[3]) {
  double sx = scale[0], sy = scale[1], sz = scale[2];
  return (float)((0.5f / std::sqrt(3.0f)) * std::sqrt(sx * sx + sy * sy + sz * sz));
}

// TransferFunction1D::BuildLinear + GenerateTexture_1D_RGBt
// (transferfunction1d.cpp:319-358, 89-118; transferfunction.h:79-82).
cvr_status cvr_tf1d_build_rgbt(const double* rgb_cp, int n_rgb, const double* a_cp, int n_a,
                               int max_density, int extinction_input, float* out_rgbt) {
  if (!out_rgbt) return CVR_ERR_ARG;
  std::vector<double> tab;
  cvr_status st = build_tf_table(rgb_cp, n_rgb, a_cp, n_a, max_density, tab);
  if (st != CVR_OK) return st;
  const int n = max_density + 1;
  for (int i = 0; i < n; i++) {
    out_rgbt[i * 4 + 0] = (float)tab[(size_t)i * 4 + 0];
    out_rgbt[i * 4 + 1] = (float)tab[(size_t)i * 4 + 1];
    out_rgbt[i * 4 + 2] = (float)tab[(size_t)i * 4 + 2];
    float v4 = (float)tab[(size_t)i * 4 + 3];
    if (!extinction_input) v4 = (float)std::log(1.0 / (1.0 - (double)v4));
    out_rgbt[i * 4 + 3] = v4;
  }
  return CVR_OK;
}

// TransferFunction1D::GetOpc(i, max_density) = Get(i, max_density).a for integer i
// below max_density (transferfunction1d.cpp:132-167): value = i * (max / max), the
// interpolation weight t = 0, so (float)((1 - 0) * tab[i] + 0 * tab[i + 1]).
cvr_status cvr_tf1d_opacity_lut(const double* rgb_cp, int n_rgb, const double* a_cp, int n_a,
                                int max_density, int n, float* out_opacity) {
  if (!out_opacity || n != CVR_VCT_TABLE_WIDTH || max_density < n) return CVR_ERR_ARG;
  std::vector<double> tab;
  cvr_status st = build_tf_table(rgb_cp, n_rgb, a_cp, n_a, max_density, tab);
  if (st != CVR_OK) return st;
  for (int i = 0; i < n; i++) {
    const double value = (double)i * ((double)max_density / (double)max_density);
    const int iv = (int)value;
    const double t = value - iv;
    out_opacity[i] = (float)((1.0 - t) * tab[(size_t)iv * 4 + 3] + t * tab[(size_t)(iv + 1) * 4 + 3]);
  }
  return CVR_OK;
}

// TransferFunction1D::GetExtN(StructuredGridVolume::GetNormalizedSample) for every
// voxel value: Get(v / (2^bits - 1), 1.0).a (transferfunction1d.cpp:132-157) as
// float, then MaterialOpacityToExtinction in double (:189-197), as float.
cvr_status cvr_tf1d_ext_lut(const double* rgb_cp, int n_rgb, const double* a_cp, int n_a,
                            int max_density, int extinction_input, int bytes_per_voxel,
                            float* out_lut) {
  if (!out_lut || (bytes_per_voxel != 1 && bytes_per_voxel != 2)) return CVR_ERR_ARG;
  std::vector<double> tab;
  cvr_status st = build_tf_table(rgb_cp, n_rgb, a_cp, n_a, max_density, tab);
  if (st != CVR_OK) return st;
  const int nv = bytes_per_voxel == 1 ? 256 : 65536;
  const double den = bytes_per_voxel == 1 ? (256.0 - 1.0) : (65536.0 - 1.0);
  for (int v = 0; v < nv; v++) {
    double value = ((double)v / den) * ((double)max_density / 1.0);
    float a;
    if (value < 0.0f || value > (float)max_density) {
      a = 0.0f;
    } else if (std::fabs(value - (float)max_density) < 0.000001) {
      a = (float)tab[(size_t)max_density * 4 + 3];
    } else {
      const int iv = (int)value;
      const double t = value - iv;
      a = (float)((1.0 - t) * tab[(size_t)iv * 4 + 3] + t * tab[(size_t)(iv + 1) * 4 + 3]);
    }
    out_lut[v] = extinction_input ? a : (float)std::log(1.0 / (1.0 - (double)a));
  }
  return CVR_OK;
}

cvr_status cvr_create(int device, cvr_ctx** out_ctx) {
  if (!out_ctx) return CVR_ERR_ARG;
  *out_ctx = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return CVR_ERR_HIP;
  if (device < 0 || device >= ndev) return CVR_ERR_ARG;
  Ctx* c = new (std::nothrow) Ctx();
  if (!c) return CVR_ERR_OOM;
  c->device = device;
  if (hipSetDevice(device) != hipSuccess ||
      hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) != hipSuccess ||
      hipMalloc(&c->d_total, sizeof(unsigned long long)) != hipSuccess) {
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;
    return CVR_ERR_HIP;
  }
  c->stream = c->own_stream;
  {
    hipDeviceProp_t prop;
    c->num_cus = hipGetDeviceProperties(&prop, device) == hipSuccess ? prop.multiProcessorCount : 256;
  }
  *out_ctx = reinterpret_cast<cvr_ctx*>(c);
  return CVR_OK;
}

void cvr_destroy(cvr_ctx* ctx) {
  Ctx* c = reinterpret_cast<Ctx*>(ctx);
  if (!c) return;
  cvr::group_release(c);
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  cvr::comm_release(c);
  free_dev(c->d_vox);
  free_dev(c->d_cells);
  free_dev(c->d_tf);
  free_dev(c->d_grad);
  free_dev(c->d_lut);
  derived_drop(c, Changed::kDestroy);
  free_dev(c->d_shade);
  for (auto& J : c->flat) cvr::flat_release(J);
  free_dev(c->d_total);
  free_dev(c->d_scratch);
  if (c->side) (void)hipStreamSynchronize(c->side);
  for (auto& o : c->oslot) {
    free_dev(o.d_order);
    free_dev(o.d_cost);
    if (o.done) (void)hipEventDestroy(o.done);
  }
  if (c->ev_frame) (void)hipEventDestroy(c->ev_frame);
  if (c->ev_counters) (void)hipEventDestroy(c->ev_counters);
  c->ev_counters = nullptr;
  c->counters_stream = nullptr;
  if (c->side) (void)hipStreamDestroy(c->side);
  free_dev(c->d_tile_stats);
  free_dev(c->d_tile_samples);
  for (hipEvent_t e : c->ev_start) (void)hipEventDestroy(e);
  for (hipEvent_t e : c->ev_stop) (void)hipEventDestroy(e);
  if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
  delete c;
}

const char* cvr_last_error(const cvr_ctx* ctx) {
  const Ctx* c = reinterpret_cast<const Ctx*>(ctx);
  return c ? c->err.c_str() : "null context";
}

cvr_status cvr_set_stream(cvr_ctx* ctx, void* stream) {
  Ctx* c = reinterpret_cast<Ctx*>(ctx);
  if (!c) return CVR_ERR_ARG;
  c->stream = (hipStream_t)stream;     // NULL = the legacy default stream
  return CVR_OK;
}

cvr_status cvr_synchronize(cvr_ctx* ctx) {
  Ctx* c = reinterpret_cast<Ctx*>(ctx);
  if (!c) return CVR_ERR_ARG;
  if (c->group) {
    cvr_status st = cvr::group_each(c, [&](cvr_ctx* _m) { return cvr_synchronize(_m); });
    if (st != CVR_OK) return st;
  }
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (c->side) HIP_TRY(c, hipStreamSynchronize(c->side));
  return CVR_OK;
}

size_t cvr_device_bytes(const cvr_ctx* ctx) {
  const Ctx* c = reinterpret_cast<const Ctx*>(ctx);
  if (!c) return 0;
  if (c->group) {
    size_t b = 0;
    for (int i = 0; i < cvr_group_size(ctx); i++)
      b += cvr_device_bytes(cvr_group_member(const_cast<cvr_ctx*>(ctx), i));
    return b;
  }
  return c->vox_bytes + c->cells_bytes + c->grad_bytes + (size_t)c->tf_n * 16 + c->scratch_bytes +
         c->lc.bytes + c->gt.bytes + c->vct.bytes + c->sbtm.bytes + c->deferred.bytes + c->adv.bytes +
         c->adv.table_bytes;
}

cvr_status cvr_copy_cells(cvr_ctx* ctx, void* out, size_t capacity) {
  Ctx* c = reinterpret_cast<Ctx*>(ctx);
  if (c && c->group) return cvr::group_call_root(c, [&](cvr_ctx* _m) { return cvr_copy_cells(_m, out, capacity); });
  if (!c || !out) return CVR_ERR_ARG;
  if (!c->d_cells) return fail(c, CVR_ERR_STATE, "cvr_copy_cells: no volume set");
  if (capacity < c->cells_bytes)
    return fail(c, CVR_ERR_ARG, "cvr_copy_cells: need %zu bytes", c->cells_bytes);
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipDeviceSynchronize());
  HIP_TRY(c, hipMemcpy(out, c->d_cells, c->cells_bytes, hipMemcpyDeviceToHost));
  return CVR_OK;
}

cvr_status cvr_set_volume(cvr_ctx* ctx, const void* voxels, int bpv, int w, int h, int d,
                          const float scale[3]) {
  Ctx* c = reinterpret_cast<Ctx*>(ctx);
  if (c && c->group) return cvr::group_each(c, [&](cvr_ctx* _m) { return cvr_set_volume(_m, voxels, bpv, w, h, d, scale); });
  if (!c) return CVR_ERR_ARG;
  return set_volume_common(c, voxels, false, bpv, w, h, d, scale);
}

cvr_status cvr_set_volume_device(cvr_ctx* ctx, const void* d_voxels, int bpv, int w, int h,
                                 int d, const float scale[3]) {
  Ctx* c = reinterpret_cast<Ctx*>(ctx);
  if (c && c->group) return cvr::group_each(c, [&](cvr_ctx* _m) { return cvr_set_volume_device(_m, d_voxels, bpv, w, h, d, scale); });
  if (!c) return CVR_ERR_ARG;
  return set_volume_common(c, d_voxels, true, bpv, w, h, d, scale);
}

cvr_status cvr_set_transfer_function(cvr_ctx* ctx, const float* rgbt, int n) {
  Ctx* c = reinterpret_cast<Ctx*>(ctx);
  if (c && c->group) return cvr::group_each(c, [&](cvr_ctx* _m) { return cvr_set_transfer_function(_m, rgbt, n); });
  if (!c) return CVR_ERR_ARG;
  if (!rgbt || n < 2 || n > 4096)
    return fail(c, CVR_ERR_ARG, "cvr_set_transfer_function: need 2 <= n <= 4096 entries");
  std::vector<float> q((size_t)n * 4);
  float amax = 0.0f;
  for (size_t i = 0; i < q.size(); i++) {
    q[i] = half_round(rgbt[i]);   // GL_RGBA16F
    if (i % 4 == 3) amax = std::isfinite(q[i]) ? std::max(amax, q[i]) : NAN;
  }
  QUIESCE(c);   // frames in flight on any stream read the state replaced below
  derived_drop(c, Changed::kTransferFunction);
  if (n != c->tf_n) {
    free_dev(c->d_tf);
    HIP_TRY(c, hipMalloc((void**)&c->d_tf, (size_t)n * 16));
    c->tf_n = n;
  }
  HIP_TRY(c, hipMemcpy(c->d_tf, q.data(), (size_t)n * 16, hipMemcpyHostToDevice));
  c->tf_max_alpha = amax;
  return skip_set_tf(c, q.data(), n);
}

cvr_status cvr_set_gradient(cvr_ctx* ctx, int mode) {
  Ctx* c = reinterpret_cast<Ctx*>(ctx);
  if (c && c->group) return cvr::group_each(c, [&](cvr_ctx* _m) { return cvr_set_gradient(_m, mode); });
  if (!c) return CVR_ERR_ARG;
  if (mode < 0 || mode > 2) return fail(c, CVR_ERR_ARG, "cvr_set_gradient: bad mode %d", mode);
  if (mode != 0 && !c->d_vox) return fail(c, CVR_ERR_STATE, "cvr_set_gradient: no volume");
  QUIESCE(c);   // frames in flight on any stream read the state replaced below
  free_dev(c->d_grad); c->grad_bytes = 0; c->grad_mode = 0;
  crtgt_invalidate(c);
  if (mode == 0) return CVR_OK;
  c->grad_bytes = cvr::cell_count(c->cells) * 48;
  HIP_TRY(c, hipMalloc(&c->d_grad, c->grad_bytes));
  uint2* tmp = nullptr;
  hipError_t e = hipMalloc((void**)&tmp, (size_t)c->N[0] * c->N[1] * c->N[2] * 8);
  if (e == hipSuccess) e = cvr::launch_gradient(*c, mode, tmp, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  (void)hipFree(tmp);
  if (e != hipSuccess) {
    free_dev(c->d_grad); c->grad_bytes = 0;
    return fail_hip(c, "cvr_set_gradient", e);
  }
  c->grad_mode = mode;
  return CVR_OK;
}

cvr_status cvr_selftest_arith(cvr_ctx* ctx, uint64_t out[3]) {
  Ctx* c = reinterpret_cast<Ctx*>(ctx);
  if (c && c->group) return cvr::group_call_root(c, [&](cvr_ctx* _m) { return cvr_selftest_arith(_m, out); });
  if (!c || !out) return CVR_ERR_ARG;
  HIP_TRY(c, hipSetDevice(c->device));
  unsigned long long* d = nullptr;
  HIP_TRY(c, hipMalloc((void**)&d, 3 * sizeof(unsigned long long)));
  hipError_t e = hipMemsetAsync(d, 0, 3 * sizeof(unsigned long long), c->stream);
  if (e == hipSuccess) e = cvr::launch_selftest_arith(-100, 200, -96, 222, d, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(out, d, 3 * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  (void)hipFree(d);
  HIP_TRY(c, e);
  return CVR_OK;
}

cvr_status cvr_multiscale_resolution(int mode, int sw, int sh, int* rw, int* rh) {
  if (!rw || !rh || sw < 1 || sh < 1 || mode < 0 || mode > 3) return CVR_ERR_ARG;
  // UpdateScreenResolutionMultiScaling, multiplier (2, 2) or (-2, -2)
  if (mode == CVR_SINGLE_RAY_PER_PIXEL) { *rw = sw; *rh = sh; }
  else if (mode == CVR_UP_SCALING_RENDER) { *rw = sw / 2; *rh = sh / 2; }
  else { *rw = sw * 2; *rh = sh * 2; }
  return (*rw >= 1 && *rh >= 1) ? CVR_OK : CVR_ERR_ARG;
}

cvr_status cvr_multiscale_filter(cvr_ctx* ctx, int mode, int kernel, void* d_frame, int fw, int fh,
                                 void* d_screen, int sw, int sh) {
  Ctx* c = reinterpret_cast<Ctx*>(ctx);
  if (c && c->group) return cvr::group_call_root(c, [&](cvr_ctx* _m) { return cvr_multiscale_filter(_m, mode, kernel, d_frame, fw, fh, d_screen, sw, sh); });
  if (!c) return CVR_ERR_ARG;
  if (!d_frame || !d_screen || mode < 1 || mode > 3 || kernel < 0 || kernel > 5 || fw < 1 ||
      fh < 1 || sw < 1 || sh < 1 || d_frame == d_screen)
    return fail(c, CVR_ERR_ARG, "cvr_multiscale_filter: bad arguments");
  const bool cardinal = kernel == CVR_FILTER_CARDINAL_BSPLINE_3 || kernel == CVR_FILTER_CARDINAL_OMOMS3;
  // the digital filter's pre-factored LU needs lines longer than its 8/9 factors
  if (cardinal && mode != CVR_MULTIPLE_RAYS_PER_PIXEL &&
      (mode == CVR_DOWN_SCALING_RENDER ? (sw < 16 || sh < 16) : (fw < 16 || fh < 16)))
    return fail(c, CVR_ERR_ARG, "cvr_multiscale_filter: cardinal kernels need >= 16 px lines");
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, cvr::launch_multiscale(mode, kernel, d_frame, fw, fh, d_screen, sw, sh, c->stream));
  return CVR_OK;
}

cvr_status cvr_screenshot_rgb8(cvr_ctx* ctx, const void* d_frame, int format, int w, int h,
                               void* d_rgb) {
  Ctx* c = reinterpret_cast<Ctx*>(ctx);
  if (c && c->group) return cvr::group_call_root(c, [&](cvr_ctx* _m) { return cvr_screenshot_rgb8(_m, d_frame, format, w, h, d_rgb); });
  if (!c) return CVR_ERR_ARG;
  if (!d_frame || !d_rgb || w < 1 || h < 1 ||
      (format != CVR_FORMAT_RGBA32F && format != CVR_FORMAT_RGBA16F))
    return fail(c, CVR_ERR_ARG, "cvr_screenshot_rgb8: bad arguments");
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, cvr::launch_screenshot(d_frame, format == CVR_FORMAT_RGBA16F, w, h, (uint8_t*)d_rgb,
                                    c->stream));
  return CVR_OK;
}

cvr_status cvr_unpack_tiles_device_n(cvr_ctx* ctx, const cvr_frame* f, const void* d_gathered,
                                     int tpr_max, int nframes, int frame_index, int format,
                                     void* d_rgba) {
  Ctx* c = reinterpret_cast<Ctx*>(ctx);
  if (c && c->group) return cvr::group_call_root(c, [&](cvr_ctx* _m) { return cvr_unpack_tiles_device_n(_m, f, d_gathered, tpr_max, nframes, frame_index, format, d_rgba); });
  if (!c) return CVR_ERR_ARG;
  if (!f || !d_gathered || !d_rgba || f->nranks < 1 || f->tile_size < 16 || tpr_max < 0 ||
      nframes < 1 || frame_index < 0 || frame_index >= nframes ||
      (format != CVR_FORMAT_RGBA32F && format != CVR_FORMAT_RGBA16F))
    return fail(c, CVR_ERR_ARG, "cvr_unpack_tiles_device: bad arguments");
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t px = format == CVR_FORMAT_RGBA16F ? 8 : 16;
  const char* src = static_cast<const char*>(d_gathered) +
                    (size_t)frame_index * tpr_max * f->tile_size * f->tile_size * px;
  HIP_TRY(c, cvr::launch_unpack_tiles(src, d_rgba, format == CVR_FORMAT_RGBA16F, f->width,
                                      f->height, f->tile_size, f->nranks, tpr_max, c->stream,
                                      (size_t)nframes * tpr_max));
  return CVR_OK;
}

cvr_status cvr_unpack_tiles_device(cvr_ctx* ctx, const cvr_frame* f, const void* d_packed,
                                   int tpr_max, int format, void* d_rgba) {
  return cvr_unpack_tiles_device_n(ctx, f, d_packed, tpr_max, 1, 0, format, d_rgba);
}

size_t cvr_tile_code_bound(int tile, int ntiles) {
  if (tile < 16 || tile % 16 != 0 || tile > 64 || ntiles < 0) return 0;
  return cvr::tile_code_bound_bytes(tile, ntiles);
}

cvr_status cvr_encode_tiles(cvr_ctx* ctx, const void* d_tiles, int tile, int ntiles, void* d_stream,
                            unsigned long long* d_bytes) {
  Ctx* c = reinterpret_cast<Ctx*>(ctx);
  if (c && c->group) return cvr::group_call_root(c, [&](cvr_ctx* _m) { return cvr_encode_tiles(_m, d_tiles, tile, ntiles, d_stream, d_bytes); });
  if (!c) return CVR_ERR_ARG;
  if ((!d_tiles && ntiles > 0) || !d_stream || !d_bytes || !cvr_tile_code_bound(tile, ntiles))
    return fail(c, CVR_ERR_ARG, "cvr_encode_tiles: bad arguments");
  HIP_TRY(c, hipSetDevice(c->device));
  if (c->encode_onepass && tile <= 32) {   // (8 tiles staged in LDS per workgroup)
    // the exchange's one-launch form: tiles in claim order (the start table says where).
    // Its counter is the caller's own length word, zeroed first, so encodes on several
    // streams never share one.
    HIP_TRY(c, hipMemsetAsync(d_bytes, 0, sizeof(unsigned long long), c->stream));
    HIP_TRY(c, cvr::launch_exchange_encode(d_tiles, tile, ntiles, ntiles, 1, d_stream, d_bytes, d_bytes,
                                           nullptr, c->stream));
    return CVR_OK;
  }
  HIP_TRY(c, cvr::launch_tile_encode(d_tiles, tile, ntiles, d_stream, d_bytes, c->stream));
  return CVR_OK;
}

cvr_status cvr_decode_tiles(cvr_ctx* ctx, const void* d_stream, int tile, int ntiles, void* d_tiles) {
  Ctx* c = reinterpret_cast<Ctx*>(ctx);
  if (c && c->group) return cvr::group_call_root(c, [&](cvr_ctx* _m) { return cvr_decode_tiles(_m, d_stream, tile, ntiles, d_tiles); });
  if (!c) return CVR_ERR_ARG;
  if (!d_stream || (!d_tiles && ntiles > 0) || !cvr_tile_code_bound(tile, ntiles))
    return fail(c, CVR_ERR_ARG, "cvr_decode_tiles: bad arguments");
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, cvr::launch_tile_decode(d_stream, tile, ntiles, d_tiles, c->stream));
  return CVR_OK;
}

#pragma GCC visibility pop
}  // extern "C"
