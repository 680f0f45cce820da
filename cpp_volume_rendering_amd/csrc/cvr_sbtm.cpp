// cvr_sbtm.cpp — slice-based directional occlusion (s_sbtm_dos,
// SBTMDirectionalOcclusionShading): the host arithmetic of Update and
// ComputeProxyGeometry (sbtmdosrenderer.cpp:122-174, 671-708, 745-777) in float, the
// slices' tap radii, the batches of the blocked kernel and the frame (sbtm.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "cvr_host.h"

using namespace cvr;

namespace cvr {

void sbtm_drop(Ctx* c) {
  free_dev(c->sbtm.d_eye);
  free_dev(c->sbtm.d_occ);
  c->sbtm.npix = 0;
  c->sbtm.bytes = 0;
}

// The tap radius of one axis, in pixels: every texel a fetch of Algorithm3 (and the
// fragment's own fetch) reads lies within r of the pixel.  cv: the slice's CVector
// component, pmax: the largest |p| of the grid along the axis, n: W or H.
// DESIGN.md 5d''' derives it: the tap's texel coordinate is x + d with |d| <=
// q n / 2 + n (4 + 2 q) 2^-24, q = |cv| pmax, the first term exact for the floats
// the kernel multiplies and the second its float rounding; the bilinear fetch reads
// floor and floor + 1, hence floor(D) + 1.  Above the int range: "does not fit".
static int tap_radius(float cv, float pmax, int n) {
  const double q = std::fabs((double)cv) * (double)pmax;
  const double D = q * (double)n * 0.5 + (double)n * (4.0 + 2.0 * q) * 0x1p-24;
  if (!(D < 1.0e6)) return 1 << 20;
  return (int)std::floor(D) + 1;
}

}  // namespace cvr

extern "C" {
#pragma GCC visibility push(default)

void cvr_sbtm_params_default(cvr_sbtm_params* p) {
  if (!p) return;
  *p = cvr_sbtm_params{};
  // sbtmdosrenderer.cpp:37-43, camera.cpp:27-28
  p->cone_half_angle_deg = 50.0f;
  p->grid_x = 2;
  p->grid_y = 2;
  p->attenuation = 1.0f;
  p->max_passes = 90000;
  p->z_near = 1.0f;
  p->z_far = 5000.0f;
}

cvr_status cvr_render_sbtm(cvr_ctx* ctx, const cvr_frame* f, const cvr_sbtm_params* p, const cvr_output* o) {
  Ctx* c = reinterpret_cast<Ctx*>(ctx);
  if (!c) return CVR_ERR_ARG;
  const char* who = "cvr_render_sbtm";
  if (c->group)
    return fail(c, CVR_ERR_ARG, "%s: a frame's pixels depend on their neighbours: not available on a group "
                                "context (cvr_create_group)", who);
  if (!f || !p || !o || !o->rgba) return fail(c, CVR_ERR_ARG, "%s: null argument", who);
  cvr_status st = check_frame_output(c, who, f, o, false);
  if (st != CVR_OK) return st;
  if (f->nranks > 1) return fail(c, CVR_ERR_ARG, "%s: whole frames only (nranks <= 1)", who);
  if (c->native_exp) return fail(c, CVR_ERR_ARG, "%s: not available with option native_exp", who);
  if (!(p->cone_half_angle_deg > 0.0f && p->cone_half_angle_deg < 90.0f))
    return fail(c, CVR_ERR_ARG, "%s: the cone half angle must lie in (0, 90) degrees", who);
  if (p->grid_x < 1 || p->grid_x > CVR_SBTM_MAX_GRID || p->grid_y < 1 || p->grid_y > CVR_SBTM_MAX_GRID)
    return fail(c, CVR_ERR_ARG, "%s: the grid must be 1..%d a side", who, CVR_SBTM_MAX_GRID);
  if (!(p->attenuation >= 0.0f && p->attenuation <= 1.0f))
    return fail(c, CVR_ERR_ARG, "%s: the attenuation must lie in [0, 1]", who);
  if (p->max_passes < 0) return fail(c, CVR_ERR_ARG, "%s: max_passes must be >= 0", who);
  if (!(p->z_near > 0.0f && p->z_near <= p->z_far) || !std::isfinite(p->z_far))
    return fail(c, CVR_ERR_ARG, "%s: the clip planes must satisfy 0 < z_near <= z_far", who);
  if (!std::isfinite(p->step)) return fail(c, CVR_ERR_ARG, "%s: the step is not finite", who);
  if (!c->d_cells || !c->d_tf) return fail(c, CVR_ERR_STATE, "%s: no volume or TF", who);

  SbtmArgs Q{};
  int ntiles = 0;
  size_t npix = 0;
  fill_frame_args(c, f, p->step, Q.a, ntiles, npix);
  Q.a.filter_bits = c->filter_bits;
  const Rc1passArgs& A = Q.a;
  const float step = A.step;

  // Update (:122-174).  mat3(View)'s row 2 is the view's z axis in world space.
  const V3 eye{A.eye[0], A.eye[1], A.eye[2]};
  const V3 cam_dir = gnormalize(V3{-A.col0[2], -A.col1[2], -A.col2[2]});
  const V3 ndir{-cam_dir.x, -cam_dir.y, -cam_dir.z};
  const V3 cam_right = gnormalize(cross(V3{0.0f, 1.0f, 0.0f}, ndir));
  const V3 cam_up = gnormalize(cross(ndir, cam_right));
  Q.right[0] = cam_right.x; Q.right[1] = cam_right.y; Q.right[2] = cam_right.z;
  Q.up[0] = cam_up.x; Q.up[1] = cam_up.y; Q.up[2] = cam_up.z;
  const double lx = c->N[0], ly = c->N[1], lz = c->N[2];
  Q.half_diag = (float)(std::sqrt(lx * lx + ly * ly + lz * lz) * 0.5f);   // volume_diagonal * 0.5f (:675)
  Q.att = p->attenuation;
  Q.gx = p->grid_x;
  Q.gy = p->grid_y;
  const float gxf = (float)Q.gx, gyf = (float)Q.gy;
  Q.gxy = gxf * gyf;
  const float extent = step * std::tan(p->cone_half_angle_deg * 3.14159265358979323846f / 180.0f);   // (:146)
  // p = ((grid_pos - GridSize / 2) / (GridSize / 2)) * OcclusionExtent (.frag:60), grid_pos += 1.0f
  float pmax_x = 0.0f, pmax_y = 0.0f;
  float gp = 0.5f;
  for (int i = 0; i < Q.gx; i++, gp += 1.0f) {
    Q.tapx[i] = ((gp - gxf / 2.0f) / (gxf / 2.0f)) * extent;
    pmax_x = std::fmax(pmax_x, std::fabs(Q.tapx[i]));
  }
  gp = 0.5f;
  for (int i = 0; i < Q.gy; i++, gp += 1.0f) {
    Q.tapy[i] = ((gp - gyf / 2.0f) / (gyf / 2.0f)) * extent;
    pmax_y = std::fmax(pmax_y, std::fabs(Q.tapy[i]));
  }
  // ComputeMinMaxZ* (:745-777): -(View * vec4(v, 1)).z over the corners of +-aabb,
  // glm's mat4 * vec4: (m0 x + m1 y) + (m2 z + m3)
  float V[16], tanh;
  cvr_camera_lookat(&f->camera, V, &tanh);
  if (f->use_view)
    for (int i = 0; i < 16; i++) V[i] = f->view[i];
  float minimum_z = +99999.0f, maximum_z = -99999.0f;
  // the order of the reference's eight calls (:761-776)
  static const int sgn[8][3] = {{1, 1, 1}, {1, -1, 1}, {-1, 1, 1}, {-1, -1, 1},
                                {1, 1, -1}, {1, -1, -1}, {-1, 1, -1}, {-1, -1, -1}};
  for (const auto& sg : sgn) {
    const float x = (float)sg[0] * A.half_grid[0], y = (float)sg[1] * A.half_grid[1],
                z = (float)sg[2] * A.half_grid[2];
    const float ptz = (V[2] * x + V[6] * y) + (V[10] * z + V[14] * 1.0f);
    minimum_z = std::fmin(minimum_z, -ptz);
    maximum_z = std::fmax(maximum_z, -ptz);
  }
  // ComputeProxyGeometry's loop (:683-708) must end
  if (!(step > 0.0f) || !std::isfinite(minimum_z) || !std::isfinite(maximum_z) ||
      !(std::fabs(maximum_z) + step > std::fabs(maximum_z)) ||
      !(std::fabs(minimum_z) + step > std::fabs(minimum_z)) ||
      ((double)maximum_z - (double)minimum_z) / (double)step > (double)CVR_SBTM_MAX_SLICES)
    return fail(c, CVR_ERR_ARG, "%s: the step must advance a float at maximum_z and cut at most %d slices", who,
                CVR_SBTM_MAX_SLICES);
  const float inv_x = 1.0f / (A.aspect * A.tan_half_fovy), inv_y = 1.0f / A.tan_half_fovy;   // glm::perspective
  std::vector<SbtmSlice> drawn;
  {
    float s = minimum_z, d0 = 0.0f;
    int passes = 0;
    while (s < maximum_z && passes < p->max_passes) {
      const float d = std::fmin(step, maximum_z - s);
      if (passes == 0) d0 = d;
      const float pos = (s + d * 0.5f) - minimum_z;              // pos_from_near (:703)
      SbtmSlice S{};
      // slice 0's quad moved by cam_dir * pos (.vert:22)
      S.depth = (minimum_z + d0 * 0.5f) + pos;
      S.plane = passes & 1;                                      // occlusion_buffer_next (:178, :230-231)
      if (S.depth >= p->z_near && S.depth <= p->z_far) {         // else every fragment is clipped
        S.c[0] = std::fmaf(cam_dir.x, S.depth, eye.x);
        S.c[1] = std::fmaf(cam_dir.y, S.depth, eye.y);
        S.c[2] = std::fmaf(cam_dir.z, S.depth, eye.z);
        S.cvx = inv_x / S.depth;                                 // equation 12 (.vert:29-31)
        S.cvy = inv_y / S.depth;
        S.rx = tap_radius(S.cvx, pmax_x, A.W);
        S.ry = tap_radius(S.cvy, pmax_y, A.H);
        drawn.push_back(S);
      }
      s = s + d;
      passes++;
    }
  }

  HIP_TRY(c, hipSetDevice(c->device));
  Ctx::Sbtm& B = c->sbtm;
  if (B.npix != npix || !B.d_eye) {
    QUIESCE(c);   // an earlier frame may still read the planes
    sbtm_drop(c);
    HIP_TRY(c, hipMalloc((void**)&B.d_eye, npix * 8));
    hipError_t e = hipMalloc((void**)&B.d_occ, npix * 8);   // two sets of two planes
    if (e != hipSuccess) {
      sbtm_drop(c);
      return fail_hip(c, who, e);
    }
    B.npix = npix;
    B.bytes = npix * 16;
  }

  hipStream_t s = c->stream;
  FrameOut fo;
  st = bind_frame_output(c, o, npix, fo);
  if (st == CVR_OK) st = frame_counters_begin(c, o, 1, s, fo);
  if (st != CVR_OK) return st;
  // set `cur` holds the planes; a blocked launch leaves them in the other set
  int cur = 0;
  SbtmPlanes P{B.d_eye, B.d_occ, B.d_occ + 2 * npix, fo.d_samples, fo.d_total};
  int launches = 0;
  st = timed_launch(c, s, [&]() -> hipError_t {
    hipError_t e = launch_sbtm_clear(P, A.W, A.H, s);
    // batches of consecutive drawn slices: the largest n <= the option whose summed
    // radii fit the kernel's halo; a slice that does not fit alone runs plain
    const size_t n = drawn.size();
    for (size_t i = 0; i < n && e == hipSuccess;) {
      SbtmBatch bt{};
      while (bt.n < c->sbtm_slices_per_launch && i + bt.n < n) {
        const SbtmSlice& S = drawn[i + bt.n];
        if (bt.ex + S.rx > kSbtmHalo || bt.ey + S.ry > kSbtmHalo) break;
        bt.s[bt.n++] = S;
        bt.ex += S.rx;
        bt.ey += S.ry;
      }
      if (bt.n == 0) {
        bt.s[0] = drawn[i];
        bt.n = 1;
      }
      P.occ = B.d_occ + (size_t)cur * 2 * npix;
      P.occ_out = B.d_occ + (size_t)(cur ^ 1) * 2 * npix;
      e = launch_sbtm_slices(*c, Q, bt, P, s);
      if (bt.n > 1) cur ^= 1;
      i += (size_t)bt.n;
      launches++;
    }
    if (e == hipSuccess) e = launch_sbtm_store(P, A.W, A.H, fo.d_out, fo.half, s);
    return e;
  });
  if (st != CVR_OK) return st;
  B.cur = cur;
  B.slices = (int)drawn.size();
  B.launches = launches;
  return frame_output_finish(c, o, fo, s);
}

cvr_status cvr_sbtm_read_occlusion(cvr_ctx* ctx, int width, int height, float* out) {
  Ctx* c = reinterpret_cast<Ctx*>(ctx);
  if (!c || !out) return CVR_ERR_ARG;
  if (c->group) return fail(c, CVR_ERR_ARG, "cvr_sbtm_read_occlusion: not available on a group context");
  const Ctx::Sbtm& B = c->sbtm;
  if (!B.d_occ) return fail(c, CVR_ERR_STATE, "cvr_sbtm_read_occlusion: no frame rendered");
  if (width < 1 || height < 1 || (size_t)width * height != B.npix)
    return fail(c, CVR_ERR_ARG, "cvr_sbtm_read_occlusion: not the last frame's viewport");
  std::vector<uint16_t> raw(2 * B.npix);
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipMemcpy(raw.data(), B.d_occ + (size_t)B.cur * 2 * B.npix, raw.size() * 2, hipMemcpyDeviceToHost));
  for (size_t i = 0; i < raw.size(); i++) out[i] = half_to_float_host(raw[i]);
  return CVR_OK;
}

#pragma GCC visibility pop
}  // extern "C"
