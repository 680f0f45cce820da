// shade_common.h — what the ShadeSample functions of the shaded renderers share
// (rc1pdosct and its light cache, rc1pextbsd, rc1pcrtgt, rc1pvctsg): the tail that
// turns the occlusion and shadow terms into a colour, the GL_LINEAR fetch of an
// RG16F 3D image, and the frame of the DOS shadow cone.  The reference types these
// out once per shader; here each is one text, so a shader cannot drift from its
// siblings.  Every function is forced inline: as a call a shader's kernel-argument
// block is copied to scratch (dos_cones.h DosShaderT::shade).
//
// Not here, on purpose: shade_phong (march_common.h) and iso.hip's shading, another
// formula on the headline path; crtgt.hip's shadow frame, which differs from the
// DOS one as its shader is written.
//
// CVR-SPEC arithmetic: the operand order of every product and sum is the shaders'
// (oracle/cvr_oracle.cpp restates it on the CPU).  Compiled -ffp-contract=off.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

#include "cvr_device.h"
#include "cvr_internal.h"
#include "march_common.h"
#include "shaded_march.h"

namespace cvr {

// ApplyPhongShading's two factors at world position wp for a non-zero gradient g:
// dd = max(0, N.L), and pw = pow(max(0, H.N), shininess).
struct PhongTerms {
  float dd, pw;
};
__device__ __forceinline__ PhongTerms phong_terms(const Rc1passArgs& A, f3 wp, f3 g) {
  const f3 eye{A.eye[0], A.eye[1], A.eye[2]};
  const f3 light{A.light[0], A.light[1], A.light[2]};
  const f3 nrm = normalize3(g);
  const f3 L = normalize3(f3{light.x - wp.x, light.y - wp.y, light.z - wp.z});
  const f3 Ve = normalize3(f3{eye.x - wp.x, eye.y - wp.y, eye.z - wp.z});
  const f3 Hv = normalize3(f3{Ve.x + L.x, Ve.y + L.y, Ve.z + L.z});
  const float dd = fmaxf(0.0f, dot3(nrm, L));
  const float ds = fmaxf(0.0f, dot3(Hv, nrm));
  return PhongTerms{dd, cvr_powf_nb(ds, A.shininess)};
}

__device__ __forceinline__ bool nonzero3(f3 g) { return g.x != 0.0f || g.y != 0.0f || g.z != 0.0f; }

// Without gradient shading every shader ends alike: (1/(ka+kd)) * (L*IOcc*ka + L*IShadow*kd)
__device__ __forceinline__ f3 combine_unshaded(float inv_k, float ka, float kd, float iocc, float isdw,
                                               f3 rgb) {
  return f3{inv_k * ((rgb.x * iocc) * ka + (rgb.x * isdw) * kd),
            inv_k * ((rgb.y * iocc) * ka + (rgb.y * isdw) * kd),
            inv_k * ((rgb.z * iocc) * ka + (rgb.z * isdw) * kd)};
}

// The tail of ShadeSample.  ka, kd, ks are the shader's gated weights (ka only with
// occlusion, kd / ks only with shadows); with both off 1 / (ka + kd) is inf and the
// colour NaN, as in the reference.  g: the gradient sample when Phong shading is
// on, else null; a zero gradient leaves the TF colour unshaded, as written.
//
// The cone form (ray_bbox_marching.comp:607-656, obj_ray_marching.comp:211-262,
// gt_ray_marching.comp:254-302 with Ispecular = vec3(1)):
//   L * ((1/(ka+kd)) * (IOcc*ka + IShadow*kd*dot_diff)) + Ispecular * (IShadow*ks*pow)
__device__ __forceinline__ f3 combine_cones(const Rc1passArgs& A, float ka, float kd, float ks, float iocc,
                                            float isdw, f3 wp, f3 rgb, const f3* g) {
  const float inv_k = 1.0f / (ka + kd);
  if (g) {   // ApplyPhongShading
    if (nonzero3(*g)) {
      const PhongTerms t = phong_terms(A, wp, *g);
      const float diff = inv_k * (iocc * ka + (isdw * kd) * t.dd);
      const float spec = (isdw * ks) * t.pw;
      return f3{fmaf(A.ispec[0], spec, rgb.x * diff), fmaf(A.ispec[1], spec, rgb.y * diff),
                fmaf(A.ispec[2], spec, rgb.z * diff)};
    }
    return rgb;
  }
  return combine_unshaded(inv_k, ka, kd, iocc, isdw, rgb);
}

// The SAT form (ebs_ray_bbox_marching.comp:528-530, vct_ray_bbox_marching.comp:179-180
// with IOcc = 1):
//   (1/(ka+kd)) * (L*IOcc*ka + IShadow*(L*kd*dot_diff)) + IShadow*(ks*Ispecular*pow)
__device__ __forceinline__ f3 combine_sat(const Rc1passArgs& A, float ka, float kd, float ks, float iocc,
                                          float isdw, f3 wp, f3 rgb, const f3* g) {
  const float inv_k = 1.0f / (ka + kd);
  if (g) {   // ApplyPhongShading
    if (nonzero3(*g)) {
      const PhongTerms t = phong_terms(A, wp, *g);
      return f3{inv_k * ((rgb.x * iocc) * ka + isdw * ((rgb.x * kd) * t.dd)) + isdw * ((ks * A.ispec[0]) * t.pw),
                inv_k * ((rgb.y * iocc) * ka + isdw * ((rgb.y * kd) * t.dd)) + isdw * ((ks * A.ispec[1]) * t.pw),
                inv_k * ((rgb.z * iocc) * ka + isdw * ((rgb.z * kd) * t.dd)) + isdw * ((ks * A.ispec[2]) * t.pw)};
    }
    return rgb;
  }
  return combine_unshaded(inv_k, ka, kd, iocc, isdw, rgb);
}

// texture(image, p / G).rg of an RG16F 3D image of d texels (one uint32 per texel,
// x fastest): GL_LINEAR, clamp-to-edge, texel coordinate fma(p, d / G, -0.5) with
// s = d / G and m = d - 1 (the convention of every other fetch here; clamping to
// [0, d - 1] gives GL's values: a coordinate in [-1, 0) reads texel 0 with any
// weight, see sample_pos).  The image holds < 2^31 texels (checked on the host):
// 32-bit indices.  FB: the weights' fraction bits (filter_bits; 0 = exact).
template <int FB>
__device__ __forceinline__ void fetch_rg16(const uint32_t* texels, const int (&d)[3], const float (&s)[3],
                                           const float (&m)[3], f3 p, float& r, float& g) {
  const float x = __builtin_amdgcn_fmed3f(fmaf(p.x, s[0], -0.5f), 0.0f, m[0]);
  const float y = __builtin_amdgcn_fmed3f(fmaf(p.y, s[1], -0.5f), 0.0f, m[1]);
  const float z = __builtin_amdgcn_fmed3f(fmaf(p.z, s[2], -0.5f), 0.0f, m[2]);
  const int ix = (int)x, iy = (int)y, iz = (int)z;
  const float ax = filter_weight<FB>(__builtin_amdgcn_fractf(x));
  const float ay = filter_weight<FB>(__builtin_amdgcn_fractf(y));
  const float az = filter_weight<FB>(__builtin_amdgcn_fractf(z));
  const int x1 = min(ix + 1, d[0] - 1), y1 = min(iy + 1, d[1] - 1), z1 = min(iz + 1, d[2] - 1);
  const int sy = d[0], sz = d[0] * d[1];
  const int r00 = iz * sz + iy * sy, r10 = iz * sz + y1 * sy;
  const int r01 = z1 * sz + iy * sy, r11 = z1 * sz + y1 * sy;
  const uint32_t t000 = texels[r00 + ix], t100 = texels[r00 + x1], t010 = texels[r10 + ix],
                 t110 = texels[r10 + x1], t001 = texels[r01 + ix], t101 = texels[r01 + x1],
                 t011 = texels[r11 + ix], t111 = texels[r11 + x1];
  float a[8], c[8];
  h2f2(t000, a[0], c[0]); h2f2(t100, a[1], c[1]); h2f2(t010, a[2], c[2]); h2f2(t110, a[3], c[3]);
  h2f2(t001, a[4], c[4]); h2f2(t101, a[5], c[5]); h2f2(t011, a[6], c[6]); h2f2(t111, a[7], c[7]);
  r = lerpf(lerpf(lerpf(a[0], a[1], ax), lerpf(a[2], a[3], ax), ay),
            lerpf(lerpf(a[4], a[5], ax), lerpf(a[6], a[7], ax), ay), az);
  g = lerpf(lerpf(lerpf(c[0], c[1], ax), lerpf(c[2], c[3], ax), ay),
            lerpf(lerpf(c[4], c[5], ax), lerpf(c[6], c[7], ax), ay), az);
}

// The frame (k, u, v) of the DOS shadow cone at wp (ShadowEvaluationKernel,
// ray_bbox_marching.comp:533-562 = lightcachecomputation.comp:492-521, before its
// Cone1RayShadow call): the light camera's own vectors for a
// directional light (shadow_type 2), else the axis toward the light and two
// crosses.  Returns false where a spot light (shadow_type 1) does not reach wp:
// no cone is traced there.
__device__ __forceinline__ bool shadow_cone_frame(const DosArgs& Q, f3 wp, f3& k, f3& u, f3& v) {
  const f3 lf{Q.lfwd[0], Q.lfwd[1], Q.lfwd[2]};
  if (Q.shadow_type == 2) {
    k = lf;
    v = f3{Q.lup[0], Q.lup[1], Q.lup[2]};
    u = f3{Q.lright[0], Q.lright[1], Q.lright[2]};
    return true;
  }
  const Rc1passArgs& A = Q.a;
  k = normalize3(f3{A.light[0] - wp.x, A.light[1] - wp.y, A.light[2] - wp.z});
  u = normalize3(cross3(k, f3{Q.lright[0], Q.lright[1], Q.lright[2]}));
  v = normalize3(cross3(k, u));
  return !(Q.shadow_type == 1 && dot3(k, lf) < Q.spot_cos);
}

}  // namespace cvr
