// ebs.hip — extinction-based shading (cppvolrend rc1pextbsd) on gfx950.
//
// The march of shaded_march.h with ShadeSample of ebs_ray_bbox_marching.comp
// (:498-550): an ambient occlusion from 15 concentric SAT boxes around the
// sample (ExtinctionAmbientOcclusion :109-146, 120 SAT fetches) and a shadow
// from a chain of SAT boxes along the dominant axis of the light direction,
// widened by the cone angle (ExtinctionDirectionalShadows / ConeX|Y|ZAxis
// :187-481; up to ~N/2 boxes of 8 fetches).  A SAT fetch is the GL_LINEAR
// texture(TexVolumeSAT3D, p / (G + 2 s)) of the float SAT (sat.hip).  The SAT
// evaluation itself lives in ebs_sat.h, shared with the pre-illumination light
// cache (ebs_lightcache.hip).
// Arithmetic follows CVR-SPEC as oracle/cvr_oracle.cpp (oracle_render_ebs_rows)
// does, op for op, so the images are bit-identical.  Compiled -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "cvr_device.h"
#include "march_common.h"
#include "shaded_march.h"
#include "shade_common.h"
#include "ebs_sat.h"

namespace cvr {

#ifndef CVR_EBS_FLAT_WAVES
#define CVR_EBS_FLAT_WAVES 1   // flat shading: the compiler's 128 VGPRs, 4 waves/SIMD
#endif
#ifndef CVR_EBS_WAVES
#define CVR_EBS_WAVES 1
#endif
template <bool RECIP_CONE, class LY>
struct EbsShaderT {
  using Args = EbsArgs;
  static constexpr int kMinWavesPerEU = CVR_EBS_WAVES;   // register budget (1: compiler's choice)
  static constexpr int kFlatWavesPerEU = CVR_EBS_FLAT_WAVES;   // flat_shade_kernel
  static constexpr bool kSplit = false;   // flat_shade_kernel calls shade() whole
  using Data = typename LY::Ptr;   // the float SAT, cell4 or plain
  static constexpr int kFB = LY::kFB;   // GL_LINEAR weights of every fetch (filter_bits)

  // ShadeSample (:498-550); `lit` counts the shadow box chains traced.
  __device__ static f3 shade(const EbsArgs& Q, typename LY::Ptr __restrict__ sat, f3 tx, f3 wp, f3,
                             f3 rgb, const f3* g, uint32_t& lit, uint32_t& fetches) {
    const Rc1passArgs& A = Q.a;
    const f3 light{A.light[0], A.light[1], A.light[2]};
    float iocc = 0.0f, isdw = 0.0f;
    if (Q.apply_occlusion) {
      iocc = ebs_occlusion<LY>(Q, sat, tx);
      fetches += 8 * Q.occ_shells;
    }
    if (Q.apply_shadow) {
      // ExtinctionDirectionalShadows (:455-481)
      const f3 cv = ebs_cone_vec(Q, light, wp);
      uint32_t boxes = 0;
      const float Stau = ebs_shadow_tau<LY, RECIP_CONE>(Q, sat, tx, cv, boxes);
      fetches += 8 * boxes;
      isdw = cvr_expf(-Stau);
      lit++;
    }
    return combine_sat(A, Q.ka, Q.kd, Q.ks, iocc, isdw, wp, rgb, g);
  }
};

template <class L>
static hipError_t launch_ebs_layout(const Ctx& c, const EbsArgs& q, typename L::Ptr sat, float4* out,
                                    uint32_t* samples, unsigned long long* shade,
                                    unsigned long long* tile_samples, hipStream_t s) {
  const bool ph = q.phong != 0;
  if (c.shade_flat)
    return q.recip_cone
               ? launch_shaded_flat<EbsShaderT<true, L>>(c, q, ph, sat, out, samples, shade, tile_samples, s)
               : launch_shaded_flat<EbsShaderT<false, L>>(c, q, ph, sat, out, samples, shade, tile_samples, s);
  if (q.recip_cone)
    return launch_shaded_march<EbsShaderT<true, L>>(c, q, ph, sat, out, samples, shade, tile_samples, s);
  return launch_shaded_march<EbsShaderT<false, L>>(c, q, ph, sat, out, samples, shade, tile_samples, s);
}

hipError_t launch_ebs(const Ctx& c, const EbsArgs& q, float4* out, uint32_t* samples,
                      unsigned long long* shade, unsigned long long* tile_samples, hipStream_t s) {
  if (q.a.filter_bits == 8)   // GL texture-unit weights (CVR-SPEC-8): the cell4 copy only
    return c.sat_layout == 1 ? hipErrorInvalidValue
                             : launch_ebs_layout<SatFB<SatCell4, 8>>(c, q, c.sat.d_cells, out, samples,
                                                                     shade, tile_samples, s);
  if (c.sat_layout == 1)
    return launch_ebs_layout<SatPlain>(c, q, c.sat.d_sat, out, samples, shade, tile_samples, s);
  return launch_ebs_layout<SatCell4>(c, q, c.sat.d_cells, out, samples, shade, tile_samples, s);
}

}  // namespace cvr
