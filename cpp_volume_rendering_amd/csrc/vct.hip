// vct.hip — voxel cone tracing (cppvolrend rc1pvctsg) on gfx950.
//
// The march of shaded_march.h with ShadeSample of vct_ray_bbox_marching.comp
// (:146-189): one cone toward the light per sample (EvaluationVoxelConeTracing,
// :97-144).  A cone sample is a textureLod of the RG16F (mean, standard deviation)
// supervoxel pyramid (vct_precompute.hip) at a fractional level, a GL_LINEAR fetch
// of the R16F pre-integration table at ((mean, stddev) + 0.5) / (255, max stddev),
// and Tvd *= pow(1 - opacity, step * corr_fact).
//
// The cone's schedule -- per sample the distance xl = apex + step / 2, the exponent
// step * corr_fact and the level log2(2 xl tan(apex angle) / 1.0) with its one or
// two pyramid levels -- depends on the cone parameters only, not on the lane, so
// one thread computes it once per parameter set (vct_schedule_kernel) and every
// lane reads it with scalar loads; only the box cut (CUT_WHEN_AWAY_FROM_VOLUME,
// :122-125) is per lane.
//
// The table (at most 255 x 255 halves, 127 KiB; 255 x 64 = 32 KiB for typical 8-bit
// data) stays in global memory: shaded_march_kernel already holds ~16 KiB of LDS per
// 64-lane workgroup (job queues, camera rays, the TF), the whole table next to it
// would cut the CU to one wave and cost 127 KiB of staging per 8x8 tile, and the
// flat shade kernel has no workgroup-wide prologue at all; a table of this size is
// resident in every XCD's 4 MiB L2 after the first tiles.  Not measured either way.
//
// Arithmetic follows CVR-SPEC (DESIGN.md 5d'') as tests/support/vct_ref.cpp does,
// op for op, so the images are bit-identical.  Compiled -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "cvr_device.h"
#include "march_common.h"
#include "shaded_march.h"
#include "shade_common.h"

namespace cvr {

// log2(x) = ln(x) * (1 / ln 2), the constant rounded to float once (CVR-SPEC)
__device__ __forceinline__ float cvr_log2f(float x) { return cvr_logf(x) * 1.44269504088896341f; }

// One thread: the recurrence apex += step, step *= rate is serial and n <= 10000.
__global__ void __launch_bounds__(64)
vct_schedule_kernel(const VctLevel* __restrict__ levels, int nl, float initial, float step, float rate,
                    float tan_apex, float corr, int n, int filter_bits, VctStep* __restrict__ out) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  float apex = initial;
  for (int is = 0; is < n; is++) {
    VctStep S;
    S.xl = apex + step * 0.5f;                                  // :115
    S.expo = step * corr;                                       // :131
    const float lam = cvr_log2f(((2.0f * S.xl) * tan_apex) / 1.0f);   // :118, DXbase = 1.0
    // textureLod under GL_LINEAR_MIPMAP_LINEAR: magnification (lambda <= 0, also a
    // NaN) reads level 0 with GL_LINEAR; a level at or above the last computed one
    // reads that one (this project's clamp: the reference uploads nothing beyond)
    int l0;
    if (!(lam > 0.0f)) {
      l0 = 0; S.nlev = 1; S.frac = 0.0f;
    } else if (lam >= (float)(nl - 1)) {
      l0 = nl - 1; S.nlev = 1; S.frac = 0.0f;
    } else {
      const float fl = floorf(lam);
      l0 = (int)fl; S.nlev = 2;
      S.frac = filter_bits == 8 ? filter_weight<8>(lam - fl) : lam - fl;
    }
    S.lv[0] = levels[l0];
    S.lv[1] = levels[S.nlev == 2 ? l0 + 1 : l0];
    out[is] = S;
    apex = apex + step;                                         // :136
    step = step * rate;                                         // :138
  }
}

template <int FB>
struct VctShaderT {
  using Args = VctArgs;
  using Data = VctData;
  static constexpr int kMinWavesPerEU = 1;    // register budget: the compiler's choice
  static constexpr int kFlatWavesPerEU = 1;
  static constexpr bool kSplit = false;       // flat_shade_kernel calls shade() whole
  static constexpr int kFB = FB;              // GL_LINEAR weights of every fetch (filter_bits)

  // texture(level, p / G).rg = (mean, standard deviation); the pyramid holds < 2^31
  // texels (checked on the host) and they are finite
  __device__ static __forceinline__ void fetch_level(const uint32_t* __restrict__ pyr, const VctLevel& L,
                                                     f3 p, float& mean, float& sd) {
    fetch_rg16<FB>(pyr + L.off, L.d, L.s, L.m, p, mean, sd);
  }

  // texture(TexPreIntegrationLookup, uv).r: GL_LINEAR, clamp-to-edge, texel
  // coordinate fma(u, n, -0.5) as the TF fetch
  __device__ static __forceinline__ float fetch_table(const VctArgs& Q, const uint16_t* __restrict__ tab,
                                                      float u, float v) {
    const float x = __builtin_amdgcn_fmed3f(fmaf(u, Q.tab_w, -0.5f), 0.0f, Q.tab_w - 1.0f);
    const float y = __builtin_amdgcn_fmed3f(fmaf(v, Q.tab_h, -0.5f), 0.0f, Q.tab_h - 1.0f);
    const int ix = (int)x, iy = (int)y;
    const float ax = filter_weight<FB>(__builtin_amdgcn_fractf(x));
    const float ay = filter_weight<FB>(__builtin_amdgcn_fractf(y));
    const int x1 = min(ix + 1, Q.tab_wi - 1), y1 = min(iy + 1, Q.tab_hi - 1);
    const int r0 = iy * Q.tab_wi, r1 = y1 * Q.tab_wi;
    const float t00 = (float)__builtin_bit_cast(_Float16, tab[r0 + ix]);
    const float t10 = (float)__builtin_bit_cast(_Float16, tab[r0 + x1]);
    const float t01 = (float)__builtin_bit_cast(_Float16, tab[r1 + ix]);
    const float t11 = (float)__builtin_bit_cast(_Float16, tab[r1 + x1]);
    return lerpf(lerpf(t00, t10, ax), lerpf(t01, t11, ax), ay);
  }

  // EvaluationVoxelConeTracing (:97-144)
  __device__ static __forceinline__ float cone(const VctArgs& Q, const VctData& D, f3 tx, f3 wp,
                                               uint32_t& fetches) {
    const Rc1passArgs& A = Q.a;
    const f3 cv = normalize3(f3{A.light[0] - wp.x, A.light[1] - wp.y, A.light[2] - wp.z});
    float tvd = 1.0f;
    for (int is = 0; is < Q.samples; is++) {
      const VctStep& S = D.steps[is];                  // wave-uniform: scalar loads
      const f3 p = vmad(cv, S.xl, tx);                 // tex_pos + cone_vec * xl_x
      if (p.x < 0.0f || p.x > Q.G[0] || p.y < 0.0f || p.y > Q.G[1] || p.z < 0.0f || p.z > Q.G[2]) break;
      float mean, sd;
      fetch_level(D.pyr, S.lv[0], p, mean, sd);
      if (S.nlev == 2) {
        float m1, s1;
        fetch_level(D.pyr, S.lv[1], p, m1, s1);
        mean = lerpf(mean, m1, S.frac);
        sd = lerpf(sd, s1, S.frac);
      }
      fetches += 8u * (uint32_t)S.nlev + 4u;
      const float op = fetch_table(Q, D.table, (mean + 0.5f) / Q.max_density, (sd + 0.5f) / Q.max_stddev);
      const float opc = 1.0f - cvr_powf_nb(1.0f - op, S.expo);   // :131
      tvd = tvd * (1.0f - opc);                                   // :134
    }
    return tvd;
  }

  // ShadeSample (:146-189); `lit` counts the cones traced.
  __device__ static __forceinline__ f3 shade(const VctArgs& Q, VctData D, f3 tx, f3 wp, f3, f3 rgb,
                                             const f3* g, uint32_t& lit, uint32_t& fetches) {
    float ivd = 0.0f;
    if (Q.apply_shadow) {
      ivd = cone(Q, D, tx, wp, fetches);
      lit++;
    }
    // (:179-180, :185) the EBS tail without an occlusion term: L*ka is (L*1)*ka exactly
    return combine_sat(Q.a, Q.ka, Q.kd, Q.ks, 1.0f, ivd, wp, rgb, g);
  }
};

hipError_t launch_vct_schedule(const VctLevel* d_levels, int nl, float initial, float step, float rate,
                               float tan_apex, float corr, int n, int filter_bits, VctStep* out,
                               hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(vct_schedule_kernel, dim3(1), dim3(64), 0, s, d_levels, nl, initial, step, rate,
                     tan_apex, corr, n, filter_bits, out);
  return hipGetLastError();
}

template <class SH>
static hipError_t launch_vct_fb(const Ctx& c, const VctArgs& q, const VctData& d, float4* out,
                                uint32_t* samples, unsigned long long* shade,
                                unsigned long long* tile_samples, hipStream_t s) {
  if (c.shade_flat) return launch_shaded_flat<SH>(c, q, q.phong != 0, d, out, samples, shade, tile_samples, s);
  return launch_shaded_march<SH>(c, q, q.phong != 0, d, out, samples, shade, tile_samples, s);
}

hipError_t launch_vct(const Ctx& c, const VctArgs& q, const VctData& data, float4* out, uint32_t* samples,
                      unsigned long long* shade, unsigned long long* tile_samples, hipStream_t s) {
  if (q.a.filter_bits == 8)   // GL texture-unit weights (CVR-SPEC-8)
    return launch_vct_fb<VctShaderT<8>>(c, q, data, out, samples, shade, tile_samples, s);
  return launch_vct_fb<VctShaderT<0>>(c, q, data, out, samples, shade, tile_samples, s);
}

}  // namespace cvr
