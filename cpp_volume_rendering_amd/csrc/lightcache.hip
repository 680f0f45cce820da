// lightcache.hip — pre-illumination of the directional-occlusion renderer
// (cppvolrend rc1pdosct with "Use Pre-Illumination", PreIlluminationStructuredVolume)
// on gfx950.
//
//  * the light cache (lightcachecomputation.comp:523-547): for every voxel of a
//    small object-space grid (32^3 in the reference, dosrcrenderer.cpp:63-64) the
//    occlusion cone toward the eye and the shadow cone toward the light, traced
//    once and stored as (Idao, Idcs) in an RG16F 3D image;
//  * the cached march (obj_ray_marching.comp:211-333): the march of the DOS
//    renderer whose ShadeSample is one GL_LINEAR fetch of that image instead of
//    two cone traces, and which composites a sample only when occlusion or shadow
//    is on (`src.a > 0 && Shade`).
//
// The cone accumulation is dos_cones.h's cone_trace, the one the on-the-fly
// renderer runs.  The voxel position and the occlusion frame are CVR-SPEC text of
// their own (DESIGN.md §5b′); tests/support/lightcache_ref.cpp restates both
// kernels on the CPU.  Compiled -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "cvr_device.h"
#include "march_common.h"
#include "shaded_march.h"
#include "dos_cones.h"

namespace cvr {

// ---------------------------------------------------------------------------
// Light-cache computation
// ---------------------------------------------------------------------------

// One wave = one 4x4x4 block of cache voxels (lane = x + 4 y + 16 z inside it):
// the 64 cones of a wave start within 4 voxels of each other along every axis, so
// at the coarse pyramid levels their taps fall into the same extinction cells.
// Every lane walks the same section table (cone_trace's uniform loads and levels);
// voxels past a ragged edge are masked out, never clamped onto their neighbours.
// 120 VGPRs, no scratch, 4 waves/SIMD (DESIGN.md §5b′).
template <int M>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4)))
light_cache_kernel(DosArgs Q, LightCacheArgs P, const uint4* __restrict__ ext,
                   uint32_t* __restrict__ out) {
  const int lane = threadIdx.x;
  int b = blockIdx.x;
  const int bx = b % P.nb[0];
  b /= P.nb[0];
  const int by = b % P.nb[1], bz = b / P.nb[1];
  const int x = bx * 4 + (lane & 3), y = by * 4 + ((lane >> 2) & 3), z = bz * 4 + (lane >> 4);
  if (x >= P.dims[0] || y >= P.dims[1] || z >= P.dims[2]) return;
  const Rc1passArgs& A = Q.a;
  // tex_pos = (storePos + 0.5) * (VolumeScales * (VolumeDimensions / LightCacheDimensions)),
  // the parenthesised factor rounded on the host (P.vs); realpos = tex_pos - G / 2
  const f3 tx{((float)x + 0.5f) * P.vs[0], ((float)y + 0.5f) * P.vs[1], ((float)z + 0.5f) * P.vs[2]};
  const f3 wp{tx.x - A.half_grid[0], tx.y - A.half_grid[1], tx.z - A.half_grid[2]};
  float idao = 1.0f, idcs = 1.0f;
  uint32_t nf = 0;
  if (Q.apply_occlusion) {
    // OcclusionEvaluationKernel (:280-292): the cone's own axis and EyeCamUp span
    // the frame (not the pixel's camera direction and (0, 1, 0) of the on-the-fly shader)
    const f3 k = normalize3(f3{A.eye[0] - wp.x, A.eye[1] - wp.y, A.eye[2] - wp.z});
    const f3 v_right = normalize3(cross3(f3{-k.x, -k.y, -k.z}, f3{P.cam_up[0], P.cam_up[1], P.cam_up[2]}));
    const f3 v_up = normalize3(cross3(k, v_right));
    idao = cone_trace<M>(Q, Q.occ, ext, tx, k, v_up, v_right, nf);
  }
  if (Q.apply_shadow) {
    // ShadowEvaluationKernel (:492-521)
    f3 k, u, v;
    const bool on = shadow_cone_frame(Q, wp, k, u, v);
    // Cone1RayShadow(pos, k, v, u) is called as (pos, k, u, v): swapped, as on the fly
    idcs = on ? cone_trace<M>(Q, Q.sdw, ext, tx, k, v, u, nf) : 0.0f;
  }
  // imageStore into the RG16F image: two halfs, round to nearest even
  const long long i = ((long long)z * P.dims[1] + y) * P.dims[0] + x;
  out[i] = f32_to_h16(idao) | (f32_to_h16(idcs) << 16);
}

hipError_t launch_light_cache(const DosArgs& q, const LightCacheArgs& p, const uint4* ext,
                              uint32_t* out, hipStream_t s) {
  LightCacheArgs P = p;
  for (int i = 0; i < 3; i++) P.nb[i] = (p.dims[i] + 3) / 4;
  const unsigned grid = (unsigned)P.nb[0] * P.nb[1] * P.nb[2];
  if (q.a.filter_bits == 8)
    hipLaunchKernelGGL(light_cache_kernel<8>, dim3(grid), dim3(64), 0, s, q, P, ext, out);
  else
    hipLaunchKernelGGL(light_cache_kernel<0>, dim3(grid), dim3(64), 0, s, q, P, ext, out);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// ShadeSample of obj_ray_marching.comp (:211-262) for the deferred march
// ---------------------------------------------------------------------------

template <int FB>
struct PreillumShaderT {
  using Args = DosArgs;
  static constexpr int kFB = FB & 0xff;
  static constexpr int kMinWavesPerEU = 4;
  static constexpr int kFlatWavesPerEU = 4;
  using Data = LightCacheView;
  static constexpr bool kSplit = false;   // one fetch: nothing to keep out of registers

  // `Shade` (:294): with occlusion and shadow both off no sample is composited
  __device__ static __forceinline__ bool gate(const DosArgs& Q) {
    return Q.apply_occlusion != 0 || Q.apply_shadow != 0;
  }

  // texture(TexVolumeLightCache, tx_pos / VolumeScaledSizes).rg (dims <= 512 per
  // axis, checked on the host)
  __device__ static __forceinline__ void fetch(const LightCacheView& C, f3 p, float& r, float& g) {
    fetch_rg16<kFB>(C.rg, C.d, C.s, C.m, p, r, g);
  }

  __device__ static __forceinline__ f3 shade(const DosArgs& Q, const LightCacheView& C, f3 tx, f3 wp, f3 cam,
                                             f3 rgb, const f3* g, uint32_t& lit, uint32_t& fetches) {
    (void)cam;
    float ia, is;
    fetch(C, tx, ia, is);
    fetches++;
    // IOcclusion / IShadow are 0 unless their switch is on (:219-234); the rest of
    // ShadeSample is the on-the-fly renderer's combine (ka, kd, ks gated in Q)
    typename DosShaderT<FB>::Vis r{Q.apply_occlusion ? ia : 0.0f, Q.apply_shadow ? is : 0.0f};
    if (Q.apply_shadow) lit++;
    return DosShaderT<FB>::combine(Q, r, wp, rgb, g);
  }
};

template <class SH>
static hipError_t launch_preillum_fb(const Ctx& c, const DosArgs& q, const LightCacheView& v, float4* out,
                                     uint32_t* samples, unsigned long long* shade,
                                     unsigned long long* tile_samples, hipStream_t s) {
  if (c.shade_flat)
    return launch_shaded_flat<SH>(c, q, q.phong != 0, v, out, samples, shade, tile_samples, s);
  return launch_shaded_march<SH>(c, q, q.phong != 0, v, out, samples, shade, tile_samples, s);
}

hipError_t launch_preillum(const Ctx& c, const DosArgs& q, const LightCacheView& v, float4* out,
                           uint32_t* samples, unsigned long long* shade,
                           unsigned long long* tile_samples, hipStream_t s) {
  if (q.a.filter_bits == 8)   // GL texture-unit weights (CVR-SPEC-8)
    return launch_preillum_fb<PreillumShaderT<8>>(c, q, v, out, samples, shade, tile_samples, s);
  return launch_preillum_fb<PreillumShaderT<0>>(c, q, v, out, samples, shade, tile_samples, s);
}

}  // namespace cvr
