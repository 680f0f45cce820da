// ebs_lightcache.hip — the light cache of the extinction-based shading renderer
// (cppvolrend rc1pextbsd with "Use Pre-Illumination") on gfx950.
//
// rc1pextbsd/lightcachecomputation.comp: for every voxel of a small object-space
// grid (32^3 in the reference, ebsrenderer.cpp:46-47) the SAT ambient occlusion
// and the SAT box-chain shadow of ebs_ray_bbox_marching.comp, evaluated once at
// the voxel centre and stored as (Iao, Ids) in the RG16F image the cached march
// reads (lightcache.hip PreillumShaderT, shared with the DOS renderer).  Neither
// term reads the camera: the boxes are centred on the voxel and the chain points
// at the light, so the cache depends on the light, the shading parameters and the
// SAT only.
//
// The two terms are ebs_sat.h's, the functions the on-the-fly shader runs; new
// here is only the voxel position (DESIGN.md §5c″).  tests/support/
// ebs_lightcache_ref.cpp restates the kernel on the CPU.  Compiled -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "cvr_device.h"
#include "march_common.h"
#include "shaded_march.h"
#include "ebs_sat.h"

namespace cvr {

// One wave = one 4x4x4 block of cache voxels (lane = x + 4 y + 16 z inside it), as
// the DOS light cache: the 64 voxels of a wave lie within 4 cache voxels of each
// other, so their boxes fall into neighbouring SAT texels.  Under a point light
// close to (or inside) the volume the lanes of a wave take different chain axes
// and chain lengths: the three cone functions run one after the other under their
// lanes' masks and each lane leaves its chain loop on its own (shadow_chain keeps
// nothing wave-uniform).  Voxels past a ragged edge are masked out, never clamped
// onto their neighbours.  Registers and occupancy: DESIGN.md §5c″.
template <class L, bool R>
__global__ void __launch_bounds__(64)
ebs_light_cache_kernel(EbsArgs Q, LightCacheArgs P, typename L::Ptr __restrict__ sat,
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
  float iao = 1.0f, ids = 1.0f;
  if (Q.apply_occlusion) iao = ebs_occlusion<L>(Q, sat, tx);
  if (Q.apply_shadow) {
    const f3 cv = ebs_cone_vec(Q, f3{A.light[0], A.light[1], A.light[2]}, wp);
    uint32_t boxes = 0;
    ids = cvr_expf(-ebs_shadow_tau<L, R>(Q, sat, tx, cv, boxes));
  }
  // imageStore into the RG16F image: two halfs, round to nearest even
  const long long i = ((long long)z * P.dims[1] + y) * P.dims[0] + x;
  out[i] = f32_to_h16(iao) | (f32_to_h16(ids) << 16);
}

template <class L>
static hipError_t launch_ebs_light_cache_layout(const EbsArgs& q, const LightCacheArgs& P, unsigned grid,
                                                typename L::Ptr sat, uint32_t* out, hipStream_t s) {
  if (q.recip_cone)
    hipLaunchKernelGGL((ebs_light_cache_kernel<L, true>), dim3(grid), dim3(64), 0, s, q, P, sat, out);
  else
    hipLaunchKernelGGL((ebs_light_cache_kernel<L, false>), dim3(grid), dim3(64), 0, s, q, P, sat, out);
  return hipGetLastError();
}

hipError_t launch_ebs_light_cache(const Ctx& c, const EbsArgs& q, const LightCacheArgs& p, uint32_t* out,
                                  hipStream_t s) {
  LightCacheArgs P = p;
  for (int i = 0; i < 3; i++) P.nb[i] = (p.dims[i] + 3) / 4;
  const unsigned grid = (unsigned)P.nb[0] * P.nb[1] * P.nb[2];
  if (q.a.filter_bits == 8)   // GL texture-unit weights (CVR-SPEC-8): the cell4 copy only, as launch_ebs
    return c.sat_layout == 1
               ? hipErrorInvalidValue
               : launch_ebs_light_cache_layout<SatFB<SatCell4, 8>>(q, P, grid, c.sat.d_cells, out, s);
  if (c.sat_layout == 1) return launch_ebs_light_cache_layout<SatPlain>(q, P, grid, c.sat.d_sat, out, s);
  return launch_ebs_light_cache_layout<SatCell4>(q, P, grid, c.sat.d_cells, out, s);
}

}  // namespace cvr
