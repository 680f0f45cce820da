// iso_common.h — device helpers the isosurface marches share (iso.hip, deferred.hip):
// the code that is the same in rc1pisocustom, rc1pisodfscustom and DeferredShading's
// geometry pass: the volume fetch, getBlockIndex and the block-table fetch, and, for
// the two that skip a block by its exit distance, the ray's reciprocal direction and
// that distance.  Those two helpers are deferred.hip's only: iso.hip's variant 1 keeps
// its own text of them, because its register-budget-tuned kernels come out 80 and
// 128 B longer when it calls the helpers instead.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "cvr_device.h"
#include "march_common.h"

namespace cvr {

constexpr uint32_t kIsoMaxIter = 1u << 22;

// texture(TexVolume, tex / VolumeGridSize).r: the rc1pass trilinear fetch at the
// texel coordinate fma(tex, N/G, -0.5), clamped to the grid (CLAMP_TO_EDGE).
__device__ __forceinline__ float iso_density(const Rc1passArgs& A, const uint4* __restrict__ cells,
                                             f3 tex, SamplePos& sp) {
  sp = sample_pos_clamped(fmaf(tex.x, A.n_over_g[0], -0.5f), fmaf(tex.y, A.n_over_g[1], -0.5f),
                          fmaf(tex.z, A.n_over_g[2], -0.5f), A);
  return trilerp_cell(cells[sp.idx], sp.ax, sp.ay, sp.az);
}

// r.Origin + r.Dir * t + VolumeGridSize * 0.5
__device__ __forceinline__ f3 iso_tex(f3 eye, f3 dir, float t, f3 hg) {
  return f3{fmaf(dir.x, t, eye.x) + hg.x, fmaf(dir.y, t, eye.y) + hg.y, fmaf(dir.z, t, eye.z) + hg.z};
}

// getBlockIndex (:86-89): floor((pos + G/2) / G * numBlocks), pos = r.Origin + t * r.Dir
// Fast path: x * (1/G) * nb is within ~2e-5 of the exact value for the block
// counts used (<= 1024 blocks), so away from an integer its floor is the
// exact one; near an integer the correctly rounded division decides.
__device__ __forceinline__ void iso_block(const IsoArgs& Q, f3 eye, f3 dir, float t, int b[3]) {
  const float p[3] = {fmaf(dir.x, t, eye.x), fmaf(dir.y, t, eye.y), fmaf(dir.z, t, eye.z)};
#pragma unroll
  for (int i = 0; i < 3; i++) {
    const float x = p[i] + Q.a.half_grid[i];
    const float ya = (x * Q.inv_g[i]) * Q.nb[i];
    const float fa = floorf(ya);
    const float margin = fmaxf(1e-3f, fabsf(ya) * 1e-5f);
    const bool sure = (ya - fa) > margin && (fa + 1.0f - ya) > margin;
    b[i] = (int)(sure ? fa : floorf((x / Q.G[i]) * Q.nb[i]));
  }
}

// texture(TexBlockMin/Max, (idx + 0.5) / numBlocks), NEAREST + REPEAT
__device__ __forceinline__ float2 iso_block_range(const IsoArgs& Q, const float2* __restrict__ mm,
                                                  const int b[3]) {
  int w[3];
#pragma unroll
  for (int i = 0; i < 3; i++) {
    const int n = Q.nbi[i];
    const int v = b[i];
    w[i] = (v >= 0 && v < n) ? v : (v < 0 && v >= -n ? v + n : (v >= n && v < 2 * n ? v - n : ((v % n) + n) % n));
  }
  return mm[((size_t)w[2] * Q.nbi[1] + w[1]) * Q.nbi[0] + w[0]];
}

// rayDirRecip of the shaders that skip by the exit distance (the V2 file :107-110,
// geometry_pass.comp:91-94), per ray
__device__ __forceinline__ void iso_ray_recip(f3 dir, float rdir[3]) {
  const float dd[3] = {dir.x, dir.y, dir.z};
#pragma unroll
  for (int i = 0; i < 3; i++)
    rdir[i] = fabsf(dd[i]) > 1e-6f ? 1.0f / dd[i]
                                   : (dd[i] > 0.0f ? 1e6f : (dd[i] < 0.0f ? -1e6f : 0.0f));
}

// calculateNextBlockIntersection of those shaders (:105-135, :89-129) from the ray's
// position `op` at t: the exit distance of block b (getBlockBounds, from the unwrapped
// index) plus up to three 1e-4 offsets
__device__ __forceinline__ float iso_block_exit(const IsoArgs& Q, const int b[3], const float op[3],
                                                const float rdir[3]) {
  float tmax[3];
#pragma unroll
  for (int i = 0; i < 3; i++) {
    const float bmin = Q.nhg[i] + Q.bs[i] * (float)b[i];
    const float bmax = bmin + Q.bs[i];
    tmax[i] = fmaxf((bmin - op[i]) * rdir[i], (bmax - op[i]) * rdir[i]);
  }
  float exitT = fminf(fminf(tmax[0], tmax[1]), tmax[2]);
  if (fabsf(exitT - tmax[0]) < 1e-5f) exitT += 1e-4f;
  if (fabsf(exitT - tmax[1]) < 1e-5f) exitT += 1e-4f;
  if (fabsf(exitT - tmax[2]) < 1e-5f) exitT += 1e-4f;
  return exitT;
}

}  // namespace cvr
