// iso_common.h — device helpers the isosurface marches share (iso.hip, deferred.hip):
// the code that is the same in rc1pisocustom, rc1pisodfscustom and DeferredShading's
// geometry pass: the volume fetch, getBlockIndex and the block-table fetch.
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

}  // namespace cvr
