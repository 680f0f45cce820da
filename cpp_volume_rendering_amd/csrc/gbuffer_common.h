// gbuffer_common.h — what the passes over the deferred G-buffer share (deferred.hip,
// advdeferred.hip): the texel a GL_NEAREST fetch at a texel edge reads, and length().
#pragma once
#include <hip/hip_runtime.h>

#include "cvr_device.h"

namespace cvr {

// texture(g, vec2(pixel) / vec2(size)) with GL_NEAREST: the texel of a texel edge
// (CVR-SPEC): clamp(int(floor(fl(fl(p / s) * s))), 0, s - 1)
__device__ __forceinline__ int edge_texel(int p, int s) {
  const float u = (float)p / (float)s;
  const int t = (int)floorf(u * (float)s);
  return min(max(t, 0), s - 1);
}

__device__ __forceinline__ float length3(f3 v) { return sqrtf(dot3(v, v)); }

}  // namespace cvr
