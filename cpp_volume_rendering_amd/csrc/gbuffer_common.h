// gbuffer_common.h — what the passes over the deferred G-buffer share (deferred.hip,
// advdeferred.hip): the texel a GL_NEAREST fetch at a texel edge reads, length(), and
// the pieces of a lighting pass that do not depend on the renderer: the pixel's
// G-buffer fetch, the Blinn-Phong terms, post_process.frag's tone map, the pixel's
// stores and counts, and the grid of a one-lane-per-pixel launch.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "cvr_device.h"
#include "march_common.h"

namespace cvr {

// texture(g, vec2(pixel) / vec2(size)) with GL_NEAREST: the texel of a texel edge
// (CVR-SPEC): clamp(int(floor(fl(fl(p / s) * s))), 0, s - 1)
__device__ __forceinline__ int edge_texel(int p, int s) {
  const float u = (float)p / (float)s;
  const int t = (int)floorf(u * (float)s);
  return min(max(t, 0), s - 1);
}

__device__ __forceinline__ float length3(f3 v) { return sqrtf(dot3(v, v)); }

// Pixel i of a W x H G-buffer as a lighting pass fetches it: the pixel, the texel its
// edge fetch reads, gPosition and gNormal (as stored) there, and the geometry pass's
// fetch count, which is the pixel's own (the slot of gNormal.w).
struct GBufferPixel {
  int px, py;
  long long texel;
  f3 pos, raw;
  uint32_t count;
};
__device__ __forceinline__ GBufferPixel gbuffer_fetch(const float4* __restrict__ gbuf, int W, int H,
                                                      long long npix, long long i) {
  GBufferPixel p;
  p.py = (int)(i / W);
  p.px = (int)(i - (long long)p.py * W);
  p.texel = (long long)edge_texel(p.py, H) * W + edge_texel(p.px, W);
  const float4 gp = gbuf[p.texel], gn = gbuf[npix + p.texel];
  p.count = __float_as_uint(gbuf[npix + i].w);
  p.pos = f3{gp.x, gp.y, gp.z};
  p.raw = f3{gn.x, gn.y, gn.z};
  return p;
}

// The Blinn-Phong vectors of both lighting_pass.comp files at the texture-space position
// `pos` with the unit normal n (the light and the eye are world-space, as written): the
// view vector and the diffuse and specular terms.
struct PhongTerms {
  f3 V;
  float diff, spec;
};
__device__ __forceinline__ PhongTerms gbuffer_phong(const float light[3], const float eye[3], f3 pos, f3 n,
                                                    float shininess) {
  const f3 L = normalize3(f3{light[0] - pos.x, light[1] - pos.y, light[2] - pos.z});
  const f3 V = normalize3(f3{eye[0] - pos.x, eye[1] - pos.y, eye[2] - pos.z});
  const f3 Hd = normalize3(f3{L.x + V.x, L.y + V.y, L.z + V.z});
  const float diff = fmaxf(dot3(n, L), 0.0f);
  const float spec = cvr_powf(fmaxf(dot3(n, Hd), 0.0f), shininess);
  return PhongTerms{V, diff, spec};
}

// post_process.frag: the quad samples finalImage at the pixel's centre, the texel itself
__device__ __forceinline__ void tone_map(float4& c, float exposure, float gamma) {
  if (exposure > 0.0f) {
    c.x = 1.0f - cvr_expf((-c.x) * exposure);
    c.y = 1.0f - cvr_expf((-c.y) * exposure);
    c.z = 1.0f - cvr_expf((-c.z) * exposure);
  }
  if (gamma > 0.0f) {
    const float e = 1.0f / gamma;
    c.x = cvr_powf(c.x, e);
    c.y = cvr_powf(c.y, e);
    c.z = cvr_powf(c.z, e);
  }
}

// The end of a lighting pass's lane, for every lane of the block (`inside`: the lane has
// a pixel): the pixel's colour and count, and the wave's counts added to `total`.
__device__ __forceinline__ void gbuffer_pixel_tail(bool inside, float4* __restrict__ out, long long i, float4 c,
                                                   int half, uint32_t* __restrict__ samples, uint32_t count,
                                                   unsigned long long* __restrict__ total) {
  if (inside) {
    store_rgba(out, i, c, half);
    if (samples) samples[i] = count;
  }
  if (total) {
    const unsigned long long v = wave_sum((unsigned long long)count);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(total, v);
  }
}

// One lane per pixel, 256 lanes a block (the kernels' __launch_bounds__)
constexpr int kPixelBlock = 256;
inline dim3 pixel_grid(long long npix) { return dim3((unsigned)((npix + kPixelBlock - 1) / kPixelBlock)); }

}  // namespace cvr
