// advdeferred.hip — the advanced deferred isosurface renderer of cppvolrend on gfx950
// ("Advanced Deferred Rendering", cppvolrend/structured/AdvancedDeferredShading): the
// two passes it adds between DeferredShading's geometry pass (deferred.hip, reused as it
// is) and its tone map:
//
//   curvature  curvature_pass.comp:18-137 over the G-buffer's normal plane: the tangent
//              frame, the four neighbour normals, the shape operator -dN * P, its 2 x 2
//              restriction, k1 / k2 and the projected direction of k1, one float4
//              (k1, k2, dir.x, dir.y) per pixel
//   shade      lighting_pass.comp:36-266 over the G-buffer and those planes (Blinn-Phong,
//              the curvature colour map, accessibility, ridge / valley lines, the flow
//              term) and post_process.frag's tone map, fused: one lane per pixel
//
// One lane per pixel, 256 lanes a block; two kernels, because the lighting pass reads the
// curvature of up to eight neighbours.  Every GLSL float expression is evaluated in the
// shader's order without contraction (-ffp-contract=off), as
// tests/support/advdeferred_ref.cpp does; dot, normalize, pow and exp are the project's
// (CVR-SPEC), a matrix product's element is the dot of a row and a column, mix(x, y, a) is
// x * (1 - a) + y * a.  Texel lookups, the curvature direction and the filtered tables are
// DESIGN.md's decisions (5d, advanced deferred shading).  Reproduced as written: NaN
// curvatures are stored and compare false; normalize of a zero projected direction is NaN;
// the second differences of both features are taken of k1; the light and the eye are
// world-space, the position texture-space.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "cvr_device.h"
#include "march_common.h"
#include "gbuffer_common.h"

namespace cvr {

namespace {

struct f2 { float x, y; };

__device__ __forceinline__ bool finitef(float x) { return fabsf(x) < __builtin_inff(); }

// texture(t, uv) with GL_NEAREST and GL_REPEAT on one axis (CVR-SPEC): floor(fl(u * size))
// modulo size; texel 0 when that product is not finite or is outside +-2^30
__device__ __forceinline__ int wrap_texel(float u, int size) {
  const float f = floorf(u * (float)size);
  if (!(fabsf(f) < 0x1p30f)) return 0;
  const int t = (int)f % size;
  return t < 0 ? t + size : t;
}

__device__ __forceinline__ long long wrap_index(float u, float v, int W, int H) {
  return (long long)wrap_texel(v, H) * W + wrap_texel(u, W);
}

// normalize of a vec2 (CVR-SPEC): v * RN(1 / RN(sqrt(fma(y, y, x * x))))
__device__ __forceinline__ f2 normalize2(f2 v) {
  const float inv = 1.0f / sqrtf(fmaf(v.y, v.y, v.x * v.x));
  return f2{v.x * inv, v.y * inv};
}

__device__ __forceinline__ f3 sub3(f3 a, f3 b) { return f3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ f3 xyz(float4 v) { return f3{v.x, v.y, v.z}; }

// the tangent frame of computeShapeOperator / computePrincipalCurvatures (:20-28, :66-72)
__device__ __forceinline__ void tangent_frame(f3 n, f3& t1, f3& t2) {
  t1 = fabsf(n.x) < fabsf(n.y) ? normalize3(cross3(f3{1.0f, 0.0f, 0.0f}, n))
                               : normalize3(cross3(f3{0.0f, 1.0f, 0.0f}, n));
  t2 = normalize3(cross3(n, t1));
}

// dot(a, S * b) for the shape operator given by its rows
__device__ __forceinline__ float form(f3 a, const f3 S[3], f3 b) {
  return dot3(a, f3{dot3(S[0], b), dot3(S[1], b), dot3(S[2], b)});
}

__global__ void __launch_bounds__(256)
adv_curvature_kernel(int W, int H, float p00, float p11, const float4* __restrict__ gbuf,
                     float4* __restrict__ curv) {
  const long long npix = (long long)W * H;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= npix) return;
  const float4* __restrict__ gnrm = gbuf + npix;
  const int py = (int)(i / W), px = (int)(i - (long long)py * W);
  const f3 raw = xyz(gnrm[(long long)edge_texel(py, H) * W + edge_texel(px, W)]);
  if (length3(raw) < 0.1f) {   // background (:113)
    curv[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    return;
  }
  const f3 n = normalize3(raw);
  f3 t1, t2;
  tangent_frame(n, t1, t2);
  // the neighbour normals at (pixel + 0.5) * texel +- texel (:31-39)
  const float tsx = 1.0f / (float)W, tsy = 1.0f / (float)H;
  const float u = ((float)px + 0.5f) * tsx, v = ((float)py + 0.5f) * tsy;
  const f3 nr = normalize3(xyz(gnrm[wrap_index(u + tsx, v, W, H)]));
  const f3 nl = normalize3(xyz(gnrm[wrap_index(u - tsx, v, W, H)]));
  const f3 nt = normalize3(xyz(gnrm[wrap_index(u, v + tsy, W, H)]));
  const f3 nb = normalize3(xyz(gnrm[wrap_index(u, v - tsy, W, H)]));
  const float dx = 2.0f * tsx, dy = 2.0f * tsy;
  const f3 ddx = sub3(nr, nl), ddy = sub3(nt, nb);
  // the rows of -dN (:53-59): -dNdx, -dNdy, -0
  const f3 r[3] = {f3{-(ddx.x / dx), -(ddx.y / dx), -(ddx.z / dx)},
                   f3{-(ddy.x / dy), -(ddy.y / dy), -(ddy.z / dy)}, f3{-0.0f, -0.0f, -0.0f}};
  // the columns of P (:46-50)
  const f3 Pc[3] = {f3{1.0f - n.x * n.x, (-n.x) * n.y, (-n.x) * n.z},
                    f3{(-n.y) * n.x, 1.0f - n.y * n.y, (-n.y) * n.z},
                    f3{(-n.z) * n.x, (-n.z) * n.y, 1.0f - n.z * n.z}};
  f3 S[3];   // the rows of -dN * P
#pragma unroll
  for (int k = 0; k < 3; k++) S[k] = f3{dot3(r[k], Pc[0]), dot3(r[k], Pc[1]), dot3(r[k], Pc[2])};
  const float a00 = form(t1, S, t1), a01 = form(t1, S, t2);
  const float a10 = form(t2, S, t1), a11 = form(t2, S, t2);
  const float trace = a00 + a11;
  const float det = a00 * a11 - a01 * a10;
  const float disc = sqrtf((trace * trace) / 4.0f - det);   // NaN below zero, stored
  const float k1 = trace / 2.0f + disc;
  const float k2 = trace / 2.0f - disc;
  // cos and sin of atan(A01, k1 - A00) without the angle (CVR-SPEC)
  const f2 d{k1 - a00, a01};
  const f2 cs = (d.x == 0.0f && d.y == 0.0f) ? f2{1.0f, 0.0f} : normalize2(d);
  const f3 dir{cs.x * t1.x + cs.y * t2.x, cs.x * t1.y + cs.y * t2.y, cs.x * t1.z + cs.y * t2.z};
  const f2 sd = normalize2(f2{p00 * dir.x, p11 * dir.y});
  curv[i] = make_float4(k1, k2, sd.x, sd.y);
}

// One axis of a GL_LINEAR, CLAMP_TO_EDGE fetch of an n-texel table (the transfer-function
// fetch's arithmetic): texels i0, i1 and the float weight; texel 0 with weight 0 when the
// coordinate is not finite
__device__ __forceinline__ void linear_axis(float u, int n, int& i0, int& i1, float& a) {
  if (!finitef(u)) {
    i0 = i1 = 0;
    a = 0.0f;
    return;
  }
  float x = fmaf(u, (float)n, -0.5f);
  x = fminf(fmaxf(x, -1.0f), (float)(n - 1));
  const float fl = floorf(x);
  a = x - fl;
  const int i = (int)fl;
  i0 = max(i, 0);
  i1 = min(i + 1, n - 1);
}

// texture(ridgeValleyMap, uv).r
__device__ __forceinline__ float ridge_fetch(const float* __restrict__ ridge, float u, float v) {
  int x0, x1, y0, y1;
  float ax, ay;
  linear_axis(u, kAdvRidgeMapSize, x0, x1, ax);
  linear_axis(v, kAdvRidgeMapSize, y0, y1, ay);
  const float* r0 = ridge + y0 * kAdvRidgeMapSize;
  const float* r1 = ridge + y1 * kAdvRidgeMapSize;
  return lerpf(lerpf(r0[x0], r0[x1], ax), lerpf(r1[x0], r1[x1], ax), ay);
}

__device__ __forceinline__ float mixf(float x, float y, float a) { return x * (1.0f - a) + y * a; }
__device__ __forceinline__ float clamp01(float x) { return fminf(fmaxf(x, 0.0f), 1.0f); }

// computeDirectionalCurvature (:36-46): the second difference of k1 along +-dir
__device__ __forceinline__ float directional(const float4* __restrict__ curv, int W, int H, float u, float v,
                                             f2 dir, float kc) {
  const float hx = 1.0f / (float)W, hy = 1.0f / (float)H;
  const float kf = curv[wrap_index(u + dir.x * hx, v + dir.y * hy, W, H)].x;
  const float kb = curv[wrap_index(u - dir.x * hx, v - dir.y * hy, W, H)].x;
  const float len = sqrtf(fmaf(hy, hy, hx * hx));
  return ((kf - 2.0f * kc) + kb) / (len * len);
}

__global__ void __launch_bounds__(256)
adv_shade_kernel(AdvShadeArgs Q, const float4* __restrict__ gbuf, const float4* __restrict__ curv,
                 const float4* __restrict__ cmap, const float* __restrict__ ridge, float4* __restrict__ out,
                 int half, uint32_t* __restrict__ samples, unsigned long long* __restrict__ total,
                 unsigned long long* __restrict__ features) {
  const int W = Q.W, H = Q.H;
  const long long npix = (long long)W * H;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const bool inside = i < npix;
  uint32_t count = 0, featured = 0;
  float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (inside) {
    const GBufferPixel g = gbuffer_fetch(gbuf, W, H, npix, i);
    count = g.count;
    if (length3(g.raw) < 0.1f) {   // background (:189)
      c = make_float4(1.0f, 1.0f, 1.0f, 1.0f);
    } else {
      const float u = (float)g.px / (float)W, v = (float)g.py / (float)H;   // texCoord (:182)
      const f3 n = normalize3(g.raw);
      const PhongTerms ph = gbuffer_phong(Q.light, Q.eye, g.pos, n, Q.shininess);
      const float4 cv = curv[g.texel];
      const float k1 = cv.x, k2 = cv.y;
      const f2 dir{cv.z, cv.w};
      // computeMeanCurvature and the colour map (:217-218)
      const float mean = (k1 + k2) * 0.5f;
      int m0, m1;
      float ma;
      linear_axis(mean * 0.5f + 0.5f, kAdvColorMapSize, m0, m1, ma);
      const float4 c0 = cmap[m0], c1 = cmap[m1];
      const float curvature[3] = {lerpf(c0.x, c1.x, ma), lerpf(c0.y, c1.y, ma), lerpf(c0.z, c1.z, ma)};
      // computeAccessibility (:88-100)
      const float ndotv = fmaxf(dot3(n, ph.V), 0.0f);
      const float access = clamp01(1.0f - Q.accessibility * (clamp01((-mean) * 2.0f) + (1.0f - ndotv)));
      // computeRidgeValley (:102-159)
      float fr = 0.0f, fg = 0.0f, fa = 0.0f;
      const float hs = 0.5f / fmaxf(Q.screen[0], Q.screen[1]);
      if (k1 > 0.5f && k1 > 1.2f * fmaxf(fabsf(k2), 0.001f) && directional(curv, W, H, u, v, dir, k1) < 0.0f) {
        const float l = curv[wrap_index(u - hs, v, W, H)].x, r = curv[wrap_index(u + hs, v, W, H)].x;
        const float up = curv[wrap_index(u, v + hs, W, H)].x, dn = curv[wrap_index(u, v - hs, W, H)].x;
        if (k1 >= l && k1 >= r && k1 >= up && k1 >= dn) {
          fr = 1.0f;
          fa = 0.8f;
        }
      }
      if (k2 < -0.5f && fabsf(k2) > 1.2f * fmaxf(fabsf(k1), 0.001f) &&
          directional(curv, W, H, u, v, f2{-dir.y, dir.x}, k1) > 0.0f) {
        const float l = curv[wrap_index(u - hs, v, W, H)].y, r = curv[wrap_index(u + hs, v, W, H)].y;
        const float up = curv[wrap_index(u, v + hs, W, H)].y, dn = curv[wrap_index(u, v - hs, W, H)].y;
        if (k2 <= l && k2 <= r && k2 <= up && k2 <= dn) {
          fg = 1.0f;
          fa = 0.8f;
        }
      }
      if (!Q.show_ridges) fr = 0.0f;   // a hidden feature keeps its alpha (:155-156)
      if (!Q.show_valleys) fg = 0.0f;
      featured = (fr != 0.0f || fg != 0.0f) ? 1u : 0u;
      // computeCurvatureFlow (:161-174)
      const float fx = u * Q.flow_scale + (dir.x * Q.time) * Q.flow_speed;
      const float fy = v * Q.flow_scale + (dir.y * Q.time) * Q.flow_speed;
      const float noise1 = ridge_fetch(ridge, fx, fy);
      const float noise2 = ridge_fetch(ridge, fx * 2.0f + Q.time * 0.5f, fy * 2.0f + Q.time * 0.5f);
      const float flow = mixf(noise1, noise2, 0.5f);
      const float feature[3] = {fr, fg, 0.0f};
      float rgb[3];
#pragma unroll
      for (int k = 0; k < 3; k++) {
        const float ambient = Q.ka * Q.light_color[k];
        const float diffuse = (Q.kd * ph.diff) * Q.light_color[k];
        const float specular = (Q.ks * ph.spec) * Q.light_color[k];
        float f = (ambient + diffuse) + specular;
        f = f * access;
        f = mixf(f, curvature[k], 0.3f);
        f = mixf(f, feature[k], fa * 0.5f);
        rgb[k] = mixf(f, flow, 0.2f);
      }
      c = make_float4(rgb[0], rgb[1], rgb[2], Q.alpha);
    }
    tone_map(c, Q.exposure, Q.gamma);
  }
  gbuffer_pixel_tail(inside, out, i, c, half, samples, count, total);
  const unsigned long long f = wave_sum((unsigned long long)featured);
  if ((threadIdx.x & 63) == 0 && f) atomicAdd(features, f);
}

}  // namespace

hipError_t launch_adv_curvature(int W, int H, float p00, float p11, const float4* gbuf, float4* curv,
                                hipStream_t s) {
  const long long npix = (long long)W * H;
  if (npix <= 0) return hipSuccess;
  hipLaunchKernelGGL(adv_curvature_kernel, pixel_grid(npix), dim3(kPixelBlock), 0, s, W, H, p00, p11, gbuf, curv);
  return hipGetLastError();
}

hipError_t launch_adv_shade(const AdvShadeArgs& q, const float4* gbuf, const float4* curv, const float4* cmap,
                            const float* ridge, float4* out, int half, uint32_t* samples,
                            unsigned long long* total, unsigned long long* features, hipStream_t s) {
  const long long npix = (long long)q.W * q.H;
  if (npix <= 0) return hipSuccess;
  hipLaunchKernelGGL(adv_shade_kernel, pixel_grid(npix), dim3(kPixelBlock), 0, s, q, gbuf, curv, cmap, ridge, out,
                     half, samples, total, features);
  return hipGetLastError();
}

}  // namespace cvr
