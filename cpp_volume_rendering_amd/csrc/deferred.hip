// deferred.hip — the deferred isosurface renderer of cppvolrend on gfx950
// ("Deferred Rendering", cppvolrend/structured/DeferredShading):
//
//   geometry   geometry_pass.comp:137-248: a first-hit isosurface march with block
//              skipping (4^3 blocks, DeferredShading.cpp:348) that stores the hit's
//              texture-space position and its central-difference normal
//              (CalculateGradient :55-75, six more volume fetches) into the G-buffer
//   shade      lighting_pass.comp:25-58 over the G-buffer and post_process.frag's
//              tone map, fused: one lane per pixel
//
// One lane per ray (8x8 tile per wave, the iso.hip tiling).  The march is the loop of
// rc1pisodfscustom (iso.hip variant 1) up to its first hit: the same skip test with an
// epsilon of 0.001, the same exit distance with up to three 1e-4 offsets, the step from
// the current density, the hit refined as t - h * (1 - tt); the volume fetch, the block
// index, the block-table fetch, the ray's reciprocal and the exit distance are
// iso_common.h's, and what the shade pass has in common with advdeferred.hip's (the
// G-buffer fetch, the Blinn-Phong terms, the tone map, the pixel's stores and counts) is
// gbuffer_common.h's.  Every GLSL float expression
// is evaluated in the shader's order without contraction (-ffp-contract=off), as
// tests/support/deferred_ref.cpp does.  Reproduced as written: a ray that
// misses the box keeps the G-buffer's clear value and is lit; normalize(0) is NaN and
// is stored; the lighting pass subtracts the texture-space position from the
// world-space light and eye; max(x, 0) of a NaN x is 0 (fmaxf, CVR-SPEC).
// Deviation: a lane stops after kIsoMaxIter iterations (iso.hip).
#include <hip/hip_runtime.h>
#include <cstdint>

#include "cvr_device.h"
#include "march_common.h"
#include "iso_common.h"
#include "gbuffer_common.h"

namespace cvr {

namespace {

// CalculateGradient (:55-75) at the texture-space position p, h = 1: six fetches
__device__ __forceinline__ f3 deferred_normal(const Rc1passArgs& A, const uint4* __restrict__ cells, f3 p) {
  SamplePos sp;
  const float x1 = iso_density(A, cells, f3{p.x + 1.0f, p.y, p.z}, sp);
  const float x2 = iso_density(A, cells, f3{p.x - 1.0f, p.y, p.z}, sp);
  const float y1 = iso_density(A, cells, f3{p.x, p.y + 1.0f, p.z}, sp);
  const float y2 = iso_density(A, cells, f3{p.x, p.y - 1.0f, p.z}, sp);
  const float z1 = iso_density(A, cells, f3{p.x, p.y, p.z + 1.0f}, sp);
  const float z2 = iso_density(A, cells, f3{p.x, p.y, p.z - 1.0f}, sp);
  return normalize3(f3{(x1 - x2) / 2.0f, (y1 - y2) / 2.0f, (z1 - z2) / 2.0f});
}

// One ray of geometry_pass.comp's main.  `dc` is the density fetched at the current t
// when `have` says so: the density of one iteration is the currentDensity of the next,
// a fetch at an unchanged t, reused but counted as the shader fetches it.
// Returns 0: the ray misses the box (nothing stored), 1: no hit, 2: hit (pos, nrm).
__device__ int deferred_march(const IsoArgs& Q, const uint4* __restrict__ cells,
                              const float2* __restrict__ mm, int px, int py, f3& pos, f3& nrm,
                              uint32_t& fetches) {
  const Rc1passArgs& A = Q.a;
  fetches = 0;
  Ray r;
  if (!ray_setup(A, px, py, r)) return 0;
  const f3 eye{A.eye[0], A.eye[1], A.eye[2]};
  const f3 hg{A.half_grid[0], A.half_grid[1], A.half_grid[2]};
  const f3 dir = r.dir;
  const float tfar = r.tfar;
  const float iso = Q.iso;
  SamplePos sp;
  float rdir[3];
  iso_ray_recip(dir, rdir);   // rayDirRecip (:91-94), per ray
  float t = r.tnear;
  float dc = iso_density(A, cells, iso_tex(eye, dir, t, hg), sp);   // prevDensity at tnear (:163)
  fetches++;
  bool have = true;
  uint32_t iters = 0;
  while (t < tfar && iters < kIsoMaxIter) {
    iters++;
    int b[3];
    iso_block(Q, eye, dir, t, b);
    const float2 m = iso_block_range(Q, mm, b);
    if (iso < m.x - 0.001f || iso > m.y + 0.001f) {   // isBlockSkippable (:130-136)
      // calculateNextBlockIntersection (:89-129) from the current position
      const float op[3] = {fmaf(dir.x, t, eye.x), fmaf(dir.y, t, eye.y), fmaf(dir.z, t, eye.z)};
      t += fmaxf(Q.step_small, iso_block_exit(Q, b, op, rdir));
      // prevDensity = texture(newPos) (:184): fetched by the shader, overwritten before use
      fetches++;
      have = false;
      continue;
    }
    const float cur = have ? dc : iso_density(A, cells, iso_tex(eye, dir, t, hg), sp);
    fetches++;
    const float step = fabsf(cur - iso) < Q.step_range ? Q.step_small
                                                        : fminf(Q.step_large, Q.half_block_len);
    const float h = fminf(step, tfar - t);
    t += h;
    const float dens = iso_density(A, cells, iso_tex(eye, dir, t, hg), sp);
    fetches++;
    dc = dens;
    have = true;
    if ((cur <= iso && iso < dens) || (cur >= iso && iso > dens)) {
      const float tt = (iso - cur) / (dens - cur);
      t = t - h * (1.0f - tt);
      pos = iso_tex(eye, dir, t, hg);
      nrm = deferred_normal(A, cells, pos);
      fetches += 6;
      return 2;
    }
  }
  return 1;
}

__global__ void __launch_bounds__(64)
deferred_geometry_kernel(IsoArgs Q, float4 clear, const uint4* __restrict__ cells,
                         const float2* __restrict__ mm, float4* __restrict__ gbuf,
                         unsigned long long* __restrict__ hits) {
  const Rc1passArgs& A = Q.a;
  const int t = screen_tile_of_block<4>(A, blockIdx.x, A.ntiles);
  const int lane = threadIdx.x;
  int px, py;
  long long oidx;
  tile_pixel(A, t, lane & 7, lane >> 3, px, py, oidx);
  const bool inside = px < A.W && py < A.H;
  int state = 0;
  if (inside) {
    f3 pos{0.f, 0.f, 0.f}, nrm{0.f, 0.f, 0.f};
    uint32_t fetches = 0;
    state = deferred_march(Q, cells, mm, px, py, pos, nrm, fetches);
    const long long npix = (long long)A.W * A.H;
    const long long i = (long long)py * A.W + px;
    float4 gp, gn;
    if (state == 2) {
      gp = make_float4(pos.x, pos.y, pos.z, 1.0f);
      gn = make_float4(nrm.x, nrm.y, nrm.z, 0.0f);
    } else if (state == 1) {
      gp = gn = make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
      gp = gn = clear;   // nothing stored: glClear's value stays
    }
    gn.w = __uint_as_float(fetches);   // the slot of gNormal.w (= gPosition.w): the count
    gbuf[i] = gp;
    gbuf[npix + i] = gn;
  }
  const unsigned long long v = wave_sum((unsigned long long)(state == 2 ? 1u : 0u));
  if (lane == 0 && v) atomicAdd(hits, v);
}

__global__ void __launch_bounds__(256)
deferred_shade_kernel(DeferredShadeArgs Q, const float4* __restrict__ gbuf, float4* __restrict__ out,
                      int half, uint32_t* __restrict__ samples, unsigned long long* __restrict__ total) {
  const long long npix = (long long)Q.W * Q.H;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const bool inside = i < npix;
  uint32_t count = 0;
  float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (inside) {
    const GBufferPixel g = gbuffer_fetch(gbuf, Q.W, Q.H, npix, i);
    count = g.count;
    const f3 pos = g.pos, n = g.raw;
    if (length3(pos) < 0.001f || length3(n) < 0.001f) {
      c = make_float4(1.0f, 1.0f, 1.0f, 1.0f);
    } else {
      const PhongTerms ph = gbuffer_phong(Q.light, Q.eye, pos, n, Q.shininess);
      float rgb[3];
#pragma unroll
      for (int k = 0; k < 3; k++) {
        const float ambient = (Q.ka * Q.light_color[k]) * Q.color[k];
        const float diffuse = ((Q.kd * ph.diff) * Q.light_color[k]) * Q.color[k];
        const float specular = (Q.ks * ph.spec) * Q.light_color[k];
        rgb[k] = (ambient + diffuse) + specular;
      }
      c = make_float4(rgb[0], rgb[1], rgb[2], Q.color[3]);
    }
    tone_map(c, Q.exposure, Q.gamma);
  }
  gbuffer_pixel_tail(inside, out, i, c, half, samples, count, total);
}

}  // namespace

hipError_t launch_deferred_geometry(const Ctx& c, const IsoArgs& q, const float clear[4], const float2* mm,
                                    float4* gbuf, unsigned long long* hits, hipStream_t s) {
  if (q.a.ntiles <= 0) return hipSuccess;
  hipLaunchKernelGGL(deferred_geometry_kernel, dim3((unsigned)q.a.ntiles), dim3(64), 0, s, q,
                     make_float4(clear[0], clear[1], clear[2], clear[3]), (const uint4*)c.d_cells, mm, gbuf,
                     hits);
  return hipGetLastError();
}

hipError_t launch_deferred_shade(const DeferredShadeArgs& q, const float4* gbuf, float4* out, int half,
                                 uint32_t* samples, unsigned long long* total, hipStream_t s) {
  const long long npix = (long long)q.W * q.H;
  if (npix <= 0) return hipSuccess;
  hipLaunchKernelGGL(deferred_shade_kernel, pixel_grid(npix), dim3(kPixelBlock), 0, s, q, gbuf, out, half, samples,
                     total);
  return hipGetLastError();
}

}  // namespace cvr
