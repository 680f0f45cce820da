// vct_precompute.hip — the supervoxel pyramid of the voxel cone tracing renderer
// (cppvolrend rc1pvctsg, VCTPreProcessing::PreProcessSuperVoxels,
// preprocessingstages.cpp:35-145) on gfx950.
//
// Level 0 holds mean = GetNormalizedSample * 255.0 (:54) and stddev 0; level i
// has floor(dim / 2) texels per axis and holds, per texel, the mean of its 8
// children's means, summed in the order vm0..vm7 of :83-91 (z fastest, then y,
// then x) and divided by 8.0, and sqrt(sum (vm_k - mean)^2 / 8) over those 8 means
// alone (:95-104; the children's deviations are not propagated).  All of it in
// double, in that order; the reference's pow(d, 2.0) is written d * d, the
// correctly rounded square (a CVR-SPEC decision, DESIGN.md 5d''; for 8-bit data
// the squares of the first levels are exact, so any pow agrees there).  The stored
// texel is double -> float -> binary16, as glTexImage3D(GL_RG16F, GL_FLOAT) does.
//
// Two kernels: level 1 from the voxels (level 0 recomputed on the fly and stored
// on the way), and level i >= 2 from the double means of level i - 1 in a scratch
// buffer of the levels >= 1 (1/7 of the volume in doubles).  fp64 throughput does
// not matter for a build that runs once per volume.  The maximum of the standard
// deviations is exact: a non-negative double orders as its bit pattern, so it is
// one 64-bit integer atomic max per wave.  Compiled -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "cvr_device.h"
#include "cvr_internal.h"

namespace cvr {

namespace {

__device__ __forceinline__ uint32_t rg16f(double mean, double stdv) {
  return f32_to_h16((float)mean) | (f32_to_h16((float)stdv) << 16);
}

// mean and standard deviation of 8 child means in the reference's order
__device__ __forceinline__ void supervoxel(const double vm[8], double& mean, double& stdv) {
  mean = (((((((vm[0] + vm[1]) + vm[2]) + vm[3]) + vm[4]) + vm[5]) + vm[6]) + vm[7]) / 8.0;
  double acc = (vm[0] - mean) * (vm[0] - mean);
#pragma unroll
  for (int k = 1; k < 8; k++) acc = acc + (vm[k] - mean) * (vm[k] - mean);
  stdv = sqrt(acc / 8.0);
}

__device__ __forceinline__ void wave_max_bits(double stdv, unsigned long long* max_bits) {
  unsigned long long b = (unsigned long long)__double_as_longlong(stdv);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_xor(b, off, 64);
    b = o > b ? o : b;
  }
  if ((threadIdx.x & 63) == 0) atomicMax(max_bits, b);
}

// Level 0 (every voxel, also those an odd dimension drops from level 1).
__global__ void __launch_bounds__(256)
vct_level0_kernel(const uint8_t* __restrict__ vox, size_t n, uint32_t* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  out[i] = rg16f(((double)vox[i] / (256.0 - 1.0)) * 255.0, 0.0);
}

// Level L (>= 1) from level L - 1: FROM_VOX reads the voxels (L == 1), else the
// parent's double means.  One thread per texel of level L, x fastest.
template <bool FROM_VOX>
__global__ void __launch_bounds__(256)
vct_level_kernel(const uint8_t* __restrict__ vox, const double* __restrict__ src, int pw, int ph,
                 int w, int h, int d, double* __restrict__ dst, uint32_t* __restrict__ out,
                 unsigned long long* __restrict__ max_bits) {
  const size_t n = (size_t)w * h * d;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  double stdv = 0.0;
  if (i < n) {
    const int iw = (int)(i % w), ih = (int)((i / w) % h), id = (int)(i / ((size_t)w * h));
    double vm[8];
#pragma unroll
    for (int k = 0; k < 8; k++) {
      // vm_k: x + (k >> 2), y + ((k >> 1) & 1), z + (k & 1) (:83-90)
      const size_t j = (size_t)(2 * iw + (k >> 2)) +
                       ((size_t)(2 * ih + ((k >> 1) & 1)) + (size_t)(2 * id + (k & 1)) * ph) * pw;
      vm[k] = FROM_VOX ? ((double)vox[j] / (256.0 - 1.0)) * 255.0 : src[j];
    }
    double mean;
    supervoxel(vm, mean, stdv);
    dst[i] = mean;
    out[i] = rg16f(mean, stdv);
  }
  wave_max_bits(stdv, max_bits);
}

}  // namespace

hipError_t launch_vct_pyramid(const Ctx& c, const VctLevel* lv, int nl, uint32_t* pyr, double* scratch,
                              unsigned long long* max_bits, hipStream_t s) {
  const uint8_t* vox = (const uint8_t*)c.d_vox;
  const size_t n0 = (size_t)lv[0].d[0] * lv[0].d[1] * lv[0].d[2];
  hipLaunchKernelGGL(vct_level0_kernel, dim3((unsigned)((n0 + 255) / 256)), dim3(256), 0, s, vox, n0, pyr);
  size_t soff = 0, prev = 0;   // scratch offsets of level L and of level L - 1
  for (int L = 1; L < nl; L++) {
    const int w = lv[L].d[0], h = lv[L].d[1], d = lv[L].d[2];
    const size_t n = (size_t)w * h * d;
    const dim3 grid((unsigned)((n + 255) / 256));
    if (L == 1)
      hipLaunchKernelGGL(vct_level_kernel<true>, grid, dim3(256), 0, s, vox, nullptr, lv[0].d[0],
                         lv[0].d[1], w, h, d, scratch + soff, pyr + lv[L].off, max_bits);
    else
      hipLaunchKernelGGL(vct_level_kernel<false>, grid, dim3(256), 0, s, nullptr, scratch + prev,
                         lv[L - 1].d[0], lv[L - 1].d[1], w, h, d, scratch + soff, pyr + lv[L].off,
                         max_bits);
    prev = soff;
    soff += n;
  }
  return hipGetLastError();
}

}  // namespace cvr
