// dos.hip — directional-occlusion shading (cppvolrend rc1pdosct) on gfx950.
//
//  * the extinction-coefficient mip volume (ExtinctionCoefficientVolume, custom
//    resolution path: extcoefvolumegenerator.cpp:230-408 and glslextgen/*.comp):
//    level 0 = 7^3-tap Gaussian of the TF opacity over the volume, level L = the
//    same Gaussian (sigma 2^L) over level L-1, then tau = -log(1 - opacity);
//    every level stored as fp16 (GL_R16F), x-fastest, levels concatenated;
//  * the ray-march of ray_bbox_marching.comp:658-734 with ShadeSample (:607-656):
//    for every sample with alpha > 0, a cone-traced ambient occlusion toward the
//    eye (Cone1/3/7RayOcclusion, :116-333) and a cone-traced shadow toward the
//    light (Cone1/3/7RayShadow, :337-562), each a trapezoid accumulation of
//    Gaussian-filtered extinctions along 1 -> 3 -> 7 rays.
//
// Arithmetic follows CVR-SPEC exactly as oracle/cvr_oracle.cpp (oracle_ext_volume,
// oracle_render_dos) so results are bit-identical.  Compiled -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "cvr_device.h"
#include "march_common.h"
#include "shaded_march.h"
#include "dos_cones.h"

namespace cvr {

// ---------------------------------------------------------------------------
// fp16 level sampling (trilinear, clamp-to-edge, texel-centre convention)
// ---------------------------------------------------------------------------

// x, y, z in texel space of a d[0] x d[1] x d[2] level.  Clamping to [0, d-1]
// gives the same values as GL's CLAMP_TO_EDGE on [-1, d-1] (see sample_pos).
__device__ __forceinline__ float sample_level(const uint16_t* __restrict__ lv, const int d[3],
                                              float x, float y, float z) {
  x = __builtin_amdgcn_fmed3f(x, 0.0f, (float)(d[0] - 1));
  y = __builtin_amdgcn_fmed3f(y, 0.0f, (float)(d[1] - 1));
  z = __builtin_amdgcn_fmed3f(z, 0.0f, (float)(d[2] - 1));
  const int ix = (int)x, iy = (int)y, iz = (int)z;
  const float ax = __builtin_amdgcn_fractf(x), ay = __builtin_amdgcn_fractf(y),
              az = __builtin_amdgcn_fractf(z);
  const int x1 = min(ix + 1, d[0] - 1), y1 = min(iy + 1, d[1] - 1), z1 = min(iz + 1, d[2] - 1);
  const long long sy = d[0], sz = (long long)d[0] * d[1];
  const long long r00 = iz * sz + iy * sy, r10 = iz * sz + y1 * sy;
  const long long r01 = z1 * sz + iy * sy, r11 = z1 * sz + y1 * sy;
  const float c00 = lerpf(h2f(lv[r00 + ix]), h2f(lv[r00 + x1]), ax);
  const float c10 = lerpf(h2f(lv[r10 + ix]), h2f(lv[r10 + x1]), ax);
  const float c01 = lerpf(h2f(lv[r01 + ix]), h2f(lv[r01 + x1]), ax);
  const float c11 = lerpf(h2f(lv[r11 + ix]), h2f(lv[r11 + x1]), ax);
  return lerpf(lerpf(c00, c10, ay), lerpf(c01, c11, ay), az);
}

// ---------------------------------------------------------------------------
// Extinction-coefficient volume
// ---------------------------------------------------------------------------

struct ExtBuildArgs {
  // the volume (cell8 layout, see sample_pos) and the opacity TF
  CellGrid cells;
  float nm1[3];
  int N[3];
  float G[3];                 // VolumeGridSize
  int tf_n;
  // this level
  int L;
  int d[3], pd[3];            // this level's and the previous level's dimensions
  float S;                    // sigma0 * 2^L
  float vs[3];                // G / d (voxel size)
};

// One thread per voxel of level L (gen_extcoefvol_anysize.comp:36-76 for L = 0,
// gen_extcoefvol_anysize_mmlevel.comp:35-78 for L >= 1).  The 343 tap weights are
// shared by the block (LDS).  L = 0 samples the volume cells and the opacity TF
// (padded alpha table in LDS); L >= 1 samples level L-1 (`prev`).
__global__ void __launch_bounds__(256)
ext_level_kernel(ExtBuildArgs E, const uint4* __restrict__ cells, const float4* __restrict__ tf,
                 const uint16_t* __restrict__ prev, uint16_t* __restrict__ out) {
  __shared__ float w_lds[343];
  __shared__ float a_lds[kMaxTfLds + 2];
  const float S = E.S, S3 = (S * S) * S, den = (2.0f * S) * S;
  for (int t = threadIdx.x; t < 343; t += blockDim.x) {
    const int tx = t / 49 - 3, ty = (t / 7) % 7 - 3, tz = t % 7 - 3;
    const float fx = (float)tx * S, fy = (float)ty * S, fz = (float)tz * S;
    w_lds[t] = S3 * cvr_expf(-((fx * fx + fy * fy) + fz * fz) / den);
  }
  if (E.L == 0)
    for (int i = threadIdx.x; i < E.tf_n + 2; i += blockDim.x)
      a_lds[i] = tf[min(max(i - 1, 0), E.tf_n - 1)].w;
  __syncthreads();
  const long long nv = (long long)E.d[0] * E.d[1] * E.d[2];
  const long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= nv) return;
  const int i = (int)(v % E.d[0]), j = (int)((v / E.d[0]) % E.d[1]),
            k = (int)(v / ((long long)E.d[0] * E.d[1]));
  const float gx = ((float)i + 0.5f) * E.vs[0], gy = ((float)j + 0.5f) * E.vs[1],
              gz = ((float)k + 0.5f) * E.vs[2];
  const float fn = (float)E.tf_n;
  float swc = 0.0f, sw = 0.0f;
  int t = 0;
  for (int tx = -3; tx <= 3; tx++)
    for (int ty = -3; ty <= 3; ty++)
      for (int tz = -3; tz <= 3; tz++, t++) {
        const float w = w_lds[t];
        const float px = gx + (float)tx * S, py = gy + (float)ty * S, pz = gz + (float)tz * S;
        const float ux = px / E.G[0], uy = py / E.G[1], uz = pz / E.G[2];
        float c = 0.0f;
        if (!(ux < 0.0f || uy < 0.0f || uz < 0.0f || ux > 1.0f || uy > 1.0f || uz > 1.0f)) {
          if (E.L == 0) {
            Rc1passArgs A;   // sample_pos reads only nm1 and the cell pitches
            A.nm1[0] = E.nm1[0]; A.nm1[1] = E.nm1[1]; A.nm1[2] = E.nm1[2];
            A.cells = E.cells;
            const SamplePos sp = sample_pos(fmaf(ux, (float)E.N[0], -0.5f),
                                            fmaf(uy, (float)E.N[1], -0.5f),
                                            fmaf(uz, (float)E.N[2], -0.5f), A);
            const float dens = trilerp_cell(cells[sp.idx], sp.ax, sp.ay, sp.az);
            // texture(TF, d).a: padded table, x = d*n - 0.5
            const float xt = fmaf(dens, fn, -0.5f);
            const float fl = floorf(xt);
            const int ti = (int)fl + 1;
            c = lerpf(a_lds[ti], a_lds[ti + 1], xt - fl);
          } else {
            c = sample_level(prev, E.pd, fmaf(ux, (float)E.pd[0], -0.5f),
                             fmaf(uy, (float)E.pd[1], -0.5f), fmaf(uz, (float)E.pd[2], -0.5f));
          }
        }
        swc = swc + w * c;
        sw = sw + w;
      }
  out[v] = f2h_rne(swc / sw);
}

// backtotau.comp:11-34: tau = -1 * log(1 - opacity), in place over all levels.
__global__ void ext_to_tau_kernel(uint16_t* __restrict__ lv, long long n) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) lv[i] = f2h_rne(-1.0f * cvr_logf(1.0f - h2f(lv[i])));
}

// The cone fetches read cell8 texels: texel (i, j, k) of a level holds its 8
// trilinear corners (i|i+1, j|j+1, k|k+1, the +1 clamped to the edge) as fp16,
// so one dwordx4 load feeds one fetch (the volume's own layout, see sample_pos).
__global__ void ext_cells_kernel(const uint16_t* __restrict__ lv, uint4* __restrict__ cells, int dx,
                                 int dy, int dz) {
  const long long n = (long long)dx * dy * dz;
  const long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n) return;
  const int i = (int)(v % dx), j = (int)((v / dx) % dy), k = (int)(v / ((long long)dx * dy));
  const int i1 = min(i + 1, dx - 1), j1 = min(j + 1, dy - 1), k1 = min(k + 1, dz - 1);
  const long long sy = dx, sz = (long long)dx * dy;
  auto at = [&](int x, int y, int z) -> uint32_t { return lv[z * sz + y * sy + x]; };
  uint4 c;
  c.x = at(i, j, k) | (at(i1, j, k) << 16);
  c.y = at(i, j1, k) | (at(i1, j1, k) << 16);
  c.z = at(i, j, k1) | (at(i1, j, k1) << 16);
  c.w = at(i, j1, k1) | (at(i1, j1, k1) << 16);
  cells[v] = c;
}

hipError_t launch_ext_volume(const Ctx& c, const float4* d_tf_rgba, int tf_n, const int res[3],
                             float sigma0, int nlevels, const long long* off, uint16_t* d_ext,
                             uint4* d_ext_cells, hipStream_t s) {
  if (tf_n > kMaxTfLds) return hipErrorInvalidValue;
  ExtBuildArgs E{};
  E.cells = c.cells;
  for (int i = 0; i < 3; i++) {
    E.N[i] = c.N[i];
    E.nm1[i] = (float)(c.N[i] - 1);
    E.G[i] = (float)c.N[i] * c.scale[i];
  }
  E.tf_n = tf_n;
  const uint4* cells = (const uint4*)c.d_cells;   // sample_pos indexes from the first cell
  for (int L = 0; L < nlevels; L++) {
    E.L = L;
    for (int i = 0; i < 3; i++) {
      E.d[i] = res[i] >> L > 1 ? res[i] >> L : 1;
      E.pd[i] = L == 0 ? 1 : (res[i] >> (L - 1) > 1 ? res[i] >> (L - 1) : 1);
      E.vs[i] = E.G[i] / (float)E.d[i];
    }
    E.S = L == 0 ? sigma0 : sigma0 * (float)(1 << L);
    const long long nv = (long long)E.d[0] * E.d[1] * E.d[2];
    hipLaunchKernelGGL(ext_level_kernel, dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, s, E,
                       cells, d_tf_rgba, L == 0 ? nullptr : d_ext + off[L - 1], d_ext + off[L]);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  const long long n = off[nlevels];
  hipLaunchKernelGGL(ext_to_tau_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, d_ext, n);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  for (int L = 0; L < nlevels; L++) {
    int d[3];
    for (int i = 0; i < 3; i++) d[i] = res[i] >> L > 1 ? res[i] >> L : 1;
    const long long nv = off[L + 1] - off[L];
    hipLaunchKernelGGL(ext_cells_kernel, dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, s,
                       d_ext + off[L], d_ext_cells + off[L], d[0], d[1], d[2]);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// The cone tracing and ShadeSample (DosShaderT) live in dos_cones.h.

template <class SH>
static hipError_t launch_dos_fb(const Ctx& c, const DosArgs& q, float4* out, uint32_t* samples,
                                unsigned long long* shade, unsigned long long* tile_samples, hipStream_t s) {
  if (c.shade_flat)
    return launch_shaded_flat<SH>(c, q, q.phong != 0, c.ext.d_cells, out, samples, shade, tile_samples, s);
  return launch_shaded_march<SH>(c, q, q.phong != 0, c.ext.d_cells, out, samples, shade, tile_samples, s);
}

hipError_t launch_dos(const Ctx& c, const DosArgs& q, float4* out, uint32_t* samples,
                      unsigned long long* shade, unsigned long long* tile_samples, hipStream_t s) {
  if (q.a.filter_bits == 8)   // GL texture-unit weights (CVR-SPEC-8)
    return launch_dos_fb<DosShaderT<8>>(c, q, out, samples, shade, tile_samples, s);
  if (q.a.exp_native)         // tolerance mode: the border attenuation's exp in hardware
    return launch_dos_fb<DosShaderT<kDosNativeExp>>(c, q, out, samples, shade, tile_samples, s);
  return launch_dos_fb<DosShaderT<0>>(c, q, out, samples, shade, tile_samples, s);
}

}  // namespace cvr
