// crtgt.hip — the ground-truth cone ray-caster (cppvolrend rc1pcrtgt,
// RC1PConeLightGroundTruthSteps: gt_ray_marching.comp) on gfx950.
//
// The march is rc1pass's; every sample with alpha > 0 is shaded by brute force:
// a bundle of secondary rays marched through the volume and the TF toward the eye
// (ConeOcclusionEvaluationRayCasting, :109-169) and one toward the light
// (ConeShadowsEvaluationRayCasting, :171-252), combined by ShadeSample (:254-302).
// One shaded sample costs (rays x steps) trilinear fetches, 10^3..10^5, so the
// parallel axis is the secondary rays, not the pixels.  A frame is progressive
// (DESIGN.md §5d′): the context holds per pixel the ray parameter, the composite,
// the iteration count and a done flag, all float / integer, and a launch round
// extends every unfinished ray by at most kCrtgtRoundSamples iterations:
//   1. crtgt_march_kernel: one lane per pixel resumes from the state and advances
//      dst.a at once (alpha does not depend on the shading, the argument of
//      shaded_march.h); every sample with tau > 0 becomes a job in the pixel's own
//      slots (position, alpha, TF colour, 1 - dst.a, gradient) and its slot is
//      appended to the round's list;
//   2. crtgt_shade_kernel: one wave per job; the lanes stride over the secondary
//      rays of a table, each marching its ray; the per-ray Vt * r and r are then
//      summed in table order (lane k's values read in turn), so a term equals the
//      shader's sequential loop bit for bit;
//   3. crtgt_fold_kernel: one lane per pixel folds its jobs into dst.rgb in sample
//      order with the flat path's fma.
//
// As written in the shader, the spot light (SdwShadowType 1) tests
// `dot(v_dir, LightCamForward) < 30.0`, which always holds: its shadow term is 0.0
// for every sample.  Reproduced as written (the (u, v) swap of DOS is the precedent).
//
// CVR-SPEC arithmetic; tests/support/crtgt_ref.cpp restates it on the CPU.
// Compiled -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "cvr_device.h"
#include "march_common.h"
#include "shaded_march.h"
#include "shade_common.h"

namespace cvr {

namespace {

constexpr int K = kCrtgtRoundSamples;

// Pixel of lane `lane` of 8x8 tile `t` (whole frames only: never packed).
__device__ __forceinline__ bool gt_pixel(const Rc1passArgs& A, int t, int lane, int& px, int& py,
                                         long long& pix) {
  tile_pixel(A, t, lane & 7, lane >> 3, px, py, pix);
  return px < A.W && py < A.H;
}

// cvr_crtgt_begin: a missed pixel, and one whose box lies behind the eye (the loop
// `for (s = 0; s < D;)` never runs), is finished at once.
__global__ void __launch_bounds__(64) crtgt_init_kernel(Rc1passArgs A, CrtgtState S) {
  int px, py;
  long long pix;
  const bool inside = gt_pixel(A, blockIdx.x, threadIdx.x, px, py, pix);
  Ray r;
  const bool live = inside && ray_setup(A, px, py, r) && 0.0f < r.D;
  if (inside) {
    S.dst[pix] = make_float4(0.f, 0.f, 0.f, 0.f);
    S.s[pix] = 0.0f;
    S.cnt[pix] = 0u;
    S.done[pix] = live ? 0u : 1u;
    S.nj[pix] = 0u;
  }
  const unsigned long long n = (unsigned long long)__popcll(__ballot(live));
  if (threadIdx.x == 0 && n) atomicAdd(&S.ctr[1], n);
}

// Round step 1.  The loop of :417-473 for at most k iterations per pixel: the step of
// the shaded marches (shaded_march.h march_fetch, march_classify, march_composite),
// without a gate, resumed from the state.
template <int FB, bool PHONG>
__global__ void __launch_bounds__(64)
crtgt_march_kernel(CrtgtArgs Q, const uint4* __restrict__ cells, const uint4* __restrict__ grad,
                   const float4* __restrict__ tf_g, CrtgtState S, int k) {
  extern __shared__ float4 tfp[];
  load_tf_lds(tfp, tf_g, Q.a.tf_n);
  const Rc1passArgs& A = Q.a;
  const int lane = threadIdx.x;
  const unsigned long long lt = (1ull << lane) - 1ull;
  int px, py;
  long long pix;
  const bool inside = gt_pixel(A, blockIdx.x, lane, px, py, pix);
  Ray r;
  bool active = inside && S.done[pix] == 0u;
  if (active) (void)ray_setup(A, px, py, r);   // a pixel that is not done hit the box
  const bool wave_in_box = __ballot(active && r.outside) == 0;   // else clamp positions
  float s = 0.0f, dst_a = 0.0f;
  if (active) {
    s = S.s[pix];
    dst_a = S.dst[pix].w;
  }
  const float fn = (float)A.tf_n;
  uint32_t cnt = 0, n = 0;
  for (int it = 0; it < k; it++) {   // wave-uniform
    if (__ballot(active) == 0) break;
    bool pushed = false;
    if (active) {
      MarchFetch f = march_fetch(A, cells, r, s, wave_in_box);
      const float4 sc = march_classify<FB>(f, tfp, fn);
      cnt++;
      march_composite<PHONG>(r, f, sc, true, grad, dst_a, s, active, [&](const ShadeJob& job) {
        job.store<PHONG>(S.jobs + ((size_t)pix * K + n) * ShadeJob::f4(PHONG));
        n++;
        pushed = true;
      });
    }
    // the iteration's jobs, appended to the round's list (their order in it is free:
    // every job has its own slot, and the fold reads the slots per pixel)
    const unsigned long long m = __ballot(pushed);
    if (m) {
      unsigned long long base = 0;
      const int first = __ffsll((long long)m) - 1;
      if (lane == first) base = atomicAdd(&S.ctr[0], (unsigned long long)__popcll(m));
      base = __shfl(base, first, 64);
      if (pushed) S.list[base + __popcll(m & lt)] = (uint32_t)(pix * K + (n - 1));
    }
  }
  if (inside) {
    S.nj[pix] = n;
    if (cnt) {
      S.s[pix] = s;
      S.dst[pix].w = dst_a;
      S.cnt[pix] += cnt;
      if (!active) S.done[pix] = 1u;
    }
  }
  const unsigned long long left = (unsigned long long)__popcll(__ballot(active));
  const unsigned long long v = wave_sum(cnt);
  if (lane == 0) {
    if (left) atomicAdd(&S.ctr[1], left);
    if (v) atomicAdd(&S.ctr[2], v);
  }
}

// texture(TexTransferFunc, texture(TexVolume, p / VolumeGridSize).r).a at a position
// that may lie anywhere (clamp-to-edge): the march's volume fetch and classify, the
// alpha column only (tau: the padded column in LDS).
template <int FB>
__device__ __forceinline__ float tau_at(const Rc1passArgs& A, const uint4* __restrict__ cells,
                                        const float* __restrict__ tau, float fn, f3 p) {
  SamplePos sp = sample_pos_clamped(fmaf(p.x, A.n_over_g[0], -0.5f), fmaf(p.y, A.n_over_g[1], -0.5f),
                                    fmaf(p.z, A.n_over_g[2], -0.5f), A);
  if (FB) quantise_weights<FB>(sp);
  const float dens = trilerp_cell(cells[sp.idx], sp.ax, sp.ay, sp.az);
  const float x = fmaf(dens, fn, -0.5f);
  const float a = filter_weight<FB>(__builtin_amdgcn_fractf(x));
  const int i = cvt_flr(x) + 1;
  return lerpf(tau[i], tau[i + 1], a);
}

__device__ __forceinline__ float lane_value(float v, int k) {   // lane k's v (k wave-uniform)
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), k));
}

// The ray loop both terms share (:118-168, :202-251), by one wave: lane l marches
// rays l, l + 64, ... of the table; after each 64 the two sums take the rays'
// values in table order.  Every lane returns Socc / Swgt.
template <int FB>
__device__ float cone_rays(const CrtgtArgs& Q, const uint4* __restrict__ cells, const float* __restrict__ tau,
                           const float* __restrict__ rays, int n, float dist, f3 tx, f3 v_right, f3 v_up,
                           f3 v_dir, int lane) {
  const Rc1passArgs& A = Q.a;
  const float fn = (float)A.tf_n;
  float sacc = 0.0f, swgt = 0.0f;
  for (int base = 0; base < n; base += 64) {   // wave-uniform
    const int i = base + lane;
    float vr = 0.0f, rw = 0.0f;
    if (i < n) {
      const float cr = rays[3 * i], cg = rays[3 * i + 1], cb = rays[3 * i + 2];
      const f3 w = normalize3(f3{fmaf(v_right.x, cr, fmaf(v_up.x, cg, v_dir.x * cb)),
                                 fmaf(v_right.y, cr, fmaf(v_up.y, cg, v_dir.y * cb)),
                                 fmaf(v_right.z, cr, fmaf(v_up.z, cg, v_dir.z * cb))});
      float vt = 1.0f;
      float s = Q.light_gap;
      float st0 = tau_at<FB>(A, cells, tau, fn, vmad(w, s, tx));   // no bounds test on the first tap
      while (s < dist) {
        const float h = fminf(Q.light_step, dist - s);
        const f3 at = vmad(w, s + h, tx);
        if (at.x < 0.0f || at.x > Q.G[0] || at.y < 0.0f || at.y > Q.G[1] || at.z < 0.0f || at.z > Q.G[2])
          break;
        const float st1 = tau_at<FB>(A, cells, tau, fn, at);
        vt = vt * cvr_expf_nb(-(((st0 + st1) * 0.5f) * h));
        if ((1.0f - vt) > 0.99f) break;
        st0 = st1;
        s = s + h;
      }
      rw = dot3(v_dir, w);
      vr = vt * rw;
    }
    const int m = min(64, n - base);
    for (int k = 0; k < m; k++) {
      sacc = sacc + lane_value(vr, k);
      swgt = swgt + lane_value(rw, k);
    }
  }
  return sacc / swgt;
}

// Round step 2.  Persistent waves (4 per workgroup) stride over the round's list.
template <int FB, bool PHONG>
__global__ void __launch_bounds__(256)
crtgt_shade_kernel(CrtgtArgs Q, const uint4* __restrict__ cells, const float4* __restrict__ tf_g,
                   CrtgtState S) {
  extern __shared__ float tau[];   // the TF's padded tau column: tau[k] = T[clamp(k-1, 0, n-1)].a
  const Rc1passArgs& A = Q.a;
  for (int i = threadIdx.x; i < A.tf_n + 2; i += blockDim.x) tau[i] = tf_g[min(max(i - 1, 0), A.tf_n - 1)].w;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const unsigned long long njobs = S.ctr[0];
  const unsigned long long nwaves = (unsigned long long)gridDim.x * 4;
  for (unsigned long long j = (unsigned long long)blockIdx.x * 4 + (threadIdx.x >> 6); j < njobs; j += nwaves) {
    const uint32_t slot = S.list[j];
    float4* jp = S.jobs + (size_t)slot * ShadeJob::f4(PHONG);
    const ShadeJob job = ShadeJob::head(jp);
    const uint32_t pix = slot / K;
    const int py = (int)(pix / (uint32_t)A.W), px = (int)(pix - (uint32_t)py * (uint32_t)A.W);
    Ray r;
    (void)ray_setup(A, px, py, r);
    const f3 cam = r.cam;
    const f3 tx = job.tx;
    const f3 wp{tx.x - A.half_grid[0], tx.y - A.half_grid[1], tx.z - A.half_grid[2]};
    float iocc = 0.0f, isdw = 0.0f;
    if (Q.apply_occlusion) {
      // the per-ray frame of main (:396-399), and v_dir = normalize(-ray_dir) (:116)
      const f3 v_right = normalize3(cross3(cam, f3{0.0f, 1.0f, 0.0f}));
      const f3 v_up = normalize3(cross3(f3{-cam.x, -cam.y, -cam.z}, v_right));
      const f3 v_dir = normalize3(f3{-cam.x, -cam.y, -cam.z});
      iocc = cone_rays<FB>(Q, cells, tau, Q.occ_rays, Q.n_occ, Q.occ_distance, tx, v_right, v_up, v_dir, lane);
    }
    if (Q.apply_shadow) {
      // Not shade_common.h's shadow_cone_frame, and not to be merged with it: this
      // shader's (v_up, v_right) are not the DOS cone's (u, v) (DOS calls its cone
      // with the two swapped), its axis is LightCamForward = -light.forward (lzaxs),
      // and it tests the spot against the literal 30.0, not SpotLightMaxAngle: all
      // as gt_ray_marching.comp (:171-252) is written.
      const f3 lz{Q.lzaxs[0], Q.lzaxs[1], Q.lzaxs[2]};
      f3 v_dir, v_up, v_right;
      bool on = true;
      if (Q.shadow_type == 2) {
        v_dir = lz;
        v_up = f3{Q.lup[0], Q.lup[1], Q.lup[2]};
        v_right = f3{Q.lright[0], Q.lright[1], Q.lright[2]};
      } else {
        v_dir = normalize3(f3{A.light[0] - wp.x, A.light[1] - wp.y, A.light[2] - wp.z});
        v_up = normalize3(cross3(v_dir, f3{Q.lright[0], Q.lright[1], Q.lright[2]}));
        v_right = normalize3(cross3(v_dir, v_up));
        // :192, as written: a cosine is never >= 30, so the spot shadow term is 0.0
        if (Q.shadow_type == 1 && dot3(v_dir, lz) < 30.0f) on = false;
      }
      if (on)
        isdw = cone_rays<FB>(Q, cells, tau, Q.sdw_rays, Q.n_sdw, Q.sdw_distance, tx, v_right, v_up, v_dir, lane);
    }
    f3 g;
    if (PHONG) g = ShadeJob::grad(jp);
    // ShadeSample (:254-302): the DOS renderer's combine with vec3(1) for the specular
    // colour (A.ispec, set by the host)
    const f3 c = combine_cones(A, Q.ka, Q.kd, Q.ks, iocc, isdw, wp, job.rgb, PHONG ? &g : nullptr);
    // the record's {rgb, w} becomes {shaded rgb * a, 1 - dst.a}: what the fold reads
    if (lane == 0) jp[ShadeJob::kRgbW] = make_float4(c.x * job.a, c.y * job.a, c.z * job.a, job.w);
  }
}

// Round step 3.  dst.rgb = fma(1 - dst.a, rgb * a, dst.rgb) per job, in sample order
// (dst.a itself was advanced by the march).
__global__ void __launch_bounds__(64) crtgt_fold_kernel(Rc1passArgs A, CrtgtState S, int f4) {
  int px, py;
  long long pix;
  if (!gt_pixel(A, blockIdx.x, threadIdx.x, px, py, pix)) return;
  const uint32_t n = S.nj[pix];
  if (n == 0) return;
  float4 dst = S.dst[pix];
  for (uint32_t j = 0; j < n; j++) {
    const float4 v = S.jobs[((size_t)pix * K + j) * f4 + ShadeJob::kRgbW];
    dst.x = fmaf(v.w, v.x, dst.x);
    dst.y = fmaf(v.w, v.y, dst.y);
    dst.z = fmaf(v.w, v.z, dst.z);
  }
  S.dst[pix] = dst;
}

__global__ void __launch_bounds__(64)
crtgt_store_kernel(Rc1passArgs A, CrtgtState S, float4* __restrict__ out, uint32_t* __restrict__ samples,
                   unsigned long long* __restrict__ total, int half) {
  if (blockIdx.x == 0 && threadIdx.x == 0 && total) atomicAdd(total, S.ctr[2]);
  int px, py;
  long long pix;
  if (!gt_pixel(A, blockIdx.x, threadIdx.x, px, py, pix)) return;
  store_rgba(out, pix, S.dst[pix], half);
  if (samples) samples[pix] = S.cnt[pix];
}

template <int FB>
hipError_t launch_round_fb(const Ctx& c, const CrtgtArgs& q, const CrtgtState& st, int k, hipStream_t s) {
  const int nt = q.a.ntiles;
  const size_t lds = (size_t)(q.a.tf_n + 2) * sizeof(float4);
  const uint4* cells = (const uint4*)c.d_cells;
  const uint4* grad = (const uint4*)c.d_grad;
  const float4* tf = (const float4*)c.d_tf;
  // 8 workgroups of 4 waves per CU, no more than the round can hold jobs
  const size_t cap = (size_t)q.a.W * q.a.H * K;
  const unsigned grid = (unsigned)std::max<size_t>(1, std::min<size_t>((size_t)std::max(c.num_cus, 1) * 8, (cap + 3) / 4));
  const size_t lds_tau = (size_t)(q.a.tf_n + 2) * sizeof(float);
  return with_phong(q.phong, [&](auto P) {
    constexpr bool PHONG = decltype(P)::value;
    hipLaunchKernelGGL((crtgt_march_kernel<FB, PHONG>), dim3(nt), dim3(64), lds, s, q, cells, grad, tf, st, k);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((crtgt_shade_kernel<FB, PHONG>), dim3(grid), dim3(256), lds_tau, s, q, cells, tf, st);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(crtgt_fold_kernel, dim3(nt), dim3(64), 0, s, q.a, st, ShadeJob::f4(PHONG));
    return hipGetLastError();
  });
}

}  // namespace

hipError_t launch_crtgt_init(const CrtgtArgs& q, const CrtgtState& st, hipStream_t s) {
  if (q.a.ntiles <= 0) return hipSuccess;
  hipLaunchKernelGGL(crtgt_init_kernel, dim3(q.a.ntiles), dim3(64), 0, s, q.a, st);
  return hipGetLastError();
}

hipError_t launch_crtgt_round(const Ctx& c, const CrtgtArgs& q, const CrtgtState& st, int k, hipStream_t s) {
  if (q.a.ntiles <= 0) return hipSuccess;
  if (q.a.tf_n > kMaxTfLds || k < 1 || k > K) return hipErrorInvalidValue;
  if (q.a.filter_bits == 8) return launch_round_fb<8>(c, q, st, k, s);
  return launch_round_fb<0>(c, q, st, k, s);
}

hipError_t launch_crtgt_store(const CrtgtArgs& q, const CrtgtState& st, float4* out, uint32_t* samples,
                              unsigned long long* total, int half, hipStream_t s) {
  if (q.a.ntiles <= 0) return hipSuccess;
  hipLaunchKernelGGL(crtgt_store_kernel, dim3(q.a.ntiles), dim3(64), 0, s, q.a, st, out, samples, total, half);
  return hipGetLastError();
}

}  // namespace cvr
