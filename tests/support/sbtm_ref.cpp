// sbtm_ref.cpp — CPU restatement of the slice-based directional occlusion renderer
// (TEST INFRASTRUCTURE ONLY, built by tests/sbtm_ref.py).
//
// sbtmdosrenderer.cpp (Update :122-174, Redraw :176-265, ComputeProxyGeometry :671-708,
// ComputeMinMaxZ* :745-777), evaluationslice.vert / .frag and the RGBA16F, GL_LINEAR,
// CLAMP_TO_EDGE attachments of layeredframebufferobject.cpp:57-62, carried through in
// float as DESIGN.md 5d''' states them: whole slices one after the other over three
// full-screen planes, nothing blocked, nothing shared with the library's host code.
//
// The oracle is frozen, so this file includes its translation unit: Tex, tf_lookup,
// filter_weight, oracle_lookat, cross3 / glm_normalize, cvr_expf and q16 are the very
// functions the pinned oracles run.  Built with the oracle's flags (-ffp-contract=off).
#include "../../oracle/cvr_oracle.cpp"

struct SbtmRef {
  OracleRc1pass base;          // volume, TF, camera, W, H, step (> 0), filter_bits
  float cone_half_angle_deg;
  int32_t grid_x, grid_y;
  float attenuation;
  int32_t max_passes;
  float z_near, z_far;
  // out: [0] passes, [1] slices drawn, [2] fetches of a texel whose pixel was discarded in
  // the slice before but written earlier (a stale value of a pixel that has left the box),
  // [3] fragments discarded by the quad test alone (inside the scaled box)
  uint64_t stats[4];
};

namespace {

struct SbtmSlice {
  float pos, depth;
  int drawn, plane;
  float c[3], cvx, cvy;
  int rx, ry;
};

struct SbtmFrame {
  float V[16], tanh, aspect;
  v3 eye, dir, right, up, half;
  float half_diag, extent, minimum_z, maximum_z;
  std::vector<float> tapx, tapy;
  std::vector<SbtmSlice> slices;   // the passes, clipped ones included
};

// The radius bound of DESIGN.md 5d''', restated: floor(D) + 1, D = q n / 2 + n (4 + 2 q) 2^-24.
int tap_radius(float cv, float pmax, int n) {
  const double q = std::fabs((double)cv) * (double)pmax;
  const double D = q * n * 0.5 + n * (4.0 + 2.0 * q) * std::ldexp(1.0, -24);
  if (!(D < 1.0e6)) return 1 << 20;
  return (int)std::floor(D) + 1;
}

void sbtm_setup(const SbtmRef& Q, SbtmFrame& F) {
  const OracleRc1pass& P = Q.base;
  oracle_lookat(P.eye, P.center, P.up, P.fovy_deg, F.V, &F.tanh);
  const float* V = F.V;
  F.aspect = P.aspect > 0 ? P.aspect : (float)P.W / (float)P.H;
  F.eye = mk(P.eye[0], P.eye[1], P.eye[2]);
  F.dir = glm_normalize(mk(-V[2], -V[6], -V[10]));
  const v3 nd = mk(-F.dir.x, -F.dir.y, -F.dir.z);
  F.right = glm_normalize(cross3(mk(0.0f, 1.0f, 0.0f), nd));
  F.up = glm_normalize(cross3(nd, F.right));
  const v3 G = mk((float)P.N[0] * P.scale[0], (float)P.N[1] * P.scale[1], (float)P.N[2] * P.scale[2]);
  F.half = mk(G.x * 0.5f, G.y * 0.5f, G.z * 0.5f);
  const double lx = P.N[0], ly = P.N[1], lz = P.N[2];
  const double diag = std::sqrt(lx * lx + ly * ly + lz * lz);
  F.half_diag = (float)(diag * 0.5f);
  F.extent = P.step * std::tan(Q.cone_half_angle_deg * 3.14159265358979323846f / 180.0f);
  const float gx = (float)Q.grid_x, gy = (float)Q.grid_y;
  float pmx = 0.0f, pmy = 0.0f;
  float g = 0.5f;
  for (int i = 0; i < Q.grid_x; i++) {
    F.tapx.push_back(((g - gx / 2.0f) / (gx / 2.0f)) * F.extent);
    pmx = std::fmax(pmx, std::fabs(F.tapx.back()));
    g += 1.0f;
  }
  g = 0.5f;
  for (int i = 0; i < Q.grid_y; i++) {
    F.tapy.push_back(((g - gy / 2.0f) / (gy / 2.0f)) * F.extent);
    pmy = std::fmax(pmy, std::fabs(F.tapy.back()));
    g += 1.0f;
  }
  F.minimum_z = +99999.0f;
  F.maximum_z = -99999.0f;
  for (int k = 0; k < 8; k++) {   // v1 .. v8 (:761-776)
    const float x = (k & 2) ? -F.half.x : F.half.x, y = (k & 1) ? -F.half.y : F.half.y,
                z = (k & 4) ? -F.half.z : F.half.z;
    const float ptz = (V[2] * x + V[6] * y) + (V[10] * z + V[14] * 1.0f);
    F.minimum_z = std::fmin(F.minimum_z, -ptz);
    F.maximum_z = std::fmax(F.maximum_z, -ptz);
  }
  const float inv_x = 1.0f / (F.aspect * F.tanh), inv_y = 1.0f / F.tanh;
  float s = F.minimum_z, d0 = 0.0f;
  int pass = 0;
  while (s < F.maximum_z && pass < Q.max_passes) {
    const float d = std::fmin(P.step, F.maximum_z - s);
    if (pass == 0) d0 = d;
    SbtmSlice S{};
    S.pos = (s + d * 0.5f) - F.minimum_z;
    S.depth = (F.minimum_z + d0 * 0.5f) + S.pos;
    S.plane = pass & 1;
    S.drawn = S.depth >= Q.z_near && S.depth <= Q.z_far;
    S.c[0] = std::fmaf(F.dir.x, S.depth, F.eye.x);
    S.c[1] = std::fmaf(F.dir.y, S.depth, F.eye.y);
    S.c[2] = std::fmaf(F.dir.z, S.depth, F.eye.z);
    S.cvx = inv_x / S.depth;
    S.cvy = inv_y / S.depth;
    S.rx = tap_radius(S.cvx, pmx, P.W);
    S.ry = tap_radius(S.cvy, pmy, P.H);
    F.slices.push_back(S);
    s = s + d;
    pass++;
  }
}

}  // namespace

// The passes of the frame: pos_from_near, depth, drawn flag and the radius bound per pass
// (arrays of `cap`); returns their number (also beyond cap).
extern "C" __attribute__((visibility("default"))) int sbtmref_slices(const SbtmRef* Q, float* pos, float* depth,
                                                                     int32_t* drawn, int32_t* rx, int32_t* ry,
                                                                     int cap) {
  SbtmFrame F;
  sbtm_setup(*Q, F);
  for (int i = 0; i < (int)F.slices.size() && i < cap; i++) {
    pos[i] = F.slices[i].pos;
    depth[i] = F.slices[i].depth;
    drawn[i] = F.slices[i].drawn;
    rx[i] = F.slices[i].rx;
    ry[i] = F.slices[i].ry;
  }
  return (int)F.slices.size();
}

// out_rgba: W*H*4 (the eye buffer's halves widened), counts: W*H, occ: 2 planes of W*H.
// Optional histories, one entry per pass and pixel, NaN where the fragment was discarded:
// hist_src (rgb, tau of the classified sample: passes*W*H*4), hist_occ (the occlusion value
// the pass wrote: passes*W*H).  reach: per pass, the largest |texel - pixel| any fetch read
// (2 ints: x, y), or null.  Returns the sum of the counts.
extern "C" __attribute__((visibility("default"))) uint64_t sbtmref_render(SbtmRef* Q, float* out_rgba,
                                                                         uint32_t* counts, float* out_occ,
                                                                         float* hist_src, float* hist_occ,
                                                                         int32_t* reach, int nthreads) {
  const OracleRc1pass& P = Q->base;
  SbtmFrame F;
  sbtm_setup(*Q, F);
  const int W = P.W, H = P.H, wb = P.filter_bits;
  const size_t npix = (size_t)W * H;
  const v3 G = mk((float)P.N[0] * P.scale[0], (float)P.N[1] * P.scale[1], (float)P.N[2] * P.scale[2]);
  const v3 nog = mk((float)P.N[0] / G.x, (float)P.N[1] / G.y, (float)P.N[2] / G.z);
  Tex vol{P.vol, {P.N[0], P.N[1], P.N[2]}, 1, wb};
  std::vector<float> eye(npix * 4, 0.0f), occ[2];
  occ[0].assign(npix, 1.0f);
  occ[1].assign(npix, 1.0f);
  std::vector<int> written[2];
  written[0].assign(npix, -1);
  written[1].assign(npix, -1);
  std::vector<uint32_t> cnt(npix, 0);
  uint64_t stale = 0, quad_only = 0, ndrawn = 0;
  const float gxy = (float)Q->grid_x * (float)Q->grid_y;
#ifdef _OPENMP
  if (nthreads > 0) omp_set_num_threads(nthreads);
#endif
  const float nanv = std::nanf("");
  for (int i = 0; i < (int)F.slices.size(); i++) {
    const SbtmSlice& S = F.slices[i];
    if (hist_src) std::fill(hist_src + (size_t)i * npix * 4, hist_src + (size_t)(i + 1) * npix * 4, nanv);
    if (hist_occ) std::fill(hist_occ + (size_t)i * npix, hist_occ + (size_t)(i + 1) * npix, nanv);
    if (reach) reach[2 * i] = reach[2 * i + 1] = 0;
    if (!S.drawn) continue;   // every fragment clipped: the planes swap all the same
    ndrawn++;
    const std::vector<float>& prev = occ[S.plane ^ 1];
    std::vector<float>& next = occ[S.plane];
    const std::vector<int>& pw = written[S.plane ^ 1];
    std::vector<int>& nw = written[S.plane];   // the pass that last wrote a pixel of the plane
    int reach_x = 0, reach_y = 0;
#pragma omp parallel for schedule(static) reduction(+ : stale, quad_only) reduction(max : reach_x, reach_y)
    for (int py = 0; py < H; py++)
      for (int px = 0; px < W; px++) {
        const size_t pix = (size_t)py * W + px;
        // texture(OcclusionBufferPrev, (u, v)).r
        auto fetch = [&](float u, float v) {
          float x = std::fmaf(u, (float)W, -0.5f), y = std::fmaf(v, (float)H, -0.5f);
          x = std::fmin(std::fmax(x, 0.0f), (float)(W - 1));
          y = std::fmin(std::fmax(y, 0.0f), (float)(H - 1));
          const float flx = std::floor(x), fly = std::floor(y);
          const float ax = filter_weight(x - flx, wb), ay = filter_weight(y - fly, wb);
          const int x0 = (int)flx, y0 = (int)fly;
          const int x1 = std::min(x0 + 1, W - 1), y1 = std::min(y0 + 1, H - 1);
          reach_x = std::max(reach_x, std::max(std::abs(x0 - px), std::abs(x1 - px)));
          reach_y = std::max(reach_y, std::max(std::abs(y0 - py), std::abs(y1 - py)));
          for (int yy : {y0, y1})
            for (int xx : {x0, x1}) {
              const int w = pw[(size_t)yy * W + xx];
              if (w >= 0 && w != i - 1) stale++;
            }
          const float r0 = lerpf(prev[(size_t)y0 * W + x0], prev[(size_t)y0 * W + x1], ax);
          const float r1 = lerpf(prev[(size_t)y1 * W + x0], prev[(size_t)y1 * W + x1], ax);
          return lerpf(r0, r1, ay);
        };
        const float u = ((float)px + 0.5f) / (float)W, v = ((float)py + 0.5f) / (float)H;
        const float vx = std::fmaf(u, 2.0f, -1.0f), vy = std::fmaf(v, 2.0f, -1.0f);
        const v3 c = mk((vx * F.tanh) * F.aspect, vy * F.tanh, -1.0f);
        const v3 d = mk(dot3(c, mk(F.V[0], F.V[1], F.V[2])), dot3(c, mk(F.V[4], F.V[5], F.V[6])),
                        dot3(c, mk(F.V[8], F.V[9], F.V[10])));
        const v3 Pw = mk(std::fmaf(d.x, S.depth, F.eye.x), std::fmaf(d.y, S.depth, F.eye.y),
                         std::fmaf(d.z, S.depth, F.eye.z));
        const v3 rel = mk(Pw.x - S.c[0], Pw.y - S.c[1], Pw.z - S.c[2]);
        const bool in_quad = std::fabs(dot3(rel, F.right)) <= F.half_diag && std::fabs(dot3(rel, F.up)) <= F.half_diag;
        const bool out_box = Pw.x > F.half.x || Pw.x < -F.half.x || Pw.y > F.half.y || Pw.y < -F.half.y ||
                             Pw.z > F.half.z || Pw.z < -F.half.z;
        if (!in_quad) {
          if (!out_box && Pw.x == Pw.x) quad_only++;
          continue;
        }
        if (out_box) continue;
        float dens, src[4];
        vol.sample(std::fmaf(Pw.x + F.half.x, nog.x, -0.5f), std::fmaf(Pw.y + F.half.y, nog.y, -0.5f),
                   std::fmaf(Pw.z + F.half.z, nog.z, -0.5f), &dens);
        tf_lookup(P.tf, P.tf_n, dens, src, wb);
        if (hist_src)
          for (int k = 0; k < 4; k++) hist_src[((size_t)i * npix + pix) * 4 + k] = src[k];
        const float e1 = -(src[3] * P.step);
        float* dst = &eye[pix * 4];
        const float o = fetch(u, v);
        const float al = 1.0f - cvr_expf(e1);
        const float om = 1.0f - dst[3];
        dst[0] = q16(std::fmaf(om, (src[0] * o) * al, dst[0]));
        dst[1] = q16(std::fmaf(om, (src[1] * o) * al, dst[1]));
        dst[2] = q16(std::fmaf(om, (src[2] * o) * al, dst[2]));
        dst[3] = q16(std::fmaf(om, al, dst[3]));
        float sum = 0.0f;
        for (int ix = 0; ix < Q->grid_x; ix++) {
          const float ptx = std::fmaf(0.5f, std::fmaf(S.cvx, F.tapx[ix], vx), 0.5f);
          for (int iy = 0; iy < Q->grid_y; iy++) {
            const float pty = std::fmaf(0.5f, std::fmaf(S.cvy, F.tapy[iy], vy), 0.5f);
            sum = sum + fetch(ptx, pty);
          }
        }
        const float on = q16((sum / gxy) * cvr_expf(e1 * Q->attenuation));
        next[pix] = on;
        nw[pix] = i;
        if (hist_occ) hist_occ[(size_t)i * npix + pix] = on;
        cnt[pix]++;
      }
    if (reach) { reach[2 * i] = reach_x; reach[2 * i + 1] = reach_y; }
  }
  uint64_t total = 0;
  for (size_t i = 0; i < npix; i++) total += cnt[i];
  std::memcpy(out_rgba, eye.data(), npix * 16);
  std::memcpy(counts, cnt.data(), npix * 4);
  std::memcpy(out_occ, occ[0].data(), npix * 4);
  std::memcpy(out_occ + npix, occ[1].data(), npix * 4);
  Q->stats[0] = F.slices.size();
  Q->stats[1] = ndrawn;
  Q->stats[2] = stale;
  Q->stats[3] = quad_only;
  return total;
}

// libm's fmaf and the oracle's expf over arrays (tests/test_sbtm.py restates the
// recurrences in numpy and needs these two operations exactly)
extern "C" __attribute__((visibility("default"))) void sbtmref_fmaf_n(const float* a, const float* b, const float* c,
                                                                     float* out, int64_t n) {
  for (int64_t i = 0; i < n; i++) out[i] = std::fmaf(a[i], b[i], c[i]);
}
extern "C" __attribute__((visibility("default"))) void sbtmref_expf_n(const float* x, float* out, int64_t n) {
  for (int64_t i = 0; i < n; i++) out[i] = cvr_expf(x[i]);
}
