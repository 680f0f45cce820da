// deferred_ref.cpp — CPU restatement of the deferred isosurface renderer
// (TEST INFRASTRUCTURE ONLY, built by tests/deferred_ref.py).
//
// cppvolrend/structured/DeferredShading: geometry_pass.comp:137-248 (with
// CalculateGradient :55-75, getBlockIndex :78-81, getBlockBounds :84-88,
// calculateNextBlockIntersection :89-129, isBlockSkippable :130-136),
// lighting_pass.comp:25-58 and post_process.frag, carried through in float as DESIGN.md
// states them: three whole passes one after the other over full-screen planes, nothing
// shared with the library's host code.
//
// The oracle is frozen, so this file includes its translation unit: Tex, oracle_lookat,
// dot3 / normalize3, cvr_expf and cvr_powf are the very functions the pinned oracles run.
// Built with the oracle's flags (-ffp-contract=off).
#include "../../oracle/cvr_oracle.cpp"

struct DeferredRef {
  OracleRc1pass base;          // volume, camera, W, H (tf, step and the Phong block unused)
  int32_t nb[3];
  const float* bmin; const float* bmax;   // nb[0]*nb[1]*nb[2] each, x fastest
  float iso, step_small, step_large, step_range;
  float color[4];
  float ka, kd, ks, shininess;
  float light_color[3], light[3];
  float exposure, gamma;
  float clear[4];
  // out: [0] hits, [1] in-box rays without a hit, [2] rays that miss the box, [3] rays
  // that took the skip branch, [4] pixels whose lighting fetch read another texel
  uint64_t stats[5];
};

namespace {

constexpr uint32_t kDeferredMaxIter = 1u << 22;   // the kernel's iteration bound

inline v3 ray_pos(v3 eye, v3 dir, float t) {
  return mk(std::fmaf(dir.x, t, eye.x), std::fmaf(dir.y, t, eye.y), std::fmaf(dir.z, t, eye.z));
}

// texture(g, vec2(pixel) / vec2(size)), GL_NEAREST (CVR-SPEC)
inline int edge_texel(int p, int s) {
  const float u = (float)p / (float)s;
  const int t = (int)std::floor(u * (float)s);
  return std::min(std::max(t, 0), s - 1);
}

inline float length3(v3 v) { return std::sqrt(dot3(v, v)); }

}  // namespace

// gpos, gnrm: W*H*4 each; lit (before the tone map), out (after): W*H*4; counts: W*H;
// unshifted (may be null): the final frame the lighting pass would give reading every
// pixel's own texel.  Returns the sum of the counts.
extern "C" __attribute__((visibility("default"))) uint64_t deferredref_render(DeferredRef* Q, float* gpos,
                                                                             float* gnrm, float* lit, float* out,
                                                                             uint32_t* counts, float* unshifted,
                                                                             int nthreads) {
  const OracleRc1pass& P = Q->base;
  float V[16], tanf;
  oracle_lookat(P.eye, P.center, P.up, P.fovy_deg, V, &tanf);
  const float aspect = P.aspect > 0 ? P.aspect : (float)P.W / (float)P.H;
  const v3 eye = mk(P.eye[0], P.eye[1], P.eye[2]);
  const float G[3] = {(float)P.N[0] * P.scale[0], (float)P.N[1] * P.scale[1], (float)P.N[2] * P.scale[2]};
  const v3 half = mk(G[0] * 0.5f, G[1] * 0.5f, G[2] * 0.5f);
  const float NoG[3] = {(float)P.N[0] / G[0], (float)P.N[1] / G[1], (float)P.N[2] / G[2]};
  const float nbf[3] = {(float)Q->nb[0], (float)Q->nb[1], (float)Q->nb[2]};
  // length(VolumeGridSize / numBlocks) * 0.5 (:201-202)
  const float bl[3] = {G[0] / nbf[0], G[1] / nbf[1], G[2] / nbf[2]};
  const float half_block = std::sqrt(std::fmaf(bl[2], bl[2], std::fmaf(bl[1], bl[1], bl[0] * bl[0]))) * 0.5f;
  Tex vol{P.vol, {P.N[0], P.N[1], P.N[2]}, 1};
  const float iso = Q->iso;
  const int W = P.W, H = P.H;
  const size_t npix = (size_t)W * H;
#ifdef _OPENMP
  if (nthreads > 0) omp_set_num_threads(nthreads);
#endif
  // texture(TexVolume, tex / VolumeGridSize).r at a texture-space position
  auto density_tex = [&](v3 tp) {
    float s;
    vol.sample(std::fmaf(tp.x, NoG[0], -0.5f), std::fmaf(tp.y, NoG[1], -0.5f), std::fmaf(tp.z, NoG[2], -0.5f), &s);
    return s;
  };
  uint64_t total = 0, hits = 0, misses = 0, off = 0, skips = 0, shifted = 0;

  // ---- geometry pass: glClear, then one invocation per pixel
#pragma omp parallel for schedule(dynamic, 1) reduction(+ : total, hits, misses, off, skips)
  for (int py = 0; py < H; py++) {
    for (int px = 0; px < W; px++) {
      const size_t pix = (size_t)py * W + px;
      for (int k = 0; k < 4; k++) gpos[pix * 4 + k] = gnrm[pix * 4 + k] = Q->clear[k];
      uint32_t cnt = 0;
      const float fx = (float)px + 0.5f, fy = (float)py + 0.5f;
      const float vx = std::fmaf(fx / (float)W, 2.0f, -1.0f);
      const float vy = std::fmaf(fy / (float)H, 2.0f, -1.0f);
      const v3 c = mk((vx * tanf) * aspect, vy * tanf, -1.0f);
      const v3 dv = mk(dot3(c, mk(V[0], V[1], V[2])), dot3(c, mk(V[4], V[5], V[6])), dot3(c, mk(V[8], V[9], V[10])));
      const v3 dir = normalize3(normalize3(dv));
      const v3 inv = mk(1.0f / dir.x, 1.0f / dir.y, 1.0f / dir.z);
      const v3 ta = mk(inv.x * (-half.x - eye.x), inv.y * (-half.y - eye.y), inv.z * (-half.z - eye.z));
      const v3 tb = mk(inv.x * (half.x - eye.x), inv.y * (half.y - eye.y), inv.z * (half.z - eye.z));
      float tnear = std::fmax(std::fmax(std::fmin(ta.x, tb.x), std::fmin(ta.y, tb.y)), std::fmin(ta.z, tb.z));
      const float tfar = std::fmin(std::fmin(std::fmax(ta.x, tb.x), std::fmax(ta.y, tb.y)), std::fmax(ta.z, tb.z));
      const bool inbox = tfar > tnear;
      tnear = std::fmax(tnear, 0.0f);
      if (!inbox) {
        off++;
        counts[pix] = 0;
        continue;
      }
      auto density = [&](float t) {
        const v3 p = ray_pos(eye, dir, t);
        return density_tex(mk(p.x + half.x, p.y + half.y, p.z + half.z));
      };
      float t = tnear;
      float prev = density(t);
      cnt++;
      bool hit = false, skipped = false;
      uint32_t iters = 0;
      const float dd[3] = {dir.x, dir.y, dir.z};
      while (t < tfar && iters < kDeferredMaxIter) {
        iters++;
        const v3 p = ray_pos(eye, dir, t);
        const float pp[3] = {p.x, p.y, p.z};
        int b[3], wr[3];
        for (int i = 0; i < 3; i++) {
          b[i] = (int)std::floor(((pp[i] + (G[i] * 0.5f)) / G[i]) * nbf[i]);
          wr[i] = ((b[i] % Q->nb[i]) + Q->nb[i]) % Q->nb[i];   // GL_REPEAT
        }
        const size_t bi = ((size_t)wr[2] * Q->nb[1] + wr[1]) * Q->nb[0] + wr[0];
        const float bmin_v = Q->bmin[bi], bmax_v = Q->bmax[bi];
        if (iso < bmin_v - 0.001f || iso > bmax_v + 0.001f) {
          skipped = true;
          float tmx[3];
          for (int i = 0; i < 3; i++) {
            const float rc = std::fabs(dd[i]) > 1e-6f ? 1.0f / dd[i]
                                                      : (dd[i] > 0.0f ? 1e6f : (dd[i] < 0.0f ? -1e6f : 0.0f));
            const float bs = G[i] / nbf[i];
            const float lo = -G[i] * 0.5f + bs * (float)b[i];
            const float hi = lo + bs;
            tmx[i] = std::fmax((lo - pp[i]) * rc, (hi - pp[i]) * rc);
          }
          float exitT = std::fmin(std::fmin(tmx[0], tmx[1]), tmx[2]);
          for (int i = 0; i < 3; i++)
            if (std::fabs(exitT - tmx[i]) < 1e-5f) exitT += 1e-4f;
          t += std::fmax(Q->step_small, exitT);
          prev = density(t);
          cnt++;
          continue;
        }
        const float cur = density(t);
        cnt++;
        const float step = std::fabs(cur - iso) < Q->step_range ? Q->step_small
                                                                : std::fmin(Q->step_large, half_block);
        const float h = std::fmin(step, tfar - t);
        prev = cur;
        t += h;
        const float dens = density(t);
        cnt++;
        if ((prev <= iso && iso < dens) || (prev >= iso && iso > dens)) {
          const float tt = (iso - prev) / (dens - prev);
          t = t - h * (1.0f - tt);
          const v3 q = ray_pos(eye, dir, t);
          const v3 ip = mk(q.x + half.x, q.y + half.y, q.z + half.z);
          const float x1 = density_tex(mk(ip.x + 1.0f, ip.y, ip.z)), x2 = density_tex(mk(ip.x - 1.0f, ip.y, ip.z));
          const float y1 = density_tex(mk(ip.x, ip.y + 1.0f, ip.z)), y2 = density_tex(mk(ip.x, ip.y - 1.0f, ip.z));
          const float z1 = density_tex(mk(ip.x, ip.y, ip.z + 1.0f)), z2 = density_tex(mk(ip.x, ip.y, ip.z - 1.0f));
          cnt += 6;
          const v3 n = normalize3(mk((x1 - x2) / 2.0f, (y1 - y2) / 2.0f, (z1 - z2) / 2.0f));
          float* gp = gpos + pix * 4;
          float* gn = gnrm + pix * 4;
          gp[0] = ip.x; gp[1] = ip.y; gp[2] = ip.z; gp[3] = 1.0f;
          gn[0] = n.x; gn[1] = n.y; gn[2] = n.z; gn[3] = 1.0f;
          hit = true;
          break;
        }
        prev = dens;
      }
      if (!hit)
        for (int k = 0; k < 4; k++) gpos[pix * 4 + k] = gnrm[pix * 4 + k] = 0.0f;
      hits += hit;
      misses += !hit;
      skips += skipped;
      counts[pix] = cnt;
      total += cnt;
    }
  }

  // ---- lighting pass, then the post-process quad
  auto light_texel = [&](size_t g, float c[4]) {
    const float* gp = gpos + g * 4;
    const float* gn = gnrm + g * 4;
    const v3 pos = mk(gp[0], gp[1], gp[2]), n = mk(gn[0], gn[1], gn[2]);
    if (length3(pos) < 0.001f || length3(n) < 0.001f) {
      c[0] = c[1] = c[2] = c[3] = 1.0f;
      return;
    }
    const v3 L = normalize3(mk(Q->light[0] - pos.x, Q->light[1] - pos.y, Q->light[2] - pos.z));
    const v3 E = normalize3(mk(eye.x - pos.x, eye.y - pos.y, eye.z - pos.z));
    const v3 Hd = normalize3(mk(L.x + E.x, L.y + E.y, L.z + E.z));
    const float diff = std::fmax(dot3(n, L), 0.0f);
    const float spec = cvr_powf(std::fmax(dot3(n, Hd), 0.0f), Q->shininess);
    for (int k = 0; k < 3; k++) {
      const float ambient = (Q->ka * Q->light_color[k]) * Q->color[k];
      const float diffuse = ((Q->kd * diff) * Q->light_color[k]) * Q->color[k];
      const float specular = (Q->ks * spec) * Q->light_color[k];
      c[k] = (ambient + diffuse) + specular;
    }
    c[3] = Q->color[3];
  };
  auto tone_map = [&](const float c[4], float* o) {
    for (int k = 0; k < 3; k++) {
      float r = c[k];
      if (Q->exposure > 0.0f) r = 1.0f - cvr_expf((-r) * Q->exposure);
      if (Q->gamma > 0.0f) r = cvr_powf(r, 1.0f / Q->gamma);
      o[k] = r;
    }
    o[3] = c[3];
  };
#pragma omp parallel for schedule(static) reduction(+ : shifted)
  for (int py = 0; py < H; py++)
    for (int px = 0; px < W; px++) {
      const size_t pix = (size_t)py * W + px;
      const int tx = edge_texel(px, W), ty = edge_texel(py, H);
      shifted += (tx != px || ty != py);
      float c[4];
      light_texel((size_t)ty * W + tx, c);
      for (int k = 0; k < 4; k++) lit[pix * 4 + k] = c[k];
      tone_map(c, out + pix * 4);
      if (unshifted) {
        light_texel(pix, c);
        tone_map(c, unshifted + pix * 4);
      }
    }
  (void)npix;
  Q->stats[0] = hits;
  Q->stats[1] = misses;
  Q->stats[2] = off;
  Q->stats[3] = skips;
  Q->stats[4] = shifted;
  return total;
}

// post_process.frag over an image of n pixels (tests restate "the tone map of the lit
// frame equals the final frame" through this entry)
extern "C" __attribute__((visibility("default"))) void deferredref_tone_map(const float* lit, float* out, int64_t n,
                                                                           float exposure, float gamma) {
  for (int64_t i = 0; i < n; i++) {
    for (int k = 0; k < 3; k++) {
      float r = lit[i * 4 + k];
      if (exposure > 0.0f) r = 1.0f - cvr_expf((-r) * exposure);
      if (gamma > 0.0f) r = cvr_powf(r, 1.0f / gamma);
      out[i * 4 + k] = r;
    }
    out[i * 4 + 3] = lit[i * 4 + 3];
  }
}

// The texel the lighting pass reads for pixel coordinate p of a side of s texels
extern "C" __attribute__((visibility("default"))) int deferredref_edge_texel(int p, int s) {
  return edge_texel(p, s);
}

// The trilinear density at texture-space positions (n x 3), for the hit-position test
extern "C" __attribute__((visibility("default"))) void deferredref_density(const DeferredRef* Q, const float* tex,
                                                                          float* out, int64_t n) {
  const OracleRc1pass& P = Q->base;
  Tex vol{P.vol, {P.N[0], P.N[1], P.N[2]}, 1};
  for (int64_t i = 0; i < n; i++) {
    const float G[3] = {(float)P.N[0] * P.scale[0], (float)P.N[1] * P.scale[1], (float)P.N[2] * P.scale[2]};
    vol.sample(std::fmaf(tex[i * 3 + 0], (float)P.N[0] / G[0], -0.5f),
               std::fmaf(tex[i * 3 + 1], (float)P.N[1] / G[1], -0.5f),
               std::fmaf(tex[i * 3 + 2], (float)P.N[2] / G[2], -0.5f), out + i);
  }
}
