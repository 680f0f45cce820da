// advdeferred_ref.cpp — CPU restatement of the advanced deferred isosurface renderer
// (TEST INFRASTRUCTURE ONLY, built by tests/advdeferred_ref.py).
//
// cppvolrend/structured/AdvancedDeferredShading: curvature_pass.comp:18-137,
// lighting_pass.comp:36-266, CreateTransferFunctions (AdvancedDeferredShading.cpp:239-293)
// and post_process.frag, carried through in float as DESIGN.md states them: whole passes
// one after the other over full-screen planes, nothing shared with the library's host
// code.  Its geometry_pass.comp is DeferredShading's (one unused uniform apart), so the
// G-buffer comes from that renderer's restatement.
//
// The oracle is frozen, so this file includes its translation unit through
// deferred_ref.cpp: Tex, dot3 / normalize3 / cross3 / lerpf, cvr_expf and cvr_powf are the
// very functions the pinned oracles run.  Built with the oracle's flags (-ffp-contract=off).
#include "deferred_ref.cpp"

struct AdvRef {
  DeferredRef d;               // the geometry pass's query (its lighting fields unused but
                               // light, light_color, color[3], exposure, gamma, shininess, ka, kd, ks)
  float flow_speed, flow_scale, time;
  int32_t show_ridges, show_valleys;
  float accessibility;
  float screen[2];             // <= 0: the frame's width / height
  float cmap_s, cmap_v;
  // out: [0] hit-or-lit pixels (not background), [1] pixels with a NaN curvature, [2] pixels
  // with finite k1 and k2 among [0], [3] ridge pixels, [4] valley pixels (both before the
  // toggles), [5] pixels whose feature colour has red or green set (after them)
  uint64_t stats[6];
};

namespace {

constexpr int kColorMap = 256, kRidgeMap = 256;

struct v2 { float x, y; };

inline bool is_finite(float x) { return std::fabs(x) < INFINITY; }

// GL_NEAREST + GL_REPEAT on one axis (CVR-SPEC)
inline int wrap_texel(float u, int size) {
  const float f = std::floor(u * (float)size);
  if (!(std::fabs(f) < 0x1p30f)) return 0;
  const int t = (int)f % size;
  return t < 0 ? t + size : t;
}
inline size_t wrap_index(float u, float v, int W, int H) {
  return (size_t)wrap_texel(v, H) * W + wrap_texel(u, W);
}

inline v2 normalize2(v2 v) {
  const float inv = 1.0f / std::sqrt(std::fmaf(v.y, v.y, v.x * v.x));
  return v2{v.x * inv, v.y * inv};
}

inline v3 at3(const float* plane, size_t i) { return mk(plane[i * 4], plane[i * 4 + 1], plane[i * 4 + 2]); }

inline float form(v3 a, const v3 S[3], v3 b) { return dot3(a, mk(dot3(S[0], b), dot3(S[1], b), dot3(S[2], b))); }

// Result[0][0], Result[1][1] of glm::perspective(fovy in degrees, aspect, ...) in float
inline void projection_scales(const OracleRc1pass& P, float& p00, float& p11) {
  const float aspect = P.aspect > 0 ? P.aspect : (float)P.W / (float)P.H;
  const float rad = P.fovy_deg * 0.01745329251994329576923690768489f;
  const float th = std::tan(rad / 2.0f);
  p00 = 1.0f / (aspect * th);
  p11 = 1.0f / th;
}

inline void linear_axis(float u, int n, int& i0, int& i1, float& a) {
  if (!is_finite(u)) {
    i0 = i1 = 0;
    a = 0.0f;
    return;
  }
  float x = std::fmaf(u, (float)n, -0.5f);
  x = std::fmin(std::fmax(x, -1.0f), (float)(n - 1));
  const float fl = std::floor(x);
  a = x - fl;
  const int i = (int)fl;
  i0 = std::max(i, 0);
  i1 = std::min(i + 1, n - 1);
}

inline float mixf(float x, float y, float a) { return x * (1.0f - a) + y * a; }
inline float clamp01(float x) { return std::fmin(std::fmax(x, 0.0f), 1.0f); }

}  // namespace

// CreateTransferFunctions: cmap 256 x 4 (rgb, 1), ridge 256 x 256 (the .r channel)
extern "C" __attribute__((visibility("default"))) void advref_tables(float s, float v, float* cmap, float* ridge) {
  for (int i = 0; i < kColorMap; i++) {
    const float t = (float)i / (float)(kColorMap - 1);
    const float h = t * 6.0f;
    const float c = v * s;
    const float x = c * (1.0f - std::fabs(std::fmod(h, 2.0f) - 1.0f));
    const float m = v - c;
    float r, g, b;
    if (h < 1.0f) { r = c; g = x; b = 0.0f; }
    else if (h < 2.0f) { r = x; g = c; b = 0.0f; }
    else if (h < 3.0f) { r = 0.0f; g = c; b = x; }
    else if (h < 4.0f) { r = 0.0f; g = x; b = c; }
    else { r = x; g = 0.0f; b = c; }
    cmap[i * 4 + 0] = r + m;
    cmap[i * 4 + 1] = g + m;
    cmap[i * 4 + 2] = b + m;
    cmap[i * 4 + 3] = 1.0f;
  }
  if (!ridge) return;
  for (int y = 0; y < kRidgeMap; y++)
    for (int x = 0; x < kRidgeMap; x++) {
      const float k1 = ((float)x / (float)(kRidgeMap - 1)) * 2.0f - 1.0f;
      const float k2 = ((float)y / (float)(kRidgeMap - 1)) * 2.0f - 1.0f;
      ridge[y * kRidgeMap + x] = std::fmax(0.0f, k1) * (k1 > k2 ? 1.0f : 0.0f);
    }
}

// The curvature pass over a normal plane gnrm (W*H*4): curv W*H*4 as (k1, k2, dir.x, dir.y)
extern "C" __attribute__((visibility("default"))) void advref_curvature(const float* gnrm, int W, int H, float p00,
                                                                       float p11, float* curv) {
  for (int py = 0; py < H; py++)
    for (int px = 0; px < W; px++) {
      float* o = curv + ((size_t)py * W + px) * 4;
      const v3 raw = at3(gnrm, (size_t)edge_texel(py, H) * W + edge_texel(px, W));
      if (length3(raw) < 0.1f) {
        o[0] = o[1] = o[2] = o[3] = 0.0f;
        continue;
      }
      const v3 n = normalize3(raw);
      const v3 t1 = std::fabs(n.x) < std::fabs(n.y) ? normalize3(cross3(mk(1.0f, 0.0f, 0.0f), n))
                                                     : normalize3(cross3(mk(0.0f, 1.0f, 0.0f), n));
      const v3 t2 = normalize3(cross3(n, t1));
      const float tsx = 1.0f / (float)W, tsy = 1.0f / (float)H;
      const float u = ((float)px + 0.5f) * tsx, v = ((float)py + 0.5f) * tsy;
      const v3 nr = normalize3(at3(gnrm, wrap_index(u + tsx, v, W, H)));
      const v3 nl = normalize3(at3(gnrm, wrap_index(u - tsx, v, W, H)));
      const v3 nt = normalize3(at3(gnrm, wrap_index(u, v + tsy, W, H)));
      const v3 nb = normalize3(at3(gnrm, wrap_index(u, v - tsy, W, H)));
      const float dx = 2.0f * tsx, dy = 2.0f * tsy;
      const v3 r[3] = {mk(-((nr.x - nl.x) / dx), -((nr.y - nl.y) / dx), -((nr.z - nl.z) / dx)),
                       mk(-((nt.x - nb.x) / dy), -((nt.y - nb.y) / dy), -((nt.z - nb.z) / dy)),
                       mk(-0.0f, -0.0f, -0.0f)};
      const v3 Pc[3] = {mk(1.0f - n.x * n.x, (-n.x) * n.y, (-n.x) * n.z),
                        mk((-n.y) * n.x, 1.0f - n.y * n.y, (-n.y) * n.z),
                        mk((-n.z) * n.x, (-n.z) * n.y, 1.0f - n.z * n.z)};
      v3 S[3];
      for (int k = 0; k < 3; k++) S[k] = mk(dot3(r[k], Pc[0]), dot3(r[k], Pc[1]), dot3(r[k], Pc[2]));
      const float a00 = form(t1, S, t1), a01 = form(t1, S, t2);
      const float a10 = form(t2, S, t1), a11 = form(t2, S, t2);
      const float trace = a00 + a11;
      const float det = a00 * a11 - a01 * a10;
      const float disc = std::sqrt((trace * trace) / 4.0f - det);
      const float k1 = trace / 2.0f + disc;
      const float k2 = trace / 2.0f - disc;
      const v2 d{k1 - a00, a01};
      const v2 cs = (d.x == 0.0f && d.y == 0.0f) ? v2{1.0f, 0.0f} : normalize2(d);
      const v3 dir = mk(cs.x * t1.x + cs.y * t2.x, cs.x * t1.y + cs.y * t2.y, cs.x * t1.z + cs.y * t2.z);
      const v2 sd = normalize2(v2{p00 * dir.x, p11 * dir.y});
      o[0] = k1; o[1] = k2; o[2] = sd.x; o[3] = sd.y;
    }
}

// The lighting pass and the tone map over planes gpos, gnrm, curv (W*H*4 each).  lit
// (before the tone map), out (after): W*H*4; flags: W*H, bit 0 ridge, bit 1 valley (before
// the toggles).  eye: viewPos.
extern "C" __attribute__((visibility("default"))) void advref_shade(AdvRef* Q, const float* eye3, const float* gpos,
                                                                   const float* gnrm, const float* curv, int W, int H,
                                                                   float* lit, float* out, uint8_t* flags) {
  const DeferredRef& D = Q->d;
  std::vector<float> cmap((size_t)kColorMap * 4), ridge((size_t)kRidgeMap * kRidgeMap);
  advref_tables(Q->cmap_s, Q->cmap_v, cmap.data(), ridge.data());
  const float ssx = Q->screen[0] > 0.0f ? Q->screen[0] : (float)W;
  const float ssy = Q->screen[1] > 0.0f ? Q->screen[1] : (float)H;
  const v3 eye = mk(eye3[0], eye3[1], eye3[2]);
  auto K = [&](float u, float v, int ch) { return curv[wrap_index(u, v, W, H) * 4 + ch]; };
  auto directional = [&](float u, float v, v2 dir, float kc) {
    const float hx = 1.0f / (float)W, hy = 1.0f / (float)H;
    const float kf = K(u + dir.x * hx, v + dir.y * hy, 0);
    const float kb = K(u - dir.x * hx, v - dir.y * hy, 0);
    const float len = std::sqrt(std::fmaf(hy, hy, hx * hx));
    return ((kf - 2.0f * kc) + kb) / (len * len);
  };
  auto ridge_fetch = [&](float u, float v) {
    int x0, x1, y0, y1;
    float ax, ay;
    linear_axis(u, kRidgeMap, x0, x1, ax);
    linear_axis(v, kRidgeMap, y0, y1, ay);
    const float* r0 = ridge.data() + (size_t)y0 * kRidgeMap;
    const float* r1 = ridge.data() + (size_t)y1 * kRidgeMap;
    return lerpf(lerpf(r0[x0], r0[x1], ax), lerpf(r1[x0], r1[x1], ax), ay);
  };
  uint64_t surface = 0, nans = 0, finite = 0, ridges = 0, valleys = 0, featured = 0;
  for (int py = 0; py < H; py++)
    for (int px = 0; px < W; px++) {
      const size_t pix = (size_t)py * W + px;
      const size_t g = (size_t)edge_texel(py, H) * W + edge_texel(px, W);
      const v3 pos = at3(gpos, g), raw = at3(gnrm, g);
      float c[4];
      flags[pix] = 0;
      if (length3(raw) < 0.1f) {
        c[0] = c[1] = c[2] = c[3] = 1.0f;
      } else {
        surface++;
        const float u = (float)px / (float)W, v = (float)py / (float)H;
        const v3 n = normalize3(raw);
        const v3 L = normalize3(mk(D.light[0] - pos.x, D.light[1] - pos.y, D.light[2] - pos.z));
        const v3 V = normalize3(mk(eye.x - pos.x, eye.y - pos.y, eye.z - pos.z));
        const v3 Hd = normalize3(mk(L.x + V.x, L.y + V.y, L.z + V.z));
        const float diff = std::fmax(dot3(n, L), 0.0f);
        const float spec = cvr_powf(std::fmax(dot3(n, Hd), 0.0f), D.shininess);
        const float k1 = curv[g * 4], k2 = curv[g * 4 + 1];
        const v2 dir{curv[g * 4 + 2], curv[g * 4 + 3]};
        if (k1 != k1 || k2 != k2) nans++;
        if (is_finite(k1) && is_finite(k2)) finite++;
        const float mean = (k1 + k2) * 0.5f;
        int m0, m1;
        float ma;
        linear_axis(mean * 0.5f + 0.5f, kColorMap, m0, m1, ma);
        float curvature[3];
        for (int k = 0; k < 3; k++) curvature[k] = lerpf(cmap[m0 * 4 + k], cmap[m1 * 4 + k], ma);
        const float ndotv = std::fmax(dot3(n, V), 0.0f);
        const float access = clamp01(1.0f - Q->accessibility * (clamp01((-mean) * 2.0f) + (1.0f - ndotv)));
        float fr = 0.0f, fg = 0.0f, fa = 0.0f;
        const float hs = 0.5f / std::fmax(ssx, ssy);
        const float dc1 = directional(u, v, dir, k1);
        if (k1 > 0.5f && k1 > 1.2f * std::fmax(std::fabs(k2), 0.001f) && dc1 < 0.0f) {
          if (k1 >= K(u - hs, v, 0) && k1 >= K(u + hs, v, 0) && k1 >= K(u, v + hs, 0) && k1 >= K(u, v - hs, 0)) {
            fr = 1.0f;
            fa = 0.8f;
          }
        }
        const float dc2 = directional(u, v, v2{-dir.y, dir.x}, k1);
        if (k2 < -0.5f && std::fabs(k2) > 1.2f * std::fmax(std::fabs(k1), 0.001f) && dc2 > 0.0f) {
          if (k2 <= K(u - hs, v, 1) && k2 <= K(u + hs, v, 1) && k2 <= K(u, v + hs, 1) && k2 <= K(u, v - hs, 1)) {
            fg = 1.0f;
            fa = 0.8f;
          }
        }
        flags[pix] = (uint8_t)((fr != 0.0f ? 1 : 0) | (fg != 0.0f ? 2 : 0));
        ridges += fr != 0.0f;
        valleys += fg != 0.0f;
        if (!Q->show_ridges) fr = 0.0f;
        if (!Q->show_valleys) fg = 0.0f;
        featured += (fr != 0.0f || fg != 0.0f);
        const float fx = u * Q->flow_scale + (dir.x * Q->time) * Q->flow_speed;
        const float fy = v * Q->flow_scale + (dir.y * Q->time) * Q->flow_speed;
        const float noise1 = ridge_fetch(fx, fy);
        const float noise2 = ridge_fetch(fx * 2.0f + Q->time * 0.5f, fy * 2.0f + Q->time * 0.5f);
        const float flow = mixf(noise1, noise2, 0.5f);
        const float feature[3] = {fr, fg, 0.0f};
        for (int k = 0; k < 3; k++) {
          const float ambient = D.ka * D.light_color[k];
          const float diffuse = (D.kd * diff) * D.light_color[k];
          const float specular = (D.ks * spec) * D.light_color[k];
          float f = (ambient + diffuse) + specular;
          f = f * access;
          f = mixf(f, curvature[k], 0.3f);
          f = mixf(f, feature[k], fa * 0.5f);
          c[k] = mixf(f, flow, 0.2f);
        }
        c[3] = D.color[3];
      }
      for (int k = 0; k < 4; k++) lit[pix * 4 + k] = c[k];
      for (int k = 0; k < 3; k++) {
        float r = c[k];
        if (D.exposure > 0.0f) r = 1.0f - cvr_expf((-r) * D.exposure);
        if (D.gamma > 0.0f) r = cvr_powf(r, 1.0f / D.gamma);
        out[pix * 4 + k] = r;
      }
      out[pix * 4 + 3] = c[3];
    }
  Q->stats[0] = surface;
  Q->stats[1] = nans;
  Q->stats[2] = finite;
  Q->stats[3] = ridges;
  Q->stats[4] = valleys;
  Q->stats[5] = featured;
}

// One frame: DeferredShading's geometry pass (its lit frame goes to scratch), the
// curvature pass for the camera's projection, the lighting pass.  Returns the sum of counts.
extern "C" __attribute__((visibility("default"))) uint64_t advref_render(AdvRef* Q, float* gpos, float* gnrm,
                                                                        float* curv, float* lit, float* out,
                                                                        uint32_t* counts, uint8_t* flags,
                                                                        int nthreads) {
  const OracleRc1pass& P = Q->d.base;
  const size_t npix = (size_t)P.W * P.H;
  std::vector<float> scratch(npix * 8);
  const uint64_t total =
      deferredref_render(&Q->d, gpos, gnrm, scratch.data(), scratch.data() + npix * 4, counts, nullptr, nthreads);
  // the restated G-buffer keeps gNormal.w; the library's slot holds the count: w is not read
  float p00, p11;
  projection_scales(P, p00, p11);
  advref_curvature(gnrm, P.W, P.H, p00, p11, curv);
  advref_shade(Q, P.eye, gpos, gnrm, curv, P.W, P.H, lit, out, flags);
  return total;
}

extern "C" __attribute__((visibility("default"))) void advref_projection(const AdvRef* Q, float* p) {
  projection_scales(Q->d.base, p[0], p[1]);
}

extern "C" __attribute__((visibility("default"))) int advref_wrap_texel(float u, int size) {
  return wrap_texel(u, size);
}
