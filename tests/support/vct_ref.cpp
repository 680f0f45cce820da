// vct_ref.cpp — CPU restatement of the voxel cone tracing renderer
// (TEST INFRASTRUCTURE ONLY, built by tests/vct_ref.py).
//
//  * vctref_pyramid:     PreProcessSuperVoxels (preprocessingstages.cpp:35-145) in double,
//                        the stored texels rounded double -> float -> binary16;
//  * vctref_table:       PreProcessPreIntegrationTable (:147-202), the loop as written;
//  * vctref_render_rows: vct_ray_bbox_marching.comp carried through in float.
//
// The oracle is frozen, so this file includes its translation unit: Tex, tf_lookup,
// filter_weight, the camera and slab code of shaded_march_rows, cvr_expf / cvr_logf /
// cvr_powf and oracle_tf_get live there and are the very functions the pinned oracles
// run.  New here is only the text this renderer adds to CVR-SPEC (DESIGN.md §5d″).
// Built with the oracle's flags (-ffp-contract=off: explicit fmaf only).
#include "../../oracle/cvr_oracle.cpp"

#include <atomic>

constexpr int kVctMaxLevels = 16;

struct VctRef {
  OracleRc1pass base;          // volume, TF, gradient, camera, W, H, step, phong, ka/kd/ks/shininess, light
  const float* pyr;            // (mean, stddev) pairs, binary16-rounded, the levels concatenated
  int32_t nl;
  int32_t dims[kVctMaxLevels][3];
  const float* table;          // tab_h rows of 255, binary16-rounded
  int32_t tab_h;
  double max_stddev;
  int32_t apply_occlusion, apply_shadow;
  float cone_step, cone_rate, cone_initial, cone_angle_deg;
  int32_t apply_correction;
  float correction_factor;
  int32_t samples;
  // out: [0] cones traced, [1] cones cut by the box, [2] cones that ran every sample,
  // [3] fetches of level 0 alone, [4] fetches of the last level alone, [5] bit l0 set for
  // every blended pair (l0, l0 + 1) fetched, [6] texel fetches (8 per level + 4 per table)
  uint64_t stats[8];
};

// Levels concatenated into out_rg (2 floats per texel); returns the level count.
extern "C" __attribute__((visibility("default"))) int vctref_pyramid(const uint8_t* vox, int w0, int h0, int d0,
                                                                     float* out_rg, int32_t* dims,
                                                                     double* max_stddev) {
  std::vector<double> prev((size_t)w0 * h0 * d0), cur;
  for (size_t i = 0; i < prev.size(); i++) {
    prev[i] = ((double)vox[i] / (256.0 - 1.0)) * 255.0;   // GetNormalizedSample * 255.0 (:54)
    out_rg[2 * i] = q16((float)prev[i]);
    out_rg[2 * i + 1] = q16((float)0.0);
  }
  dims[0] = w0; dims[1] = h0; dims[2] = d0;
  int nl = 1;
  size_t off = prev.size();
  double mx = 0.0;
  int vw = w0, vh = h0;
  for (int w = w0 / 2, h = h0 / 2, d = d0 / 2; w * h * d >= 1 && nl < kVctMaxLevels; w /= 2, h /= 2, d /= 2, nl++) {
    cur.assign((size_t)w * h * d, 0.0);
    for (int id = 0; id < d; id++)
      for (int ih = 0; ih < h; ih++)
        for (int iw = 0; iw < w; iw++) {
          double vm[8];
          for (int k = 0; k < 8; k++)   // vm_k: x + (k >> 2), y + ((k >> 1) & 1), z + (k & 1) (:83-90)
            vm[k] = prev[(size_t)(2 * iw + (k >> 2)) +
                         ((size_t)(2 * ih + ((k >> 1) & 1)) + (size_t)(2 * id + (k & 1)) * vh) * vw];
          const double mean = (((((((vm[0] + vm[1]) + vm[2]) + vm[3]) + vm[4]) + vm[5]) + vm[6]) + vm[7]) / 8.0;
          double acc = (vm[0] - mean) * (vm[0] - mean);   // pow(., 2.0) as a product (CVR-SPEC)
          for (int k = 1; k < 8; k++) acc = acc + (vm[k] - mean) * (vm[k] - mean);
          const double sd = std::sqrt(acc / 8.0);
          const size_t i = (size_t)iw + ((size_t)ih + (size_t)id * h) * w;
          cur[i] = mean;
          out_rg[2 * (off + i)] = q16((float)mean);
          out_rg[2 * (off + i) + 1] = q16((float)sd);
          mx = std::max(sd, mx);
        }
    dims[3 * nl] = w; dims[3 * nl + 1] = h; dims[3 * nl + 2] = d;
    off += cur.size();
    prev.swap(cur);
    vw = w; vh = h;
  }
  *max_stddev = mx;
  return nl;
}

// out: ceil(max_stddev) rows of 255.  tf_table: the double TF of 256 entries (oracle_tf_build_double).
extern "C" __attribute__((visibility("default"))) int vctref_table(const double* tf_table, double max_stddev,
                                                                   float* out) {
  const double dens = 256.0 - 1.0;               // GetMaxDensity()
  const int w = (int)std::ceil(dens), h = (int)std::ceil(max_stddev);
  auto opc = [&](double value) {                 // GetOpc(value, dens_val)
    float g[4];
    oracle_tf_get(tf_table, 255, value, (double)(int)dens, g);
    return g[3];
  };
  for (int iw = 0; iw < w; iw++)
    for (int ih = 0; ih < h; ih++) {
      const double mean = iw, sd = ih;
      const int dens_val = (int)dens;
      double sg = 0.0, sw = 0.0;
      if (std::fabs(sd) > 0.0001) {
        for (int i = 0; i < dens_val; i++) {
          const double x = i;
          const double nf = 1.0 / (sd * std::sqrt(2.0 * 3.14159265358979323846264338327950288));
          const double W = nf * std::exp(-((x - mean) * (x - mean)) / (2.0 * sd * sd));
          sg += W * opc(i);
          sw += W;
        }
        sg = sg / sw;
      } else {
        sg = opc(mean);
      }
      out[iw + ih * w] = q16((float)sg);
    }
  return h;
}

namespace {

inline float cvr_log2f(float x) { return cvr_logf(x) * 1.44269504088896341f; }

struct VctScene {
  const VctRef* Q;
  v3 G;
  std::vector<int64_t> off;
  int wbits;
  // one trilinear sample of level L (Tex::sample: clamp-to-edge, texel centres)
  void level(int L, v3 p, float rg[2]) const {
    const int32_t* d = Q->dims[L];
    Tex t{Q->pyr + 2 * off[L], {d[0], d[1], d[2]}, 2, wbits};
    const v3 s = mk((float)d[0] / G.x, (float)d[1] / G.y, (float)d[2] / G.z);
    t.sample(std::fmaf(p.x, s.x, -0.5f), std::fmaf(p.y, s.y, -0.5f), std::fmaf(p.z, s.z, -0.5f), rg);
  }
  // textureLod(TexSuperVoxelsVolume, p / G, lam).rg under GL_LINEAR_MIPMAP_LINEAR
  int lod(v3 p, float lam, float rg[2], uint64_t st[8]) const {
    const int nl = Q->nl;
    if (!(lam > 0.0f)) { level(0, p, rg); st[3]++; return 1; }
    if (lam >= (float)(nl - 1)) { level(nl - 1, p, rg); st[4]++; return 1; }
    const float fl = std::floor(lam);
    const int l0 = (int)fl;
    const float f = filter_weight(lam - fl, wbits);
    float a[2], b[2];
    level(l0, p, a);
    level(l0 + 1, p, b);
    rg[0] = lerpf(a[0], b[0], f);
    rg[1] = lerpf(a[1], b[1], f);
    st[5] |= 1ull << l0;
    return 2;
  }
  // texture(TexPreIntegrationLookup, (u, v)).r: bilinear, clamp-to-edge
  float lookup(float u, float v) const {
    const int w = 255, h = Q->tab_h;
    float x = std::fmaf(u, (float)w, -0.5f), y = std::fmaf(v, (float)h, -0.5f);
    x = std::fmin(std::fmax(x, -1.0f), (float)(w - 1));
    y = std::fmin(std::fmax(y, -1.0f), (float)(h - 1));
    const float flx = std::floor(x), fly = std::floor(y);
    const float ax = filter_weight(x - flx, wbits), ay = filter_weight(y - fly, wbits);
    const int ix = (int)flx, iy = (int)fly;
    const int x0 = std::max(ix, 0), x1 = std::min(ix + 1, w - 1);
    const int y0 = std::max(iy, 0), y1 = std::min(iy + 1, h - 1);
    const float* t = Q->table;
    return lerpf(lerpf(t[y0 * w + x0], t[y0 * w + x1], ax), lerpf(t[y1 * w + x0], t[y1 * w + x1], ax), ay);
  }
};

}  // namespace

// Rows [y0, y1) of the frame.  out: W*H*4, counts: W*H; returns their sum.
extern "C" __attribute__((visibility("default"))) uint64_t vctref_render_rows(VctRef* Q, int y0, int y1,
                                                                             float* out_rgba,
                                                                             uint32_t* out_counts, int nthreads) {
  const OracleRc1pass& P = Q->base;
  const v3 G = mk((float)P.N[0] * P.scale[0], (float)P.N[1] * P.scale[1], (float)P.N[2] * P.scale[2]);
  const v3 light = mk(P.light[0], P.light[1], P.light[2]);
  VctScene S{Q, G, {}, P.filter_bits};
  S.off.assign(Q->nl + 1, 0);
  for (int L = 0; L < Q->nl; L++)
    S.off[L + 1] = S.off[L] + (int64_t)Q->dims[L][0] * Q->dims[L][1] * Q->dims[L][2];
  // the uniforms of Update (vctrenderer.cpp:145-170), float
  const float tan_apex = std::tan(Q->cone_angle_deg * 3.14159265358979323846f / 180.0f);
  const float corr = (float)(Q->apply_correction ? 1 : 0) * Q->correction_factor;   // corr_fact (:97)
  const float max_density = 255.0f, max_sd = (float)Q->max_stddev;
  const float ka = Q->apply_occlusion ? P.ka : 0.0f;
  const float kd = Q->apply_shadow ? P.kd : 0.0f;
  const float ks = Q->apply_shadow ? P.ks : 0.0f;
  std::atomic<uint64_t> stats[8];
  for (auto& s : stats) s = 0;
  // EvaluationVoxelConeTracing (:97-144)
  auto cone = [&](v3 tx, v3 wp) {
    uint64_t st[8] = {};
    float tvd = 1.0f;
    const v3 cv = normalize3(mk(light.x - wp.x, light.y - wp.y, light.z - wp.z));
    float apex = Q->cone_initial, step = Q->cone_step;
    int is = 0;
    while (is < Q->samples) {
      const float xl = apex + step * 0.5f;
      const float lam = cvr_log2f(((2.0f * xl) * tan_apex) / 1.0f);
      const v3 p = vmad(cv, xl, tx);
      if (p.x < 0.0f || p.x > G.x || p.y < 0.0f || p.y > G.y || p.z < 0.0f || p.z > G.z) break;
      float rg[2];
      st[6] += 8 * S.lod(p, lam, rg, st) + 4;
      float op = S.lookup((rg[0] + 0.5f) / max_density, (rg[1] + 0.5f) / max_sd);
      op = 1.0f - cvr_powf(1.0f - op, step * corr);
      tvd = tvd * (1.0f - op);
      apex = apex + step;
      step = step * Q->cone_rate;
      is = is + 1;
    }
    st[0] = 1;
    st[is < Q->samples ? 1 : 2] = 1;
    for (int k = 0; k < 8; k++)
      if (k == 5) stats[k].fetch_or(st[k]);
      else stats[k].fetch_add(st[k]);
    return tvd;
  };
  auto shade = [&](float* src, v3 tx, v3 wp, v3, float x, float y, float z) {
    float ivd = 0.0f;
    if (Q->apply_shadow) ivd = cone(tx, wp);
    // ShadeSample (:146-189): the EBS tail without an occlusion term (L*ka is (L*1)*ka exactly)
    float g[3];
    combine_sat(P, ka, kd, ks, 1.0f, ivd, wp, src, shading_gradient(P, x, y, z, g));
  };
  const uint64_t total = shaded_march_rows(P, y0, y1, out_rgba, out_counts, nthreads, shade);
  for (int k = 0; k < 8; k++) Q->stats[k] = stats[k];
  return total;
}
