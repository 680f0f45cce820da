// crtgt_ref.cpp — CPU restatement of the ground-truth cone ray-caster
// (TEST INFRASTRUCTURE ONLY, built by tests/crtgt_ref.py).
//
//  * gtref_render_rows: gt_ray_marching.comp carried through in float: the march of
//    the shaded renderers with ShadeSample's two bundles of secondary rays.
//
// The oracle is frozen, so this file includes its translation unit: Tex, tf_lookup,
// the camera and slab code of shaded_march_rows, ShadeSample's tail (combine_cones)
// and cvr_expf / cvr_powf live in anonymous namespaces there and are the very
// functions the pinned oracles run.  New here is only the text the ground-truth
// renderer adds to CVR-SPEC (DESIGN.md §5d′): the per-ray frame, the secondary-ray
// loop and the shadow frames.
// Built with the oracle's flags (-ffp-contract=off: explicit fmaf only).
#include "../../oracle/cvr_oracle.cpp"

struct GtRef {
  OracleRc1pass base;          // volume, TF, gradient, camera, W, H, step, phong, ka/kd/ks/shininess, light
  float light_forward[3], light_up[3], light_right[3];   // cvr_light (forward = -LightCamForward)
  float light_gap, light_step;
  int32_t apply_occlusion, apply_shadow, shadow_type;
  float occ_distance, sdw_distance;
  int32_t n_occ, n_sdw;
  const float* occ_rays;       // n x (r, g, b), already rounded to binary16
  const float* sdw_rays;
};

namespace {

struct GtScene {
  Tex vol;
  const float* tf;
  int tf_n, wbits;
  v3 G, NoG;
  float gap, lstep;
  // texture(TexTransferFunc, texture(TexVolume, p / G).r).a
  float tau(v3 p) const {
    float dens, c[4];
    vol.sample(std::fmaf(p.x, NoG.x, -0.5f), std::fmaf(p.y, NoG.y, -0.5f), std::fmaf(p.z, NoG.z, -0.5f), &dens);
    tf_lookup(tf, tf_n, dens, c, wbits);
    return c[3];
  }
  // the ray loop of :118-168 / :202-251
  float cone(const float* rays, int n, float dist, v3 tx, v3 v_right, v3 v_up, v3 v_dir) const {
    float sacc = 0.0f, swgt = 0.0f;
    for (int i = 0; i < n; i++) {
      const float* c = rays + 3 * i;
      const v3 w = normalize3(mk(std::fmaf(v_right.x, c[0], std::fmaf(v_up.x, c[1], v_dir.x * c[2])),
                                 std::fmaf(v_right.y, c[0], std::fmaf(v_up.y, c[1], v_dir.y * c[2])),
                                 std::fmaf(v_right.z, c[0], std::fmaf(v_up.z, c[1], v_dir.z * c[2]))));
      float vt = 1.0f;
      float s = gap;
      float st0 = tau(vmad(w, s, tx));
      while (s < dist) {
        const float h = std::fmin(lstep, dist - s);
        const v3 at = vmad(w, s + h, tx);
        if (at.x < 0.0f || at.x > G.x || at.y < 0.0f || at.y > G.y || at.z < 0.0f || at.z > G.z) break;
        const float st1 = tau(at);
        vt = vt * cvr_expf(-(((st0 + st1) * 0.5f) * h));
        if ((1.0f - vt) > 0.99f) break;
        st0 = st1;
        s = s + h;
      }
      const float r = dot3(v_dir, w);
      sacc = sacc + vt * r;
      swgt = swgt + r;
    }
    return sacc / swgt;
  }
};

}  // namespace

// Rows [y0, y1) of the converged frame.  out: W*H*4, counts: W*H; returns their sum.
extern "C" __attribute__((visibility("default"))) uint64_t gtref_render_rows(const GtRef* Q, int y0, int y1,
                                                                            float* out_rgba, uint32_t* out_counts,
                                                                            int nthreads) {
  const OracleRc1pass& P = Q->base;
  const v3 G = mk((float)P.N[0] * P.scale[0], (float)P.N[1] * P.scale[1], (float)P.N[2] * P.scale[2]);
  const v3 light = mk(P.light[0], P.light[1], P.light[2]);
  // LightCamForward = -forward (crtgtrenderer.cpp:227), LightCamUp, LightCamRight
  const v3 lz = mk(-Q->light_forward[0], -Q->light_forward[1], -Q->light_forward[2]);
  const v3 lup = mk(Q->light_up[0], Q->light_up[1], Q->light_up[2]);
  const v3 lright = mk(Q->light_right[0], Q->light_right[1], Q->light_right[2]);
  const GtScene S{Tex{P.vol, {P.N[0], P.N[1], P.N[2]}, 1, P.filter_bits}, P.tf, P.tf_n, P.filter_bits, G,
                  mk((float)P.N[0] / G.x, (float)P.N[1] / G.y, (float)P.N[2] / G.z), Q->light_gap, Q->light_step};
  const float ka = Q->apply_occlusion ? P.ka : 0.0f;
  const float kd = Q->apply_shadow ? P.kd : 0.0f;
  const float ks = Q->apply_shadow ? P.ks : 0.0f;
  auto shade = [&](float* src, v3 tx, v3 wp, v3 cam_dir, float x, float y, float z) {
    float iocc = 0.0f, isdw = 0.0f;
    if (Q->apply_occlusion) {
      // the per-ray frame (:396-399) and v_dir = normalize(-ray_dir) (:116)
      const v3 v_right = normalize3(cross3(cam_dir, mk(0.0f, 1.0f, 0.0f)));
      const v3 ncam = mk(-cam_dir.x, -cam_dir.y, -cam_dir.z);
      const v3 v_up = normalize3(cross3(ncam, v_right));
      iocc = S.cone(Q->occ_rays, Q->n_occ, Q->occ_distance, tx, v_right, v_up, normalize3(ncam));
    }
    if (Q->apply_shadow) {
      // this shader's own frame, not the oracle's shadow_cone_frame (other axes, -forward, 30.0)
      v3 v_dir, v_up, v_right;
      bool on = true;
      if (Q->shadow_type == 2) {
        v_dir = lz; v_up = lup; v_right = lright;
      } else {
        v_dir = normalize3(mk(light.x - wp.x, light.y - wp.y, light.z - wp.z));
        v_up = normalize3(cross3(v_dir, lright));
        v_right = normalize3(cross3(v_dir, v_up));
        if (Q->shadow_type == 1 && dot3(v_dir, lz) < 30.0f) on = false;   // :192, as written
      }
      if (on) isdw = S.cone(Q->sdw_rays, Q->n_sdw, Q->sdw_distance, tx, v_right, v_up, v_dir);
    }
    // ShadeSample (:254-302): the DOS combine with vec3(1) for the specular colour
    // (P.ispec, set by crtgt_ref.py; fma(1, spec, x) rounds as x + spec)
    float g[3];
    combine_cones(P, ka, kd, ks, iocc, isdw, wp, src, shading_gradient(P, x, y, z, g));
  };
  return shaded_march_rows(P, y0, y1, out_rgba, out_counts, nthreads, shade);
}
