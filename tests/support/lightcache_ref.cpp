// lightcache_ref.cpp — CPU restatement of the DOS renderer's pre-illumination
// (TEST INFRASTRUCTURE ONLY, built by tests/lightcache_ref.py).
//
//  * lcref_dos_cache:   lightcachecomputation.comp:523-547, the light cache;
//  * lcref_render_rows: obj_ray_marching.comp:211-333, the march over a cache.
//
// The oracle is frozen, so this file includes its translation unit: cone_trace,
// ExtVol, Tex, tf_lookup and shaded_march_rows live in anonymous namespaces there
// and are the very functions the on-the-fly DOS oracle (already pinned) runs.  New
// here is only the text DESIGN.md §5b′ adds to CVR-SPEC: the voxel position, the
// occlusion frame, the cache fetch and the `&& Shade` gate.  Built with the
// oracle's flags (-ffp-contract=off: explicit fmaf only).
#include "../../oracle/cvr_oracle.cpp"

namespace {

ExtVol make_ext(const OracleDos* Q, v3 G) {
  const OracleRc1pass& P = Q->base;
  ExtVol E{Q->ext, {Q->ext_res[0], Q->ext_res[1], Q->ext_res[2]}, Q->ext_levels, G, {}, P.filter_bits};
  E.off.assign(E.nl + 1, 0);
  for (int L = 0; L < E.nl; L++) {
    int d[3];
    ext_level_dims(E.res, L, d);
    E.off[L + 1] = E.off[L] + (int64_t)d[0] * d[1] * d[2];
  }
  return E;
}

}  // namespace

// The light cache of Q's cones for a cache of dims voxels: out_rg receives
// 2 * dims[0] * dims[1] * dims[2] binary16 bit patterns (Idao, Idcs), x-fastest.
// Of Q->base it reads the volume size and scale, the camera (eye, center, up),
// the light position and filter_bits.
extern "C" __attribute__((visibility("default"))) void lcref_dos_cache(const OracleDos* Q, const int dims[3],
                                                                       uint16_t* out_rg, int nthreads) {
  const OracleRc1pass& P = Q->base;
  const v3 eye = mk(P.eye[0], P.eye[1], P.eye[2]);
  const v3 G = mk((float)P.N[0] * P.scale[0], (float)P.N[1] * P.scale[1], (float)P.N[2] * P.scale[2]);
  const v3 half = mk(G.x * 0.5f, G.y * 0.5f, G.z * 0.5f);
  const float spot_cos = dos_spot_cos(Q);
  const ExtVol E = make_ext(Q, G);
  // VolumeScales * (VolumeDimensions / LightCacheDimensions) (:537)
  const v3 vs = mk(P.scale[0] * ((float)P.N[0] / (float)dims[0]), P.scale[1] * ((float)P.N[1] / (float)dims[1]),
                   P.scale[2] * ((float)P.N[2] / (float)dims[2]));
  // EyeCamUp: Camera::GetCameraVectors (camera.cpp:336-341), glm arithmetic
  const v3 dir = glm_normalize(mk(P.center[0] - eye.x, P.center[1] - eye.y, P.center[2] - eye.z));
  const v3 fwd = mk(-dir.x, -dir.y, -dir.z);
  const v3 right = glm_normalize(cross3(mk(P.up[0], P.up[1], P.up[2]), fwd));
  const v3 cup = glm_normalize(cross3(fwd, right));
#ifdef _OPENMP
  if (nthreads > 0) omp_set_num_threads(nthreads);
#endif
#pragma omp parallel for schedule(dynamic, 1) collapse(2)
  for (int z = 0; z < dims[2]; z++)
    for (int y = 0; y < dims[1]; y++)
      for (int x = 0; x < dims[0]; x++) {
        const v3 tx = mk(((float)x + 0.5f) * vs.x, ((float)y + 0.5f) * vs.y, ((float)z + 0.5f) * vs.z);
        const v3 wp = mk(tx.x - half.x, tx.y - half.y, tx.z - half.z);
        float idao = 1.0f, idcs = 1.0f;
        if (Q->apply_occlusion) {   // OcclusionEvaluationKernel (:280-292)
          const v3 k = normalize3(mk(eye.x - wp.x, eye.y - wp.y, eye.z - wp.z));
          const v3 v_right = normalize3(cross3(mk(-k.x, -k.y, -k.z), cup));
          const v3 v_up = normalize3(cross3(k, v_right));
          idao = cone_trace(E, Q->occ, tx, k, v_up, v_right);
        }
        if (Q->apply_shadow) {      // ShadowEvaluationKernel (:492-521)
          v3 k, u, v;
          const bool lit = shadow_cone_frame(Q, spot_cos, wp, k, u, v);
          // Cone1RayShadow(pos, k, v, u) is called as (pos, k, u, v): swapped
          idcs = lit ? cone_trace(E, Q->sdw, tx, k, v, u) : 0.0f;
        }
        const int64_t i = ((int64_t)z * dims[1] + y) * dims[0] + x;
        out_rg[2 * i] = float_to_half(idao);
        out_rg[2 * i + 1] = float_to_half(idcs);
      }
}

// Rows [y0, y1) of the march of obj_ray_marching.comp over the cache `rg`
// (binary16 bit patterns as lcref_dos_cache writes them).  out: W*H*4, counts: W*H.
extern "C" __attribute__((visibility("default"))) uint64_t lcref_render_rows(
    const OracleDos* Q, const uint16_t* rg, const int dims[3], int y0, int y1, float* out_rgba,
    uint32_t* out_counts, int nthreads) {
  OracleRc1pass P = Q->base;
  const v3 G = mk((float)P.N[0] * P.scale[0], (float)P.N[1] * P.scale[1], (float)P.N[2] * P.scale[2]);
  const size_t nv = (size_t)dims[0] * dims[1] * dims[2];
  std::vector<float> cf(2 * nv);
  for (size_t i = 0; i < 2 * nv; i++) cf[i] = half_to_float(rg[i]);
  Tex cache{cf.data(), {dims[0], dims[1], dims[2]}, 2, P.filter_bits};
  // texel coordinate fma(p, L / G, -0.5), L / G rounded once
  const v3 LoG = mk((float)dims[0] / G.x, (float)dims[1] / G.y, (float)dims[2] / G.z);
  const bool Shade = Q->apply_occlusion || Q->apply_shadow;   // :294
  const float ka = Q->apply_occlusion ? P.ka : 0.0f;
  const float kd = Q->apply_shadow ? P.kd : 0.0f;
  const float ks = Q->apply_shadow ? P.ks : 0.0f;
  auto shade = [&](float* src, v3 tx, v3 wp, v3, float x, float y, float z) {
    float ia[2];
    cache.sample(std::fmaf(tx.x, LoG.x, -0.5f), std::fmaf(tx.y, LoG.y, -0.5f), std::fmaf(tx.z, LoG.z, -0.5f), ia);
    const float iocc = Q->apply_occlusion ? ia[0] : 0.0f;
    const float isdw = Q->apply_shadow ? ia[1] : 0.0f;
    float g[3];
    combine_cones(P, ka, kd, ks, iocc, isdw, wp, src, shading_gradient(P, x, y, z, g));
  };
  // `if (src.a > 0 && Shade)` (:312): with Shade off no sample is composited and no
  // ray terminates early, which is the shared march over a TF without opacity (its
  // loop, and so its counts, do not depend on the TF otherwise).
  std::vector<float> tf0;
  if (!Shade) {
    tf0.assign(P.tf, P.tf + (size_t)P.tf_n * 4);
    for (int i = 0; i < P.tf_n; i++) tf0[(size_t)i * 4 + 3] = 0.0f;
    P.tf = tf0.data();
  }
  return shaded_march_rows(P, y0, y1, out_rgba, out_counts, nthreads, shade);
}
