// ebs_lightcache_ref.cpp — CPU restatement of the EBS renderer's light cache
// (TEST INFRASTRUCTURE ONLY, built by tests/ebs_lightcache_ref.py).
//
//  * lcref_ebs_cache: rc1pextbsd/lightcachecomputation.comp, the light cache of the
//    SAT ambient occlusion and the SAT box-chain shadow.
//
// The oracle is frozen, so this file includes its translation unit: Sat,
// ebs_occlusion and cone_x / cone_y / cone_z live in an anonymous namespace there
// and are the very functions the on-the-fly EBS oracle (already pinned) runs.  The
// shader's AO and shadow functions are the same text as ebs_ray_bbox_marching.comp's.
// New here is only the text DESIGN.md §5c″ adds to CVR-SPEC: the voxel position
// (the DOS cache's own, §5b′) and the two terms evaluated there.  The march over the
// cache is lightcache_ref.cpp's lcref_render_rows.  Built with the oracle's flags
// (-ffp-contract=off: explicit fmaf only).
#include "../../oracle/cvr_oracle.cpp"

// The light cache of Q's occlusion and shadow for a cache of dims voxels: out_rg
// receives 2 * dims[0] * dims[1] * dims[2] binary16 bit patterns (Iao, Ids),
// x-fastest.  Of Q->base it reads the volume size and scale, the light position
// and filter_bits; nothing of the camera.
extern "C" __attribute__((visibility("default"))) void lcref_ebs_cache(const OracleEbs* Q, const int dims[3],
                                                                       uint16_t* out_rg, int nthreads) {
  const OracleRc1pass& P = Q->base;
  const v3 light = mk(P.light[0], P.light[1], P.light[2]);
  // the uniforms of oracle_render_ebs_rows
  Sat T;
  T.t = Tex{Q->sat, {Q->sat_dims[0], Q->sat_dims[1], Q->sat_dims[2]}, 1, P.filter_bits};
  T.S = mk(P.scale[0], P.scale[1], P.scale[2]);
  T.G = mk((float)P.N[0] * P.scale[0], (float)P.N[1] * P.scale[1], (float)P.N[2] * P.scale[2]);
  T.inv_vs = mk(1.0f / (T.G.x + T.S.x * 2.0f), 1.0f / (T.G.y + T.S.y * 2.0f), 1.0f / (T.G.z + T.S.z * 2.0f));
  T.nsat = mk((float)Q->sat_dims[0], (float)Q->sat_dims[1], (float)Q->sat_dims[2]);
  T.min_sat = mk(T.S.x * 0.5f, T.S.y * 0.5f, T.S.z * 0.5f);
  T.max_sat = mk(T.G.x + T.S.x * 1.5f, T.G.y + T.S.y * 1.5f, T.G.z + T.S.z * 1.5f);
  const ConeCS cs{std::cos(Q->cone_angle), std::sin(Q->cone_angle), std::cos(-Q->cone_angle),
                  std::sin(-Q->cone_angle)};
  const v3 lfwd = mk(Q->light_forward[0], Q->light_forward[1], Q->light_forward[2]);
  const v3 half = mk(T.G.x * 0.5f, T.G.y * 0.5f, T.G.z * 0.5f);
  // VolumeScales * (VolumeDimensions / LightCacheDimensions)
  const v3 vs = mk(P.scale[0] * ((float)P.N[0] / (float)dims[0]), P.scale[1] * ((float)P.N[1] / (float)dims[1]),
                   P.scale[2] * ((float)P.N[2] / (float)dims[2]));
#ifdef _OPENMP
  if (nthreads > 0) omp_set_num_threads(nthreads);
#endif
#pragma omp parallel for schedule(dynamic, 1) collapse(2)
  for (int z = 0; z < dims[2]; z++)
    for (int y = 0; y < dims[1]; y++)
      for (int x = 0; x < dims[0]; x++) {
        const v3 tx = mk(((float)x + 0.5f) * vs.x, ((float)y + 0.5f) * vs.y, ((float)z + 0.5f) * vs.z);
        const v3 wp = mk(tx.x - half.x, tx.y - half.y, tx.z - half.z);
        float iao = 1.0f, ids = 1.0f;
        if (Q->apply_occlusion) iao = ebs_occlusion(T, tx, Q->occ_shells, Q->occ_radius);
        if (Q->apply_shadow) {
          // ExtinctionDirectionalShadows (lightcachecomputation.comp:426-437)
          const v3 cv = Q->shadow_type == 0 ? normalize3(mk(light.x - wp.x, light.y - wp.y, light.z - wp.z))
                                            : normalize3(lfwd);
          const v3 ac = mk(std::fabs(cv.x), std::fabs(cv.y), std::fabs(cv.z));
          float Stau;
          if (ac.z > ac.x && ac.z > ac.y) Stau = cone_z(T, *Q, cs, tx, cv);
          else if (ac.y > ac.x) Stau = cone_y(T, *Q, cs, tx, cv);
          else Stau = cone_x(T, *Q, cs, tx, cv);
          ids = cvr_expf(-Stau);
        }
        const int64_t i = ((int64_t)z * dims[1] + y) * dims[0] + x;
        out_rg[2 * i] = float_to_half(iao);
        out_rg[2 * i + 1] = float_to_half(ids);
      }
}
