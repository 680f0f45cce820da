#!/usr/bin/env python
"""How far the approximate lighting paths are from the ground truth (DESIGN.md §5d′, §5d″).

On the bench scene at a reduced size (Marschner-Lobb --size^3 -> --res^2, the bonsai
TF, the "Initial State" camera, light 0 of the reference's list) six frames are taken
on one GPU:

  * the ground truth: cvr_render_crtgt with --rays secondary rays per term, the
    reference's default steps (gap 1.0, step 0.5) and distances (diagonal * 0.50 / 0.75),
    the occlusion rays within the DOS occlusion cone's half angle (20 deg) and the
    shadow rays within its shadow cone's (0.5 deg), a point light;
  * cvr_render_dosct            (cone occlusion + point-light cone shadow, on the fly);
  * cvr_render_dosct_preillum   (the same through a 32^3 light cache);
  * cvr_render_extbsd           (SAT occlusion + point-light SAT shadow);
  * cvr_render_vct              (voxel cone tracing shadow, the reference's defaults);
  * cvr_render_sbtm             (slice-based directional occlusion, the reference's defaults:
                                 occlusion toward the eye only, no light term).

Prints the SSIM of each against the ground truth (cpp_volume_rendering_amd/ssim.py: the
frames as screenshots over white) and the ground truth's time per frame, as a table and
as one JSON line (also appended to --out when given).  No threshold: a measurement.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from cpp_volume_rendering_amd import datasets as D  # noqa: E402
from cpp_volume_rendering_amd.renderer import (Camera, DataManager,  # noqa: E402
                                               RC1PConeLightGroundTruthSteps,
                                               RC1PConeTracingDirOcclusionShading,
                                               RC1PExtinctionBasedShading, RC1PVoxelConeTracingSGPU,
                                               RenderingParameters, SBTMDirectionalOcclusionShading,
                                               build_ext_lut, build_opacity_lut, build_tf_rgbt)
from cpp_volume_rendering_amd.ssim import ssim_rgba  # noqa: E402


def frame_of(r, cam):
    r.PrepareRender(cam)
    r.Redraw(count_samples=False)
    torch.cuda.synchronize()
    return r.rgba.cpu().numpy()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, default=128, help="volume N^3")
    ap.add_argument("--res", type=int, default=256, help="frame W = H")
    ap.add_argument("--rays", type=int, default=256, help="secondary rays per term")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    n, W = a.size, a.res
    vol, scale = D.marschner_lobb_u8(n), D.voxel_scale(n)
    dm = DataManager()
    dm.SetVolume(vol, scale)
    dm.SetTransferFunction(build_tf_rgbt(D.BONSAI_TF_RGB, D.BONSAI_TF_ALPHA),
                           build_tf_rgbt(D.BONSAI_TF_RGB, D.BONSAI_TF_ALPHA, extinction_input=True))
    dm.SetExtinctionTable(build_ext_lut(D.BONSAI_TF_RGB, D.BONSAI_TF_ALPHA))
    dm.SetOpacityTable(build_opacity_lut(D.BONSAI_TF_RGB, D.BONSAI_TF_ALPHA))
    rp = RenderingParameters(W, W, light_position=D.LIGHT_LIST0_POSITION)
    cam = Camera(**D.INITIAL_STATE_CAMERA)

    # the ground truth: one Redraw takes the frame to convergence
    gt = RC1PConeLightGroundTruthSteps(0, samples_per_redraw=2 ** 30, ray_seed=a.seed)
    gt.SetExternalResources(dm, rp)
    assert gt.Init(W, W)
    gt.m_apply_occlusion = gt.m_apply_shadows = True
    gt.m_occ_num_rays_sampled = gt.m_sdw_num_rays_sampled = a.rays
    gt.m_occ_cone_aperture_angle, gt.m_sdw_cone_aperture_angle = 20.0, 0.5
    gt.SetLightParametersOutdated()
    t0 = time.perf_counter()
    truth = frame_of(gt, cam)
    gt_ms = (time.perf_counter() - t0) * 1e3
    assert not gt.frame_outdated
    res = dict(tool="gt_quality", size=n, res=W, rays=a.rays, seed=a.seed, light_gap=gt.m_u_light_ray_initial_step,
               light_step=gt.m_u_light_ray_step_size, occ_distance=gt.m_occ_cone_distance_eval,
               sdw_distance=gt.m_sdw_cone_distance_eval, ground_truth_ms=gt_ms,
               gt_device_bytes=gt.device.device_bytes(), device=torch.cuda.get_device_name(0), ssim={})
    gt.Clean()

    def dos(pre):
        r = RC1PConeTracingDirOcclusionShading(0, pre_illumination=pre)
        r.glsl_apply_shadow = True
        return r

    for name, r in (("cvr_render_dosct", dos(False)), ("cvr_render_dosct_preillum", dos(True)),
                    ("cvr_render_extbsd", RC1PExtinctionBasedShading(0)),
                    ("cvr_render_vct", RC1PVoxelConeTracingSGPU(0)),
                    ("cvr_render_sbtm", SBTMDirectionalOcclusionShading(0))):
        r.SetExternalResources(dm, rp)
        assert r.Init(W, W)
        res["ssim"][name] = ssim_rgba(frame_of(r, cam), truth)
        r.Clean()

    print(f"ground truth: {n}^3 -> {W}^2, {a.rays} rays per term, {gt_ms:.1f} ms per frame")
    print("| frame | SSIM against the ground truth |")
    print("|---|---|")
    for name, v in res["ssim"].items():
        print(f"| `{name}` | {v:.4f} |")
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
