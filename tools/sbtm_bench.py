#!/usr/bin/env python
"""Frame time of the slice-based directional occlusion renderer by batch size (DESIGN.md §5d‴).

On one GPU, in ONE run: Marschner-Lobb --size^3 (512), the bonsai TF, the "Initial State"
camera, the reference's defaults (a 2 x 2 grid, half angle 50 deg), at each of --res
(2048 and 1024): cvr_render_sbtm with option sbtm_slices_per_launch 1 (the plain form: one
launch per slice, the planes in global memory), 2, 4, 8 and 16 (the blocked form: the planes
of a 64^2 screen tile and its halo in LDS).  Beside them the frame of cvr_render_dosct,
bench.py's config 4, on the same scene, for context.

Frame times are HIP events around the render call, medians over --steps frames after
--warmup untimed ones, in milliseconds, with the spread (min, max).  Prints one JSON line per
setting (also appended to --out when given).  A measurement: no target.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from cpp_volume_rendering_amd import _native as N  # noqa: E402
from cpp_volume_rendering_amd import datasets as D  # noqa: E402
from cpp_volume_rendering_amd.renderer import (Camera, DataManager,  # noqa: E402
                                               RC1PConeTracingDirOcclusionShading, RenderingParameters,
                                               SBTMDirectionalOcclusionShading, build_tf_rgbt)

BATCHES = (1, 2, 4, 8, 16)


def timed_frames(r, cam, steps, warmup):
    r.PrepareRender(cam)
    ms = []
    for i in range(warmup + steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r.Redraw(count_samples=False)
        b.record()
        torch.cuda.synchronize()
        if i >= warmup:
            ms.append(a.elapsed_time(b))
    return dict(median=statistics.median(ms), min=min(ms), max=max(ms), n=len(ms))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, default=512, help="volume N^3")
    ap.add_argument("--res", type=int, nargs="+", default=[2048, 1024], help="frame W = H")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    n = a.size
    vol, scale = D.marschner_lobb_u8(n), D.voxel_scale(n)
    dm = DataManager()
    dm.SetVolume(vol, scale)
    dm.SetTransferFunction(build_tf_rgbt(D.BONSAI_TF_RGB, D.BONSAI_TF_ALPHA),
                           build_tf_rgbt(D.BONSAI_TF_RGB, D.BONSAI_TF_ALPHA, extinction_input=True))
    cam = Camera(**D.INITIAL_STATE_CAMERA)
    lines = []
    for W in a.res:
        rp = RenderingParameters(W, W, light_position=D.LIGHT_LIST0_POSITION)
        base = dict(tool="sbtm_bench", size=n, res=W, device=torch.cuda.get_device_name(0))
        r = SBTMDirectionalOcclusionShading(0)
        r.SetExternalResources(dm, rp)
        assert r.Init(W, W)
        for k in BATCHES:
            N.check(N.lib().cvr_set_option(r.device.handle, b"sbtm_slices_per_launch", k), "option")
            t = timed_frames(r, cam, a.steps, a.warmup)
            h = r.device.handle
            lines.append(dict(base, renderer="cvr_render_sbtm", slices_per_launch=k, frame_ms=t,
                              slices=N.lib().cvr_get_option(h, b"sbtm_slices"),
                              launches=N.lib().cvr_get_option(h, b"sbtm_launches")))
            print(json.dumps(lines[-1]), flush=True)
        r.Clean()
        d = RC1PConeTracingDirOcclusionShading(0)
        d.glsl_apply_shadow = True                # config 4: occlusion + point-light shadow
        d.SetExternalResources(dm, rp)
        assert d.Init(W, W)
        lines.append(dict(base, renderer="cvr_render_dosct", frame_ms=timed_frames(d, cam, a.steps, a.warmup)))
        print(json.dumps(lines[-1]), flush=True)
        d.Clean()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for l in lines:
                f.write(json.dumps(l) + "\n")


if __name__ == "__main__":
    main()
