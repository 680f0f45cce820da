#!/usr/bin/env python
"""Precompute and frame time of the voxel cone tracing renderer (DESIGN.md §5d″).

On one GPU, in ONE run: Marschner-Lobb --size^3 (512) -> --res^2 (2048), the bonsai TF, the
"Initial State" camera, light 0 of the reference's list:

  * precompute:  cvr_vct_precompute after a new volume (the pyramid kernels and the host's
                 table), and after a new TF alone (the table), wall time around the call;
  * frame:       cvr_render_vct with the reference's defaults (vctrenderer.cpp:33-43);
  * DOS frame:   cvr_render_dosct, bench.py's config 4 (cone occlusion + point-light cone
                 shadow), the same volume, camera and resolution.

Frame times are HIP events around the render call, medians over --steps frames after
--warmup untimed ones, in milliseconds, with the spread (min, max).  Prints one JSON line
(also appended to --out when given).  A measurement: no target.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from cpp_volume_rendering_amd import datasets as D  # noqa: E402
from cpp_volume_rendering_amd.renderer import (Camera, DataManager,  # noqa: E402
                                               RC1PConeTracingDirOcclusionShading,
                                               RC1PVoxelConeTracingSGPU, RenderingParameters,
                                               build_opacity_lut, build_tf_rgbt)


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
    ap.add_argument("--res", type=int, default=2048, help="frame W = H")
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    n, W = a.size, a.res
    vol, scale = D.marschner_lobb_u8(n), D.voxel_scale(n)
    dm = DataManager()
    dm.SetVolume(vol, scale)
    dm.SetTransferFunction(build_tf_rgbt(D.BONSAI_TF_RGB, D.BONSAI_TF_ALPHA),
                           build_tf_rgbt(D.BONSAI_TF_RGB, D.BONSAI_TF_ALPHA, extinction_input=True))
    dm.SetOpacityTable(build_opacity_lut(D.BONSAI_TF_RGB, D.BONSAI_TF_ALPHA))
    rp = RenderingParameters(W, W, light_position=D.LIGHT_LIST0_POSITION)
    cam = Camera(**D.INITIAL_STATE_CAMERA)
    res = dict(tool="vct_bench", size=n, res=W, device=torch.cuda.get_device_name(0))

    v = RC1PVoxelConeTracingSGPU(0)
    v.SetExternalResources(dm, rp)
    assert v.Init(W, W)                       # builds once (untimed: the first launch of the kernels)
    dev = v.device
    pre, tab = [], []
    for _ in range(3):
        dev.set_volume(dm.volume, dm.scale)   # drops the pyramid and the table
        dev.set_transfer_function(dm.tf_rgbt)
        dev.vct_set_opacity(dm.opacity_lut)
        dev.synchronize()
        t0 = time.perf_counter()
        dev.vct_precompute()
        dev.synchronize()
        pre.append((time.perf_counter() - t0) * 1e3)
        dev.set_transfer_function(dm.tf_rgbt)  # drops the table alone
        dev.vct_set_opacity(dm.opacity_lut)
        t0 = time.perf_counter()
        dev.vct_precompute()
        dev.synchronize()
        tab.append((time.perf_counter() - t0) * 1e3)
    info = dev.vct_info()
    res.update(precompute_ms=dict(median=statistics.median(pre), min=min(pre), max=max(pre), n=len(pre)),
               table_only_ms=dict(median=statistics.median(tab), min=min(tab), max=max(tab), n=len(tab)),
               levels=info.levels, max_stddev=info.max_stddev, table_height=info.table_height)
    res["vct_frame_ms"] = timed_frames(v, cam, a.steps, a.warmup)
    res["vct_device_bytes"] = dev.device_bytes()
    v.Clean()

    d = RC1PConeTracingDirOcclusionShading(0)
    d.glsl_apply_shadow = True                # config 4: occlusion + point-light shadow
    d.SetExternalResources(dm, rp)
    assert d.Init(W, W)
    res["dos_frame_ms"] = timed_frames(d, cam, a.steps, a.warmup)
    d.Clean()
    res["vct_over_dos"] = res["vct_frame_ms"]["median"] / res["dos_frame_ms"]["median"]

    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
