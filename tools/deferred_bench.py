#!/usr/bin/env python
"""Pass times of the deferred isosurface renderer (deferred isosurface shading).

On one GPU, in ONE run: Marschner-Lobb --size^3 (512), isovalue 0.5, the "Initial State"
camera, the reference's defaults, at each of --res (2048 and 1024): cvr_deferred_geometry (the
march into the G-buffer), cvr_deferred_shade (lighting and tone map over the kept G-buffer:
the relight-only frame), and cvr_render_deferred (both, as one frame).  A second line per
resolution, ungated, reports cvr_render_iso variant 0 on the same scene and camera, as the
nearest existing renderer.

With --advanced, a further line per resolution reports the advanced deferred renderer on the
same scene and camera: cvr_deferred_geometry (its geometry pass is that one),
cvr_advdeferred_curvature, cvr_advdeferred_shade (the feature-lighting pass and tone map: the
relight-only frame) and cvr_render_advdeferred (all three as one frame).

Times are HIP events around the call, medians over --steps frames after --warmup untimed
ones, in milliseconds, with the spread (min, max).  Prints one JSON line per renderer (also
appended to --out when given).  A measurement: no target.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from cpp_volume_rendering_amd import _native as N  # noqa: E402
from cpp_volume_rendering_amd import datasets as D  # noqa: E402
from cpp_volume_rendering_amd.renderer import (AdvancedDeferredShading, Camera,  # noqa: E402
                                               CustomRayCasting1PassIsoAdapt, DataManager, DeferredShading,
                                               RenderingParameters)


def timed(call, steps, warmup):
    ms = []
    for i in range(warmup + steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        torch.cuda.synchronize()
        if i >= warmup:
            ms.append(a.elapsed_time(b))
    return dict(median=statistics.median(ms), min=min(ms), max=max(ms), n=len(ms))


def advanced(a, dm, rp, cam, W, base):
    """The advanced deferred renderer's pass times at W x W: one JSON line."""
    L = N.lib()
    r = AdvancedDeferredShading(0)
    r.SetExternalResources(dm, rp)
    assert r.Init(W, W)
    r.Update(cam)
    h = r.device.handle
    r.device.set_stream(torch.cuda.current_stream(0).cuda_stream)
    out = N.Output(r.rgba.data_ptr(), None, None, 1, N.FORMAT_RGBA32F)
    frame, p = r._frame, r._params
    g = N.DeferredParams()
    L.cvr_deferred_params_default(ctypes.byref(g))
    g.isovalue, g.step_small, g.step_large, g.step_range = p.isovalue, p.step_small, p.step_large, p.step_range
    g.num_blocks[:] = list(p.num_blocks)
    g.gbuffer_clear[:] = list(p.gbuffer_clear)

    def geometry():
        N.check(L.cvr_deferred_geometry(h, ctypes.byref(frame), ctypes.byref(g)), "cvr_deferred_geometry", h)

    def curvature():
        N.check(L.cvr_advdeferred_curvature(h, ctypes.byref(frame), ctypes.byref(p)), "cvr_advdeferred_curvature", h)

    def shade():
        N.check(L.cvr_advdeferred_shade(h, W, W, ctypes.byref(p), ctypes.byref(out)), "cvr_advdeferred_shade", h)

    def whole():
        N.check(L.cvr_render_advdeferred(h, ctypes.byref(frame), ctypes.byref(p), ctypes.byref(out)),
                "cvr_render_advdeferred", h)

    line = dict(base, renderer="cvr_render_advdeferred", geometry_ms=timed(geometry, a.steps, a.warmup),
                curvature_ms=timed(curvature, a.steps, a.warmup), shade_ms=timed(shade, a.steps, a.warmup),
                frame_ms=timed(whole, a.steps, a.warmup), relight_ms=timed(shade, a.steps, a.warmup),
                hits=L.cvr_get_option(h, b"deferred_hits"),
                ridge_pixels=L.cvr_get_option(h, b"advdeferred_ridge_pixels"))
    r.Clean()
    return line


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, default=512, help="volume N^3")
    ap.add_argument("--res", type=int, nargs="+", default=[2048, 1024], help="frame W = H")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--advanced", action="store_true", help="also time the advanced deferred renderer's passes")
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    n = a.size
    dm = DataManager()
    dm.SetVolume(D.marschner_lobb_u8(n), D.voxel_scale(n))
    cam = Camera(**D.INITIAL_STATE_CAMERA)
    L = N.lib()
    lines = []
    for W in a.res:
        rp = RenderingParameters(W, W, light_position=D.LIGHT_LIST0_POSITION)
        base = dict(tool="deferred_bench", size=n, res=W, device=torch.cuda.get_device_name(0))
        r = DeferredShading(0)
        r.SetExternalResources(dm, rp)
        assert r.Init(W, W)
        r.Update(cam)
        h = r.device.handle
        s = torch.cuda.current_stream(0)
        r.device.set_stream(s.cuda_stream)
        out = N.Output(r.rgba.data_ptr(), None, None, 1, N.FORMAT_RGBA32F)
        frame, p = r._frame, r._params

        def geometry():
            N.check(L.cvr_deferred_geometry(h, ctypes.byref(frame), ctypes.byref(p)), "cvr_deferred_geometry", h)

        def shade():
            N.check(L.cvr_deferred_shade(h, W, W, ctypes.byref(p), ctypes.byref(out)), "cvr_deferred_shade", h)

        def whole():
            N.check(L.cvr_render_deferred(h, ctypes.byref(frame), ctypes.byref(p), ctypes.byref(out)),
                    "cvr_render_deferred", h)

        lines.append(dict(base, renderer="cvr_render_deferred",
                          geometry_ms=timed(geometry, a.steps, a.warmup),
                          shade_ms=timed(shade, a.steps, a.warmup),          # = the relight-only frame
                          frame_ms=timed(whole, a.steps, a.warmup),
                          relight_ms=timed(shade, a.steps, a.warmup),
                          hits=L.cvr_get_option(h, b"deferred_hits")))
        print(json.dumps(lines[-1]), flush=True)
        r.Clean()
        if a.advanced:
            lines.append(advanced(a, dm, rp, cam, W, base))
            print(json.dumps(lines[-1]), flush=True)
        i = CustomRayCasting1PassIsoAdapt(0)
        i.SetExternalResources(dm, rp)
        assert i.Init(W, W)
        i.PrepareRender(cam)
        lines.append(dict(base, renderer="cvr_render_iso", variant=0,
                          frame_ms=timed(lambda: i.Redraw(count_samples=False), a.steps, a.warmup)))
        print(json.dumps(lines[-1]), flush=True)
        i.Clean()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for l in lines:
                f.write(json.dumps(l) + "\n")


if __name__ == "__main__":
    main()
