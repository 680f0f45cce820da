#!/usr/bin/env python
"""Frame time and image cost of pre-illumination (DESIGN.md §5b′, §5c″).

--renderer dos (the default):

bench.py's config-4 frame (Marschner-Lobb 512^3 -> 2048^2, cone occlusion + point-light
cone shadow, the "Initial State" camera), timed three ways in ONE run on one GPU:

  * on the fly:       cvr_render_dosct (two cone traces per sample);
  * pre-illuminated:  per light-cache resolution (32^3, 64^3, 128^3) the compute
                      (cvr_compute_light_cache_dosct) and the cached march
                      (cvr_render_preillum) timed separately with HIP events, and the SSIM
                      of the frame against the on-the-fly frame (the cost of the switch);
  * shadow-only orbit: occlusion off, the camera moving over the reference's camera
                      list: cvr_render_dosct_preillum skips the compute, against
                      cvr_render_dosct on the same views.

--renderer ebs: bench.py's config-5 frame (Marschner-Lobb 1024^3 -> 1024^2, SAT ambient
occlusion + point-light SAT shadow; --size 512 for a second point), in ONE run:

  * on the fly:       cvr_render_extbsd;
  * pre-illuminated:  per light-cache resolution the compute (cvr_compute_light_cache_extbsd)
                      and the cached march timed separately, the frame's SSIM against the
                      on-the-fly frame over the pixels finite in both frames, and that share
                      (at 1024^3 the float SAT leaves most of the on-the-fly frame inf / NaN);
  * orbit:            the light fixed, the camera moving over the reference's camera list:
                      cvr_render_extbsd_preillum computes once for all views.

Prints one JSON line (also appended to --out when given).  Times are medians over
--steps frames after --warmup untimed ones, in milliseconds.
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
from cpp_volume_rendering_amd.renderer import (Camera, DataManager,  # noqa: E402
                                               RC1PConeTracingDirOcclusionShading,
                                               RC1PExtinctionBasedShading, RenderingParameters,
                                               build_ext_lut, build_tf_rgbt, make_frame,
                                               read_camera_state)
from cpp_volume_rendering_amd.ssim import ssim_rgba  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--renderer", choices=["dos", "ebs"], default="dos")
    ap.add_argument("--size", type=int, default=0, help="volume N^3 (default: dos 512, ebs 1024)")
    ap.add_argument("--res", type=int, default=0, help="frame W = H (default: dos 2048, ebs 1024)")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--caches", default="32,64,128")
    ap.add_argument("--orbit-views", type=int, default=8)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.renderer == "ebs":
        return main_ebs(a)

    n, W = a.size or 512, a.res or 2048
    vol, scale = D.marschner_lobb_u8(n), D.voxel_scale(n)
    dm = DataManager()
    dm.SetVolume(vol, scale)
    dm.SetTransferFunction(build_tf_rgbt(D.BONSAI_TF_RGB, D.BONSAI_TF_ALPHA),
                           build_tf_rgbt(D.BONSAI_TF_RGB, D.BONSAI_TF_ALPHA, extinction_input=True))
    r = RC1PConeTracingDirOcclusionShading(0)
    r.glsl_apply_shadow = True            # config 4: cone AO + cone shadows (point light)
    r.SetExternalResources(dm, RenderingParameters(W, W, light_position=D.LIGHT_LIST0_POSITION))
    assert r.Init(W, W)
    cam = Camera(**D.INITIAL_STATE_CAMERA)
    r.PrepareRender(cam)
    L, h = N.lib(), r.device.handle
    stream = torch.cuda.current_stream(0)
    r.device.set_stream(stream.cuda_stream)
    img = torch.zeros((W, W, 4), dtype=torch.float32, device="cuda")
    out = N.Output(img.data_ptr(), None, None, 1, N.FORMAT_RGBA32F)

    def timed(fn, frames=None):
        """Median ms of fn(frame) over the timed frames (HIP events on the render stream)."""
        frames = frames or [make_frame(cam, W, W)]
        for i in range(a.warmup):
            fn(frames[i % len(frames)])
        ms = []
        for i in range(max(a.steps, len(frames))):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn(frames[i % len(frames)])
            e1.record(stream)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return statistics.median(ms)

    def call(entry, *args):
        N.check(getattr(L, entry)(h, *args), entry, h)

    p = r._params
    res = dict(tool="preillum_bench", size=n, res=W, steps=a.steps, warmup=a.warmup,
               device=torch.cuda.get_device_name(0))
    res["on_the_fly_ms"] = timed(lambda f: call("cvr_render_dosct", ctypes.byref(f), ctypes.byref(p),
                                                ctypes.byref(out)))
    torch.cuda.synchronize()
    fly = img.cpu().numpy()
    res["preillum"] = {}
    for c in [int(x) for x in a.caches.split(",")]:
        dims = (ctypes.c_int * 3)(c, c, c)
        compute = timed(lambda f: call("cvr_compute_light_cache_dosct", ctypes.byref(f), ctypes.byref(p), dims))
        march = timed(lambda f: call("cvr_render_preillum", ctypes.byref(f), ctypes.byref(p), ctypes.byref(out)))
        torch.cuda.synchronize()
        res["preillum"][str(c)] = dict(
            compute_ms=compute, march_ms=march, frame_ms=compute + march,
            speedup_march=res["on_the_fly_ms"] / march,
            speedup_frame=res["on_the_fly_ms"] / (compute + march),
            ssim_vs_on_the_fly=ssim_rgba(img.cpu().numpy(), fly),
            cache_bytes=4 * c ** 3)
    # shadow only, the camera orbiting: the cache does not depend on the eye
    p.apply_occlusion = 0
    path = os.path.join(ROOT, "tests", "golden", "list_camera_states")
    cnt = ctypes.c_int()
    N.check(L.cvr_read_camera_state(path.encode(), 0, N.Camera(), None, 0, cnt), "camera list")
    views = [make_frame(read_camera_state(path, i), W, W) for i in range(min(cnt.value, a.orbit_views))]
    dims = (ctypes.c_int * 3)(32, 32, 32)
    b0 = L.cvr_get_option(h, b"light_cache_builds")
    orbit_fly = timed(lambda f: call("cvr_render_dosct", ctypes.byref(f), ctypes.byref(p), ctypes.byref(out)),
                      views)
    orbit_pre = timed(lambda f: call("cvr_render_dosct_preillum", ctypes.byref(f), ctypes.byref(p), dims,
                                     ctypes.byref(out)), views)
    res["shadow_only_orbit"] = dict(views=len(views), cache=32, on_the_fly_ms=orbit_fly, preillum_ms=orbit_pre,
                                    speedup=orbit_fly / orbit_pre,
                                    computes=L.cvr_get_option(h, b"light_cache_builds") - b0)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
    r.Clean()


def finite_ssim(img, ref):
    """SSIM over the pixels finite in both frames (the others zeroed in both), and their share."""
    import numpy as np
    ok = np.isfinite(img).all(axis=-1) & np.isfinite(ref).all(axis=-1)
    a, b = np.where(ok[..., None], img, 0.0), np.where(ok[..., None], ref, 0.0)
    return ssim_rgba(a.astype("float32"), b.astype("float32")), float(ok.mean())


def main_ebs(a):
    n, W = a.size or 1024, a.res or 1024
    vol, scale = D.marschner_lobb_u8(n), D.voxel_scale(n)
    dm = DataManager()
    dm.SetVolume(vol, scale)
    dm.SetTransferFunction(build_tf_rgbt(D.BONSAI_TF_RGB, D.BONSAI_TF_ALPHA))
    dm.SetExtinctionTable(build_ext_lut(D.BONSAI_TF_RGB, D.BONSAI_TF_ALPHA))
    r = RC1PExtinctionBasedShading(0)     # config 5: SAT AO + SAT shadows (point light)
    r.SetExternalResources(dm, RenderingParameters(W, W, light_position=D.LIGHT_LIST0_POSITION))
    assert r.Init(W, W)
    cam = Camera(**D.INITIAL_STATE_CAMERA)
    r.PrepareRender(cam)
    L, h = N.lib(), r.device.handle
    stream = torch.cuda.current_stream(0)
    r.device.set_stream(stream.cuda_stream)
    img = torch.zeros((W, W, 4), dtype=torch.float32, device="cuda")
    out = N.Output(img.data_ptr(), None, None, 1, N.FORMAT_RGBA32F)

    def timed(fn, frames=None):
        """Median ms of fn(frame) over the timed frames (HIP events on the render stream)."""
        frames = frames or [make_frame(cam, W, W)]
        for i in range(a.warmup):
            fn(frames[i % len(frames)])
        ms = []
        for i in range(max(a.steps, len(frames))):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn(frames[i % len(frames)])
            e1.record(stream)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return statistics.median(ms)

    def call(entry, *args):
        N.check(getattr(L, entry)(h, *args), entry, h)

    p = r._params
    res = dict(tool="preillum_bench", renderer="ebs", size=n, res=W, steps=a.steps, warmup=a.warmup,
               device=torch.cuda.get_device_name(0))
    res["on_the_fly_ms"] = timed(lambda f: call("cvr_render_extbsd", ctypes.byref(f), ctypes.byref(p),
                                                ctypes.byref(out)))
    torch.cuda.synchronize()
    fly = img.cpu().numpy()
    res["preillum"] = {}
    for c in [int(x) for x in a.caches.split(",")]:
        dims = (ctypes.c_int * 3)(c, c, c)
        compute = timed(lambda f: call("cvr_compute_light_cache_extbsd", ctypes.byref(p), dims))
        # the cache is fresh (computed above with these parameters): the march alone
        b0 = L.cvr_get_option(h, b"light_cache_builds")
        march = timed(lambda f: call("cvr_render_extbsd_preillum", ctypes.byref(f), ctypes.byref(p), dims,
                                     ctypes.byref(out)))
        assert L.cvr_get_option(h, b"light_cache_builds") == b0
        torch.cuda.synchronize()
        ssim, share = finite_ssim(img.cpu().numpy(), fly)
        res["preillum"][str(c)] = dict(
            compute_ms=compute, march_ms=march, frame_ms=compute + march,
            speedup_march=res["on_the_fly_ms"] / march,
            speedup_frame=res["on_the_fly_ms"] / (compute + march),
            ssim_finite_vs_on_the_fly=ssim, finite_share=share, cache_bytes=4 * c ** 3)
    # the light fixed, the camera orbiting: the cache does not depend on the camera
    path = os.path.join(ROOT, "tests", "golden", "list_camera_states")
    cnt = ctypes.c_int()
    N.check(L.cvr_read_camera_state(path.encode(), 0, N.Camera(), None, 0, cnt), "camera list")
    views = [make_frame(read_camera_state(path, i), W, W) for i in range(min(cnt.value, a.orbit_views))]
    dims = (ctypes.c_int * 3)(32, 32, 32)
    orbit_fly = timed(lambda f: call("cvr_render_extbsd", ctypes.byref(f), ctypes.byref(p), ctypes.byref(out)),
                      views)
    b0 = L.cvr_get_option(h, b"light_cache_builds")
    orbit_pre = timed(lambda f: call("cvr_render_extbsd_preillum", ctypes.byref(f), ctypes.byref(p), dims,
                                     ctypes.byref(out)), views)
    res["orbit"] = dict(views=len(views), cache=32, on_the_fly_ms=orbit_fly, preillum_ms=orbit_pre,
                        speedup=orbit_fly / orbit_pre,
                        computes=L.cvr_get_option(h, b"light_cache_builds") - b0)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
    r.Clean()


if __name__ == "__main__":
    main()
