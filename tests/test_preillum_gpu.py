"""GPU parity of the DOS renderer's pre-illumination against its CPU restatement
(tests/support/lightcache_ref.cpp), bit for bit:
  * the light cache (lightcache.hip light_cache_kernel vs lightcachecomputation.comp
    restated over the oracle's cone_trace), as uint16 patterns;
  * the cached march (PreillumShaderT through the shared march vs obj_ray_marching.comp
    restated), over the GPU's own cache: RGBA, per-pixel counts, total;
  * the cache object of the C-ABI: upload / copy back, the skip logic of
    cvr_render_dosct_preillum, invalidation, errors, and the Python renderer's switch.
Setup: test_dos_gpu.py's own (tests/preillum_cases.py)."""
import contextlib
import ctypes

import numpy as np
import pytest

import lightcache_ref as R
import preillum_cases as C
from cpp_volume_rendering_amd import _native as N
from cpp_volume_rendering_amd.renderer import (Camera, DataManager, Device,
                                               RC1PConeTracingDirOcclusionShading,
                                               RenderingParameters, default_cone_params,
                                               make_frame)

from test_rc1pass_gpu import assert_bitexact

pytestmark = pytest.mark.gpu


def setup(d):
    vol, scale, _, tf, tf_rgba, _, _ = C.scene()
    d.set_volume(vol, scale)
    d.set_transfer_function(tf)
    d.set_gradient(N.GRADIENT_FINITE_DIFFERENCES)
    d.set_extinction_volume(tf_rgba, C.EXT_RES)


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    d = Device(0)
    setup(d)
    yield d
    d.close()


@pytest.fixture(scope="module")
def step():
    import oracle as O
    return O.default_step(C.scene()[1])


@contextlib.contextmanager
def option(d, key, value):
    L = N.lib()
    old = L.cvr_get_option(d.handle, key)
    N.check(L.cvr_set_option(d.handle, key, value), key.decode(), d.handle)
    try:
        yield
    finally:
        L.cvr_set_option(d.handle, key, old)


def dos_params(case, step, phong=False, **over):
    p = N.DosParams()
    p.step = step
    p.apply_gradient_shading = int(phong)
    p.ka, p.kd, p.ks, p.shininess = 0.5, 0.5, 0.8, 30.0
    p.ispecular[:] = [1.0, 1.0, 1.0]
    for k in ("position", "forward", "up", "right"):
        getattr(p.light, k)[:] = list(C.LIGHT0[k])
    p.light.spot_angle_deg = C.LIGHT0["spot_angle_deg"]
    f = dict(C.flags(case), **over)
    p.apply_occlusion, p.apply_shadow, p.shadow_type = (int(f["apply_occlusion"]), int(f["apply_shadow"]),
                                                        f["shadow_type"])
    p.occlusion = case["occ"]() if "occ" in case else default_cone_params(True)
    p.shadow = default_cone_params(False)
    return p


def dims_c(dims):
    return (ctypes.c_int * 3)(*dims)


def render(d, entry, cam, W, H, p, dims=None):
    """One frame through cvr_render_preillum / cvr_render_dosct_preillum (host outputs)."""
    frame = make_frame(Camera(**cam), W, H)
    rgba = np.zeros((H, W, 4), np.float32)
    cnt = np.zeros((H, W), np.uint32)
    total = np.zeros(1, np.uint64)
    out = N.Output(rgba.ctypes.data, cnt.ctypes.data, total.ctypes.data, 0)
    L = N.lib()
    if dims is None:
        st = getattr(L, entry)(d.handle, ctypes.byref(frame), ctypes.byref(p), ctypes.byref(out))
    else:
        st = getattr(L, entry)(d.handle, ctypes.byref(frame), ctypes.byref(p), dims_c(dims), ctypes.byref(out))
    N.check(st, entry, d.handle)
    return rgba, cnt, int(total[0])


def ref_render(cache, cam, W, H, step, p, phong=False, filter_bits=0):
    _, scale, vol16, tf, _, _, grad = C.scene()
    return R.render(vol16, scale, tf, cache, cam, W, H, step, C.LIGHT0,
                    apply_occlusion=bool(p.apply_occlusion), apply_shadow=bool(p.apply_shadow),
                    grad=grad if phong else None, phong=phong, filter_bits=filter_bits)


def builds(d):
    return N.lib().cvr_get_option(d.handle, b"light_cache_builds")


# ---------------------------------------------------------------------------------------
# the light cache
# ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("filter_bits", [0, 8])
@pytest.mark.parametrize("dims", C.CACHE_DIMS, ids=lambda d: "x".join(map(str, d)))
@pytest.mark.parametrize("name", sorted(C.CACHE_CASES))
def test_cache_bitexact_vs_reference(dev, step, name, dims, filter_bits):
    case = C.CACHE_CASES[name]
    p = dos_params(case, step)
    frame = make_frame(Camera(**case.get("cam", C.INITIAL)), 64, 48)
    with option(dev, b"filter_bits", filter_bits):
        dev.compute_light_cache(frame, p, dims)
        got = dev.light_cache().view(np.uint16)
    want = C.ref_cache(name, dims, filter_bits)
    assert got.shape == want.shape == (dims[2], dims[1], dims[0], 2)
    assert_bitexact(got, want, f"{name} {dims} filter_bits {filter_bits}")
    # the compared terms are not constant (from the inside eye every occlusion cone runs
    # its whole length through the volume: that channel alone is all 0.0)
    live = want[..., [c for c, on in ((0, p.apply_occlusion), (1, p.apply_shadow)) if on]]
    assert ((live != 0) & (live != 0x3C00)).mean() >= 0.05


# ---------------------------------------------------------------------------------------
# the cached march
# ---------------------------------------------------------------------------------------

MARCH_CASES = {
    #           cache case,   cache dims,    Phong, filter_bits, flags of the march
    "occlusion": ("occlusion", (20, 12, 9), False, 0, {}),
    "both": ("both_point", (32, 32, 32), False, 0, {}),
    "phong_fd": ("both_point", (20, 12, 9), True, 0, {}),
    "inside": ("inside", (32, 32, 32), False, 0, {}),
    "filter8": ("both_point", (20, 12, 9), False, 8, {}),
    "both_off": ("both_point", (20, 12, 9), False, 0, dict(apply_occlusion=False, apply_shadow=False)),
}


@pytest.mark.parametrize("flat", [1, 0])
@pytest.mark.parametrize("W,H", [(96, 80), (77, 53)])
@pytest.mark.parametrize("name", sorted(MARCH_CASES))
def test_march_bitexact_vs_reference(dev, step, name, W, H, flat):
    cname, dims, phong, fb, over = MARCH_CASES[name]
    case = C.CACHE_CASES[cname]
    cam = case.get("cam", C.INITIAL)
    with option(dev, b"filter_bits", fb), option(dev, b"shade_flat", flat):
        dev.compute_light_cache(make_frame(Camera(**cam), W, H), dos_params(case, step), dims)
        cache = dev.light_cache()             # the GPU's own cache: both sides read these halfs
        p = dos_params(case, step, phong=phong, **over)
        g_rgba, g_cnt, g_total = render(dev, "cvr_render_preillum", cam, W, H, p)
    o_rgba, o_cnt, o_total = ref_render(cache, cam, W, H, step, p, phong=phong, filter_bits=fb)
    assert_bitexact(g_cnt, o_cnt, f"{name} counts")
    assert_bitexact(g_rgba, o_rgba, f"{name} rgba")
    assert g_total == o_total == int(o_cnt.sum()) > 0
    if name == "both_off":
        assert not g_rgba.any()               # `src.a > 0 && Shade`: nothing composited
    else:
        assert o_rgba[..., 3].max() > 0.5     # the frame is not empty


# ---------------------------------------------------------------------------------------
# the cache object
# ---------------------------------------------------------------------------------------

def test_set_light_cache_round_trip(dev, step):
    dims = (20, 12, 9)
    want = C.ref_cache("both_point", dims)
    dev.set_light_cache(want)
    got = dev.light_cache().view(np.uint16)
    assert_bitexact(got, want, "uploaded cache")
    p = dos_params(C.CACHE_CASES["both_point"], step)
    W, H = 77, 53
    g = render(dev, "cvr_render_preillum", C.INITIAL, W, H, p)
    o = ref_render(want, C.INITIAL, W, H, step, p)
    assert_bitexact(g[1], o[1], "counts over the uploaded cache")
    assert_bitexact(g[0], o[0], "rgba over the uploaded cache")
    assert g[2] == o[2]


def test_dosct_preillum_skips_unchanged_computes(step):
    """Update in one call: the compute runs only when something the cache depends on
    changed; a shadow-only cache survives camera motion."""
    d = Device(0)
    try:
        setup(d)
        dims = (20, 12, 9)
        W, H = 77, 53
        both = dos_params(C.CACHE_CASES["both_point"], step)
        before = d.device_bytes()
        d.compute_light_cache(make_frame(Camera(**C.INITIAL), W, H), both, dims)
        assert d.device_bytes() - before == 4 * dims[0] * dims[1] * dims[2]
        assert builds(d) == 1
        a = render(d, "cvr_render_dosct_preillum", C.INITIAL, W, H, both, dims)
        b = render(d, "cvr_render_dosct_preillum", C.INITIAL, W, H, both, dims)
        assert builds(d) == 1                  # same inputs as the compute above
        assert_bitexact(a[0], b[0], "same inputs, same frame")
        o = ref_render(C.ref_cache("both_point", dims), C.INITIAL, W, H, step, both)
        assert_bitexact(a[0], o[0], "one-call frame vs reference")
        render(d, "cvr_render_dosct_preillum", C.MOVED, W, H, both, dims)
        assert builds(d) == 2                  # occlusion on: the eye counts
        render(d, "cvr_render_dosct_preillum", C.MOVED, W, H, both, (32, 32, 32))
        assert builds(d) == 3                  # other dims
        sdw = dos_params(C.CACHE_CASES["shadow_only"], step)
        render(d, "cvr_render_dosct_preillum", C.INITIAL, W, H, sdw, dims)
        assert builds(d) == 4                  # other flags and dims
        g = render(d, "cvr_render_dosct_preillum", C.MOVED, W, H, sdw, dims)
        assert builds(d) == 4                  # shadow only: the eye does not count
        o = ref_render(C.ref_cache("shadow_only", dims), C.MOVED, W, H, step, sdw)
        assert_bitexact(g[1], o[1], "moved shadow-only counts")
        assert_bitexact(g[0], o[0], "moved shadow-only rgba")
        sdw.light.position[0] += 10.0
        render(d, "cvr_render_dosct_preillum", C.MOVED, W, H, sdw, dims)
        assert builds(d) == 5                  # the light counts
        # a new pyramid drops the cache
        d.set_extinction_volume(C.scene()[4], C.EXT_RES)
        L = N.lib()
        assert L.cvr_copy_light_cache(d.handle, None, 0, dims_c(dims)) == N.CVR_ERR_STATE
        img = np.zeros((H, W, 4), np.float32)
        out = N.Output(img.ctypes.data, None, None, 0)
        fr = make_frame(Camera(**C.MOVED), W, H)
        assert L.cvr_render_preillum(d.handle, ctypes.byref(fr), ctypes.byref(sdw),
                                     ctypes.byref(out)) == N.CVR_ERR_STATE
        render(d, "cvr_render_dosct_preillum", C.MOVED, W, H, sdw, dims)
        assert builds(d) == 6
    finally:
        d.close()


def test_errors(dev, step):
    L = N.lib()
    p = dos_params(C.CACHE_CASES["both_point"], step)
    fr = make_frame(Camera(**C.INITIAL), 16, 16)
    img = np.zeros((16, 16, 4), np.float32)
    out = N.Output(img.ctypes.data, None, None, 0)
    half = np.zeros(2 * 32 * 32 * 513, np.uint16)
    for bad in ((1, 32, 32), (32, 32, 513), (32, 0, 32)):
        b = dims_c(bad)
        assert L.cvr_compute_light_cache_dosct(dev.handle, ctypes.byref(fr), ctypes.byref(p), b) == N.CVR_ERR_ARG
        assert L.cvr_set_light_cache(dev.handle, half.ctypes.data, b) == N.CVR_ERR_ARG
        assert L.cvr_render_dosct_preillum(dev.handle, ctypes.byref(fr), ctypes.byref(p), b,
                                           ctypes.byref(out)) == N.CVR_ERR_ARG
    ok = dims_c((32, 32, 32))
    with option(dev, b"native_exp", 1):        # tolerance mode: no light-cache form
        assert L.cvr_compute_light_cache_dosct(dev.handle, ctypes.byref(fr), ctypes.byref(p), ok) == N.CVR_ERR_ARG
    # state errors on a fresh context: no pyramid, no cache
    d = Device(0)
    try:
        vol, scale, _, tf, _, _, _ = C.scene()
        assert L.cvr_compute_light_cache_dosct(d.handle, ctypes.byref(fr), ctypes.byref(p), ok) == N.CVR_ERR_STATE
        d.set_volume(vol, scale)
        d.set_transfer_function(tf)
        assert L.cvr_compute_light_cache_dosct(d.handle, ctypes.byref(fr), ctypes.byref(p), ok) == N.CVR_ERR_STATE
        assert L.cvr_render_preillum(d.handle, ctypes.byref(fr), ctypes.byref(p),
                                     ctypes.byref(out)) == N.CVR_ERR_STATE
        assert L.cvr_copy_light_cache(d.handle, None, 0, ok) == N.CVR_ERR_STATE
        assert builds(d) == 0
    finally:
        d.close()
    # a group context refuses every new entry point
    grp = Device(devices=[0, 0])
    try:
        calls = [
            lambda: L.cvr_compute_light_cache_dosct(grp.handle, ctypes.byref(fr), ctypes.byref(p), ok),
            lambda: L.cvr_set_light_cache(grp.handle, half.ctypes.data, ok),
            lambda: L.cvr_copy_light_cache(grp.handle, None, 0, ok),
            lambda: L.cvr_render_preillum(grp.handle, ctypes.byref(fr), ctypes.byref(p), ctypes.byref(out)),
            lambda: L.cvr_render_dosct_preillum(grp.handle, ctypes.byref(fr), ctypes.byref(p), ok,
                                                ctypes.byref(out)),
        ]
        for call in calls:
            assert call() == N.CVR_ERR_STATE
            assert b"group" in L.cvr_last_error(grp.handle)
    finally:
        grp.close()


def test_python_renderer_switch(dev, step):
    """RC1PConeTracingDirOcclusionShading(pre_illumination=True) renders the frame of
    cvr_render_dosct_preillum; the default stays the on-the-fly renderer."""
    import torch
    vol, scale, _, tf, tf_rgba, _, _ = C.scene()
    dm = DataManager()
    dm.SetVolume(vol, scale)
    dm.SetTransferFunction(tf, tf_rgba)
    W, H = 96, 80
    rp = RenderingParameters(W, H, light_position=C.LIGHT0["position"], light_forward=C.LIGHT0["forward"],
                             light_up=C.LIGHT0["up"], light_right=C.LIGHT0["right"],
                             spot_light_angle=C.LIGHT0["spot_angle_deg"])
    assert RC1PConeTracingDirOcclusionShading().pre_illumination is False
    assert RC1PConeTracingDirOcclusionShading().light_cache_resolution == (32, 32, 32)
    r = RC1PConeTracingDirOcclusionShading(0, pre_illumination=True, light_cache_resolution=(20, 12, 9))
    r.glsl_apply_shadow = True
    r.ext_res = C.EXT_RES
    r.SetExternalResources(dm, rp)
    assert r.Init(W, H)
    try:
        r.m_u_step_size = step
        r.PrepareRender(Camera(**C.INITIAL))
        r.Redraw()
        torch.cuda.synchronize()
        got = r.rgba.cpu().numpy()
        assert builds(r.device) == 1
        assert r.device.light_cache().shape == (9, 12, 20, 2)
    finally:
        r.Clean()
    p = dos_params(C.CACHE_CASES["both_point"], step)
    want = render(dev, "cvr_render_dosct_preillum", C.INITIAL, W, H, p, (20, 12, 9))
    assert_bitexact(got, want[0], "Python renderer vs the C-ABI path")
    assert want[0][..., 3].max() > 0.5
