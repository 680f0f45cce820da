"""GPU parity of the EBS renderer's pre-illumination against its CPU restatement, bit for
bit:
  * the light cache (ebs_lightcache.hip ebs_light_cache_kernel vs rc1pextbsd/
    lightcachecomputation.comp restated over the oracle's Sat / ebs_occlusion /
    cone_x|y|z, tests/support/ebs_lightcache_ref.cpp), as uint16 patterns, in both SAT
    layouts and with CVR-SPEC-8 weights;
  * the frame of cvr_render_extbsd_preillum vs obj_ray_marching.comp restated
    (lightcache_ref.render) over the reference cache: RGBA, per-pixel counts, total;
  * the same march as the DOS switch, the skip logic of cvr_render_extbsd_preillum,
    errors, and the Python renderer's switch.
Setup: test_ebs_gpu.py's own (tests/ebs_preillum_cases.py)."""
import contextlib
import ctypes

import numpy as np
import pytest

import ebs_preillum_cases as C
import lightcache_ref as R
from cpp_volume_rendering_amd import _native as N
from cpp_volume_rendering_amd.renderer import (Camera, DataManager, Device,
                                               RC1PExtinctionBasedShading, RenderingParameters,
                                               default_cone_params, make_frame)

from test_rc1pass_gpu import assert_bitexact

pytestmark = pytest.mark.gpu

ORBIT = [dict(eye=(600.0 * np.cos(a), 150.0, 600.0 * np.sin(a)), center=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0))
         for a in np.linspace(0.0, 2.0 * np.pi, 8, endpoint=False)]


def setup(d):
    vol, scale, _, tf, lut, _, _ = C.scene()
    d.set_volume(vol, scale)
    d.set_transfer_function(tf)
    d.set_gradient(N.GRADIENT_FINITE_DIFFERENCES)
    d.set_extinction_sat(lut)


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


def dims_c(dims):
    return (ctypes.c_int * 3)(*dims)


def render(d, cam, W, H, p, dims):
    """One frame through cvr_render_extbsd_preillum (host outputs)."""
    frame = make_frame(Camera(**cam), W, H)
    rgba = np.zeros((H, W, 4), np.float32)
    cnt = np.zeros((H, W), np.uint32)
    total = np.zeros(1, np.uint64)
    out = N.Output(rgba.ctypes.data, cnt.ctypes.data, total.ctypes.data, 0)
    N.check(N.lib().cvr_render_extbsd_preillum(d.handle, ctypes.byref(frame), ctypes.byref(p), dims_c(dims),
                                               ctypes.byref(out)), "cvr_render_extbsd_preillum", d.handle)
    return rgba, cnt, int(total[0])


def ref_render(cache, cam, W, H, step, p, phong=False):
    """obj_ray_marching.comp over `cache` with the march inputs of `p`."""
    _, scale, vol16, tf, _, _, grad = C.scene()
    light = dict(position=tuple(p.light_pos), forward=(0.0, 0.0, 0.0), up=(0.0, 0.0, 0.0),
                 right=(0.0, 0.0, 0.0), spot_angle_deg=0.0)
    return R.render(vol16, scale, tf, cache, cam, W, H, step, light,
                    apply_occlusion=bool(p.apply_occlusion), apply_shadow=bool(p.apply_shadow),
                    grad=grad if phong else None, phong=phong)


def builds(d):
    return N.lib().cvr_get_option(d.handle, b"light_cache_builds")


# ---------------------------------------------------------------------------------------
# the light cache
# ---------------------------------------------------------------------------------------

def check_cache(dev, step, name, dims, filter_bits=0):
    p = C.ebs_params(step=step, **C.CASES[name])
    with option(dev, b"filter_bits", filter_bits):
        dev.compute_light_cache_extbsd(p, dims)
        got = dev.light_cache().view(np.uint16)
    want = C.ref_cache(name, dims, filter_bits)
    assert got.shape == want.shape == (dims[2], dims[1], dims[0], 2)
    bad = int((got != want).sum())
    print(f"{name} {dims} filter_bits {filter_bits}: {bad} of {want.size} halfs differ")
    assert_bitexact(got, want, f"{name} {dims} filter_bits {filter_bits}")


@pytest.mark.parametrize("dims", C.CACHE_DIMS, ids=lambda d: "x".join(map(str, d)))
@pytest.mark.parametrize("name", sorted(C.CASES))
def test_cache_bitexact_vs_reference(dev, step, name, dims):
    check_cache(dev, step, name, dims)


@pytest.mark.parametrize("name", ["defaults_point", "cone_60", "light_inside"])
def test_cache_plain_sat_layout(dev, step, name):
    """sat_layout 1 (the plain float SAT) gives the reference's bits too."""
    with option(dev, b"sat_layout", 1):
        check_cache(dev, step, name, C.CACHE_DIMS[0])
    check_cache(dev, step, name, C.CACHE_DIMS[0])    # and back on the cell4 copy (rebuilt)


@pytest.mark.parametrize("name", ["defaults_point", "light_inside"])
def test_cache_filter_bits_8(dev, step, name):
    check_cache(dev, step, name, C.CACHE_DIMS[0], filter_bits=8)


# ---------------------------------------------------------------------------------------
# the frame
# ---------------------------------------------------------------------------------------

MARCH_CASES = {
    #                  cache case,      cache dims,   camera,   W,  H, Phong, flags of the march
    "defaults_point": ("defaults_point", (16, 16, 16), C.INITIAL, 80, 64, False, {}),
    "occlusion_only": ("occlusion_only", (10, 7, 5), C.INITIAL, 80, 64, False, {}),
    "shadow_only": ("shadow_only", (10, 7, 5), C.INITIAL, 57, 43, False, {}),
    "phong_fd": ("defaults_point", (10, 7, 5), C.INITIAL, 80, 64, True, {}),
    "ragged_inside": ("defaults_point", (10, 7, 5), C.INSIDE, 57, 43, False, {}),
    "both_off": ("defaults_point", (10, 7, 5), C.INITIAL, 57, 43, False,
                 dict(apply_occlusion=False, apply_shadow=False)),
}


@pytest.mark.parametrize("name", sorted(MARCH_CASES))
def test_frame_bitexact_vs_reference(dev, step, name):
    cname, dims, cam, W, H, phong, over = MARCH_CASES[name]
    kw = dict(C.CASES[cname], phong=phong, **over)
    p = C.ebs_params(step=step, **kw)
    frames = []
    for flat in (1, 0):
        with option(dev, b"shade_flat", flat):
            frames.append(render(dev, cam, W, H, p, dims))
    g_rgba, g_cnt, g_total = frames[0]
    if over:      # both switches off: the cache computed is all 1.0 and nothing reads it
        cache = np.full((dims[2], dims[1], dims[0], 2), 0x3C00, np.uint16)
        assert_bitexact(dev.light_cache().view(np.uint16), cache, "cache with both terms off")
    else:
        cache = C.ref_cache(cname, dims)
    o_rgba, o_cnt, o_total = ref_render(cache, cam, W, H, step, p, phong=phong)
    assert_bitexact(g_cnt, o_cnt, f"{name} counts")
    assert_bitexact(g_rgba, o_rgba, f"{name} rgba")
    assert g_total == o_total == int(o_cnt.sum()) > 0
    assert_bitexact(frames[1][1], g_cnt, f"{name} counts, shade_flat 0 vs 1")
    assert_bitexact(frames[1][0], g_rgba, f"{name} rgba, shade_flat 0 vs 1")
    assert frames[1][2] == g_total
    if name == "both_off":
        assert not g_rgba.any()                # `src.a > 0 && Shade`: nothing composited
    else:
        assert o_rgba[..., 3].max() > 0.5      # the frame is not empty


def test_same_march_as_the_dos_switch(dev, step):
    """The GPU's EBS cache, uploaded with cvr_set_light_cache and rendered by
    cvr_render_preillum with the equivalent cvr_dos_params, gives the frame of
    cvr_render_extbsd_preillum."""
    dims, (W, H) = (10, 7, 5), (80, 64)
    p = C.ebs_params(step=step, phong=True)
    want = render(dev, C.INITIAL, W, H, p, dims)
    cache = dev.light_cache()
    dev.set_light_cache(cache)
    q = N.DosParams()
    q.step, q.apply_gradient_shading = p.step, 1
    q.ka, q.kd, q.ks, q.shininess = p.ka, p.kd, p.ks, p.shininess
    q.ispecular[:] = list(p.ispecular)
    q.light.position[:] = list(p.light_pos)
    q.apply_occlusion, q.apply_shadow, q.shadow_type = 1, 1, 0
    q.occlusion, q.shadow = default_cone_params(True), default_cone_params(False)
    frame = make_frame(Camera(**C.INITIAL), W, H)
    rgba = np.zeros((H, W, 4), np.float32)
    cnt = np.zeros((H, W), np.uint32)
    total = np.zeros(1, np.uint64)
    out = N.Output(rgba.ctypes.data, cnt.ctypes.data, total.ctypes.data, 0)
    N.check(N.lib().cvr_render_preillum(dev.handle, ctypes.byref(frame), ctypes.byref(q), ctypes.byref(out)),
            "cvr_render_preillum", dev.handle)
    assert_bitexact(cnt, want[1], "counts through cvr_render_preillum")
    assert_bitexact(rgba, want[0], "rgba through cvr_render_preillum")
    assert int(total[0]) == want[2]
    assert want[0][..., 3].max() > 0.5


# ---------------------------------------------------------------------------------------
# the cache object
# ---------------------------------------------------------------------------------------

def test_extbsd_preillum_skips_unchanged_computes(step, bonsai_tf_rgba):
    """Update in one call: one compute serves a whole orbit (the camera never enters the
    key); the compute runs again only when something the cache depends on changed."""
    d = Device(0)
    try:
        setup(d)
        dims, (W, H) = (10, 7, 5), (57, 43)
        kw = dict(step=step)
        p = C.ebs_params(**kw)
        assert builds(d) == 0
        first = None
        for cam in ORBIT:
            g = render(d, cam, W, H, p, dims)
            first = first or g
        assert builds(d) == 1                                  # 8 views, one compute
        o = ref_render(C.ref_cache("defaults_point", dims), ORBIT[0], W, H, step, p)
        assert_bitexact(first[0], o[0], "orbit view 0 vs reference")
        n = 1

        def frame_builds(q, dd=dims):
            render(d, ORBIT[3], W, H, q, dd)
            return builds(d)

        kw["light"] = (C.LIGHT_POS[0] + 10.0, C.LIGHT_POS[1], C.LIGHT_POS[2])
        n += 1; assert frame_builds(C.ebs_params(**kw)) == n   # a moved light
        kw["shells"] = 9
        n += 1; assert frame_builds(C.ebs_params(**kw)) == n   # other occlusion shells
        kw["interval"] = 3.0
        n += 1; assert frame_builds(C.ebs_params(**kw)) == n   # another shadow parameter
        assert frame_builds(C.ebs_params(**kw)) == n           # nothing changed
        n += 1; assert frame_builds(C.ebs_params(**kw), (16, 16, 16)) == n   # other dims
        n += 1; assert frame_builds(C.ebs_params(**kw)) == n   # and back
        d.set_extinction_sat(C.scene()[4])                     # a new SAT drops the cache
        assert N.lib().cvr_copy_light_cache(d.handle, None, 0, dims_c(dims)) == N.CVR_ERR_STATE
        n += 1; assert frame_builds(C.ebs_params(**kw)) == n
        # a DOS compute in between takes the cache object: the EBS frame recomputes
        d.set_extinction_volume(bonsai_tf_rgba, (16, 16, 16))
        q = N.DosParams()
        q.step = step
        q.ka, q.kd, q.ks, q.shininess = 0.5, 0.5, 0.8, 30.0
        q.light.position[:] = list(C.LIGHT_POS)
        q.light.right[:] = [1.0, 0.0, 0.0]
        q.apply_occlusion, q.apply_shadow = 1, 0
        q.occlusion, q.shadow = default_cone_params(True), default_cone_params(False)
        d.compute_light_cache(make_frame(Camera(**ORBIT[3]), W, H), q, dims)
        n += 1; assert builds(d) == n
        n += 1; assert frame_builds(C.ebs_params(**kw)) == n
        # a shadow parameter changed while shadow is off does not reach the cache
        kw["apply_shadow"] = False
        n += 1; assert frame_builds(C.ebs_params(**kw)) == n   # the switch itself counts
        kw["interval"], kw["angle"] = 5.0, 7.0
        kw["light"] = C.LIGHT_INSIDE
        g = render(d, ORBIT[5], W, H, C.ebs_params(**kw), dims)
        assert builds(d) == n
        assert g[0][..., 3].max() > 0.5
    finally:
        d.close()


def test_errors(dev, step, bonsai_tf):
    L = N.lib()
    p = C.ebs_params(step=step)
    fr = make_frame(Camera(**C.INITIAL), 16, 16)
    img = np.zeros((16, 16, 4), np.float32)
    out = N.Output(img.ctypes.data, None, None, 0)
    ok = dims_c((8, 8, 8))
    for bad in ((1, 32, 32), (32, 32, 513), (32, 0, 32)):
        b = dims_c(bad)
        assert L.cvr_compute_light_cache_extbsd(dev.handle, ctypes.byref(p), b) == N.CVR_ERR_ARG
        assert L.cvr_render_extbsd_preillum(dev.handle, ctypes.byref(fr), ctypes.byref(p), b,
                                            ctypes.byref(out)) == N.CVR_ERR_ARG
    with option(dev, b"native_exp", 1):        # tolerance mode: no light-cache form (as the DOS compute)
        assert L.cvr_compute_light_cache_extbsd(dev.handle, ctypes.byref(p), ok) == N.CVR_ERR_ARG
    # filter_bits 8 reads the cell4 copy only: the frame's own error
    with option(dev, b"filter_bits", 8), option(dev, b"sat_layout", 1):
        want = L.cvr_render_extbsd(dev.handle, ctypes.byref(fr), ctypes.byref(p), ctypes.byref(out))
        assert want == N.CVR_ERR_ARG
        assert L.cvr_compute_light_cache_extbsd(dev.handle, ctypes.byref(p), ok) == want
        assert L.cvr_render_extbsd_preillum(dev.handle, ctypes.byref(fr), ctypes.byref(p), ok,
                                            ctypes.byref(out)) == want
    # no SAT on a fresh context
    d = Device(0)
    try:
        vol, scale, _, tf, _, _, _ = C.scene()
        assert L.cvr_compute_light_cache_extbsd(d.handle, ctypes.byref(p), ok) == N.CVR_ERR_STATE
        d.set_volume(vol, scale)
        d.set_transfer_function(tf)
        assert L.cvr_compute_light_cache_extbsd(d.handle, ctypes.byref(p), ok) == N.CVR_ERR_STATE
        assert L.cvr_render_extbsd_preillum(d.handle, ctypes.byref(fr), ctypes.byref(p), ok,
                                            ctypes.byref(out)) == N.CVR_ERR_STATE
        assert builds(d) == 0
    finally:
        d.close()
    # a group context refuses both entry points
    grp = Device(devices=[0, 0])
    try:
        for call in (lambda: L.cvr_compute_light_cache_extbsd(grp.handle, ctypes.byref(p), ok),
                     lambda: L.cvr_render_extbsd_preillum(grp.handle, ctypes.byref(fr), ctypes.byref(p), ok,
                                                          ctypes.byref(out))):
            assert call() == N.CVR_ERR_STATE
            assert b"group" in L.cvr_last_error(grp.handle)
    finally:
        grp.close()


def test_python_renderer_switch(dev, step):
    """RC1PExtinctionBasedShading(pre_illumination=True) renders the frame of
    cvr_render_extbsd_preillum; the default stays the on-the-fly renderer."""
    import torch
    vol, scale, _, tf, lut, _, _ = C.scene()
    dm = DataManager()
    dm.SetVolume(vol, scale)
    dm.SetTransferFunction(tf)
    dm.SetExtinctionTable(lut)
    W, H = 80, 64
    rp = RenderingParameters(W, H, light_position=C.LIGHT_POS, light_forward=C.LIGHT_FWD)
    assert RC1PExtinctionBasedShading().pre_illumination is False
    assert RC1PExtinctionBasedShading().light_cache_resolution == (32, 32, 32)
    r = RC1PExtinctionBasedShading(0, pre_illumination=True, light_cache_resolution=(10, 7, 5))
    r.SetExternalResources(dm, rp)
    assert r.Init(W, H)
    try:
        r.m_u_step_size = step
        r.PrepareRender(Camera(**C.INITIAL))
        r.Redraw()
        torch.cuda.synchronize()
        got = r.rgba.cpu().numpy()
        assert builds(r.device) == 1
        assert r.device.light_cache().shape == (5, 7, 10, 2)
    finally:
        r.Clean()
    want = render(dev, C.INITIAL, W, H, C.ebs_params(step=step), (10, 7, 5))
    assert_bitexact(got, want[0], "Python renderer vs the C-ABI path")
    assert want[0][..., 3].max() > 0.5
