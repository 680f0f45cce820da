"""GPU parity of the ground-truth cone ray-caster (crtgt.hip) against its CPU restatement
(tests/support/crtgt_ref.cpp), bit for bit: RGBA, per-pixel counts, total; the progressive
frame's independence of how the march is cut into calls; the binary16 ray tables; the
outputs, errors, memory accounting and the Python renderer class.
Setup: tests/crtgt_cases.py (the scene of tests/preillum_cases.py)."""
import contextlib
import ctypes

import numpy as np
import pytest

import crtgt_cases as C
from cpp_volume_rendering_amd import _native as N
from cpp_volume_rendering_amd.renderer import (Camera, DataManager, Device,
                                               RC1PConeLightGroundTruthSteps,
                                               RenderingParameters, make_frame)

from test_rc1pass_gpu import assert_bitexact

pytestmark = pytest.mark.gpu


def setup(d):
    vol, scale, _, tf, _, _ = C.scene()
    d.set_volume(vol, scale)
    d.set_transfer_function(tf)
    d.set_gradient(N.GRADIENT_FINITE_DIFFERENCES)


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    d = Device(0)
    setup(d)
    yield d
    d.close()


@contextlib.contextmanager
def option(d, key, value):
    L = N.lib()
    old = L.cvr_get_option(d.handle, key)
    N.check(L.cvr_set_option(d.handle, key, value), key.decode(), d.handle)
    try:
        yield
    finally:
        L.cvr_set_option(d.handle, key, old)


def params(name):
    occ_on, sdw_on, stype, phong, _, _, _ = C.CASES[name]
    p = N.CrtgtParams()
    N.lib().cvr_crtgt_params_default(ctypes.byref(p))
    p.step = C.scene()[5]
    p.apply_gradient_shading = int(phong)
    for k in ("position", "forward", "up", "right"):
        getattr(p.light, k)[:] = list(C.LIGHT0[k])
    p.light.spot_angle_deg = C.LIGHT0["spot_angle_deg"]
    p.light_gap, p.light_step = C.LIGHT_GAP, C.LIGHT_STEP
    p.apply_occlusion, p.occ_distance = int(occ_on), C.OCC_DISTANCE
    p.apply_shadow, p.sdw_distance = int(sdw_on), C.SDW_DISTANCE
    p.shadow_type = stype
    return p


def host_out(W, H, fmt=N.FORMAT_RGBA32F):
    rgba = np.zeros((H, W, 4), np.float16 if fmt == N.FORMAT_RGBA16F else np.float32)
    cnt = np.zeros((H, W), np.uint32)
    total = np.zeros(1, np.uint64)
    return rgba, cnt, total, N.Output(rgba.ctypes.data, cnt.ctypes.data, total.ctypes.data, 0, fmt)


def tables(name, occ=None, sdw=None):
    o, s = C.rays(C.CASES[name][6])
    return (o if occ is None else occ), (s if sdw is None else sdw)


def render(d, name, W, H, occ=None, sdw=None, fmt=N.FORMAT_RGBA32F):
    """One frame through cvr_render_crtgt (host outputs)."""
    occ, sdw = tables(name, occ, sdw)
    occ, sdw = np.ascontiguousarray(occ, np.float32), np.ascontiguousarray(sdw, np.float32)
    frame = make_frame(Camera(**C.CASES[name][4]), W, H)
    p = params(name)
    rgba, cnt, total, out = host_out(W, H, fmt)
    N.check(N.lib().cvr_render_crtgt(d.handle, ctypes.byref(frame), ctypes.byref(p), N.fptr(occ),
                                     occ.shape[0], N.fptr(sdw), sdw.shape[0], ctypes.byref(out)),
            "cvr_render_crtgt", d.handle)
    return rgba, cnt, int(total[0])


def stepped(d, name, W, H, chunk):
    """begin, then advance(chunk) until converged: the frame and the unfinished counts."""
    occ, sdw = tables(name)
    d.crtgt_begin(make_frame(Camera(**C.CASES[name][4]), W, H), params(name), occ, sdw)
    lefts = []
    for _ in range(10000):
        rgba, cnt, total, out = host_out(W, H)
        lefts.append(d.crtgt_advance(chunk, out))
        if lefts[-1] == 0:
            break
    return (rgba, cnt, int(total[0])), lefts


# ---------------------------------------------------------------------------------------
# bit-exact against the CPU reference
# ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("W,H", C.FRAMES)
@pytest.mark.parametrize("name", sorted(C.CASES))
def test_bitexact_vs_reference(dev, name, W, H):
    fb = C.CASES[name][5]
    with option(dev, b"filter_bits", fb):
        g_rgba, g_cnt, g_total = render(dev, name, W, H)
    o_rgba, o_cnt, o_total = C.reference(name, W, H)
    assert_bitexact(g_cnt, o_cnt, f"{name} counts")
    if name == "both_off":   # NaN where either side has one (a NaN's sign and payload are not pinned)
        nan = np.isnan(o_rgba)
        assert np.array_equal(np.isnan(g_rgba), nan)
        assert_bitexact(np.where(nan, 0.0, g_rgba).astype(np.float32), np.where(nan, 0.0, o_rgba).astype(np.float32),
                        f"{name} rgba")
    else:
        assert np.isfinite(o_rgba).all()
        assert_bitexact(g_rgba, o_rgba, f"{name} rgba")
    assert g_total == o_total == int(o_cnt.sum()) > 0
    if name == "both_off":
        comp = C.plain("INITIAL", W, H)[..., 3] > 0
        assert comp.any() and np.isnan(g_rgba[..., :3][comp]).all()   # 0 * (1 / 0)
        assert not g_rgba[~comp].any()
    else:
        C.assert_shading_visible(name, W, H)
    if name == "both_spot":
        # the shadow term is 0 everywhere, as written: the occlusion term under
        # 1 / (ka + kd) = 1 instead of 1 / ka = 2, exactly half the colour
        occ = C.reference("occlusion", W, H)[0]
        assert np.array_equal(g_rgba[..., :3], 0.5 * occ[..., :3])
        assert np.array_equal(g_rgba[..., 3], occ[..., 3])


# ---------------------------------------------------------------------------------------
# the progressive frame
# ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,W,H", [("both_point", 77, 53), ("phong_fd", 96, 80)])
def test_chunk_independence(dev, name, W, H):
    one, lefts1 = stepped(dev, name, W, H, 1)
    seven, lefts7 = stepped(dev, name, W, H, 7)
    # one more advance changes nothing and reports 0
    rgba, cnt, total, out = host_out(W, H)
    assert dev.crtgt_advance(7, out) == 0
    whole = render(dev, name, W, H)
    for got, what in ((seven, "advance(7)"), ((rgba, cnt, int(total[0])), "one more advance"), (whole, "render")):
        assert_bitexact(got[1], one[1], f"{what} counts")
        assert_bitexact(got[0], one[0], f"{what} rgba")
        assert got[2] == one[2]
    assert_bitexact(one[0], C.reference(name, W, H)[0], "advance(1) vs reference")
    for lefts in (lefts1, lefts7):
        assert lefts[-1] == 0 and all(a >= b for a, b in zip(lefts, lefts[1:]))
    assert len(lefts1) == int(one[1].max()) and len(lefts7) == -(-int(one[1].max()) // 7)
    assert 0 < lefts1[0] <= W * H


def test_binary16_tables(dev):
    """Tables that are not exact in binary16 give the frame of the same tables rounded on
    the host: the renderer stores RGB16F."""
    name, (W, H) = "both_point", C.FRAMES[1]
    occ, sdw = C.rays()
    occ_h = occ.astype(np.float16).astype(np.float32)
    sdw_h = sdw.astype(np.float16).astype(np.float32)
    assert not np.array_equal(occ, occ_h) and not np.array_equal(sdw, sdw_h)
    a = render(dev, name, W, H, occ, sdw)
    b = render(dev, name, W, H, occ_h, sdw_h)
    assert_bitexact(a[0], b[0], "float tables vs pre-rounded tables")
    assert_bitexact(a[0], C.reference(name, W, H)[0], "vs reference")


def test_outputs(dev):
    import torch
    name, (W, H) = "both_point", C.FRAMES[1]
    want = C.reference(name, W, H)
    half = render(dev, name, W, H, fmt=N.FORMAT_RGBA16F)
    assert_bitexact(half[0].view(np.uint16), want[0].astype(np.float16).view(np.uint16), "RGBA16F")
    assert_bitexact(half[1], want[1], "RGBA16F counts")
    # device pointers: the frame of the host path; the total is added to the caller's
    occ, sdw = tables(name)
    dev.crtgt_begin(make_frame(Camera(**C.CASES[name][4]), W, H), params(name), occ, sdw)
    s = torch.cuda.current_stream(0)
    dev.set_stream(s.cuda_stream)
    rgba = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
    cnt = torch.zeros((H, W), dtype=torch.int32, device="cuda:0")
    total = torch.full((1,), 5, dtype=torch.int64, device="cuda:0")
    out = N.Output(rgba.data_ptr(), cnt.data_ptr(), total.data_ptr(), 1, N.FORMAT_RGBA32F)
    while dev.crtgt_advance(16, None) > 0:     # no copy until converged
        pass
    assert dev.crtgt_advance(16, out) == 0
    torch.cuda.synchronize()
    assert_bitexact(rgba.cpu().numpy(), want[0], "device rgba")
    assert_bitexact(cnt.cpu().numpy().view(np.uint32), want[1], "device counts")
    assert int(total.item()) == 5 + want[2]


# ---------------------------------------------------------------------------------------
# errors, memory
# ---------------------------------------------------------------------------------------

def test_errors(dev):
    L = N.lib()
    name = "both_point"
    occ, sdw = (np.ascontiguousarray(t) for t in C.rays())
    big = np.zeros((N.CRTGT_MAX_RAYS + 1, 3), np.float32)
    big[:, 2] = 1.0
    p = params(name)
    fr = make_frame(Camera(**C.INITIAL), 16, 16)
    rgba, cnt, total, out = host_out(16, 16)

    def begin(d=dev, frame=fr, prm=p, o=occ, no=None, s=sdw, ns=None):
        return L.cvr_crtgt_begin(d.handle, ctypes.byref(frame), ctypes.byref(prm), N.fptr(o),
                                 o.shape[0] if no is None else no, N.fptr(s), s.shape[0] if ns is None else ns)

    assert begin(no=0) == N.CVR_ERR_ARG and begin(ns=0) == N.CVR_ERR_ARG      # n = 0, term on
    assert begin(o=big) == N.CVR_ERR_ARG and begin(s=big) == N.CVR_ERR_ARG    # n = 10001
    off = params("occlusion")
    assert begin(prm=off, ns=0) == N.CVR_OK                                   # n = 0, term off
    split = make_frame(Camera(**C.INITIAL), 32, 32, tile_size=16, rank=0, nranks=2)
    assert begin(frame=split) == N.CVR_ERR_ARG
    bad = params(name)
    bad.light_step = 0.0
    assert begin(prm=bad) == N.CVR_ERR_ARG                                    # the ray loop would not end
    bad.light_step, bad.shadow_type = C.LIGHT_STEP, 3
    assert begin(prm=bad) == N.CVR_ERR_ARG
    with option(dev, b"native_exp", 1):
        assert begin() == N.CVR_ERR_ARG
        assert L.cvr_render_crtgt(dev.handle, ctypes.byref(fr), ctypes.byref(p), N.fptr(occ), occ.shape[0],
                                  N.fptr(sdw), sdw.shape[0], ctypes.byref(out)) == N.CVR_ERR_ARG
    assert begin() == N.CVR_OK
    left = ctypes.c_ulonglong()
    assert L.cvr_crtgt_advance(dev.handle, 0, ctypes.byref(out), ctypes.byref(left)) == N.CVR_ERR_ARG
    assert L.cvr_crtgt_advance(dev.handle, 1, ctypes.byref(out), ctypes.byref(left)) == N.CVR_OK
    # a fresh context: nothing to march, then no frame in progress, then a new TF ends one
    d = Device(0)
    try:
        vol, scale, _, tf, _, _ = C.scene()
        assert begin(d=d) == N.CVR_ERR_STATE                                  # no volume or TF
        d.set_volume(vol, scale)
        d.set_transfer_function(tf)
        ph = params("phong_fd")
        assert begin(d=d, prm=ph) == N.CVR_ERR_STATE                          # Phong without a gradient
        assert L.cvr_crtgt_advance(d.handle, 1, ctypes.byref(out), ctypes.byref(left)) == N.CVR_ERR_STATE
        before = d.device_bytes()
        assert begin(d=d) == N.CVR_OK
        # the documented storage: 32 B of state and 4 x (2 float4 + a list entry) of jobs
        # per pixel, 24 B of counters, 12 B per ray
        assert d.device_bytes() - before == 16 * 16 * (32 + 4 * 36) + 24 + 12 * (occ.shape[0] + sdw.shape[0])
        assert L.cvr_crtgt_advance(d.handle, 1, ctypes.byref(out), ctypes.byref(left)) == N.CVR_OK
        d.set_transfer_function(tf)
        assert L.cvr_crtgt_advance(d.handle, 1, ctypes.byref(out), ctypes.byref(left)) == N.CVR_ERR_STATE
        assert b"cvr_crtgt_begin" in L.cvr_last_error(d.handle)
    finally:
        d.close()
    grp = Device(devices=[0, 0])
    try:
        calls = [
            lambda: begin(d=grp),
            lambda: L.cvr_crtgt_advance(grp.handle, 1, ctypes.byref(out), ctypes.byref(left)),
            lambda: L.cvr_render_crtgt(grp.handle, ctypes.byref(fr), ctypes.byref(p), N.fptr(occ), occ.shape[0],
                                       N.fptr(sdw), sdw.shape[0], ctypes.byref(out)),
        ]
        for call in calls:
            assert call() == N.CVR_ERR_STATE
            assert b"group" in L.cvr_last_error(grp.handle)
    finally:
        grp.close()


# ---------------------------------------------------------------------------------------
# the Python renderer
# ---------------------------------------------------------------------------------------

def test_python_renderer(dev):
    """RC1PConeLightGroundTruthSteps mirrors the reference's members and defaults, advances
    samples_per_redraw iterations per Redraw and converges to the C-ABI frame."""
    import torch
    r = RC1PConeLightGroundTruthSteps()
    assert r.GetName() == "1-Pass - Ray Casting - Cone Ground Truth (Steps)"
    assert r.GetAbbreviationName() == "s_1rc_gt_c"
    assert (r.m_apply_occlusion, r.m_occ_num_rays_sampled, r.m_occ_cone_aperture_angle) == (False, 1, 90.0)
    assert (r.m_apply_shadows, r.m_sdw_num_rays_sampled, r.m_sdw_cone_aperture_angle) == (False, 1, 1.0)
    assert (r.m_u_light_ray_initial_step, r.m_u_light_ray_step_size, r.m_shadow_type) == (1.0, 0.5, 0)
    name, (W, H) = "both_point", C.FRAMES[0]
    vol, scale, _, tf, _, step = C.scene()
    dm = DataManager()
    dm.SetVolume(vol, scale)
    dm.SetTransferFunction(tf)
    rp = RenderingParameters(W, H, light_position=C.LIGHT0["position"], light_forward=C.LIGHT0["forward"],
                             light_up=C.LIGHT0["up"], light_right=C.LIGHT0["right"],
                             spot_light_angle=C.LIGHT0["spot_angle_deg"])
    r = RC1PConeLightGroundTruthSteps(0, samples_per_redraw=5, ray_seed=C.SEED)
    r.SetExternalResources(dm, rp)
    assert r.Init(W, H)
    try:
        assert abs(r.m_occ_cone_distance_eval - np.sqrt(3.0) * 256.0) < 1e-3      # diagonal * 0.50
        assert abs(r.m_sdw_cone_distance_eval - np.sqrt(3.0) * 384.0) < 1e-3      # diagonal * 0.75
        assert r.m_u_step_size == step
        r.m_apply_occlusion, r.m_apply_shadows = True, True
        r.m_occ_num_rays_sampled, r.m_occ_cone_aperture_angle = C.N_OCC, C.OCC_APERTURE
        r.m_sdw_num_rays_sampled, r.m_sdw_cone_aperture_angle = C.N_SDW, C.SDW_APERTURE
        r.m_u_light_ray_initial_step, r.m_u_light_ray_step_size = C.LIGHT_GAP, C.LIGHT_STEP
        r.m_occ_cone_distance_eval, r.m_sdw_cone_distance_eval = C.OCC_DISTANCE, C.SDW_DISTANCE
        r.SetLightParametersOutdated()
        r.PrepareRender(Camera(**C.INITIAL))
        assert r.frame_outdated
        redraws = 0
        while r.frame_outdated:
            r.Redraw()
            redraws += 1
        torch.cuda.synchronize()
        got = r.rgba.cpu().numpy()
        cnt = r.samples.cpu().numpy().view(np.uint32)
        total = int(r.total.item())
        r.Redraw()                                   # a converged frame is kept
        torch.cuda.synchronize()
        assert np.array_equal(r.rgba.cpu().numpy(), got, equal_nan=True)
    finally:
        r.Clean()
    want = render(dev, name, W, H)
    assert_bitexact(got, want[0], "Python renderer vs the C-ABI path")
    assert_bitexact(cnt, want[1], "Python renderer counts")
    assert total == want[2] and redraws == -(-int(want[1].max()) // 5)
    assert want[0][..., 3].max() > 0.5
