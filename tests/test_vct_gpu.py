"""GPU parity of the voxel cone tracing renderer (vct.hip, vct_precompute.hip) against its CPU
restatement (tests/support/vct_ref.cpp), bit for bit: the pyramid, the table, RGBA, per-pixel
counts and the total; shade_flat 0 / 1, the screen-tile split, invalidation, the outputs,
errors, memory accounting and the Python renderer class.
Setup: tests/vct_cases.py (the scenes of tests/crtgt_cases.py and tests/aniso_cases.py)."""
import contextlib
import ctypes
import math

import numpy as np
import pytest

import aniso_cases as A
import vct_cases as C
import vct_ref as R
from cpp_volume_rendering_amd import _native as N
from cpp_volume_rendering_amd import datasets as D
from cpp_volume_rendering_amd.renderer import (Camera, DataManager, Device, RC1PVoxelConeTracingSGPU,
                                               RenderingParameters, build_opacity_lut, make_frame)

from test_rc1pass_gpu import assert_bitexact

pytestmark = pytest.mark.gpu


def setup(d, which="cubic"):
    vol, scale, _, tf, _, _ = C.scene(which)
    d.set_volume(vol, scale)
    d.set_transfer_function(tf)
    d.vct_set_opacity(C.opacity_lut())
    d.set_gradient(N.GRADIENT_FINITE_DIFFERENCES)


@pytest.fixture(scope="module")
def devs():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    ds = {}
    for which in ("cubic", "aniso"):
        ds[which] = Device(0)
        setup(ds[which], which)
    yield ds
    for d in ds.values():
        d.close()


@pytest.fixture(scope="module")
def dev(devs):
    return devs["cubic"]


@contextlib.contextmanager
def option(d, key, value):
    L = N.lib()
    old = L.cvr_get_option(d.handle, key)
    N.check(L.cvr_set_option(d.handle, key, value), key.decode(), d.handle)
    try:
        yield
    finally:
        L.cvr_set_option(d.handle, key, old)


def host_out(W, H, fmt=N.FORMAT_RGBA32F):
    rgba = np.zeros((H, W, 4), np.float16 if fmt == N.FORMAT_RGBA16F else np.float32)
    cnt = np.zeros((H, W), np.uint32)
    total = np.zeros(1, np.uint64)
    return rgba, cnt, total, N.Output(rgba.ctypes.data, cnt.ctypes.data, total.ctypes.data, 0, fmt)


def render(d, name, W, H, fmt=N.FORMAT_RGBA32F, p=None):
    """One frame of a case through cvr_render_vct (host outputs)."""
    frame = make_frame(Camera(**C.CASES[name][5]), W, H)
    p = p or C.params(name)
    rgba, cnt, total, out = host_out(W, H, fmt)
    N.check(N.lib().cvr_render_vct(d.handle, ctypes.byref(frame), ctypes.byref(p), ctypes.byref(out)),
            "cvr_render_vct", d.handle)
    return rgba, cnt, int(total[0])


def assert_frame(got, want, what):
    assert_bitexact(got[1], want[1], f"{what} counts")
    nan = np.isnan(want[0])
    assert np.array_equal(np.isnan(got[0]), nan), f"{what}: NaN positions"
    assert_bitexact(np.where(nan, 0.0, got[0]).astype(np.float32), np.where(nan, 0.0, want[0]).astype(np.float32),
                    f"{what} rgba")
    assert got[2] == want[2] == int(want[1].sum()) > 0


def bits16(a):
    return np.ascontiguousarray(a, np.float32).astype(np.float16).view(np.uint16)


# ---------------------------------------------------------------------------------------
# precompute
# ---------------------------------------------------------------------------------------

def check_precompute(d, pyr, tab):
    levels, mx = pyr
    d.vct_precompute()
    info = d.vct_info()
    assert info.levels == len(levels) and info.max_stddev == mx
    assert [tuple(info.dims[l]) for l in range(info.levels)] == [l.shape[2::-1] for l in levels]
    for L, (got, want) in enumerate(zip(d.vct_pyramid(), levels)):
        assert got.shape == want.shape
        assert_bitexact(got, want, f"pyramid level {L}")
    if tab is not None:
        assert (info.table_width, info.table_height) == (255, math.ceil(mx)) == tab.shape[::-1]
        assert_bitexact(d.vct_table(), tab, "table")


@pytest.mark.parametrize("which", ["cubic", "aniso"])
def test_precompute_bitexact(devs, which):
    check_precompute(devs[which], *C.precomputed(which))
    builds = N.lib().cvr_get_option(devs[which].handle, b"vct_pyramid_builds")
    devs[which].vct_precompute()                                   # idempotent
    assert N.lib().cvr_get_option(devs[which].handle, b"vct_pyramid_builds") == builds == 1


def test_precompute_small_and_constant_volumes():
    d = Device(0)
    try:
        vol = np.random.default_rng(5).integers(0, 256, (3, 5, 7), dtype=np.uint8)   # 7 x 5 x 3: 2 levels
        d.set_volume(vol, (1.0, 1.0, 1.0))
        d.vct_set_opacity(C.opacity_lut())
        pyr = R.pyramid(vol)
        assert len(pyr[0]) == 2
        check_precompute(d, pyr, R.table(vol, C.tf_table(), pyr[1]))
        d.set_volume(np.full((8, 8, 8), 77, np.uint8), (1.0, 1.0, 1.0))
        assert d.vct_info().levels == 0
        d.vct_set_opacity(C.opacity_lut())
        assert N.lib().cvr_vct_precompute(d.handle) == N.CVR_ERR_ARG           # a table of height 0
        assert b"standard deviation" in N.lib().cvr_last_error(d.handle)
        info = d.vct_info()
        assert info.levels == 4 and info.max_stddev == 0.0 and info.table_height == 0
    finally:
        d.close()


# ---------------------------------------------------------------------------------------
# frames, bit for bit against the CPU reference
# ---------------------------------------------------------------------------------------

FRAME_CASES = [(n, W, H) for n in sorted(C.CASES) for (W, H) in C.frames(n)]


@pytest.mark.parametrize("name,W,H", FRAME_CASES)
def test_bitexact_vs_reference(devs, name, W, H):
    d = devs[C.CASES[name][0]]
    with option(d, b"filter_bits", C.CASES[name][6]):
        got = render(d, name, W, H)
    want = C.reference(name, W, H)
    assert_frame(got, want, name)
    if name == "both_off":
        comp = C.plain(name, W, H)[0][..., 3] > 0
        assert comp.any() and np.isnan(got[0][..., :3][comp]).all()   # 0 * (1 / 0)
        assert not got[0][~comp].any()
    else:
        assert np.isfinite(want[0]).all()
    if name in C.SHADOWED:
        C.assert_shading_visible(name, W, H)


@pytest.mark.parametrize("name", ["clamped_top", "phong_fd"])
def test_shade_flat_gives_the_same_bits(dev, name):
    W, H = C.FRAMES[1]
    with option(dev, b"shade_flat", 0):
        wave = render(dev, name, W, H)
    with option(dev, b"shade_flat", 1):
        flat = render(dev, name, W, H)
    assert_frame(wave, C.reference(name, W, H), f"{name} per-wave")
    assert_frame(flat, wave, f"{name} flat vs per-wave")


def test_shade_counters(dev):
    """lit counts the cones traced, fetches 8 texels per level touched plus 4 per table fetch."""
    name, (W, H) = "multi_level", C.FRAMES[1]
    with option(dev, b"shade_counters", 1):
        render(dev, name, W, H)
        ctr = (ctypes.c_uint64 * 3)()
        N.check(N.lib().cvr_read_shade_counters(dev.handle, ctr), "cvr_read_shade_counters", dev.handle)
    st = C.reference(name, W, H)[3]
    assert (ctr[1], ctr[2]) == (st["cones"], st["fetches"]) and ctr[0] == st["cones"]


def test_split_over_two_ranks(dev):
    from cpp_volume_rendering_amd import screen_tiles as T
    name, (W, H), tile, nranks = "multi_level", C.FRAMES[0], 16, 2
    full = render(dev, name, W, H)
    p = C.params(name)
    tpr = T.max_tiles_per_rank(W, H, tile, nranks)
    packed = np.zeros((nranks, tpr, tile, tile, 4), np.float32)
    tot = 0
    for r in range(nranks):
        k = T.tiles_for_rank(W, H, tile, r, nranks)
        rgba = np.zeros((k, tile, tile, 4), np.float32)
        total = np.zeros(1, np.uint64)
        out = N.Output(rgba.ctypes.data, None, total.ctypes.data, 0)
        fr = make_frame(Camera(**C.CASES[name][5]), W, H, tile, r, nranks)
        N.check(N.lib().cvr_render_vct(dev.handle, ctypes.byref(fr), ctypes.byref(p), ctypes.byref(out)),
                "vct tiles", dev.handle)
        packed[r, :k] = rgba
        tot += int(total[0])
    assert tot == full[2]
    assert_bitexact(T.unpack(packed, W, H, tile, nranks), full[0], "vct tiles")
    assert_bitexact(full[0], C.reference(name, W, H)[0], "vs reference")


def test_group_context_matches_one_device():
    name, (W, H) = "multi_level", C.FRAMES[1]
    grp = Device(devices=[0, 0])
    try:
        setup(grp)
        assert_frame(render(grp, name, W, H), C.reference(name, W, H), "group")
    finally:
        grp.close()


# ---------------------------------------------------------------------------------------
# invalidation
# ---------------------------------------------------------------------------------------

def test_invalidation():
    import oracle as O
    L = N.lib()
    name, (W, H) = "multi_level", C.FRAMES[1]
    alpha = [(a * 0.5, v) for a, v in D.BONSAI_TF_ALPHA]
    tf2 = O.tf_rgbt(O.tf_table_double(D.BONSAI_TF_RGB, alpha))
    lut2 = build_opacity_lut(D.BONSAI_TF_RGB, alpha)
    d, fresh = Device(0), Device(0)
    try:
        setup(d)
        first = render(d, name, W, H)
        assert_frame(first, C.reference(name, W, H), "before")
        assert L.cvr_get_option(d.handle, b"vct_pyramid_builds") == 1
        d.set_transfer_function(tf2)
        assert d.vct_info().table_height == 0 and d.vct_info().levels == 6      # the table is gone
        fr = make_frame(Camera(**C.INITIAL), W, H)
        p = C.params(name)
        keep = host_out(W, H)               # the arrays `out` points at stay alive
        out = keep[3]
        assert L.cvr_render_vct(d.handle, ctypes.byref(fr), ctypes.byref(p), ctypes.byref(out)) == N.CVR_ERR_STATE
        d.vct_set_opacity(lut2)
        second = render(d, name, W, H)
        assert L.cvr_get_option(d.handle, b"vct_pyramid_builds") == 1           # the table alone was rebuilt
        vol, scale, _, _, _, _ = C.scene("cubic")
        fresh.set_volume(vol, scale)
        fresh.set_transfer_function(tf2)
        fresh.vct_set_opacity(lut2)
        assert_frame(second, render(fresh, name, W, H), "after a new TF vs a fresh context")
        assert_bitexact(d.vct_table(), fresh.vct_table(), "table")
        assert not np.array_equal(second[0], first[0])
        # a new volume: both are rebuilt
        avol, ascale = C.scene("aniso")[:2]
        d.set_volume(avol, ascale)
        assert d.vct_info().levels == 0
        d.set_transfer_function(C.scene("aniso")[3])
        d.vct_set_opacity(C.opacity_lut())
        aw, ah = C.ANISO_FRAME
        assert_frame(render(d, "aniso_outside", aw, ah), C.reference("aniso_outside", aw, ah), "after a new volume")
        assert L.cvr_get_option(d.handle, b"vct_pyramid_builds") == 2
    finally:
        d.close()
        fresh.close()


# ---------------------------------------------------------------------------------------
# outputs
# ---------------------------------------------------------------------------------------

def test_outputs(dev):
    import torch
    name, (W, H) = "clamped_top", C.FRAMES[1]
    want = C.reference(name, W, H)
    half = render(dev, name, W, H, fmt=N.FORMAT_RGBA16F)
    assert_bitexact(half[0].view(np.uint16), want[0].astype(np.float16).view(np.uint16), "RGBA16F")
    assert_bitexact(half[1], want[1], "RGBA16F counts")
    # device pointers: the frame of the host path; the total is added to the caller's
    s = torch.cuda.current_stream(0)
    dev.set_stream(s.cuda_stream)
    try:
        rgba = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
        cnt = torch.zeros((H, W), dtype=torch.int32, device="cuda:0")
        total = torch.full((1,), 5, dtype=torch.int64, device="cuda:0")
        out = N.Output(rgba.data_ptr(), cnt.data_ptr(), total.data_ptr(), 1, N.FORMAT_RGBA32F)
        fr = make_frame(Camera(**C.CASES[name][5]), W, H)
        p = C.params(name)
        N.check(N.lib().cvr_render_vct(dev.handle, ctypes.byref(fr), ctypes.byref(p), ctypes.byref(out)),
                "cvr_render_vct", dev.handle)
        torch.cuda.synchronize()
        assert_bitexact(rgba.cpu().numpy(), want[0], "device rgba")
        assert_bitexact(cnt.cpu().numpy().view(np.uint32), want[1], "device counts")
        assert int(total.item()) == 5 + want[2]
    finally:
        dev.set_stream(None)


# ---------------------------------------------------------------------------------------
# errors, memory
# ---------------------------------------------------------------------------------------

def test_errors_and_memory(dev):
    L = N.lib()
    name = "multi_level"
    fr = make_frame(Camera(**C.INITIAL), 16, 16)
    keep = host_out(16, 16)             # the arrays `out` points at stay alive
    out = keep[3]

    def go(d=dev, prm=None, frame=fr):
        return L.cvr_render_vct(d.handle, ctypes.byref(frame), ctypes.byref(prm or C.params(name)), ctypes.byref(out))

    assert go() == N.CVR_OK
    for field, bad in (("samples", -1), ("samples", N.VCT_MAX_SAMPLES + 1), ("cone_step", 0.0),
                       ("cone_step", -1.0), ("cone_step_increase_rate", 0.99), ("cone_apex_angle_deg", 0.0),
                       ("cone_apex_angle_deg", 90.0), ("cone_apex_angle_deg", float("nan"))):
        p = C.params(name)
        setattr(p, field, bad)
        assert go(prm=p) == N.CVR_ERR_ARG, (field, bad)
    with option(dev, b"native_exp", 1):
        assert go() == N.CVR_ERR_ARG
    assert go(frame=make_frame(Camera(**C.INITIAL), 32, 32, tile_size=8, rank=0, nranks=2)) == N.CVR_ERR_ARG
    assert L.cvr_vct_set_opacity(dev.handle, N.fptr(np.zeros(254, np.float32)), 254) == N.CVR_ERR_ARG
    bad_lut = np.array(C.opacity_lut())
    bad_lut[3] = np.inf
    assert L.cvr_vct_set_opacity(dev.handle, N.fptr(bad_lut), 255) == N.CVR_ERR_ARG
    assert go() == N.CVR_OK                                                   # the refused calls changed nothing
    d = Device(0)
    try:
        vol, scale, _, tf, _, _ = C.scene("cubic")
        assert go(d=d) == N.CVR_ERR_STATE                                     # no volume or TF
        assert L.cvr_vct_precompute(d.handle) == N.CVR_ERR_STATE
        buf = np.zeros(8, np.float32)
        assert L.cvr_vct_read_pyramid(d.handle, 0, N.fptr(buf)) == N.CVR_ERR_STATE
        assert L.cvr_vct_read_table(d.handle, N.fptr(buf)) == N.CVR_ERR_STATE
        d.set_volume(vol, scale)
        d.set_transfer_function(tf)
        assert go(d=d) == N.CVR_ERR_STATE and b"cvr_vct_set_opacity" in L.cvr_last_error(d.handle)
        d.vct_set_opacity(C.opacity_lut())
        assert go(d=d, prm=C.params("phong_fd")) == N.CVR_ERR_STATE             # Phong without a gradient
        # memory: 4 B per pyramid texel, 640 B of level addressing, 2 B x 255 x height of table,
        # 96 B per cone sample of the schedule
        before = d.device_bytes()
        d.vct_precompute()
        texels = sum(a * b * c for a, b, c in R.level_dims(vol.shape))
        h = math.ceil(C.precomputed("cubic")[0][1])
        assert d.device_bytes() - before == 4 * texels + 640 + 2 * 255 * h
        assert L.cvr_vct_read_pyramid(d.handle, 6, N.fptr(buf)) == N.CVR_ERR_ARG
        assert go(d=d, prm=C.params("samples0")) == N.CVR_OK                  # a schedule of one entry
        before = d.device_bytes()
        assert go(d=d) == N.CVR_OK
        assert d.device_bytes() - before == 96 * (C.MULTI["samples"] - 1)
        d.set_volume(vol.astype(np.uint16) * 257, scale)                      # 2-byte data
        d.set_transfer_function(tf)
        d.vct_set_opacity(C.opacity_lut())
        assert go(d=d) == N.CVR_ERR_ARG and b"1-byte" in L.cvr_last_error(d.handle)
        assert L.cvr_vct_precompute(d.handle) == N.CVR_ERR_ARG
    finally:
        d.close()


# ---------------------------------------------------------------------------------------
# the Python renderer
# ---------------------------------------------------------------------------------------

def test_python_renderer(dev):
    import torch
    r = RC1PVoxelConeTracingSGPU()
    assert r.GetName() == "1-Pass - Ray Casting - Voxel Cone Tracing"
    assert r.GetAbbreviationName() == "s_1rc_vct"
    assert (r.apply_ambient_occlusion, r.apply_voxel_cone_tracing, r.apply_correction_factor) == (True, True, True)
    assert (r.cone_step_size, r.cone_step_size_increase_rate, r.cone_initial_step) == (2.0, 1.0, 2.0)
    assert (r.cone_apex_angle, r.opacity_correction_factor, r.cone_number_of_samples) == (2.0, 2.0, 50)
    assert r.m_u_step_size == 0.5 and r.m_apply_gradient_shading is False
    name, (W, H) = "clamped_top", C.FRAMES[0]
    vol, scale, _, tf, _, step = C.scene("cubic")
    dm = DataManager()
    dm.SetVolume(vol, scale)
    dm.SetTransferFunction(tf)
    rp = RenderingParameters(W, H, light_position=C.LIGHT0["position"], light_forward=C.LIGHT0["forward"],
                             light_up=C.LIGHT0["up"], light_right=C.LIGHT0["right"],
                             spot_light_angle=C.LIGHT0["spot_angle_deg"])
    r.SetExternalResources(dm, rp)
    assert not r.Init(W, H)                                   # no opacities yet
    dm.SetOpacityTable(build_opacity_lut(D.BONSAI_TF_RGB, D.BONSAI_TF_ALPHA))
    assert r.Init(W, H)
    try:
        assert r.m_u_step_size == step
        assert r.device.vct_info().levels == 6                # Init precomputes
        cone = C.CASES[name][1]
        r.cone_step_size, r.cone_step_size_increase_rate = cone["step"], cone["rate"]
        r.cone_initial_step, r.cone_apex_angle = cone["initial"], cone["angle_deg"]
        r.cone_number_of_samples = cone["samples"]
        r.PrepareRender(Camera(**C.INITIAL))
        r.Redraw()
        torch.cuda.synchronize()
        got = (r.rgba.cpu().numpy(), r.samples.cpu().numpy().view(np.uint32), int(r.total.item()))
    finally:
        r.Clean()
    assert_frame(got, render(dev, name, W, H), "Python renderer vs the C-ABI path")
