"""GPU parity of the slice-based directional occlusion renderer (sbtm.hip) against its CPU
restatement (tests/support/sbtm_ref.cpp), tolerance 0: RGBA bits, per-pixel counts, the total
and both final occlusion planes, at sbtm_slices_per_launch 1 (one launch per slice, the planes
in global memory), 3 and 8 (the blocked kernel: the planes of a screen tile and its halo in
LDS).  Also the outputs, the argument errors, the memory accounting and the Python renderer
class.  Setup and the reasons for each camera: tests/sbtm_cases.py."""
import ctypes

import numpy as np
import pytest

import sbtm_cases as C
from cpp_volume_rendering_amd import _native as N
from cpp_volume_rendering_amd.renderer import (Camera, DataManager, Device, RenderingParameters,
                                               SBTMDirectionalOcclusionShading, make_frame)

from test_rc1pass_gpu import assert_bitexact

pytestmark = pytest.mark.gpu
KS = (1, 3, 8)


def opt(d, key, value=None):
    if value is None:
        return N.lib().cvr_get_option(d.handle, key)
    N.check(N.lib().cvr_set_option(d.handle, key, value), key.decode(), d.handle)


@pytest.fixture(scope="module")
def devs():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    ds = {}
    for which in ("small8", "small16", "aniso"):
        s = C.scene(which)
        ds[which] = Device(0)
        ds[which].set_volume(s.vol, s.scale)
        ds[which].set_transfer_function(s.tf)
    yield ds
    for d in ds.values():
        d.close()


def host_out(W, H, fmt=N.FORMAT_RGBA32F):
    rgba = np.zeros((H, W, 4), np.float16 if fmt == N.FORMAT_RGBA16F else np.float32)
    cnt = np.zeros((H, W), np.uint32)
    total = np.zeros(1, np.uint64)
    return rgba, cnt, total, N.Output(rgba.ctypes.data, cnt.ctypes.data, total.ctypes.data, 0, fmt)


def render(d, name, W, H, K, fmt=N.FORMAT_RGBA32F, cam=None, case=None):
    """One frame of a case at sbtm_slices_per_launch K (host outputs): rgba, counts, total,
    the two occlusion planes, slices drawn, launches."""
    which, case_cam, _, _, fb = case or C.CASES[name]
    opt(d, b"filter_bits", fb)
    opt(d, b"sbtm_slices_per_launch", K)
    frame = make_frame(Camera(**(cam or case_cam)), W, H)
    p = C.params(name, case)
    rgba, cnt, total, out = host_out(W, H, fmt)
    N.check(N.lib().cvr_render_sbtm(d.handle, ctypes.byref(frame), ctypes.byref(p), ctypes.byref(out)),
            "cvr_render_sbtm", d.handle)
    occ = np.zeros((2, H, W), np.float32)
    N.check(N.lib().cvr_sbtm_read_occlusion(d.handle, W, H, N.fptr(occ)), "cvr_sbtm_read_occlusion", d.handle)
    opt(d, b"filter_bits", 0)
    return rgba, cnt, int(total[0]), occ, opt(d, b"sbtm_slices"), opt(d, b"sbtm_launches")


def assert_frame(got, want, what):
    assert_bitexact(got[1], want.counts, f"{what} counts")
    assert_bitexact(got[0], want.rgba, f"{what} rgba")
    assert_bitexact(got[3], want.occ, f"{what} occlusion planes")
    assert got[2] == want.total == int(want.counts.sum())


def case_frames():
    return [(n, W, H) for n in C.CASES for (W, H) in C.frames(n)]


@pytest.mark.parametrize("name,W,H", case_frames())
def test_frame_bitexact_at_every_batch_size(devs, name, W, H):
    d = devs[C.CASES[name][0]]
    want = C.reference(name, W, H)
    for K in KS:
        got = render(d, name, W, H, K)
        assert_frame(got, want, f"{name} {W}x{H} K={K}")
        slices, launches = got[4], got[5]
        assert slices == want.stats["drawn"]
        if K == 1 or name == "fallback":
            assert launches == slices                   # one launch per slice: the plain form
        else:
            assert launches < slices                    # the blocked form ran


def test_a_frame_of_a_thousand_tiles_blocked_equals_plain(devs):
    """33 x 33 tiles, more workgroups than the card holds at once, so late tiles start after
    early ones (and the empty corner tiles at once) have stored their planes: the blocked
    form must still load its halos' values of before the launch.  Against the plain form,
    which the tests above hold to the CPU reference and in which no workgroup reads a plane
    that its launch writes."""
    d = devs["small8"]
    W, H = C.BIG
    plain = render(d, None, W, H, 1, fmt=N.FORMAT_RGBA16F, case=C.BIG_CASE)
    assert plain[5] == plain[4] and plain[2] > 10 ** 7 and plain[3].min() < 0.9
    for K in (3, 8):
        got = render(d, None, W, H, K, fmt=N.FORMAT_RGBA16F, case=C.BIG_CASE)
        assert got[5] * 2 <= got[4] + 1                       # radii <= 6: two slices always fit the halo
        assert_bitexact(got[0].view(np.uint16), plain[0].view(np.uint16), f"K={K} rgba")
        assert_bitexact(got[1], plain[1], f"K={K} counts")
        assert_bitexact(got[3], plain[3], f"K={K} occlusion planes")
        assert got[2] == plain[2]


def test_both_formats_and_device_output(devs):
    import torch
    name, (W, H) = "wide_3x2", C.FRAMES[1]
    d = devs["small8"]
    want = C.reference(name, W, H)
    for K in (1, 8):
        half = render(d, name, W, H, K, fmt=N.FORMAT_RGBA16F)
        assert_bitexact(half[0].view(np.uint16), want.rgba.astype(np.float16).view(np.uint16), "RGBA16F")
        assert np.array_equal(half[0].astype(np.float32), want.rgba)      # the eye buffer is binary16
        assert_bitexact(half[1], want.counts, "RGBA16F counts")
        # device pointers on the caller's stream; the total is added to the caller's
        opt(d, b"sbtm_slices_per_launch", K)
        s = torch.cuda.current_stream(0)
        d.set_stream(s.cuda_stream)
        for fmt, dt in ((N.FORMAT_RGBA32F, torch.float32), (N.FORMAT_RGBA16F, torch.float16)):
            rgba = torch.zeros((H, W, 4), dtype=dt, device="cuda:0")
            cnt = torch.zeros((H, W), dtype=torch.int32, device="cuda:0")
            total = torch.full((1,), 5, dtype=torch.int64, device="cuda:0")
            out = N.Output(rgba.data_ptr(), cnt.data_ptr(), total.data_ptr(), 1, fmt)
            frame, p = make_frame(Camera(**C.CASES[name][1]), W, H), C.params(name)
            N.check(N.lib().cvr_render_sbtm(d.handle, ctypes.byref(frame), ctypes.byref(p), ctypes.byref(out)),
                    "cvr_render_sbtm", d.handle)
            torch.cuda.synchronize()
            assert_bitexact(rgba.float().cpu().numpy(), want.rgba, "device rgba")
            assert_bitexact(cnt.cpu().numpy().view(np.uint32), want.counts, "device counts")
            assert int(total.item()) == 5 + want.total
            # without counts and total
            out = N.Output(rgba.zero_().data_ptr(), None, None, 1, fmt)
            N.check(N.lib().cvr_render_sbtm(d.handle, ctypes.byref(frame), ctypes.byref(p), ctypes.byref(out)),
                    "cvr_render_sbtm", d.handle)
            torch.cuda.synchronize()
            assert_bitexact(rgba.float().cpu().numpy(), want.rgba, "device rgba, no counts")
        d.set_stream(None)


def test_two_frames_back_to_back_leave_no_state(devs):
    d = devs["small8"]
    W, H = C.FRAMES[0]
    for K in (1, 3):
        a = render(d, "wide_3x3", W, H, K)
        b = render(d, "wide_3x2", W, H, K)                # another camera, grid and attenuation
        a2 = render(d, "wide_3x3", W, H, K)
        assert_frame(b, C.reference("wide_3x2", W, H), "second frame")
        for x, y in zip(a[:4], a2[:4]):
            assert np.array_equal(x, y)
        small = render(d, "defaults", *C.FRAMES[1], K)    # another viewport: the planes are reallocated
        assert_frame(small, C.reference("defaults", *C.FRAMES[1]), "smaller viewport")


def test_memory_accounting(devs):
    s = C.scene("small8")
    d = Device(0)
    try:
        d.set_volume(s.vol, s.scale)
        d.set_transfer_function(s.tf)
        before = d.device_bytes()
        W, H = C.FRAMES[0]
        rgba = render(d, "defaults", W, H, 3)[0]
        scratch = rgba.nbytes + W * H * 4                 # the host output's staging (rgba, counts)
        assert d.device_bytes() == before + 16 * W * H + scratch
        d.set_transfer_function(s.tf)                     # drops the planes
        assert d.device_bytes() == before + scratch
        occ = np.zeros((2, H, W), np.float32)
        assert N.lib().cvr_sbtm_read_occlusion(d.handle, W, H, N.fptr(occ)) == N.CVR_ERR_STATE
    finally:
        d.close()


def test_argument_errors(devs):
    L = N.lib()
    d = devs["small8"]
    W, H = C.FRAMES[0]
    rgba, cnt, total, out = host_out(W, H)
    frame = make_frame(Camera(**C.FAR), W, H)

    def call(dev, fr=frame, p=None, o=out):
        p = p or C.params("defaults")
        return L.cvr_render_sbtm(dev.handle, ctypes.byref(fr), ctypes.byref(p), ctypes.byref(o))

    assert call(d) == N.CVR_OK
    tiles = make_frame(Camera(**C.FAR), W, H)
    tiles.tile_size, tiles.rank, tiles.nranks = 16, 0, 2
    assert call(d, fr=tiles) == N.CVR_ERR_ARG and b"whole frames" in L.cvr_last_error(d.handle)
    for field, bad in (("cone_half_angle_deg", 0.0), ("cone_half_angle_deg", 90.0), ("grid_x", 0), ("grid_y", 17),
                       ("attenuation", -0.1), ("attenuation", 1.5), ("max_passes", -1), ("z_near", 0.0),
                       ("z_far", 0.5), ("step", 1e-12), ("step", float("nan"))):
        p = C.params("defaults")
        setattr(p, field, bad)
        assert call(d, p=p) == N.CVR_ERR_ARG, field
    opt(d, b"native_exp", 1)
    assert call(d) == N.CVR_ERR_ARG
    opt(d, b"native_exp", 0)
    assert L.cvr_set_option(d.handle, b"sbtm_slices_per_launch", 0) == N.CVR_ERR_ARG
    assert L.cvr_set_option(d.handle, b"sbtm_slices_per_launch", 17) == N.CVR_ERR_ARG
    assert L.cvr_set_option(d.handle, b"sbtm_slices", 1) == N.CVR_ERR_ARG        # read-only
    bad_out = N.Output(rgba.ctypes.data, None, None, 0, 7)
    assert call(d, o=bad_out) == N.CVR_ERR_ARG
    occ = np.zeros((2, H, W + 1), np.float32)
    assert L.cvr_sbtm_read_occlusion(d.handle, W + 1, H, N.fptr(occ)) == N.CVR_ERR_ARG
    # no TF, then no volume
    s = C.scene("small8")
    e = Device(0)
    try:
        assert call(e) == N.CVR_ERR_STATE
        e.set_volume(s.vol, s.scale)
        assert call(e) == N.CVR_ERR_STATE and b"no volume or TF" in L.cvr_last_error(e.handle)
    finally:
        e.close()
    g = Device(devices=[0, 0])
    try:
        g.set_volume(s.vol, s.scale)
        g.set_transfer_function(s.tf)
        assert call(g) == N.CVR_ERR_ARG and b"group" in L.cvr_last_error(g.handle)
    finally:
        g.close()
    assert call(d) == N.CVR_OK


def test_python_renderer_class(devs):
    import torch
    s = C.scene("small8")
    W, H = C.FRAMES[0]
    want = C.reference("wide_3x3", W, H)
    r = SBTMDirectionalOcclusionShading(0)
    try:
        assert r.GetName() == "Slice-based - Directional Occlusion" and r.GetAbbreviationName() == "s_sbtm_dos"
        dm = DataManager()
        dm.SetVolume(s.vol, s.scale)
        dm.SetTransferFunction(s.tf)
        r.SetExternalResources(dm, RenderingParameters(W, H))
        assert r.Init(W, H)
        r.cone_half_angle, r.grid_size = 80.0, (3, 3)
        r.Update(Camera(**C.FAR))
        r.Redraw()
        torch.cuda.synchronize()
        assert_bitexact(r.rgba.cpu().numpy(), want.rgba, "renderer class rgba")
        assert int(r.total.item()) == want.total and r.number_of_passes == want.stats["drawn"]
    finally:
        r.Clean()
