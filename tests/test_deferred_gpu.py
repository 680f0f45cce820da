"""GPU parity of the deferred isosurface renderer (deferred.hip) against its CPU restatement
(tests/support/deferred_ref.cpp), tolerance 0, NaNs equal by position whatever their payload:
RGBA, per-pixel counts, the total, both G-buffer planes and the hit count, for every case and
frame of tests/deferred_cases.py.  Also the relight path (shade passes over one kept
G-buffer, no geometry launch), the outputs, the context's state and memory accounting, the
argument errors and the Python renderer class."""
import ctypes

import numpy as np
import pytest

import deferred_cases as C
from cpp_volume_rendering_amd import _native as N
from cpp_volume_rendering_amd.renderer import (Camera, DataManager, DeferredShading, Device,
                                               RenderingParameters, make_frame)

pytestmark = pytest.mark.gpu
L = N.lib


def opt(d, key):
    return L().cvr_get_option(d.handle, key)


def assert_same(a, b, what):
    """Tolerance 0; a NaN equals a NaN at the same place."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape, what
    diff = ~((a == b) | ((a != a) & (b != b)))
    n = int(diff.sum())
    if n:
        idx = np.argwhere(diff)[:5]
        raise AssertionError(f"{what}: {n} mismatches, first at {idx.tolist()}: "
                             f"gpu={a[tuple(idx[0])]} reference={b[tuple(idx[0])]}")


@pytest.fixture(scope="module")
def devs():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    ds = {}
    for which in ("small8", "small16", "aniso"):
        s = C.scene(which)
        ds[which] = Device(0)
        ds[which].set_volume(s.vol, s.scale)
    yield ds
    for d in ds.values():
        d.close()


def host_out(W, H, fmt=N.FORMAT_RGBA32F):
    rgba = np.zeros((H, W, 4), np.float16 if fmt == N.FORMAT_RGBA16F else np.float32)
    cnt = np.zeros((H, W), np.uint32)
    total = np.zeros(1, np.uint64)
    return rgba, cnt, total, N.Output(rgba.ctypes.data, cnt.ctypes.data, total.ctypes.data, 0, fmt)


def frame_of(name, W, H, cam=None):
    return make_frame(Camera(**(cam or C.CASES[name][1])), W, H)


def render(d, name, W, H, fmt=N.FORMAT_RGBA32F, extra=None, cam=None):
    """cvr_render_deferred of a case into host outputs: rgba, counts, total."""
    frame, p = frame_of(name, W, H, cam), C.params(name, extra)
    rgba, cnt, total, out = host_out(W, H, fmt)
    N.check(L().cvr_render_deferred(d.handle, ctypes.byref(frame), ctypes.byref(p), ctypes.byref(out)),
            "cvr_render_deferred", d.handle)
    return rgba, cnt, int(total[0])


def gbuffer(d, W, H):
    gp, gn = np.zeros((H, W, 4), np.float32), np.zeros((H, W, 4), np.float32)
    N.check(L().cvr_deferred_read_gbuffer(d.handle, W, H, N.fptr(gp), N.fptr(gn)), "cvr_deferred_read_gbuffer",
            d.handle)
    return gp, gn


def assert_frame(got, want, what):
    assert_same(got[1], want.counts, f"{what} counts")
    assert_same(got[0], want.rgba, f"{what} rgba")
    assert got[2] == want.total == int(want.counts.sum())


@pytest.mark.parametrize("name,W,H", C.all_frames())
def test_frame_and_g_buffer_bitexact(devs, name, W, H):
    d = devs[C.CASES[name][0]]
    want = C.reference(name, W, H)
    got = render(d, name, W, H)
    assert_frame(got, want, f"{name} {W}x{H}")
    gp, gn = gbuffer(d, W, H)
    assert_same(gp, want.gpos, "gPosition")
    assert_same(gn, want.gnrm, "gNormal")
    assert opt(d, b"deferred_hits") == want.stats["hits"]


def test_both_formats_and_device_output(devs):
    import torch
    name, (W, H) = "long_step", C.FRAMES[0]
    d = devs["small8"]
    want = C.reference(name, W, H)
    half = render(d, name, W, H, fmt=N.FORMAT_RGBA16F)
    with np.errstate(over="ignore"):
        want16 = want.rgba.astype(np.float16)
    assert_same(half[0], want16, "RGBA16F")
    assert_same(half[1], want.counts, "RGBA16F counts")
    assert half[2] == want.total
    s = torch.cuda.current_stream(0)
    d.set_stream(s.cuda_stream)
    try:
        for fmt, dt, ref in ((N.FORMAT_RGBA32F, torch.float32, want.rgba), (N.FORMAT_RGBA16F, torch.float16, want16)):
            rgba = torch.zeros((H, W, 4), dtype=dt, device="cuda:0")
            cnt = torch.zeros((H, W), dtype=torch.int32, device="cuda:0")
            total = torch.full((1,), 5, dtype=torch.int64, device="cuda:0")
            out = N.Output(rgba.data_ptr(), cnt.data_ptr(), total.data_ptr(), 1, fmt)
            frame, p = frame_of(name, W, H), C.params(name)
            N.check(L().cvr_render_deferred(d.handle, ctypes.byref(frame), ctypes.byref(p), ctypes.byref(out)),
                    "cvr_render_deferred", d.handle)
            torch.cuda.synchronize()
            assert_same(rgba.cpu().numpy(), ref, "device rgba")
            assert_same(cnt.cpu().numpy().view(np.uint32), want.counts, "device counts")
            assert int(total.item()) == 5 + want.total      # added to the caller's
            out = N.Output(rgba.zero_().data_ptr(), None, None, 1, fmt)      # without counts and total
            N.check(L().cvr_render_deferred(d.handle, ctypes.byref(frame), ctypes.byref(p), ctypes.byref(out)),
                    "cvr_render_deferred", d.handle)
            torch.cuda.synchronize()
            assert_same(rgba.cpu().numpy(), ref, "device rgba, no counts")
    finally:
        d.set_stream(None)


@pytest.mark.parametrize("name,W,H", [("defaults", *C.FRAMES[0]), ("aniso", *C.FRAMES[1])])
def test_relight_shades_the_kept_g_buffer_without_a_geometry_launch(devs, name, W, H):
    d = devs[C.CASES[name][0]]
    frame, p = frame_of(name, W, H), C.params(name)
    N.check(L().cvr_deferred_geometry(d.handle, ctypes.byref(frame), ctypes.byref(p)), "cvr_deferred_geometry",
            d.handle)
    launches = opt(d, b"deferred_launches")
    for extra in C.RELIGHT:
        want = C.reference(name, W, H, extra)
        q = C.params(name, extra)
        rgba, cnt, total, out = host_out(W, H)
        assert opt(d, b"deferred_launches") == launches
        N.check(L().cvr_deferred_shade(d.handle, W, H, ctypes.byref(q), ctypes.byref(out)), "cvr_deferred_shade",
                d.handle)
        assert opt(d, b"deferred_launches") == launches
        assert_frame((rgba, cnt, int(total[0])), want, f"relight {extra}")
    # the relit frames differ from one another: the settings reach the shader
    a, b = (C.reference(name, W, H, e).rgba for e in C.RELIGHT[:2])
    assert (a != b).any()
    # the camera eye is the kept frame's: a full frame with the last setting gives the same
    assert_frame(render(d, name, W, H, extra=C.RELIGHT[2]), C.reference(name, W, H, C.RELIGHT[2]), "full frame")
    assert opt(d, b"deferred_launches") == launches + 1


def test_two_cameras_back_to_back_leave_no_state(devs):
    d = devs["small8"]
    W, H = C.FRAMES[0]
    a = render(d, "defaults", W, H)
    b = render(d, "long_step", W, H)
    a2 = render(d, "defaults", W, H)
    assert_frame(b, C.reference("long_step", W, H), "second frame")
    for x, y in zip(a[:2], a2[:2]):
        assert_same(x, y, "first frame again")
    assert a[2] == a2[2]
    small = render(d, "defaults", 24, 16, cam=C.MOVED)        # another viewport: the G-buffer is reallocated
    s = C.scene("small8")
    import deferred_ref as R
    assert_frame(small, R.render(s.vol16, s.vol, s.scale, C.MOVED, 24, 16), "smaller viewport")
    gp, gn = np.zeros((16, 24, 4), np.float32), np.zeros((16, 24, 4), np.float32)
    assert L().cvr_deferred_read_gbuffer(d.handle, W, H, N.fptr(gp), N.fptr(gn)) == N.CVR_ERR_ARG
    assert L().cvr_deferred_read_gbuffer(d.handle, 24, 16, N.fptr(gp), N.fptr(gn)) == N.CVR_OK


def test_memory_accounting_and_the_drop_with_the_volume():
    s = C.scene("small8")
    d = Device(0)
    try:
        d.set_volume(s.vol, s.scale)
        before = d.device_bytes()
        W, H = C.FRAMES[0]
        rgba = render(d, "defaults", W, H)[0]
        scratch = rgba.nbytes + W * H * 4                     # the host output's staging (rgba, counts)
        assert d.device_bytes() == before + 32 * W * H + scratch
        frame, p = frame_of("defaults", 24, 16), C.params("defaults")
        N.check(L().cvr_deferred_geometry(d.handle, ctypes.byref(frame), ctypes.byref(p)), "geometry", d.handle)
        assert d.device_bytes() == before + 32 * 24 * 16 + scratch
        d.set_volume(s.vol, s.scale)                          # drops the G-buffer
        assert d.device_bytes() == before + scratch
        o = host_out(24, 16)
        assert L().cvr_deferred_shade(d.handle, 24, 16, ctypes.byref(p), ctypes.byref(o[3])) == N.CVR_ERR_STATE
        gp, gn = np.zeros((16, 24, 4), np.float32), np.zeros((16, 24, 4), np.float32)
        assert L().cvr_deferred_read_gbuffer(d.handle, 24, 16, N.fptr(gp), N.fptr(gn)) == N.CVR_ERR_STATE
        assert opt(d, b"deferred_hits") == -1
    finally:
        d.close()


def test_argument_errors_launch_nothing(devs):
    d = devs["small8"]
    W, H = C.FRAMES[1]
    rgba, cnt, total, out = host_out(W, H)
    frame = frame_of("defaults", W, H)
    nan = float("nan")

    def call(dev, fr=frame, p=None, o=out):
        p = p or C.params("defaults")
        return L().cvr_render_deferred(dev.handle, ctypes.byref(fr) if fr is not None else None,
                                       ctypes.byref(p), ctypes.byref(o) if o is not None else None)

    assert call(d) == N.CVR_OK
    want = rgba.copy()
    launches, hits = opt(d, b"deferred_launches"), opt(d, b"deferred_hits")
    tiles = frame_of("defaults", W, H)
    tiles.tile_size, tiles.rank, tiles.nranks = 16, 0, 2
    assert call(d, fr=tiles) == N.CVR_ERR_ARG and b"whole frames" in L().cvr_last_error(d.handle)
    p0 = C.params("defaults")
    assert L().cvr_deferred_geometry(d.handle, ctypes.byref(tiles), ctypes.byref(p0)) == N.CVR_ERR_ARG
    assert call(d, fr=None) == N.CVR_ERR_ARG and call(d, o=None) == N.CVR_ERR_ARG
    assert L().cvr_render_deferred(d.handle, ctypes.byref(frame), None, ctypes.byref(out)) == N.CVR_ERR_ARG
    assert L().cvr_deferred_geometry(d.handle, None, ctypes.byref(p0)) == N.CVR_ERR_ARG
    assert L().cvr_deferred_shade(d.handle, W, H, None, ctypes.byref(out)) == N.CVR_ERR_ARG
    assert L().cvr_deferred_read_gbuffer(d.handle, W, H, None, None) == N.CVR_ERR_ARG
    assert call(d, o=N.Output(None, None, None, 0, N.FORMAT_RGBA32F)) == N.CVR_ERR_ARG
    assert call(d, o=N.Output(rgba.ctypes.data, None, None, 0, 7)) == N.CVR_ERR_ARG
    for field, bad in (("step_small", 0.0), ("step_small", -0.05), ("step_small", nan), ("step_large", 0.0),
                       ("step_large", nan), ("step_range", 0.0), ("step_range", nan), ("isovalue", nan),
                       ("ka", -0.1), ("kd", -0.1), ("ks", -0.1), ("ka", nan), ("shininess", nan),
                       ("exposure", nan), ("gamma", nan)):
        p = C.params("defaults")
        setattr(p, field, bad)
        assert call(d, p=p) == N.CVR_ERR_ARG, (field, bad)
    for field, i, bad in (("color", 1, -0.5), ("color", 3, nan), ("light_color", 2, -1.0), ("light_pos", 0, nan),
                          ("gbuffer_clear", 0, nan), ("num_blocks", 0, 1025), ("num_blocks", 2, 0)):
        p = C.params("defaults")
        getattr(p, field)[i] = bad
        assert call(d, p=p) == N.CVR_ERR_ARG, (field, i, bad)
    # shade with a size that is not the G-buffer's; the relight path checks its own fields
    assert L().cvr_deferred_shade(d.handle, W + 1, H, ctypes.byref(p0), ctypes.byref(out)) == N.CVR_ERR_ARG
    p = C.params("defaults")
    p.ks = -1.0
    assert L().cvr_deferred_shade(d.handle, W, H, ctypes.byref(p), ctypes.byref(out)) == N.CVR_ERR_ARG
    # nothing of this launched anything or touched the kept G-buffer and the output
    assert opt(d, b"deferred_launches") == launches and opt(d, b"deferred_hits") == hits
    assert_same(rgba, want, "the output after the refused calls")
    assert L().cvr_set_option(d.handle, b"deferred_hits", 1) == N.CVR_ERR_ARG        # read-only
    # no volume set
    s = C.scene("small8")
    e = Device(0)
    try:
        assert call(e) == N.CVR_ERR_STATE and b"no volume" in L().cvr_last_error(e.handle)
        assert L().cvr_deferred_geometry(e.handle, ctypes.byref(frame), ctypes.byref(p0)) == N.CVR_ERR_STATE
        assert opt(e, b"deferred_launches") == 0
    finally:
        e.close()
    g = Device(devices=[0, 0])
    try:
        g.set_volume(s.vol, s.scale)
        assert call(g) == N.CVR_ERR_ARG and b"group" in L().cvr_last_error(g.handle)
        assert L().cvr_deferred_geometry(g.handle, ctypes.byref(frame), ctypes.byref(p0)) == N.CVR_ERR_ARG
        assert L().cvr_deferred_shade(g.handle, W, H, ctypes.byref(p0), ctypes.byref(out)) == N.CVR_ERR_ARG
    finally:
        g.close()
    assert call(d) == N.CVR_OK
    assert_same(rgba, want, "the frame again")


def test_python_renderer_class(devs):
    import torch
    s = C.scene("small8")
    W, H = C.FRAMES[0]
    r = DeferredShading(0)
    try:
        dm = DataManager()
        dm.SetVolume(s.vol, s.scale)
        rp = RenderingParameters(W, H)
        r.SetExternalResources(dm, rp)
        assert r.Init(W, H)
        r.Update(Camera(**C.CASES["defaults"][1]))
        r.Redraw()
        torch.cuda.synchronize()
        want = C.reference("defaults", W, H)
        assert_same(r.rgba.cpu().numpy(), want.rgba, "renderer class rgba")
        assert_same(r.samples.cpu().numpy().view(np.uint32), want.counts, "renderer class counts")
        assert int(r.total.item()) == want.total and r.geometry_launches == 1
        # only the light moved: the second Update marks no geometry outdated
        rp.light_position = C.RELIGHT[2]["light_pos"]
        r.exposure, r.gamma = 0.0, 0.0
        rp.blinnphong_ks = 0.0
        r.Update(Camera(**C.CASES["defaults"][1]))
        r.Redraw()
        torch.cuda.synchronize()
        want = C.reference("defaults", W, H, C.RELIGHT[2])
        assert_same(r.rgba.cpu().numpy(), want.rgba, "relit rgba")
        assert int(r.total.item()) == want.total and r.geometry_launches == 1
        # a march parameter or the camera changed: the geometry pass runs again
        r.m_u_step_size_large, r.m_u_step_size_range = 3.0, 0.3
        r.Update(Camera(**C.MOVED))
        r.Redraw()
        torch.cuda.synchronize()
        want = C.reference("long_step", W, H, C.RELIGHT[2])
        assert_same(r.rgba.cpu().numpy(), want.rgba, "moved camera rgba")
        assert r.geometry_launches == 2
    finally:
        r.Clean()
