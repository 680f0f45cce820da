"""GPU parity of the advanced deferred isosurface renderer (advdeferred.hip) against its CPU
restatement (tests/support/advdeferred_ref.cpp), tolerance 0, NaNs equal by position whatever
their payload: RGBA in both formats, per-pixel counts, the total, the three curvature planes
and the feature-pixel count, for every case and frame of tests/advdeferred_cases.py.  Also the
relight path (lighting passes over one kept G-buffer and one set of curvature planes), the
planes' invalidation by any geometry pass, the argument errors, the memory accounting, the
deferred renderer interleaved on the same context, and the Python renderer class.  Error paths
are refused calls only."""
import ctypes

import numpy as np
import pytest

import advdeferred_cases as C
import deferred_cases as DC
from cpp_volume_rendering_amd import _native as N
from cpp_volume_rendering_amd.renderer import (AdvancedDeferredShading, Camera, DataManager, Device,
                                               RenderingParameters, make_frame)
from test_deferred_gpu import assert_same, host_out

pytestmark = pytest.mark.gpu
L = N.lib
TABLE_BYTES = 256 * 16 + 256 * 256 * 4


def opt(d, key):
    return L().cvr_get_option(d.handle, key)


def counters(d):
    return tuple(opt(d, k) for k in (b"deferred_launches", b"advdeferred_curvature_launches", b"deferred_hits",
                                     b"advdeferred_ridge_pixels"))


@pytest.fixture(scope="module")
def devs():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    ds = {}
    for which in ("small8", "small16", "aniso", "ramp"):
        s = C.scene(which)
        ds[which] = Device(0)
        ds[which].set_volume(s.vol, s.scale)
    yield ds
    for d in ds.values():
        d.close()


def frame_of(name, W, H, cam=None):
    return make_frame(Camera(**(cam or C.CASES[name][1])), W, H)


def render(d, name, W, H, fmt=N.FORMAT_RGBA32F, extra=None):
    """cvr_render_advdeferred of a case into host outputs: rgba, counts, total."""
    frame, p = frame_of(name, W, H), C.params(name, extra)
    rgba, cnt, total, out = host_out(W, H, fmt)
    N.check(L().cvr_render_advdeferred(d.handle, ctypes.byref(frame), ctypes.byref(p), ctypes.byref(out)),
            "cvr_render_advdeferred", d.handle)
    return rgba, cnt, int(total[0])


def planes(d, W, H):
    k1, k2, dr = np.zeros((H, W), np.float32), np.zeros((H, W), np.float32), np.zeros((H, W, 2), np.float32)
    N.check(L().cvr_advdeferred_read_curvature(d.handle, W, H, N.fptr(k1), N.fptr(k2), N.fptr(dr)),
            "cvr_advdeferred_read_curvature", d.handle)
    return k1, k2, dr


def assert_frame(got, want, what):
    assert_same(got[1], want.counts, f"{what} counts")
    assert_same(got[0], want.rgba, f"{what} rgba")
    assert got[2] == want.total == int(want.counts.sum())


def assert_planes(d, W, H, want):
    k1, k2, dr = planes(d, W, H)
    assert_same(k1, want.k1, "k1")
    assert_same(k2, want.k2, "k2")
    assert_same(dr, want.dir, "curvature direction")


@pytest.mark.parametrize("name,W,H", C.all_frames())
def test_frame_planes_and_feature_count_bitexact(devs, name, W, H):
    d = devs[C.CASES[name][0]]
    want = C.reference(name, W, H)
    got = render(d, name, W, H)
    assert_frame(got, want, f"{name} {W}x{H}")
    assert_planes(d, W, H, want)
    assert opt(d, b"advdeferred_ridge_pixels") == want.stats["featured"]
    half = render(d, name, W, H, fmt=N.FORMAT_RGBA16F)
    with np.errstate(over="ignore"):
        assert_same(half[0], want.rgba.astype(np.float16), "RGBA16F")
    assert_same(half[1], want.counts, "RGBA16F counts")
    assert half[2] == want.total


@pytest.mark.parametrize("name,W,H", [("defaults", *C.FRAMES[0]), ("aniso", *C.FRAMES[1])])
def test_relight_runs_the_lighting_pass_alone(devs, name, W, H):
    d = devs[C.CASES[name][0]]
    frame, p = frame_of(name, W, H), C.params(name)
    g = DC.params("defaults", {k: C.merged(name)[k] for k in ("isovalue", "step_small", "step_large", "step_range",
                                                               "num_blocks", "gbuffer_clear")})
    N.check(L().cvr_deferred_geometry(d.handle, ctypes.byref(frame), ctypes.byref(g)), "geometry", d.handle)
    N.check(L().cvr_advdeferred_curvature(d.handle, ctypes.byref(frame), ctypes.byref(p)), "curvature", d.handle)
    launches = counters(d)[:2]
    assert_planes(d, W, H, C.reference(name, W, H))
    for extra in C.RELIGHT:
        want = C.reference(name, W, H, extra)
        q = C.params(name, extra)
        rgba, cnt, total, out = host_out(W, H)
        N.check(L().cvr_advdeferred_shade(d.handle, W, H, ctypes.byref(q), ctypes.byref(out)),
                "cvr_advdeferred_shade", d.handle)
        assert counters(d)[:2] == launches
        assert_frame((rgba, cnt, int(total[0])), want, f"relight {extra}")
        assert opt(d, b"advdeferred_ridge_pixels") == want.stats["featured"]
    a, b, c = (C.reference(name, W, H, e).rgba for e in C.RELIGHT)
    assert (a != b).any() and (b != c).any()                  # the settings reach the shader
    # a full frame with the last setting gives the same, with one more launch of each pass
    assert_frame(render(d, name, W, H, extra=C.RELIGHT[2]), C.reference(name, W, H, C.RELIGHT[2]), "full frame")
    assert counters(d)[:2] == (launches[0] + 1, launches[1] + 1)


def test_a_geometry_pass_invalidates_the_planes(devs):
    d = devs["small8"]
    W, H = C.FRAMES[1]
    render(d, "defaults", W, H)
    keep = host_out(W, H)                                     # the Output points into these arrays
    p, out = C.params("defaults"), keep[3]
    assert L().cvr_advdeferred_shade(d.handle, W, H, ctypes.byref(p), ctypes.byref(out)) == N.CVR_OK
    frame, g = frame_of("defaults", W, H), DC.params("defaults")
    N.check(L().cvr_deferred_geometry(d.handle, ctypes.byref(frame), ctypes.byref(g)), "geometry", d.handle)
    before = counters(d)
    assert L().cvr_advdeferred_shade(d.handle, W, H, ctypes.byref(p), ctypes.byref(out)) == N.CVR_ERR_STATE
    k = np.zeros((H, W, 2), np.float32)
    assert L().cvr_advdeferred_read_curvature(d.handle, W, H, N.fptr(k), N.fptr(k), N.fptr(k)) == N.CVR_ERR_STATE
    assert counters(d) == before
    # the curvature pass over that G-buffer makes them valid again; another size is refused
    small = frame_of("defaults", 24, 16)
    assert L().cvr_advdeferred_curvature(d.handle, ctypes.byref(small), ctypes.byref(p)) == N.CVR_ERR_STATE
    assert L().cvr_advdeferred_curvature(d.handle, ctypes.byref(frame), ctypes.byref(p)) == N.CVR_OK
    assert L().cvr_advdeferred_shade(d.handle, W, H, ctypes.byref(p), ctypes.byref(out)) == N.CVR_OK
    # the deferred renderer's own frame marches too
    DCout = host_out(W, H)
    N.check(L().cvr_render_deferred(d.handle, ctypes.byref(frame), ctypes.byref(g), ctypes.byref(DCout[3])),
            "cvr_render_deferred", d.handle)
    assert L().cvr_advdeferred_shade(d.handle, W, H, ctypes.byref(p), ctypes.byref(out)) == N.CVR_ERR_STATE


def test_argument_errors_launch_nothing(devs):
    d = devs["small8"]
    W, H = C.FRAMES[1]
    rgba, cnt, total, out = host_out(W, H)
    frame = frame_of("defaults", W, H)
    nan = float("nan")

    def call(dev, fr=frame, p=None, o=out):
        p = p or C.params("defaults")
        return L().cvr_render_advdeferred(dev.handle, ctypes.byref(fr) if fr is not None else None,
                                          ctypes.byref(p), ctypes.byref(o) if o is not None else None)

    assert call(d) == N.CVR_OK
    want = rgba.copy()
    before = counters(d)
    tiles = frame_of("defaults", W, H)
    tiles.tile_size, tiles.rank, tiles.nranks = 16, 0, 2
    p0 = C.params("defaults")
    assert call(d, fr=tiles) == N.CVR_ERR_ARG and b"whole frames" in L().cvr_last_error(d.handle)
    assert L().cvr_advdeferred_curvature(d.handle, ctypes.byref(tiles), ctypes.byref(p0)) == N.CVR_ERR_ARG
    assert call(d, fr=None) == N.CVR_ERR_ARG and call(d, o=None) == N.CVR_ERR_ARG
    assert L().cvr_render_advdeferred(d.handle, ctypes.byref(frame), None, ctypes.byref(out)) == N.CVR_ERR_ARG
    assert L().cvr_advdeferred_curvature(d.handle, None, ctypes.byref(p0)) == N.CVR_ERR_ARG
    assert L().cvr_advdeferred_curvature(d.handle, ctypes.byref(frame), None) == N.CVR_ERR_ARG
    assert L().cvr_advdeferred_shade(d.handle, W, H, None, ctypes.byref(out)) == N.CVR_ERR_ARG
    assert L().cvr_advdeferred_shade(d.handle, W, H, ctypes.byref(p0), None) == N.CVR_ERR_ARG
    assert L().cvr_advdeferred_read_curvature(d.handle, W, H, None, None, None) == N.CVR_ERR_ARG
    assert call(d, o=N.Output(None, None, None, 0, N.FORMAT_RGBA32F)) == N.CVR_ERR_ARG
    assert call(d, o=N.Output(rgba.ctypes.data, None, None, 0, 7)) == N.CVR_ERR_ARG
    for field, bad in (("step_small", 0.0), ("step_small", nan), ("step_large", -1.0), ("step_range", nan),
                       ("isovalue", nan), ("ka", -0.1), ("kd", nan), ("ks", -0.1), ("shininess", nan),
                       ("exposure", nan), ("gamma", nan), ("flow_speed", nan), ("flow_scale", nan), ("time", nan),
                       ("accessibility_strength", nan), ("colormap_s", nan), ("colormap_v", nan)):
        p = C.params("defaults")
        setattr(p, field, bad)
        assert call(d, p=p) == N.CVR_ERR_ARG, (field, bad)
    for field, i, bad in (("color", 1, -0.5), ("color", 3, nan), ("light_color", 2, -1.0), ("light_pos", 0, nan),
                          ("gbuffer_clear", 0, nan), ("num_blocks", 0, 1025), ("num_blocks", 2, 0),
                          ("screen_size", 1, nan)):
        p = C.params("defaults")
        getattr(p, field)[i] = bad
        assert call(d, p=p) == N.CVR_ERR_ARG, (field, i, bad)
    # the relight path: a size that is not the G-buffer's, and its own fields
    assert L().cvr_advdeferred_shade(d.handle, W + 1, H, ctypes.byref(p0), ctypes.byref(out)) == N.CVR_ERR_ARG
    k = np.zeros((H + 1, W, 2), np.float32)
    assert L().cvr_advdeferred_read_curvature(d.handle, W, H + 1, N.fptr(k), N.fptr(k), N.fptr(k)) == N.CVR_ERR_ARG
    p = C.params("defaults")
    p.time = nan
    assert L().cvr_advdeferred_shade(d.handle, W, H, ctypes.byref(p), ctypes.byref(out)) == N.CVR_ERR_ARG
    assert L().cvr_advdeferred_curvature(d.handle, ctypes.byref(frame), ctypes.byref(p)) == N.CVR_ERR_ARG
    # nothing of this launched anything or touched the kept planes and the output
    assert counters(d) == before
    assert_same(rgba, want, "the output after the refused calls")
    assert_planes(d, W, H, C.reference("defaults", W, H))
    for key in (b"advdeferred_curvature_launches", b"advdeferred_ridge_pixels"):
        assert L().cvr_set_option(d.handle, key, 1) == N.CVR_ERR_ARG        # read-only
    s = C.scene("small8")
    e = Device(0)
    try:                                                      # no volume set, no frame yet
        assert call(e) == N.CVR_ERR_STATE and b"no volume" in L().cvr_last_error(e.handle)
        assert L().cvr_advdeferred_curvature(e.handle, ctypes.byref(frame), ctypes.byref(p0)) == N.CVR_ERR_STATE
        assert L().cvr_advdeferred_shade(e.handle, W, H, ctypes.byref(p0), ctypes.byref(out)) == N.CVR_ERR_STATE
        assert counters(e) == (0, 0, -1, -1)
    finally:
        e.close()
    g = Device(devices=[0, 0])
    try:
        g.set_volume(s.vol, s.scale)
        assert call(g) == N.CVR_ERR_ARG and b"group" in L().cvr_last_error(g.handle)
        assert L().cvr_advdeferred_curvature(g.handle, ctypes.byref(frame), ctypes.byref(p0)) == N.CVR_ERR_ARG
        assert L().cvr_advdeferred_shade(g.handle, W, H, ctypes.byref(p0), ctypes.byref(out)) == N.CVR_ERR_ARG
    finally:
        g.close()
    assert call(d) == N.CVR_OK
    assert_same(rgba, want, "the frame again")


def test_memory_accounting_and_the_drop_with_the_volume():
    s = C.scene("small8")
    d = Device(0)
    try:
        d.set_volume(s.vol, s.scale)
        before = d.device_bytes()
        W, H = C.FRAMES[0]
        rgba = render(d, "defaults", W, H)[0]
        scratch = rgba.nbytes + W * H * 4                     # the host output's staging (rgba, counts)
        assert d.device_bytes() == before + (32 + 16) * W * H + TABLE_BYTES + scratch
        frame, g = frame_of("defaults", 24, 16), DC.params("defaults")
        N.check(L().cvr_deferred_geometry(d.handle, ctypes.byref(frame), ctypes.byref(g)), "geometry", d.handle)
        assert d.device_bytes() == before + 32 * 24 * 16 + TABLE_BYTES + scratch     # another viewport: planes gone
        p = C.params("defaults")
        N.check(L().cvr_advdeferred_curvature(d.handle, ctypes.byref(frame), ctypes.byref(p)), "curvature", d.handle)
        assert d.device_bytes() == before + (32 + 16) * 24 * 16 + TABLE_BYTES + scratch
        d.set_volume(s.vol, s.scale)                          # drops the G-buffer and the planes
        assert d.device_bytes() == before + TABLE_BYTES + scratch
        o = host_out(24, 16)
        assert L().cvr_advdeferred_shade(d.handle, 24, 16, ctypes.byref(p), ctypes.byref(o[3])) == N.CVR_ERR_STATE
        assert L().cvr_advdeferred_curvature(d.handle, ctypes.byref(frame), ctypes.byref(p)) == N.CVR_ERR_STATE
    finally:
        d.close()


def test_the_deferred_renderer_is_unchanged_between_advanced_frames(devs):
    d = devs["small8"]
    W, H = C.FRAMES[0]
    for name in ("defaults", "long_step", "blocks8"):
        render(d, "flow", W, H)
        frame, p = make_frame(Camera(**DC.CASES[name][1]), W, H), DC.params(name)
        rgba, cnt, total, out = host_out(W, H)
        N.check(L().cvr_render_deferred(d.handle, ctypes.byref(frame), ctypes.byref(p), ctypes.byref(out)),
                "cvr_render_deferred", d.handle)
        want = DC.reference(name, W, H)
        assert_frame((rgba, cnt, int(total[0])), want, f"deferred {name}")
        # the relight path of the deferred renderer over its own G-buffer, after an advanced
        # lighting pass was refused on it
        q, other = C.params("defaults"), host_out(W, H)
        assert L().cvr_advdeferred_shade(d.handle, W, H, ctypes.byref(q), ctypes.byref(other[3])) == N.CVR_ERR_STATE
        N.check(L().cvr_deferred_shade(d.handle, W, H, ctypes.byref(p), ctypes.byref(out)), "cvr_deferred_shade",
                d.handle)
        assert_frame((rgba, cnt, int(total[0])), want, f"deferred relight {name}")
    assert_frame(render(d, "flow", W, H), C.reference("flow", W, H), "advanced after deferred")


def test_python_renderer_class(devs):
    import torch
    s = C.scene("small8")
    W, H = C.FRAMES[0]
    r = AdvancedDeferredShading(0)
    try:
        assert r.GetName() == "Advanced Deferred Rendering" and r.GetAbbreviationName() == "iso"
        space = {}
        r.FillParameterSpace(space)
        assert space == dict(StepSizeSmall=(0.01, 0.25, 0.05), StepSizeLarge=(0.25, 2.0, 0.25),
                             StepSizeRange=(0.05, 0.26, 0.05))
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
        assert int(r.total.item()) == want.total
        assert (r.geometry_launches, r.curvature_launches) == (1, 1)
        assert r.ridge_pixels == want.stats["featured"]
        for got, ref in zip(r.curvature_planes(), (want.k1, want.k2, want.dir)):
            assert_same(got, ref, "renderer class planes")
        # only lighting and feature parameters changed: the lighting pass alone
        e = C.RELIGHT[2]
        rp.light_position = e["light_pos"]
        r.exposure, r.gamma, r.ks = e["exposure"], e["gamma"], e["ks"]
        r.m_current_time, r.m_flow_scale, r.screen_size = e["time"], e["flow_scale"], e["screen_size"]
        r.Update(Camera(**C.CASES["defaults"][1]))
        r.Redraw()
        torch.cuda.synchronize()
        want = C.reference("defaults", W, H, e)
        assert_same(r.rgba.cpu().numpy(), want.rgba, "relit rgba")
        assert int(r.total.item()) == want.total
        assert (r.geometry_launches, r.curvature_launches) == (1, 1)
        # the camera changed: all three passes run again
        r.m_u_step_size_large, r.m_u_step_size_range = 3.0, 0.3
        r.Update(Camera(**DC.MOVED))
        r.Redraw()
        torch.cuda.synchronize()
        want = C.reference("long_step", W, H, e)
        assert_same(r.rgba.cpu().numpy(), want.rgba, "moved camera rgba")
        assert (r.geometry_launches, r.curvature_launches) == (2, 2)
    finally:
        r.Clean()
