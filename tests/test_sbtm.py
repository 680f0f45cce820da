"""The CPU restatement of the slice-based directional occlusion renderer
(tests/support/sbtm_ref.cpp), checked against things it does not itself compute (no GPU).

tests/test_sbtm_gpu.py holds the library to this reference bit for bit; here the reference
is held to numpy restatements of the slice loop and of the two recurrences that remain when
a term is switched off, to the meaning of its own buffers (a discarded pixel keeps the
plane's value of two slices earlier), and to a symmetry of the scene.  The conditions the
GPU cases rely on (frames that composite, occlusion that bites, radii that reach past one
pixel and past the blocked kernel's halo) are asserted on the reference alone.
"""
import numpy as np
import pytest

import sbtm_cases as C
import sbtm_ref as R
from test_literal import gate

F32 = np.float32


def half(a):
    return np.asarray(a, F32).astype(np.float16).astype(F32)


def all_frames():
    return [(n, W, H) for n in C.CASES for (W, H) in C.frames(n)]


@pytest.mark.parametrize("name,W,H", all_frames())
def test_cases_meet_the_conditions_the_gpu_tests_rely_on(name, W, H):
    r = C.reference(name, W, H)
    par = dict(R.DEFAULTS, **C.CASES[name][3])
    drawn = r.slices["drawn"]
    n = int(drawn.sum())
    assert n == r.stats["drawn"] and n % 3 != 0 and n % 8 != 0 and n >= 5
    assert r.total == int(r.counts.sum())
    if name in C.EMPTY:
        assert r.total == 0 and not r.rgba.any() and (r.occ == 1.0).all()
        return
    assert (r.rgba[..., 3] > 0).mean() >= 0.20
    if par["attenuation"] > 0:
        assert r.occ.min() < 0.9
    rx, ry = r.slices["rx"][drawn], r.slices["ry"][drawn]
    if name in C.WIDE:
        assert max(rx.max(), ry.max()) >= 3
    if name == "fallback":
        # beyond the halo, and no two consecutive slices fit it together
        assert max(rx.max(), ry.max()) > C.HALO
        assert (np.maximum(rx, ry)[:-1] + np.maximum(rx, ry)[1:] > C.HALO).all()
    else:
        # two consecutive slices fit somewhere: the blocked kernel runs
        assert ((rx[:-1] + rx[1:] <= C.HALO) & (ry[:-1] + ry[1:] <= C.HALO)).any()


@pytest.mark.parametrize("name,W,H", all_frames())
def test_no_fetch_leaves_the_radius_bound(name, W, H):
    """The library's blocked kernel relies on the bound (DESIGN 5d'''); the reference
    measures what its fetches really read."""
    r = C.reference(name, W, H)
    assert (r.reach[:, 0] <= r.slices["rx"]).all() and (r.reach[:, 1] <= r.slices["ry"]).all()
    assert (r.slices["rx"] >= 1).all() and (r.slices["ry"] >= 1).all()


@pytest.mark.parametrize("name", ["defaults", "short_last", "near", "aniso"])
def test_slice_list_is_the_while_loop(name):
    """ComputeMinMaxZ* and ComputeProxyGeometry's loop in a few lines of numpy float32."""
    import oracle as O
    which, cam, _, par, _ = C.CASES[name]
    s = C.scene(which)
    step = F32(C.case_step(name))
    V, _ = O.lookat(cam["eye"], cam["center"], cam["up"])
    V = np.asarray(V, F32)
    d, h, w = s.vol.shape
    hx, hy, hz = (F32(n) * F32(sc) * F32(0.5) for n, sc in zip((w, h, d), s.scale))
    zs = [-((V[2] * x + V[6] * y) + (V[10] * z + V[14] * F32(1))) for x in (hx, -hx) for y in (hy, -hy)
          for z in (hz, -hz)]
    zmin, zmax = F32(min(zs)), F32(max(zs))
    pos, t, d0 = [], zmin, None
    while t < zmax:
        dd = min(step, F32(zmax - t))
        d0 = dd if d0 is None else d0
        pos.append(F32(F32(t + F32(dd * F32(0.5))) - zmin))
        t = F32(t + dd)
    pos = np.array(pos, F32)
    depth = (F32(zmin + F32(d0 * F32(0.5))) + pos).astype(F32)
    sl = R.slices(s.vol16, s.scale, s.tf, cam, 48, 40, float(step), par)
    assert np.array_equal(sl["pos"], pos) and np.array_equal(sl["depth"], depth)
    q = dict(R.DEFAULTS, **par)
    assert np.array_equal(sl["drawn"], (depth >= q["z_near"]) & (depth <= q["z_far"]))
    if name == "short_last":
        assert F32(zmax - zmin) % step > 0.05      # the last slice is short
    if name in ("near", "aniso"):
        assert 0 < sl["drawn"].sum() < len(pos)    # the near clip removes slices


def replay(r, step, att):
    """The planes a frame's history implies: a pass writes the pixels it kept, the others keep
    what the plane held.  Yields (pass, kept mask, the plane read) before each write."""
    planes = np.ones_like(r.occ)
    for i in np.flatnonzero(r.slices["drawn"]):
        kept = ~np.isnan(r.occ_hist[i])
        yield i, kept, planes[(i & 1) ^ 1].copy()
        planes[i & 1][kept] = r.occ_hist[i][kept]
    r.replayed = planes


def test_without_attenuation_the_frame_is_plain_compositing():
    """attenuation 0: exp(0) = 1 and a mean of ones is one, so every stored occlusion value is
    exactly 1 and the eye buffer is half-rounded front-to-back compositing of the samples."""
    r = C.reference("att0", 48, 40, history=True)
    step = F32(C.case_step("att0"))
    assert (r.occ == 1.0).all() and (r.occ_hist[~np.isnan(r.occ_hist)] == 1.0).all()
    dst = np.zeros_like(r.rgba)
    for i, kept, _ in replay(r, step, 0.0):
        src = r.src[i][kept]
        al = F32(1) - R.expf(-(src[:, 3] * step))
        d = dst[kept]
        om = F32(1) - d[:, 3]
        out = np.stack([R.fmaf(om, (src[:, k] * F32(1)) * al, d[:, k]) for k in range(3)] +
                       [R.fmaf(om, al, d[:, 3])], axis=-1)
        dst[kept] = half(out)
    assert np.array_equal(dst, r.rgba)
    assert np.array_equal(r.counts, (~np.isnan(r.occ_hist)).sum(axis=0))
    assert (r.rgba[..., 3] > 0.5).any()


def own_centre_fetch(prev, W, H):
    """texture(plane, p_t) of a 1 x 1 grid in numpy: p = 0, so p_d = xy_d exactly and p_t =
    fma(0.5, xy_d, 0.5); then the GL_LINEAR fetch of DESIGN 5d‴ with libm's fmaf."""
    def axis(n):
        u = (np.arange(n, dtype=F32) + F32(0.5)) / F32(n)
        pt = R.fmaf(F32(0.5), R.fmaf(u, F32(2), F32(-1)), F32(0.5))
        t = np.clip(R.fmaf(pt, F32(n), F32(-0.5)), F32(0), F32(n - 1))
        i0 = np.floor(t).astype(np.int64)
        return i0, np.minimum(i0 + 1, n - 1), (t - i0.astype(F32)).astype(F32)
    x0, x1, ax = axis(W)
    y0, y1, ay = axis(H)
    ax = np.broadcast_to(ax, (H, W))
    ay = np.broadcast_to(ay[:, None], (H, W))

    def lerp(a, b, w):
        return R.fmaf(w, (b - a).astype(F32), a)
    r0 = lerp(prev[y0][:, x0], prev[y0][:, x1], ax)
    r1 = lerp(prev[y1][:, x0], prev[y1][:, x1], ax)
    return lerp(r0, r1, ay)


def test_one_tap_follows_the_pixels_own_column():
    """A 1 x 1 grid: the only tap is the pixel's own centre, and each pixel's occlusion
    follows occ <- half(fetch(occ) exp(-st step att)), restated in numpy, exactly."""
    W, H = 48, 40
    r = C.reference("grid1", W, H, history=True)
    step = F32(C.case_step("grid1"))
    seen = 0
    for i, kept, prev in replay(r, step, 1.0):
        if not kept.any():
            continue
        tau = r.src[i][kept][:, 3]
        got = own_centre_fetch(prev, W, H)[kept]
        want = half((got / F32(1.0)) * R.expf(-(tau * step) * F32(1.0)))
        assert np.array_equal(want, r.occ_hist[i][kept])
        # and the fetch is the pixel's own value but for the rounding of p_t (4 W 2^-24 px)
        assert np.abs(got - prev[kept]).max() <= 2.0 ** -15
        seen += int(kept.sum())
    assert seen == r.total > 1000
    assert np.array_equal(r.replayed, r.occ)


@pytest.mark.parametrize("name", ["defaults", "wide_3x3"])
def test_a_pixel_that_left_the_box_keeps_its_last_two_values(name):
    """The planes at the end are, per pixel, the last value each was written with -- a pixel
    behind the silhouette is not cleared -- and neighbours' taps did read such values."""
    r = C.reference(name, 48, 40, history=True)
    for _ in replay(r, 0, 0):
        pass
    assert np.array_equal(r.replayed, r.occ)
    kept = ~np.isnan(r.occ_hist)
    last = np.where(kept.any(axis=0), kept.shape[0] - 1 - kept[::-1].argmax(axis=0), -1)
    drawn_last = int(np.flatnonzero(r.slices["drawn"])[-1])
    left = (last >= 0) & (last < drawn_last - 1)          # written once, then discarded for good
    assert left.sum() > 50 and (r.occ[:, left] < 1.0).any()
    assert r.stats["stale_reads"] > 100


def test_max_passes_cuts_the_frame():
    full = C.reference("max5", 48, 40, history=True)      # max_passes 5 at a long step
    which, cam, step, par, fb = C.CASES["max5"]
    s = C.scene(which)
    whole = R.render(s.vol16, s.scale, s.tf, cam, 48, 40, step, dict(par, max_passes=90000), fb, history=True)
    assert full.stats["passes"] == 5 < whole.stats["passes"]
    assert np.array_equal(full.occ_hist, whole.occ_hist[:5], equal_nan=True)
    assert np.array_equal(full.counts, (~np.isnan(whole.occ_hist[:5])).sum(axis=0))
    assert whole.total > full.total > 0
    none = R.render(s.vol16, s.scale, s.tf, cam, 48, 40, step, dict(par, max_passes=0), fb)
    assert none.total == 0 and not none.rgba.any()


def test_the_near_clip_removes_slices():
    r = C.reference("near", 48, 40, history=True)
    clipped = ~r.slices["drawn"]
    assert clipped.any() and (r.slices["depth"][clipped] < 1.0).all()
    assert np.isnan(r.occ_hist[clipped]).all()
    which, cam, step, par, fb = C.CASES["near"]
    s = C.scene(which)
    open_ = R.render(s.vol16, s.scale, s.tf, cam, 48, 40, C.case_step("near"), dict(par, z_near=1e-3), fb)
    assert open_.stats["drawn"] > r.stats["drawn"] and open_.total > r.total
    assert (open_.counts >= r.counts).all() and (open_.counts > r.counts).any()


def test_a_scaled_volume_sticks_out_of_the_quad():
    """The quad's half side is the voxel diagonal, unscaled: at scale ~10 the quad test, not
    the box test, ends most fragments; at scale ~1 it ends none."""
    assert C.reference("aniso", 48, 40).stats["quad_only"] > 1000
    assert C.reference("defaults", 48, 40).stats["quad_only"] == 0


def test_mirrored_scene_gives_the_mirrored_frame():
    """The twin of tests/test_axis_rotation.py, adapted: that file's cyclic relabelling moves
    the world's y axis, which this renderer's quad hangs on (cam_right = cross((0, 1, 0),
    -cam_dir)), so its twin is another picture by construction.  The swap of x and z keeps y:
    volume transpose(2, 1, 0), scale and camera swapped.  It is a reflection, so the frame
    comes out mirrored left to right; cam_right and cam_up change sign at most, which the
    quad's |dot| tests do not see.  Pixel centres mirror up to rounding: the project's gate."""
    which, cam, _, par, fb = C.CASES["aniso"]
    step = C.case_step("aniso")
    a = C.reference("aniso", 48, 40)
    m = C.scene("mirror")
    b = R.render(m.vol16, m.scale, m.tf, C.mirror_camera(cam), 48, 40, step, par, fb)
    g = gate(a.rgba, b.rgba[:, ::-1])
    print(g, (a.counts != b.counts[:, ::-1]).mean())
    assert g["frac_over"] <= 1e-3 and g["max"] <= 2e-2 and g["ssim"] >= 0.99, g
    assert (a.counts != b.counts[:, ::-1]).mean() <= 0.02
    # the negative control: the twin with the scale left as it was is another scene
    c = R.render(m.vol16, C.scene("aniso").scale, m.tf, C.mirror_camera(cam), 48, 40, step, par, fb)
    assert gate(a.rgba, c.rgba[:, ::-1])["frac_over"] > 0.05
