"""The CPU restatement of the deferred isosurface renderer (tests/support/deferred_ref.cpp),
checked against things it does not itself compute (no GPU).

tests/test_deferred_gpu.py holds the library to this reference bit for bit; here the
reference is held to the pinned oracle's isosurface march (the geometry pass is the loop of
rc1pisodfscustom up to its first hit), to the meaning of its own G-buffer (a hit lies where
the trilinear density crosses the isovalue, its normal has unit length), to the texel-edge
convention's published lists of shifted pixels, and to a symmetry of the scene.  The
conditions the GPU cases rely on (frames with hits, in-box misses and background; rays that
take the skip branch; shifted lighting fetches that change a colour) are asserted on the
reference alone."""
import csv
import ctypes
import os
import subprocess

import numpy as np
import pytest

import deferred_cases as C
import deferred_ref as R
from cpp_volume_rendering_amd import _native as N
from cpp_volume_rendering_amd import evaluation as E
from cpp_volume_rendering_amd.renderer import DeferredShading
from test_literal import gate

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def same(a, b):
    """Tolerance 0, NaNs equal by position whatever their payload."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.array_equal(a, b, equal_nan=True))


@pytest.mark.parametrize("name,W,H", C.all_frames())
def test_cases_meet_the_conditions_the_gpu_tests_rely_on(name, W, H):
    r = C.reference(name, W, H)
    st = r.stats
    assert st["hits"] + st["misses"] + st["off_box"] == W * H
    assert r.total == int(r.counts.sum(dtype=np.uint64))
    assert ((r.counts == 0) == ~inbox(r)).all()
    if name in C.EMPTY:
        assert st["hits"] == 0 and st["misses"] > 0 and st["off_box"] > 0
        return
    assert st["hits"] >= 0.20 * W * H
    assert st["misses"] >= 1
    if name in C.NO_OFF_BOX:
        assert st["off_box"] == 0        # from inside a convex box every ray is in it
    else:
        assert st["off_box"] >= 1
    if name in C.NO_SKIP:
        assert st["skip_rays"] == 0
    # the numbers of shifted pixels the convention gives for these sizes
    cols, rows = C.SHIFTED_COLUMNS[W], C.SHIFTED_COLUMNS[H]
    assert st["shifted"] == len(cols) * H + len(rows) * W - len(cols) * len(rows)


def inbox(r):
    """Pixels whose ray is in the box: hit (w = 1 on both planes) or miss (both planes 0)."""
    hit = r.gpos[..., 3] == 1.0
    miss = ~r.gpos.any(axis=-1) & ~r.gnrm.any(axis=-1)
    return hit | miss


def test_some_case_takes_the_skip_branch():
    assert any(C.reference(n, *C.FRAMES[1]).stats["skip_rays"] > 0 for n in C.CASES if n not in C.EMPTY)
    assert C.reference("blocks1", *C.FRAMES[0]).stats["skip_rays"] == 0


@pytest.mark.parametrize("s,shifted", sorted(C.SHIFTED_COLUMNS.items()))
def test_texel_edge_convention_shifts_the_published_pixels(s, shifted):
    """clamp(int(floor(fl(fl(p / s) * s))), 0, s - 1) in float32, restated in numpy."""
    p = np.arange(s, dtype=F32)
    t = np.clip(np.floor((p / F32(s)) * F32(s)).astype(np.int64), 0, s - 1)
    assert [R.edge_texel(i, s) for i in range(s)] == t.tolist()
    assert tuple(np.nonzero(t != np.arange(s))[0]) == shifted
    assert (t[list(shifted)] == np.array(shifted) - 1).all()


@pytest.mark.parametrize("name", [n for n in C.CASES if n not in C.EMPTY and n not in C.NO_OFF_BOX])
def test_a_shifted_pixel_changes_its_colour(name):
    W, H = C.FRAMES[0]
    r = C.reference(name, W, H)
    diff = (r.rgba != r.unshifted).any(axis=-1)
    assert diff.any()
    ys, xs = np.nonzero(diff)
    assert all(x in C.SHIFTED_COLUMNS[W] or y in C.SHIFTED_COLUMNS[H] for y, x in zip(ys, xs))
    # and without a shift the two are one frame
    q = C.reference(name, *C.FRAMES[1])
    assert same(q.rgba, q.unshifted)


@pytest.mark.parametrize("name,W,H", C.all_frames())
def test_g_buffer_holds_what_the_shader_stores(name, W, H):
    r = C.reference(name, W, H)
    q = C.merged(name)
    hit = r.gpos[..., 3] == 1.0
    assert int(hit.sum()) == r.stats["hits"]
    # off the box both planes keep the clear value
    off = r.counts == 0
    assert int(off.sum()) == r.stats["off_box"]
    assert (r.gpos[off] == F32(q["gbuffer_clear"])).all() and (r.gnrm[off] == F32(q["gbuffer_clear"])).all()
    assert (r.gnrm[..., 3] == r.gpos[..., 3]).all()
    if not hit.any():
        return
    # normals: unit length or NaN (normalize of a zero gradient)
    n = r.gnrm[hit][:, :3].astype(np.float64)
    ln = np.sqrt((n * n).sum(axis=1))
    assert (np.isnan(ln) | (np.abs(ln - 1.0) < 1e-6)).all()


def _crossing_within(name, W, H, reach):
    """Per hit of a case: do the trilinear densities sampled along the ray over
    [-reach, +reach] around the stored position straddle the isovalue?"""
    r = C.reference(name, W, H)
    q = C.merged(name)
    hit = r.gpos[..., 3] == 1.0
    s = C.scene(C.CASES[name][0])
    pos = r.gpos[hit][:, :3].astype(np.float64)
    half = 0.5 * np.array([s.vol.shape[2 - a] * s.scale[a] for a in range(3)])
    d = pos - half - np.array(C.CASES[name][1]["eye"], np.float64)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    n = 2 * int(np.ceil(reach / q["step_small"])) * 16 + 1
    dens = np.stack([R.density(s.vol16, s.scale, pos + o * d) for o in np.linspace(-reach, reach, n)], axis=1)
    iso = float(F32(q["isovalue"]))
    slack = 1e-5                          # float32 rounding of the positions and the fetch
    return (dens.min(axis=1) <= iso + slack) & (dens.max(axis=1) >= iso - slack)


@pytest.mark.parametrize("name,W,H", [f for f in C.all_frames() if f[0] not in C.EMPTY])
def test_hit_positions_lie_on_a_crossing_within_the_step_that_found_it(name, W, H):
    """What the loop guarantees: the hit is refined linearly inside the step [t - h, t] whose
    ends straddle the isovalue, so a crossing of the (continuous) trilinear density lies
    within h of it, and h <= max(step_small, min(step_large, half a block diagonal))."""
    q = C.merged(name)
    s = C.scene(C.CASES[name][0])
    bl = [s.vol.shape[2 - a] * s.scale[a] / q["num_blocks"][a] for a in range(3)]
    h = max(q["step_small"], min(q["step_large"], 0.5 * float(np.sqrt(sum(b * b for b in bl)))))
    assert _crossing_within(name, W, H, h).all()


@pytest.mark.parametrize("name,W,H", [f for f in C.all_frames() if f[0] not in C.EMPTY])
def test_hit_positions_lie_within_one_small_step_of_a_crossing(name, W, H):
    """The margin of the refinement: at most one step_small along the ray, for every hit.
    The loop itself guarantees only the step that found the hit (the test above): it picks
    the step from the density at the step's start, so a step that starts outside
    StepSizeRange of the isovalue is a long one even when it crosses the surface.  The
    cameras of tests/deferred_cases.py were picked on the reference so that no hit of any
    frame does that; this test is the condition they were picked for."""
    ok = _crossing_within(name, W, H, C.merged(name)["step_small"])
    print(name, W, H, "beyond one step_small:", int((~ok).sum()), "of", len(ok))
    assert ok.all()


@pytest.mark.parametrize("name", ["defaults", "u16", "high_iso", "aniso"])
def test_geometry_pass_is_the_oracles_block_march_up_to_the_first_hit(name):
    """oracle_render_iso variant 1 (rc1pisodfscustom) is the same loop; with an opaque colour
    it stops at its first hit.  Its alpha says which pixels hit, and its counts are the
    geometry pass's less the six gradient fetches of a hit."""
    import oracle as O
    which, cam, par = C.CASES[name]
    q = C.merged(name)
    s = C.scene(which)
    W, H = C.FRAMES[1]
    r = C.reference(name, W, H)
    rgba, cnt, total, _ = O.render_iso(s.vol16, s.vol, s.scale, cam, W, H, variant=1, nb=q["num_blocks"],
                                       isovalue=q["isovalue"], step_small=q["step_small"],
                                       step_large=q["step_large"], step_range=q["step_range"],
                                       color=(1.0, 1.0, 1.0, 1.0))
    hit = r.gpos[..., 3] == 1.0
    assert ((rgba[..., 3] > 0) == hit).all()
    assert (cnt + 6 * hit == r.counts).all()
    assert total + 6 * int(hit.sum()) == r.total


@pytest.mark.parametrize("name", list(C.CASES))
def test_tone_map_of_the_lit_frame_is_the_final_frame(name):
    W, H = C.FRAMES[0] if C.CASES[name][0] != "aniso" else C.FRAMES[1]
    r = C.reference(name, W, H)
    q = C.merged(name)
    assert same(R.tone_map(r.lit, q["exposure"], q["gamma"]), r.rgba)
    # and in float64 numpy within float32 rounding of exp and pow
    x = r.lit[..., :3].astype(np.float64)
    if q["exposure"] > 0:
        x = 1.0 - np.exp(-x * q["exposure"])
    if q["gamma"] > 0:
        x = np.power(x, 1.0 / q["gamma"])
    assert np.allclose(x, r.rgba[..., :3], rtol=2e-6, atol=2e-6, equal_nan=True)
    assert (r.rgba[..., 3] == r.lit[..., 3]).all()
    # alpha: objectColor's where lit, 1 where both planes are near zero
    assert set(np.unique(r.rgba[..., 3])) <= {F32(q["color"][3]), F32(1.0)}


def test_off_box_pixels_are_lit_with_the_clear_value():
    """(1, 1, 1, 0) passes the length() < 0.001 test: lit with the unnormalised normal."""
    W, H = C.FRAMES[1]
    r = C.reference("defaults", W, H)
    off = r.counts == 0
    assert off.any()
    assert not (r.lit[off] == 1.0).all(axis=-1).any()
    assert len(np.unique(r.lit[off], axis=0)) == 1        # one texel value, one colour
    # in-box misses are the shader's (1, 1, 1, 1)
    miss = (r.counts > 0) & (r.gpos[..., 3] == 0.0)
    assert miss.any() and (r.lit[miss] == 1.0).all()


def test_mirrored_scene_gives_the_mirrored_frame():
    """The twin of tests/test_sbtm.py: the swap of the world's x and z axes (volume
    transpose(2, 1, 0), scale, camera, light) is a reflection, so the frame comes out
    mirrored left to right (at 48 x 40 no lighting fetch is shifted).  The G-buffer's
    positions come out with x and z swapped.  Pixel centres mirror up to rounding: the
    project's gate."""
    which, cam, par = C.CASES["aniso"]
    W, H = C.FRAMES[1]
    a = C.reference("aniso", W, H)
    m = C.scene("mirror")
    q = dict(par, light_pos=R.LIGHT0[::-1])
    b = R.render(m.vol16, m.vol, m.scale, C.S.mirror_camera(cam), W, H, q)
    g = gate(a.rgba, b.rgba[:, ::-1])
    print(g, (a.counts != b.counts[:, ::-1]).mean())
    assert g["frac_over"] <= 1e-3 and g["max"] <= 2e-2 and g["ssim"] >= 0.99, g
    assert (a.counts != b.counts[:, ::-1]).mean() <= 0.02
    both = (a.gpos[..., 3] == 1.0) & (b.gpos[:, ::-1, 3] == 1.0)
    assert both.mean() > 0.2
    d = np.abs(a.gpos[both][:, :3] - b.gpos[:, ::-1][both][:, 2::-1])
    assert np.median(d) < 1e-2
    # the negative control: the twin with the scale left as it was is another scene
    c = R.render(m.vol16, m.vol, C.scene("aniso").scale, C.S.mirror_camera(cam), W, H, q)
    assert gate(a.rgba, c.rgba[:, ::-1])["frac_over"] > 0.05


def test_params_default_and_struct_size(tmp_path):
    p = N.DeferredParams()
    N.lib().cvr_deferred_params_default(ctypes.byref(p))
    d = R.DEFAULTS
    for k in ("isovalue", "step_small", "step_large", "step_range", "ka", "kd", "ks", "shininess", "exposure",
              "gamma"):
        assert getattr(p, k) == F32(d[k]), k
    for k in ("num_blocks", "color", "light_color", "light_pos", "gbuffer_clear"):
        assert [F32(v) for v in getattr(p, k)] == [F32(v) for v in d[k]], k
    # the reference's constructor (DeferredShading.cpp:123-127), Init (:348) and Redraw (:538-539)
    assert (p.isovalue, p.step_small, p.step_large, p.step_range) == (0.5, F32(0.05), 1.0, F32(0.1))
    assert tuple(p.num_blocks) == (4, 4, 4) and tuple(p.gbuffer_clear) == (1.0, 1.0, 1.0, 0.0)
    assert (p.exposure, p.gamma) == (1.0, F32(2.2))
    # sizeof in C
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include "cvr.h"\nint main(void) { printf("%zu", sizeof(cvr_deferred_params)); '
                   'return 0; }\n')
    exe = tmp_path / "size"
    subprocess.run([os.environ.get("CC", "gcc"), "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    assert int(subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout) == \
        ctypes.sizeof(N.DeferredParams) == 4 * 27


def test_python_class_mirrors_the_reference():
    r = DeferredShading()
    assert r.GetName() == "Deferred Rendering" and r.GetAbbreviationName() == "iso"
    assert (r.m_u_isovalue, r.m_u_step_size_small, r.m_u_step_size_large, r.m_u_step_size_range) == \
        (0.5, F32(0.05), 1.0, F32(0.1))
    assert r.m_u_color == (F32(0.66), F32(0.6), F32(0.05), 1.0) and r.m_apply_gradient_shading is False
    assert r.Init(8, 8) is False                     # no volume: GetCurrentVolumeTexture() == nullptr


def test_parameter_space_covers_every_recorded_row():
    """data/Deferred Shading/Deferred Shading.csv: the class's parameter space enumerates
    the 200 recorded rows, values as std::to_string prints them, in the same order, one
    image file per row."""
    r = DeferredShading()
    before = (r.m_u_step_size_small, r.m_u_step_size_large, r.m_u_step_size_range)
    ps = E.ParameterSpace.from_renderer(r)
    assert [ps.GetDimensionName(i) for i in range(3)] == ["StepSizeSmall", "StepSizeLarge", "StepSizeRange"]
    ps.StartEvaluation()
    rows = []
    while True:
        rows.append([ps.GetDimensionValue(i) for i in range(ps.GetNumDimensions())])
        if not ps.IncrEvaluation():
            break
    ps.EndEvaluation()
    with open(os.path.join(GOLDEN, "deferred_eval_params.csv")) as f:
        ref = list(csv.reader(f))[1:]
    assert len(ref) == 200 and rows == [row[:3] for row in ref]
    assert [row[3] for row in ref] == ["%04d.png" % i for i in range(200)]
    assert (r.m_u_step_size_small, r.m_u_step_size_large, r.m_u_step_size_range) == before
