"""The ground-truth cone ray-caster, CPU side: the ray tables of cvr_crtgt_build_rays, the
defaults of cvr_crtgt_params_default, and the sanity of the CPU restatement
(tests/support/crtgt_ref.cpp) the GPU kernels are compared with bit for bit in
tests/test_crtgt_gpu.py."""
import ctypes
import math

import numpy as np
import pytest

import crtgt_cases as C
import crtgt_ref as R
from cpp_volume_rendering_amd import _native as N
from cpp_volume_rendering_amd.renderer import build_crtgt_rays


def test_reference_builds():
    assert hasattr(R.lib(), "gtref_render_rows")


def test_build_rays_deterministic_unit_and_inside_the_cone():
    for occ_ap, n_occ, sdw_ap, n_sdw, seed in ((60.0, 13, 3.0, 5, 7), (90.0, 300, 1.0, 200, 1), (20.0, 1, 45.0, 1, 0)):
        occ, sdw = build_crtgt_rays(occ_ap, n_occ, sdw_ap, n_sdw, seed)
        occ2, sdw2 = build_crtgt_rays(occ_ap, n_occ, sdw_ap, n_sdw, seed)
        assert occ.shape == (n_occ, 3) and sdw.shape == (n_sdw, 3)
        assert np.array_equal(occ, occ2) and np.array_equal(sdw, sdw2)
        for tab, ap in ((occ, occ_ap), (sdw, sdw_ap)):
            t = tab.astype(np.float64)
            assert np.abs(np.linalg.norm(t, axis=1) - 1.0).max() <= 1e-6
            # within the aperture of +z: cos(angle to z) >= cos(aperture), float rounding aside
            assert (t[:, 2] >= math.cos(math.radians(ap)) - 1e-6).all()
    a, _ = build_crtgt_rays(60.0, 13, 3.0, 5, 7)
    b, _ = build_crtgt_rays(60.0, 13, 3.0, 5, 8)
    assert not np.array_equal(a, b)                      # the seed matters
    one, _ = build_crtgt_rays(60.0, 13, 3.0, 5, 1)
    zero, _ = build_crtgt_rays(60.0, 13, 3.0, 5, 0)
    assert np.array_equal(one, zero)                     # seed 0 -> 1 (minstd_rand0)
    assert len({tuple(r) for r in a}) == 13              # the rays differ from each other


def test_build_rays_first_draw_is_minstd_rand0():
    """x1 = 16807 * seed, u = (x1 - 1) / 2147483646: theta of ray 0, phi from the second draw."""
    occ, _ = build_crtgt_rays(90.0, 1, 1.0, 0, 3)
    x1 = 16807 * 3
    x2 = (16807 * x1) % 2147483647
    theta = np.float32(np.float32((x1 - 1) / 2147483646.0) * np.float32(np.float32(math.pi) * np.float32(0.5)))
    phi = np.float32(np.float32((x2 - 1) / 2147483646.0) * np.float32(np.float32(math.pi) * np.float32(2.0)))
    want = np.array([math.sin(theta) * math.cos(phi), math.sin(theta) * math.sin(phi), math.cos(theta)])
    assert np.abs(occ[0] - want).max() <= 1e-6


def test_shadow_table_continues_the_occlusion_generator():
    _, sdw = build_crtgt_rays(60.0, 3, 3.0, 2, 7)
    _, five = build_crtgt_rays(60.0, 0, 3.0, 5, 7)
    assert np.array_equal(sdw, five[3:])


def test_build_rays_accepts_zero_rays_for_an_off_term():
    L = N.lib()
    buf = np.zeros((4, 3), np.float32)
    assert L.cvr_crtgt_build_rays(60.0, 0, 3.0, 4, 1, None, N.fptr(buf)) == N.CVR_OK
    assert L.cvr_crtgt_build_rays(60.0, 4, 3.0, 0, 1, N.fptr(buf), None) == N.CVR_OK
    assert L.cvr_crtgt_build_rays(60.0, 0, 3.0, 0, 1, None, None) == N.CVR_OK
    assert L.cvr_crtgt_build_rays(60.0, 4, 3.0, 0, 1, None, None) == N.CVR_ERR_ARG
    assert L.cvr_crtgt_build_rays(60.0, -1, 3.0, 0, 1, None, None) == N.CVR_ERR_ARG
    assert L.cvr_crtgt_build_rays(60.0, N.CRTGT_MAX_RAYS + 1, 3.0, 0, 1, N.fptr(buf), None) == N.CVR_ERR_ARG


def test_params_default():
    p = N.CrtgtParams()
    N.lib().cvr_crtgt_params_default(ctypes.byref(p))
    assert p.step == 0.0                                  # <= 0: cvr_default_step
    assert p.apply_gradient_shading == 0
    assert (p.light_gap, p.light_step) == (1.0, 0.5)
    assert (p.apply_occlusion, p.apply_shadow, p.shadow_type) == (0, 0, 0)
    assert p.occ_distance == 0.0 and p.sdw_distance == 0.0   # <= 0: diagonal * 0.50 / 0.75
    assert [p.ka, p.kd] == [0.5, 0.5] and abs(p.ks - 0.8) < 1e-7 and p.shininess == 30.0
    assert np.allclose(list(p.light.position), C.LIGHT0["position"])
    assert ctypes.sizeof(N.CrtgtParams) == 4 * (6 + 13 + 2 + 5)


def test_null_context_is_refused():
    L = N.lib()
    assert L.cvr_crtgt_begin(None, None, None, None, 0, None, 0) == N.CVR_ERR_ARG
    assert L.cvr_crtgt_advance(None, 1, None, None) == N.CVR_ERR_ARG
    assert L.cvr_render_crtgt(None, None, None, None, 0, None, 0, None) == N.CVR_ERR_ARG


def test_reference_one_axial_ray_differs_from_plain_rc1pass():
    """One occlusion ray along the cone's own axis (+z of the cone), no shadow: the frame
    keeps rc1pass's alpha and counts and darkens its colour."""
    import oracle as O
    _, scale, vol16, tf, _, step = C.scene()
    W, H = C.FRAMES[1]
    rgba, cnt, total = R.render(vol16, scale, tf, C.INITIAL, W, H, step, C.LIGHT0,
                                occ_rays=[[0.0, 0.0, 1.0]], apply_occlusion=True,
                                light_gap=C.LIGHT_GAP, light_step=C.LIGHT_STEP, occ_distance=C.OCC_DISTANCE)
    base, bcnt, btotal = O.render_rc1pass(vol16, scale, tf, C.INITIAL, W, H, step)
    assert np.array_equal(cnt, bcnt) and total == btotal == int(cnt.sum())
    assert np.array_equal(rgba[..., 3], base[..., 3]) and base[..., 3].max() > 0.5
    assert np.isfinite(rgba).all()
    assert (rgba[..., :3] <= base[..., :3]).all()         # a visibility in [0, 1] scales the colour
    comp = base[..., 3] > 0
    assert (np.abs(rgba[..., :3] - base[..., :3]).max(axis=-1) > 1e-3)[comp].mean() >= 0.05


def test_reference_both_terms_off_is_nan():
    """1 / (ka + kd) with both switches off is inf, and 0 * inf NaN, as in DOS."""
    W, H = C.FRAMES[1]
    rgba, cnt, _ = C.reference("both_off", W, H)
    base = C.plain("INITIAL", W, H)
    comp = base[..., 3] > 0
    assert comp.any() and np.isnan(rgba[..., :3][comp]).all()
    assert not rgba[~comp].any()
    assert np.array_equal(rgba[..., 3], base[..., 3])


@pytest.mark.parametrize("name", [n for n in sorted(C.CASES) if n != "both_off"])
def test_reference_cases_are_not_degenerate(name):
    C.assert_shading_visible(name, *C.FRAMES[1])


def test_reference_spot_shadow_is_zero_as_written():
    """`dot(v_dir, LightCamForward) < 30.0` always holds: the spot frame is the occlusion
    term alone under 1 / (ka + kd) = 1 instead of 1 / ka = 2, exactly half the colour."""
    W, H = C.FRAMES[1]
    spot = C.reference("both_spot", W, H)[0]
    occ = C.reference("occlusion", W, H)[0]
    assert np.array_equal(spot[..., :3], 0.5 * occ[..., :3])
    assert np.array_equal(spot[..., 3], occ[..., 3])
    assert not np.array_equal(C.reference("both_point", W, H)[0], spot)
