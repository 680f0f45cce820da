"""GPU parity of the shaded renderers on the non-cubic, anisotropic scene of
tests/aniso_cases.py, bit for bit: RGBA, per-pixel counts and totals of
cvr_render_dosct, cvr_render_extbsd, the two light caches and their cached frames, and
cvr_render_crtgt, against the references the cubic cases use (oracle.render_dos /
render_ebs, lightcache_ref, ebs_lightcache_ref, crtgt_ref).  Volume (44, 40, 33), scale
(9.0, 11.5, 7.25), pyramid (40, 32, 24), caches (20, 12, 9) and (10, 7, 5): no two axes
agree in any size, so an axis taken for another in a pyramid address, a cone tap, a SAT
corner clamp, a cache voxel's position or a secondary ray's bounds moves the pixels.
(That the references themselves keep their axes apart: tests/test_axis_rotation.py.)"""
import ctypes

import numpy as np
import pytest

import aniso_cases as A
import crtgt_cases as G
from cpp_volume_rendering_amd import _native as N
from cpp_volume_rendering_amd.renderer import Camera, Device, default_cone_params, make_frame

from test_crtgt_gpu import host_out
from test_dos_gpu import gpu_dos
from test_dos_gpu import setup as dos_setup
from test_ebs_gpu import gpu_ebs
from test_ebs_preillum_gpu import render as ebs_preillum_render
from test_preillum_gpu import dos_params, option
from test_preillum_gpu import render as dos_preillum_render
from test_rc1pass_gpu import assert_bitexact

pytestmark = pytest.mark.gpu


def device():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return Device(0)


def assert_frame(got, want, what):
    assert_bitexact(got[1], want[1], f"{what} counts")
    assert_bitexact(got[0], want[0], f"{what} rgba")
    assert got[2] == want[2] == int(want[1].sum()) > 0


# ---------------------------------------------------------------------------------------
# cvr_render_dosct
# ---------------------------------------------------------------------------------------

def dos_device(bits=8):
    d = device()
    s = A.scene(bits)
    dos_setup(d, s.vol, s.scale, s.tf, s.tf_rgba, A.EXT_RES, gmode=N.GRADIENT_FINITE_DIFFERENCES)
    return d


@pytest.fixture(scope="module")
def dos_dev():
    d = dos_device()
    yield d
    d.close()


def check_pyramid(d, bits):
    want = A.pyramid(bits)
    got = d.extinction_levels()
    assert len(got) == len(want) == 6
    for L, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape
        assert_bitexact(g, w, f"level {L} ({bits}-bit voxels)")
    assert want[0].shape == A.EXT_RES[::-1] and want[0].max() > 0


def test_dos_pyramid_levels(dos_dev):
    check_pyramid(dos_dev, 8)


def render_dos(d, name, W, H, bits=8):
    occ_on, sdw_on, stype, phong, cam, occ = A.DOS_CASES[name]
    return gpu_dos(d, A.camera(cam), W, H, A.scene(bits).step, A.OCC[occ](), default_cone_params(False),
                   apply_occlusion=occ_on, apply_shadow=sdw_on, shadow_type=stype, light=A.LIGHT0, phong=phong)


DOS_FRAMES = [("occlusion", 96, 80), ("both_point", 96, 80), ("both_spot", 77, 53), ("both_dir", 96, 80),
              ("phong_fd", 96, 80), ("inside", 96, 80), ("inside", 77, 53), ("occ7", 77, 53),
              ("occ1_point", 96, 80), ("occ1_dir", 96, 80), ("occ1_phong", 77, 53), ("shadow_only", 96, 80)]


@pytest.mark.parametrize("name,W,H", DOS_FRAMES)
def test_dos_frame(dos_dev, name, W, H):
    want = A.dos_frame(name, W, H)
    A.assert_visible(want[0], A.DOS_CASES[name][4], W, H)
    assert_frame(render_dos(dos_dev, name, W, H), want, f"DOS {name} {W}x{H}")


@pytest.mark.parametrize("name,W,H", [("both_spot", 77, 53), ("phong_fd", 96, 80)])
def test_dos_frame_per_wave(dos_dev, name, W, H):
    """shade_flat 0 (the per-wave deferred kernel) gives the reference's bits too."""
    with option(dos_dev, b"shade_flat", 0):
        got = render_dos(dos_dev, name, W, H)
    assert_frame(got, A.dos_frame(name, W, H), f"DOS {name} per wave")


def test_dos_frame_filter_bits_8(dos_dev):
    want = A.dos_frame("both_point", 96, 80, fb=8)
    A.assert_visible(want[0], fb=8)
    with option(dos_dev, b"filter_bits", 8):
        got = render_dos(dos_dev, "both_point", 96, 80)
    assert_frame(got, want, "DOS both_point, 8-bit weights")
    assert (want[0].view(np.uint32) != A.dos_frame("both_point")[0].view(np.uint32)).mean() > 0.05


def test_dos_u16():
    d = dos_device(16)
    try:
        check_pyramid(d, 16)
        want = A.dos_frame("both_point", 96, 80, bits=16)
        A.assert_visible(want[0], bits=16)
        assert_frame(render_dos(d, "both_point", 96, 80, bits=16), want, "DOS both_point, 16-bit voxels")
    finally:
        d.close()


# ---------------------------------------------------------------------------------------
# cvr_compute_light_cache_dosct, cvr_render_dosct_preillum
# ---------------------------------------------------------------------------------------

def dos_case_params(name):
    occ_on, sdw_on, stype, phong, _, occ = A.DOS_CASES[name]
    case = dict(apply_occlusion=occ_on, apply_shadow=sdw_on, shadow_type=stype, occ=A.OCC[occ])
    return dos_params(case, A.scene().step, phong=phong)


@pytest.mark.parametrize("name", ["both_point", "both_spot", "both_dir", "inside"])
def test_dos_light_cache(dos_dev, name):
    frame = make_frame(Camera(**A.camera(A.DOS_CASES[name][4])), 64, 48)
    dos_dev.compute_light_cache(frame, dos_case_params(name), A.DOS_DIMS)
    got = dos_dev.light_cache().view(np.uint16)
    want = A.dos_cache(name)
    assert got.shape == want.shape == A.DOS_DIMS[::-1] + (2,)
    assert_bitexact(got, want, f"DOS cache {name}")
    live = want[..., [1] if name == "inside" else [0, 1]]   # inside: the occlusion is all 0.0
    assert ((live != 0) & (live != 0x3C00)).mean() >= 0.05


@pytest.mark.parametrize("name,W,H", [("both_point", 96, 80), ("inside", 77, 53)])
def test_dos_cached_frame(dos_dev, name, W, H):
    cam = A.DOS_CASES[name][4]
    want = A.dos_cached_frame(name, W, H)
    A.assert_visible(want[0], cam, W, H)
    got = dos_preillum_render(dos_dev, "cvr_render_dosct_preillum", A.camera(cam), W, H, dos_case_params(name),
                              A.DOS_DIMS)
    assert_frame(got, want, f"DOS cached frame {name}")


# ---------------------------------------------------------------------------------------
# cvr_render_extbsd
# ---------------------------------------------------------------------------------------

def ebs_device(bits=8):
    d = device()
    s = A.scene(bits)
    d.set_volume(s.vol, s.scale)
    d.set_transfer_function(s.tf)
    d.set_gradient(N.GRADIENT_FINITE_DIFFERENCES)
    d.set_extinction_sat(A.sat(bits)[0])
    return d


@pytest.fixture(scope="module")
def ebs_dev():
    d = ebs_device()
    yield d
    d.close()


def test_ebs_sat(ebs_dev):
    want = A.sat()[1]
    assert want.shape == (46, 42, 35)
    assert_bitexact(ebs_dev.extinction_sat(), want, "SAT")


def render_ebs(d, name, W, H, bits=8):
    cam = A.EBS_CASES[name].get("cam", "outside")
    return gpu_ebs(d, A.camera(cam), W, H, A.ebs_params(name, A.scene(bits).step))


EBS_FRAMES = [("defaults_point", 96, 80), ("occlusion_only", 96, 80), ("shadow_only", 96, 80),
              ("directional", 96, 80), ("shadow_dir_only", 77, 53), ("phong", 96, 80), ("wide_cone", 77, 53),
              ("cone_60", 96, 80), ("inside", 77, 53), ("light_inside", 96, 80)]


@pytest.mark.parametrize("name,W,H", EBS_FRAMES)
def test_ebs_frame(ebs_dev, name, W, H):
    want = A.ebs_frame(name, W, H)
    A.assert_visible(want[0], A.EBS_CASES[name].get("cam", "outside"), W, H)
    assert_frame(render_ebs(ebs_dev, name, W, H), want, f"EBS {name} {W}x{H}")


@pytest.mark.parametrize("name", ["defaults_point", "cone_60"])
def test_ebs_frame_plain_sat_layout(ebs_dev, name):
    with option(ebs_dev, b"sat_layout", 1):
        got = render_ebs(ebs_dev, name, 96, 80)
    assert_frame(got, A.ebs_frame(name), f"EBS {name}, sat_layout 1")
    assert_frame(render_ebs(ebs_dev, name, 96, 80), A.ebs_frame(name), f"EBS {name}, back on sat_layout 0")


def test_ebs_frame_per_wave(ebs_dev):
    with option(ebs_dev, b"shade_flat", 0):
        got = render_ebs(ebs_dev, "phong", 96, 80)
    assert_frame(got, A.ebs_frame("phong"), "EBS phong per wave")


def test_ebs_frame_filter_bits_8(ebs_dev):
    want = A.ebs_frame("directional", 96, 80, fb=8)
    A.assert_visible(want[0], fb=8)
    assert N.lib().cvr_get_option(ebs_dev.handle, b"sat_layout") == 0
    with option(ebs_dev, b"filter_bits", 8):
        got = render_ebs(ebs_dev, "directional", 96, 80)
    assert_frame(got, want, "EBS directional, 8-bit weights")
    assert (want[0].view(np.uint32) != A.ebs_frame("directional")[0].view(np.uint32)).mean() > 0.05


def test_ebs_u16():
    d = ebs_device(16)
    try:
        assert_bitexact(d.extinction_sat(), A.sat(16)[1], "SAT, 16-bit voxels")
        want = A.ebs_frame("defaults_point", 96, 80, bits=16)
        A.assert_visible(want[0], bits=16)
        assert_frame(render_ebs(d, "defaults_point", 96, 80, bits=16), want, "EBS defaults_point, 16-bit voxels")
    finally:
        d.close()


# ---------------------------------------------------------------------------------------
# cvr_compute_light_cache_extbsd, cvr_render_extbsd_preillum
# ---------------------------------------------------------------------------------------

def check_ebs_cache(d, name):
    d.compute_light_cache_extbsd(A.ebs_params(name, A.scene().step), A.EBS_DIMS)
    got = d.light_cache().view(np.uint16)
    want = A.ebs_cache(name)
    assert got.shape == want.shape == A.EBS_DIMS[::-1] + (2,)
    assert_bitexact(got, want, f"EBS cache {name}")
    assert ((want != 0) & (want != 0x3C00)).mean() >= 0.05


@pytest.mark.parametrize("name", ["defaults_point", "directional", "wide_cone", "light_inside"])
def test_ebs_light_cache(ebs_dev, name):
    check_ebs_cache(ebs_dev, name)


def test_ebs_light_cache_plain_sat_layout(ebs_dev):
    with option(ebs_dev, b"sat_layout", 1):
        check_ebs_cache(ebs_dev, "light_inside")
    check_ebs_cache(ebs_dev, "light_inside")         # and back on the cell4 copy (rebuilt)


@pytest.mark.parametrize("name,W,H", [("defaults_point", 96, 80), ("inside", 77, 53)])
def test_ebs_cached_frame(ebs_dev, name, W, H):
    cam = A.EBS_CASES[name].get("cam", "outside")
    want = A.ebs_cached_frame(name, W, H)
    A.assert_visible(want[0], cam, W, H)
    got = ebs_preillum_render(ebs_dev, A.camera(cam), W, H, A.ebs_params(name, A.scene().step), A.EBS_DIMS)
    assert_frame(got, want, f"EBS cached frame {name}")


# ---------------------------------------------------------------------------------------
# cvr_render_crtgt
# ---------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def gt_dev():
    d = device()
    s = A.scene()
    d.set_volume(s.vol, s.scale)
    d.set_transfer_function(s.tf)
    d.set_gradient(N.GRADIENT_FINITE_DIFFERENCES)
    yield d
    d.close()


def crtgt_inputs(name, W, H):
    """(frame, params, occlusion table, shadow table) of an A.CRTGT_CASES entry."""
    occ_on, sdw_on, stype, phong, cam, n_occ = A.CRTGT_CASES[name]
    p = N.CrtgtParams()
    N.lib().cvr_crtgt_params_default(ctypes.byref(p))
    p.step = A.scene().step
    p.apply_gradient_shading = int(phong)
    for k in ("position", "forward", "up", "right"):
        getattr(p.light, k)[:] = list(A.LIGHT0[k])
    p.light.spot_angle_deg = A.LIGHT0["spot_angle_deg"]
    p.light_gap, p.light_step = G.LIGHT_GAP, G.LIGHT_STEP
    p.apply_occlusion, p.occ_distance = int(occ_on), G.OCC_DISTANCE
    p.apply_shadow, p.sdw_distance = int(sdw_on), G.SDW_DISTANCE
    p.shadow_type = stype
    occ, sdw = (np.ascontiguousarray(t, np.float32) for t in G.rays(n_occ))
    return make_frame(Camera(**A.camera(cam)), W, H), p, occ, sdw


CRTGT_FRAMES = [("both_point", 96, 80), ("both_point", 77, 53), ("both_dir", 96, 80), ("phong_fd", 96, 80),
                ("inside", 77, 53), ("occ70", 96, 80), ("shadow_point", 96, 80), ("shadow_dir", 77, 53)]


@pytest.mark.parametrize("name,W,H", CRTGT_FRAMES)
def test_crtgt_frame(gt_dev, name, W, H):
    want = A.crtgt_frame(name, W, H)
    assert np.isfinite(want[0]).all()
    A.assert_visible(want[0], A.CRTGT_CASES[name][4], W, H)
    frame, p, occ, sdw = crtgt_inputs(name, W, H)
    rgba, cnt, total, out = host_out(W, H)
    N.check(N.lib().cvr_render_crtgt(gt_dev.handle, ctypes.byref(frame), ctypes.byref(p), N.fptr(occ),
                                     occ.shape[0], N.fptr(sdw), sdw.shape[0], ctypes.byref(out)),
            "cvr_render_crtgt", gt_dev.handle)
    assert_frame((rgba, cnt, int(total[0])), want, f"crtgt {name} {W}x{H}")


def test_crtgt_advance_one_by_one(gt_dev):
    """advance(1) until converged gives the frame of cvr_render_crtgt."""
    name, (W, H) = "both_point", A.FRAMES[1]
    want = A.crtgt_frame(name, W, H)
    frame, p, occ, sdw = crtgt_inputs(name, W, H)
    gt_dev.crtgt_begin(frame, p, occ, sdw)
    calls = 1
    while gt_dev.crtgt_advance(1, None) > 0:         # no copy until converged
        calls += 1
        assert calls <= int(want[1].max())
    assert calls == int(want[1].max())
    rgba, cnt, total, out = host_out(W, H)
    assert gt_dev.crtgt_advance(1, out) == 0
    assert_frame((rgba, cnt, int(total[0])), want, "crtgt advance(1)")
