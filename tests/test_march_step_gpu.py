"""The march step every deferred march shares (shaded_march.h march_fetch, march_classify,
march_composite), through each kernel that calls it and each template argument it takes,
bit for bit against the oracle and the CPU restatements:

    the per-wave kernel     option shade_flat 0, and as the device-side fallback of the flat
                            pipeline (debug_flat_limit 1 on a frame after the one that sized
                            the stream's job list)
    the count / emit pair   the flat pipeline (the default)
    crtgt_march_kernel      cvr_render_crtgt

each for DOS, EBS and VCT (the three shader types the first two are instantiated with), with
and without Phong and with filter_bits 0 and 8.  One small scene that takes every branch of
the step: a 20 x 16 x 12 volume with unequal voxel sizes, a 36 x 20 viewport (partial tiles,
lanes outside the image), a view from outside in which rays miss the box and one from
inside it (positions clamped), and a TF with an empty range (all-empty rounds, the cell
skip) and an opaque one (the early-ray-termination break).  References are computed once
per session and shared read-only."""
import ctypes
import functools
import math

import numpy as np
import pytest

import aniso_cases as A
import crtgt_cases as G
import ebs_preillum_cases as E
import vct_cases as V
from cpp_volume_rendering_amd import _native as N
from cpp_volume_rendering_amd import datasets as D
from cpp_volume_rendering_amd.renderer import Camera, Device, default_cone_params, make_frame

from test_rc1pass_gpu import assert_bitexact

W, H = 36, 20
SCALE = (24.0, 30.0, 38.0)                  # a box of 480 x 480 x 456
EXT_RES = (16, 16, 8)
# (the step is 15.6: alpha 0.004 composites ~0.06 per sample, alpha 0.2 ends a ray in two)
TF_ALPHA = ((0.0, 0), (0.0, 70), (0.004, 90), (0.004, 150), (0.2, 170), (0.2, 255))
CAMS = {"outside": dict(eye=(-480.0, 190.0, 670.0), center=(10.0, -5.0, 20.0), up=(0.0, 1.0, 0.0)),
        "inside": A.INSIDE}                  # (10, -20, 30): inside the half box (240, 240, 228)
LIGHT0 = A.LIGHT0
CONE = V.MULTI
ROUTES = ("flat", "per_wave", "fallback")


@functools.lru_cache(maxsize=None)
def scene():
    import oracle as O
    from types import SimpleNamespace
    vol = D.marschner_lobb_u8(20)[4:16, :16, :].copy()          # (z, y, x) = (12, 16, 20)
    table = O.tf_table_double(D.BONSAI_TF_RGB, TF_ALPHA)
    diag = math.sqrt(sum((n * s) ** 2 for n, s in zip(vol.shape[::-1], SCALE)))
    return SimpleNamespace(vol=vol, scale=SCALE, vol16=O.volume_r16f(vol), tf=O.tf_rgbt(table),
                           tf_rgba=O.tf_rgbt(table, extinction_input=True), grad=O.gradient(vol, "fd"),
                           step=O.default_step(SCALE), diag=diag)


def _ro(out):
    for a in out[:2]:
        a.setflags(write=False)
    return out[:3]


@functools.lru_cache(maxsize=None)
def plain(cam):
    import oracle as O
    s = scene()
    return _ro(O.render_rc1pass(s.vol16, s.scale, s.tf, CAMS[cam], W, H, s.step))


def dos_tables():
    s = scene()
    return (A.cone_tables(default_cone_params(True), s.diag, 0.50),
            A.cone_tables(default_cone_params(False), s.diag, 0.75))


def ebs_params(phong):
    return E.ebs_params(step=scene().step, phong=phong, light=LIGHT0["position"], light_forward=LIGHT0["forward"])


@functools.lru_cache(maxsize=None)
def reference(renderer, phong, fb, cam):
    import oracle as O
    s = scene()
    grad = s.grad if phong else None
    if renderer == "dos":
        occ, sdw = dos_tables()
        levels = O.ext_volume(s.vol16, s.scale, s.tf_rgba, EXT_RES)
        return _ro(O.render_dos(s.vol16, s.scale, s.tf, levels, CAMS[cam], W, H, s.step, occ, sdw,
                                apply_occlusion=True, apply_shadow=True, shadow_type=0, light=LIGHT0, grad=grad,
                                phong=phong, filter_bits=fb))
    if renderer == "ebs":
        p = ebs_params(phong)
        return _ro(O.render_ebs(s.vol16, s.scale, s.tf, A_sat()[1], CAMS[cam], W, H, s.step,
                                light=tuple(p.light_pos), light_forward=tuple(p.light_forward), grad=grad,
                                phong=phong, filter_bits=fb, **A._ebs_kw(p)))
    if renderer == "vct":
        import vct_ref as R
        pyr = R.pyramid(s.vol)
        tab = R.table(s.vol, V.tf_table(), pyr[1])
        return _ro(R.render(s.vol16, s.scale, s.tf, CAMS[cam], W, H, s.step, LIGHT0, pyr, tab, CONE,
                            apply_occlusion=True, apply_shadow=True, grad=grad, phong=phong, filter_bits=fb))
    import crtgt_ref as C
    occ, sdw = G.rays(G.N_OCC)
    return _ro(C.render(s.vol16, s.scale, s.tf, CAMS[cam], W, H, s.step, LIGHT0, occ, sdw, apply_occlusion=True,
                        apply_shadow=True, shadow_type=0, light_gap=G.LIGHT_GAP, light_step=G.LIGHT_STEP,
                        occ_distance=G.OCC_DISTANCE, sdw_distance=G.SDW_DISTANCE, grad=grad, phong=phong,
                        filter_bits=fb))


@functools.lru_cache(maxsize=None)
def A_sat():
    """(ext lut, float SAT) of the scene's volume, as the EBS renderer builds them."""
    import oracle as O
    from test_ebs import lib_ext_lut
    lut = lib_ext_lut(1)
    t = O.sat_build(scene().vol, lut).astype(np.float32)
    t.setflags(write=False)
    return lut, t


def test_scene_takes_every_branch_of_the_step():
    """On the oracle's plain march of the two views (no GPU)."""
    s = scene()
    assert s.vol.shape == (12, 16, 20) and s.vol.min() < 70 and s.vol.max() > 170
    assert (s.tf[:70, 3] == 0).all() and (s.tf[90:, 3] > 0).all()
    out_rgba, out_cnt, _ = plain("outside")
    in_rgba, in_cnt, _ = plain("inside")
    assert (out_cnt == 0).any() and (out_cnt > 0).mean() > 0.3          # rays that miss, rays that hit
    assert (in_cnt > 0).all()                                           # the eye inside: every ray marches
    for rgba in (out_rgba, in_rgba):
        assert (rgba[..., 3] > 0.99).any()                              # the ERT break fires
    assert ((out_cnt > 0) & (out_rgba[..., 3] <= 0.99)).any()           # and rays that run to D
    # a ray that ended by ERT took fewer samples than the longest one
    assert out_cnt[out_rgba[..., 3] > 0.99].min() < out_cnt.max()


# ---------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------

def option(d, key, value):
    from test_crtgt_gpu import option as opt
    return opt(d, key, value)


def host_out():
    rgba = np.zeros((H, W, 4), np.float32)
    cnt = np.zeros((H, W), np.uint32)
    total = np.zeros(1, np.uint64)
    return rgba, cnt, total, N.Output(rgba.ctypes.data, cnt.ctypes.data, total.ctypes.data, 0)


@pytest.fixture(scope="module")
def devs():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    s = scene()
    ds = {}
    for name in ("dos", "ebs", "vct", "crtgt"):
        d = ds[name] = Device(0)
        d.set_volume(s.vol, s.scale)
        d.set_transfer_function(s.tf)
        d.set_gradient(N.GRADIENT_FINITE_DIFFERENCES)
    ds["dos"].set_extinction_volume(s.tf_rgba, EXT_RES, 1.0)
    ds["ebs"].set_extinction_sat(A_sat()[0])
    ds["vct"].vct_set_opacity(V.opacity_lut())
    yield ds
    for d in ds.values():
        d.close()


def vct_params(phong):
    p = N.VctParams()
    N.lib().cvr_vct_params_default(ctypes.byref(p))
    p.step = scene().step
    p.apply_gradient_shading = int(phong)
    for k in ("position", "forward", "up", "right"):
        getattr(p.light, k)[:] = list(LIGHT0[k])
    p.light.spot_angle_deg = LIGHT0["spot_angle_deg"]
    p.apply_occlusion, p.apply_shadow = 1, 1
    p.cone_step, p.cone_step_increase_rate = CONE["step"], CONE["rate"]
    p.cone_initial_step, p.cone_apex_angle_deg = CONE["initial"], CONE["angle_deg"]
    p.apply_correction, p.correction_factor = int(CONE["correction"]), CONE["factor"]
    p.samples = CONE["samples"]
    return p


def render(d, renderer, phong, cam):
    s = scene()
    if renderer == "dos":
        from test_dos_gpu import gpu_dos
        return gpu_dos(d, CAMS[cam], W, H, s.step, default_cone_params(True), default_cone_params(False),
                       apply_occlusion=True, apply_shadow=True, shadow_type=0, light=LIGHT0, phong=phong)
    if renderer == "ebs":
        from test_ebs_gpu import gpu_ebs
        return gpu_ebs(d, CAMS[cam], W, H, ebs_params(phong))
    frame = make_frame(Camera(**CAMS[cam]), W, H)
    rgba, cnt, total, out = host_out()
    if renderer == "vct":
        p = vct_params(phong)
        N.check(N.lib().cvr_render_vct(d.handle, ctypes.byref(frame), ctypes.byref(p), ctypes.byref(out)),
                "cvr_render_vct", d.handle)
    else:
        p = N.CrtgtParams()
        N.lib().cvr_crtgt_params_default(ctypes.byref(p))
        p.step = s.step
        p.apply_gradient_shading = int(phong)
        for k in ("position", "forward", "up", "right"):
            getattr(p.light, k)[:] = list(LIGHT0[k])
        p.light.spot_angle_deg = LIGHT0["spot_angle_deg"]
        p.light_gap, p.light_step = G.LIGHT_GAP, G.LIGHT_STEP
        p.apply_occlusion, p.occ_distance = 1, G.OCC_DISTANCE
        p.apply_shadow, p.sdw_distance = 1, G.SDW_DISTANCE
        p.shadow_type = 0
        occ, sdw = (np.ascontiguousarray(t, np.float32) for t in G.rays(G.N_OCC))
        N.check(N.lib().cvr_render_crtgt(d.handle, ctypes.byref(frame), ctypes.byref(p), N.fptr(occ), occ.shape[0],
                                         N.fptr(sdw), sdw.shape[0], ctypes.byref(out)), "cvr_render_crtgt", d.handle)
    return rgba, cnt, int(total[0])


def assert_frame(got, want, what):
    assert np.isfinite(want[0]).all()
    assert_bitexact(got[1], want[1], f"{what} counts")
    assert_bitexact(got[0], want[0], f"{what} rgba")
    assert got[2] == want[2] == int(want[1].sum()) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("fb", [0, 8])
@pytest.mark.parametrize("phong", [False, True])
@pytest.mark.parametrize("renderer", ["dos", "ebs", "vct"])
def test_shaded_march_bitexact(devs, renderer, phong, fb, route):
    d = devs[renderer]
    with option(d, b"filter_bits", fb):
        for cam in CAMS:
            want = reference(renderer, phong, fb, cam)
            if route == "per_wave":
                with option(d, b"shade_flat", 0):
                    got = render(d, renderer, phong, cam)
            elif route == "fallback":
                render(d, renderer, phong, cam)          # sizes the stream's job list: limits apply after it
                with option(d, b"debug_flat_limit", 1):  # no frame here has <= 1 job: the list does not fit
                    got = render(d, renderer, phong, cam)
            else:
                got = render(d, renderer, phong, cam)
            assert_frame(got, want, f"{renderer} phong={phong} fb={fb} {cam} ({route})")


@pytest.mark.gpu
@pytest.mark.parametrize("fb", [0, 8])
@pytest.mark.parametrize("phong", [False, True])
def test_crtgt_march_bitexact(devs, phong, fb):
    d = devs["crtgt"]
    with option(d, b"filter_bits", fb):
        for cam in CAMS:
            assert_frame(render(d, "crtgt", phong, cam), reference("crtgt", phong, fb, cam),
                         f"crtgt phong={phong} fb={fb} {cam}")
