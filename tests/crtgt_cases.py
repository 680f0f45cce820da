"""Scene and cases shared by tests/test_crtgt.py (CPU) and tests/test_crtgt_gpu.py: the
scene of tests/preillum_cases.py (Marschner-Lobb 48^3, D.voxel_scale(48), the bonsai TF,
LIGHT0, its three cameras) without the extinction pyramid, which the ground truth does
not read.  References are computed once per session and shared read-only."""
import functools

import numpy as np

import preillum_cases as P
from cpp_volume_rendering_amd import datasets as D

N_VOX = P.N_VOX
INITIAL, INSIDE, MOVED, LIGHT0 = P.INITIAL, P.INSIDE, P.MOVED, P.LIGHT0
FRAMES = ((96, 80), (77, 53))          # the second is ragged against the 8x8 tiles

# Secondary rays kept short: the box is 512 units wide and a voxel 10.67, so a light
# step of 6 with these distances gives 21 steps toward the eye and 26 toward the light.
LIGHT_GAP, LIGHT_STEP = 4.0, 6.0
OCC_DISTANCE, SDW_DISTANCE = 130.0, 160.0
N_OCC, OCC_APERTURE = 13, 60.0
N_SDW, SDW_APERTURE = 5, 3.0
N_OCC_WIDE = 70                        # more rays than a wave has lanes
SEED = 7

#         occlusion, shadow, shadow type, Phong, camera, filter_bits, occlusion rays
CASES = {
    "occlusion": (True, False, 0, False, INITIAL, 0, N_OCC),
    "both_point": (True, True, 0, False, INITIAL, 0, N_OCC),
    "both_spot": (True, True, 1, False, INITIAL, 0, N_OCC),
    "both_dir": (True, True, 2, False, INITIAL, 0, N_OCC),
    "shadow_only": (False, True, 0, False, INITIAL, 0, N_OCC),
    "phong_fd": (True, True, 0, True, MOVED, 0, N_OCC),
    "inside": (True, True, 0, False, INSIDE, 0, N_OCC),
    "filter8": (True, True, 0, False, INITIAL, 8, N_OCC),
    "occ70": (True, False, 0, False, INITIAL, 0, N_OCC_WIDE),
    "both_off": (False, False, 0, False, INITIAL, 0, N_OCC),
}


@functools.lru_cache(maxsize=None)
def scene():
    """(vol u8, scale, vol16, tf_rgbt, FD gradient, default step): computed once."""
    import oracle as O
    vol = D.marschner_lobb_u8(N_VOX)
    scale = D.voxel_scale(N_VOX)
    tf = O.tf_rgbt(O.tf_table_double(D.BONSAI_TF_RGB, D.BONSAI_TF_ALPHA))
    return vol, scale, O.volume_r16f(vol), tf, O.gradient(vol, "fd"), O.default_step(scale)


@functools.lru_cache(maxsize=None)
def rays(n_occ=N_OCC):
    """The two tables of a case, as cvr_crtgt_build_rays draws them (float, not yet halves)."""
    from cpp_volume_rendering_amd.renderer import build_crtgt_rays
    occ, sdw = build_crtgt_rays(OCC_APERTURE, n_occ, SDW_APERTURE, N_SDW, SEED)
    occ.setflags(write=False)
    sdw.setflags(write=False)
    return occ, sdw


@functools.lru_cache(maxsize=None)
def reference(name, W, H):
    """The CPU reference's converged frame of a case: (rgba, counts, total), read-only."""
    import crtgt_ref as R
    occ_on, sdw_on, stype, phong, cam, fb, n_occ = CASES[name]
    _, scale, vol16, tf, grad, step = scene()
    occ, sdw = rays(n_occ)
    rgba, cnt, total = R.render(vol16, scale, tf, cam, W, H, step, LIGHT0, occ, sdw,
                                apply_occlusion=occ_on, apply_shadow=sdw_on, shadow_type=stype,
                                light_gap=LIGHT_GAP, light_step=LIGHT_STEP, occ_distance=OCC_DISTANCE,
                                sdw_distance=SDW_DISTANCE, grad=grad if phong else None, phong=phong,
                                filter_bits=fb)
    rgba.setflags(write=False)
    cnt.setflags(write=False)
    return rgba, cnt, total


@functools.lru_cache(maxsize=None)
def plain(cam_key, W, H, fb=0):
    """Plain rc1pass (the oracle) of the same frame: what the shading is compared with."""
    import oracle as O
    cam = {"INITIAL": INITIAL, "INSIDE": INSIDE, "MOVED": MOVED}[cam_key]
    _, scale, vol16, tf, _, step = scene()
    rgba, _, _ = O.render_rc1pass(vol16, scale, tf, cam, W, H, step, filter_bits=fb)
    rgba.setflags(write=False)
    return rgba


def cam_key(cam):
    return "INITIAL" if cam is INITIAL else ("INSIDE" if cam is INSIDE else "MOVED")


def assert_shading_visible(name, W, H):
    """The two conditions every non-degenerate case meets on the reference's own output:
    the frame is not empty, and the shading changes at least 5 % of the composited pixels."""
    rgba = reference(name, W, H)[0]
    cam, fb = CASES[name][4], CASES[name][5]
    base = plain(cam_key(cam), W, H, fb)
    assert rgba[..., 3].max() > 0.5
    comp = base[..., 3] > 0
    diff = np.abs(rgba[..., :3] - base[..., :3]).max(axis=-1) > 1e-3
    assert comp.any() and (diff & comp).sum() >= 0.05 * comp.sum()
