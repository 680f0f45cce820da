"""Scenes and cases shared by tests/test_sbtm.py (CPU) and tests/test_sbtm_gpu.py; a plain
module, not a conftest.

    small8     marschner_lobb_u8(24)[:, :20, :17]: voxels (z, y, x) = (24, 20, 17), scale
               (1.0, 1.25, 0.75): the box 17 x 25 x 18 (half diagonal 17.6) lies inside the
               slice quad (half side 17.8, the voxel diagonal unscaled)
    small16    the same as 16-bit data (v * 257 + 3)
    aniso      the scene of tests/aniso_cases.py: voxels (44, 40, 33), scale (9.0, 11.5, 7.25);
               its box (297 x 460 x 319) sticks far out of the quad (half side 34): the quad
               clips it
    mirror     aniso with the world's x and z axes swapped (volume transpose(2, 1, 0), scale,
               camera): see test_sbtm.py's twin test

The cameras were picked on the CPU reference so that the conditions asserted in
tests/test_sbtm.py hold: every frame composites at least 20 % of its pixels, occlusion
falls below 0.9 wherever attenuation > 0, the "wide" cases reach a tap radius of 3 px or
more, the "fallback" case one beyond the blocked kernel's 16 px halo, and every case draws a
number of slices that neither 3 nor 8 divides.

References are computed once per session (functools.lru_cache) and shared read-only."""
import ctypes
import functools
from types import SimpleNamespace

import numpy as np

import aniso_cases as A
from cpp_volume_rendering_amd import _native as N
from cpp_volume_rendering_amd import datasets as D

FRAMES = ((48, 40), (37, 29))            # no tile size divides either; one tile of the blocked kernel
TILES = (150, 137)                       # 3 x 3 of its 64 x 64 tiles, ragged in both axes
BIG = (2112, 2080)                       # 33 x 33 tiles (GPU only: blocked against plain)
HALO = 16                                # sbtm.hip's LDS region: most halo pixels per side
SMALL_SCALE = (1.0, 1.25, 0.75)

FAR = dict(eye=(22.0, 14.0, 36.0), center=(0.5, -0.5, 1.0), up=(0.0, 1.0, 0.0))
MOVED = dict(eye=(-30.0, 9.0, 28.0), center=(1.0, 0.0, -1.0), up=(0.0, 1.0, 0.0))
# 3.6 from the box's front face (z = 9): CVector ~ 2 / depth, and with a long step and a wide
# cone every slice's radius is more than half the halo, so no two fit one launch
CLOSE = dict(eye=(1.0, 0.5, 12.6), center=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0))
# 0.7 from the front face: the slices nearer than z_near = 1 are clipped
NEAR = dict(eye=(1.0, 0.5, 9.7), center=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0))
# looking straight down: cross((0, 1, 0), -cam_dir) = 0, a NaN quad
DOWN = dict(eye=(0.0, 40.0, 0.0), center=(0.0, 0.0, 0.0), up=(0.0, 0.0, -1.0))
ANISO_CAM = dict(eye=(-60.0, 25.0, 85.0), center=(2.0, -1.0, 4.0), up=(0.0, 1.0, 0.0))

#        scene, camera, step (0: the default), parameters, filter_bits
CASES = {
    "defaults": ("small8", FAR, 0.0, {}, 0),
    "u16": ("small16", FAR, 0.0, {}, 0),
    "grid1": ("small8", FAR, 0.0, dict(grid=(1, 1)), 0),
    "wide_3x3": ("small8", FAR, 0.0, dict(grid=(3, 3), angle=80.0), 0),
    "wide_3x2": ("small8", MOVED, 0.0, dict(grid=(3, 2), angle=80.0, attenuation=0.5), 0),
    "att0": ("small8", FAR, 0.0, dict(attenuation=0.0), 0),
    "short_last": ("small8", MOVED, 0.73, {}, 0),
    "max5": ("small8", FAR, 3.7, dict(max_passes=5), 0),
    "fallback": ("small8", CLOSE, 1.6, dict(angle=80.0, grid=(3, 3)), 0),
    "near": ("small8", NEAR, 0.0, {}, 0),
    "nan_quad": ("small8", DOWN, 0.0, {}, 0),
    "filter8": ("small8", MOVED, 0.0, dict(grid=(3, 3)), 8),
    "aniso": ("aniso", ANISO_CAM, 5.3, dict(grid=(3, 3), angle=80.0), 0),
    # several tiles: radii of 3 to 5 px, so three slices fit the halo and a tile's halo holds
    # its neighbours' values; the corner tiles see no box and finish at once
    "tiles_small": ("small8", FAR, 0.0, dict(grid=(3, 3), angle=65.0), 0),
    # radii from 3 px (far) to hundreds (near): plain and blocked launches in one frame
    "tiles_aniso": ("aniso", ANISO_CAM, 5.3, dict(grid=(3, 3), angle=60.0), 0),
}
# BIG's parameters: radii of 3 to 6 px at that width
BIG_CASE = ("small8", FAR, 0.0, dict(grid=(3, 3), angle=10.0), 0)
WIDE = ("wide_3x3", "wide_3x2", "aniso", "tiles_small", "tiles_aniso")
# cases whose frame is (partly) empty by construction
EMPTY = ("nan_quad",)


def frames(name):
    if name.startswith("tiles_"):
        return (TILES,)
    return FRAMES if CASES[name][0] != "aniso" else (FRAMES[0],)


@functools.lru_cache(maxsize=None)
def scene(which):
    """vol, scale, vol16, tf, step (the default step) of a scene."""
    import oracle as O
    table = O.tf_table_double(D.BONSAI_TF_RGB, D.BONSAI_TF_ALPHA)
    if which in ("small8", "small16"):
        vol = D.marschner_lobb_u8(24)[:, :20, :17].copy()
        if which == "small16":
            vol = vol.astype(np.uint16) * 257 + 3
        scale = SMALL_SCALE
    elif which == "aniso":
        vol, scale = A.volume(8), A.SCALE
    else:
        assert which == "mirror"
        vol = np.ascontiguousarray(A.volume(8).transpose(2, 1, 0))
        scale = A.SCALE[::-1]
    return SimpleNamespace(vol=vol, scale=scale, vol16=O.volume_r16f(vol), tf=O.tf_rgbt(table),
                           step=O.default_step(scale))


def mirror_camera(cam):
    """A camera under the swap of the world's x and z axes."""
    return dict(cam, eye=cam["eye"][::-1], center=cam["center"][::-1], up=cam["up"][::-1])


def case_step(name):
    which, _, step, _, _ = CASES[name]
    return step if step > 0 else scene(which).step


@functools.lru_cache(maxsize=None)
def reference(name, W, H, history=False):
    """The CPU reference's frame of a case (sbtm_ref.render's namespace), read-only."""
    import sbtm_ref as R
    which, cam, _, par, fb = CASES[name]
    s = scene(which)
    return R.render(s.vol16, s.scale, s.tf, cam, W, H, case_step(name), par, fb, history=history)


def params(name, case=None):
    """cvr_sbtm_params of a case."""
    import sbtm_ref as R
    _, _, step, par, _ = case or CASES[name]
    q = dict(R.DEFAULTS, **par)
    p = N.SbtmParams()
    N.lib().cvr_sbtm_params_default(ctypes.byref(p))
    p.step = step
    p.cone_half_angle_deg = q["angle"]
    p.grid_x, p.grid_y = q["grid"]
    p.attenuation = q["attenuation"]
    p.max_passes = q["max_passes"]
    p.z_near, p.z_far = q["z_near"], q["z_far"]
    return p
