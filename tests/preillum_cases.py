"""Scene and cases shared by tests/test_preillum.py (CPU) and tests/test_preillum_gpu.py:
test_dos_gpu.py's own setup (Marschner-Lobb 48^3, D.voxel_scale(48), pyramid 64^3, the
bonsai TF), built once per session."""
import ctypes
import functools
import math

import numpy as np

from cpp_volume_rendering_amd import _native as N
from cpp_volume_rendering_amd import datasets as D
from cpp_volume_rendering_amd.renderer import default_cone_params

N_VOX = 48
EXT_RES = (64, 64, 64)
INITIAL = D.INITIAL_STATE_CAMERA
# DOS_CASES["inside"] of test_dos_gpu.py: the eye inside the box
INSIDE = dict(eye=(10.0, -20.0, 30.0), center=(100.0, 50.0, -200.0), up=(0.0, 1.0, 0.0))
MOVED = dict(eye=(-300.0, 120.0, 420.0), center=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0))
# light 0 of the reference's light list (test_dos_gpu.LIGHT0).  The spot angle is 28
# degrees, not the list's 20: this volume shadows itself heavily (most voxels' shadow
# rounds to 0.0 under the point light already), and with 28 the reference cache holds
# 13 % voxels outside the cone and 7 % non-zero shadow voxels at both cache sizes below
# (asserted in test_preillum.py); with 20 only 3 % are non-zero.
LIGHT0 = dict(position=(-206.873, -51.0699, 557.011), forward=(-0.346883, -0.0856335, 0.933991),
              up=(-0.0298143, 0.996327, 0.0802758), right=(0.937434, -0.0, 0.348162),
              spot_angle_deg=28.0)
# ragged in every axis (no multiple of the 4^3 wave block), and the reference's default
CACHE_DIMS = ((20, 12, 9), (32, 32, 32))


def occ7():
    c = default_cone_params(True)
    c.half_angle_deg, c.max_packing, c.covered_distance = 30.0, 2, 300.0
    return c


CACHE_CASES = {
    "occlusion": dict(),
    "both_point": dict(apply_shadow=True, shadow_type=0),
    "both_spot": dict(apply_shadow=True, shadow_type=1),
    "both_dir": dict(apply_shadow=True, shadow_type=2),
    "shadow_only": dict(apply_occlusion=False, apply_shadow=True, shadow_type=0),
    "occ7": dict(occ=occ7),
    "inside": dict(apply_shadow=True, shadow_type=0, cam=INSIDE),
}


def flags(case):
    return dict(apply_occlusion=case.get("apply_occlusion", True),
                apply_shadow=case.get("apply_shadow", False), shadow_type=case.get("shadow_type", 0))


def cone_tables(params, frac):
    """cvr_build_cone_tables with the renderer's default covered distance (diagonal * frac)."""
    scale = D.voxel_scale(N_VOX)
    diag = math.sqrt(sum((N_VOX * s) ** 2 for s in scale))
    p = N.ConeParams.from_buffer_copy(params)
    if p.covered_distance <= 0:
        p.covered_distance = float(np.float32(diag * np.float32(frac)))
    t = N.ConeTables()
    N.check(N.lib().cvr_build_cone_tables(ctypes.byref(p), 1.0, ctypes.byref(t)), "cones")
    return t


@functools.lru_cache(maxsize=None)
def scene():
    """(vol u8, scale, vol16, tf_rgbt, tf_rgba, pyramid levels, FD gradient): computed once."""
    import oracle as O
    vol = D.marschner_lobb_u8(N_VOX)
    scale = D.voxel_scale(N_VOX)
    table = O.tf_table_double(D.BONSAI_TF_RGB, D.BONSAI_TF_ALPHA)
    tf = O.tf_rgbt(table)
    tf_rgba = O.tf_rgbt(table, extinction_input=True)
    vol16 = O.volume_r16f(vol)
    levels = O.ext_volume(vol16, scale, tf_rgba, EXT_RES)
    grad = O.gradient(vol, "fd")
    return vol, scale, vol16, tf, tf_rgba, levels, grad


@functools.lru_cache(maxsize=None)
def ref_cache(name, dims, filter_bits=0):
    """The reference light cache of a CACHE_CASES entry: (dz, dy, dx, 2) uint16, read-only."""
    import lightcache_ref as R
    case = CACHE_CASES[name]
    _, scale, vol16, _, _, levels, _ = scene()
    occ = case["occ"]() if "occ" in case else default_cone_params(True)
    c = R.dos_cache(vol16, scale, levels, case.get("cam", INITIAL), dims, cone_tables(occ, 0.50),
                    cone_tables(default_cone_params(False), 0.75), LIGHT0, filter_bits=filter_bits,
                    **flags(case))
    c.setflags(write=False)
    return c
