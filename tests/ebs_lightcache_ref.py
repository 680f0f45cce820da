"""CPU reference of the EBS renderer's light cache (tests only; not a conftest).

Builds tests/support/ebs_lightcache_ref.cpp -- which includes the oracle's translation
unit, so the SAT arithmetic is the pinned oracle's own -- with oracle/Makefile's flags
into tests/support/build/ and binds its function:

    ebs_cache(...)    rc1pextbsd/lightcachecomputation.comp: the (dz, dy, dx, 2) uint16 cache

The march over a cache is lightcache_ref.render (obj_ray_marching.comp is one shader for
both renderers).
"""
from __future__ import annotations

import ctypes
import math

import numpy as np

from oracle import oracle as O   # the module itself: its struct mirrors and _params helper
from ref_build import build_and_load


def _bind(L):
    L.lcref_ebs_cache.argtypes = [ctypes.POINTER(O.OracleEbs), ctypes.POINTER(ctypes.c_int),
                                  ctypes.c_void_p, ctypes.c_int]
    L.lcref_ebs_cache.restype = None


def lib():
    return build_and_load("ebs_lightcache_ref", _bind)


def ebs_cache(n_xyz, scale, sat_f32, dims, light, light_forward, apply_occlusion=True, occ_shells=15,
              occ_radius=1.0, apply_shadow=True, shadow_type=0, cone_angle_deg=1.0, interval=2.0,
              initial_step=2.0, ui_weight=1.0, max_distance=None, filter_bits=0,
              threads: int = 0) -> np.ndarray:
    """The light cache of the EBS terms: (dz, dy, dx, 2) uint16 (binary16 Iao, Ids).
    n_xyz = the volume's (w, h, d), dims = (dx, dy, dz); the parameters are
    oracle.render_ebs's.  Neither the volume's values, the TF nor a camera reach the
    cache (only the SAT does)."""
    sat = np.ascontiguousarray(sat_f32, np.float32)
    w, h, d = (int(v) for v in n_xyz)
    assert sat.shape == (d + 2, h + 2, w + 2)
    vol = np.zeros((d, h, w), np.float32)          # its shape alone is read
    tf = np.zeros((2, 4), np.float32)
    cam = dict(eye=(0.0, 0.0, 1.0), center=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0))
    Q = O.OracleEbs()
    Q.base = O._params(vol, scale, tf, None, cam, 1, 1, 1.0, False, 0.5, 0.5, 0.8, 30.0,
                       (1.0, 1.0, 1.0), light)
    Q.base.filter_bits = int(filter_bits)
    Q.sat = sat.ctypes.data
    Q.sat_dims[:] = list(sat.shape[::-1])
    Q.apply_occlusion, Q.occ_shells, Q.occ_radius = int(apply_occlusion), int(occ_shells), float(occ_radius)
    Q.apply_shadow, Q.shadow_type = int(apply_shadow), int(shadow_type)
    # DirSdwConeAngle uniform: (float)(angle * glm::pi<double>() / 180.0) (ebsrenderer.cpp:161)
    Q.cone_angle = float(np.float32(cone_angle_deg * math.pi / 180.0))
    Q.interval, Q.initial_step, Q.ui_weight = float(interval), float(initial_step), float(ui_weight)
    Q.max_distance = O.ebs_max_distance((w, h, d), scale) if max_distance is None else float(max_distance)
    Q.light_forward[:] = [float(v) for v in light_forward]
    dd = (ctypes.c_int * 3)(*[int(v) for v in dims])
    out = np.zeros((dd[2], dd[1], dd[0], 2), np.uint16)
    lib().lcref_ebs_cache(ctypes.byref(Q), dd, out.ctypes.data, int(threads))
    return out
