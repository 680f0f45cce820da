"""CPU reference of the DOS renderer's pre-illumination (tests only; not a conftest).

Builds tests/support/lightcache_ref.cpp -- which includes the oracle's translation
unit, so the cone arithmetic is the pinned oracle's own -- with oracle/Makefile's
flags into tests/support/build/ and binds its two functions:

    dos_cache(...)    lightcachecomputation.comp: the (dz, dy, dx, 2) uint16 light cache
    render(...)       obj_ray_marching.comp over a cache: (rgba, counts, total)
"""
from __future__ import annotations

import ctypes

import numpy as np

from oracle import oracle as O   # the module itself: its struct mirrors and _params / _cone helpers
from ref_build import build_and_load


def _bind(L):
    P, I = ctypes.c_void_p, ctypes.c_int
    IP = ctypes.POINTER(ctypes.c_int)
    L.lcref_dos_cache.argtypes = [ctypes.POINTER(O.OracleDos), IP, P, I]
    L.lcref_dos_cache.restype = None
    L.lcref_render_rows.argtypes = [ctypes.POINTER(O.OracleDos), P, IP, I, I, P, P, I]
    L.lcref_render_rows.restype = ctypes.c_uint64


def lib():
    return build_and_load("lightcache_ref", _bind)


def _dos(vol16, scale, tf_rgbt, ext_levels, camera, W, H, step, occ_tables, sdw_tables,
         apply_occlusion, apply_shadow, shadow_type, light, grad, phong, shading, filter_bits, keep):
    """OracleDos as oracle.render_dos fills it (ext_levels / tables may be None for the march)."""
    tf = O._q16_array(tf_rgbt)
    keep += [vol16, tf, grad]
    ka, kd, ks, shininess = shading
    Q = O.OracleDos()
    Q.base = O._params(vol16, scale, tf, grad, camera, W, H, step, phong, ka, kd, ks, shininess,
                       (1.0, 1.0, 1.0), light["position"])
    Q.base.filter_bits = int(filter_bits)
    if ext_levels is not None:
        flat = np.ascontiguousarray(np.concatenate([l.ravel() for l in ext_levels]), np.float32)
        keep.append(flat)
        Q.ext = flat.ctypes.data
        Q.ext_res[:] = list(ext_levels[0].shape[::-1])
        Q.ext_levels = len(ext_levels)
    Q.apply_occlusion, Q.apply_shadow, Q.shadow_type = int(apply_occlusion), int(apply_shadow), int(shadow_type)
    Q.light_forward[:] = [float(v) for v in light["forward"]]
    Q.light_up[:] = [float(v) for v in light["up"]]
    Q.light_right[:] = [float(v) for v in light["right"]]
    Q.spot_angle_deg = float(light["spot_angle_deg"])
    if occ_tables is not None:
        Q.occ = O._cone(occ_tables, keep)
        Q.sdw = O._cone(sdw_tables, keep)
    return Q


def dos_cache(vol16, scale, ext_levels, camera, dims, occ_tables, sdw_tables, light,
              apply_occlusion=True, apply_shadow=False, shadow_type=0, filter_bits=0,
              threads: int = 0) -> np.ndarray:
    """The light cache of the DOS cones: (dz, dy, dx, 2) uint16 (binary16 Idao, Idcs).
    dims = (dx, dy, dz).  The TF does not reach the cache (only the pyramid does)."""
    vol16 = np.ascontiguousarray(vol16, np.float32)
    keep = []
    tf = np.zeros((2, 4), np.float32)
    Q = _dos(vol16, scale, tf, ext_levels, camera, 1, 1, 1.0, occ_tables, sdw_tables,
             apply_occlusion, apply_shadow, shadow_type, light, None, False,
             (0.5, 0.5, 0.8, 30.0), filter_bits, keep)
    d = (ctypes.c_int * 3)(*[int(v) for v in dims])
    out = np.zeros((d[2], d[1], d[0], 2), np.uint16)
    lib().lcref_dos_cache(ctypes.byref(Q), d, out.ctypes.data, int(threads))
    return out


def render(vol16, scale, tf_rgbt, cache_rg, camera, W, H, step, light, apply_occlusion=True,
           apply_shadow=False, grad=None, phong=False, shading=(0.5, 0.5, 0.8, 30.0),
           filter_bits=0, threads: int = 0):
    """One frame of obj_ray_marching.comp over cache_rg ((dz, dy, dx, 2) uint16 / float16).
    Returns (rgba HxWx4, counts HxW, total)."""
    vol16 = np.ascontiguousarray(vol16, np.float32)
    if grad is not None:
        grad = np.ascontiguousarray(grad, np.float32)
    rg = np.ascontiguousarray(cache_rg).view(np.uint16)
    keep = [rg]
    Q = _dos(vol16, scale, tf_rgbt, None, camera, W, H, step, None, None, apply_occlusion,
             apply_shadow, 0, light, grad, phong, shading, filter_bits, keep)
    d = (ctypes.c_int * 3)(rg.shape[2], rg.shape[1], rg.shape[0])
    rgba = np.zeros((H, W, 4), np.float32)
    cnt = np.zeros((H, W), np.uint32)
    S = lib().lcref_render_rows(ctypes.byref(Q), rg.ctypes.data, d, 0, H, rgba.ctypes.data,
                                cnt.ctypes.data, int(threads))
    return rgba, cnt, int(S)
