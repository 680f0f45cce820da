"""CPU reference of the ground-truth cone ray-caster (tests only; not a conftest).

Builds tests/support/crtgt_ref.cpp -- which includes the oracle's translation unit, so
Tex, tf_lookup, the camera and slab code and the exp are the pinned oracle's own -- with
oracle/Makefile's flags into tests/support/build/ and binds its function:

    render(...)       gt_ray_marching.comp carried through in float: (rgba, counts, total)
"""
from __future__ import annotations

import ctypes

import numpy as np

from oracle import oracle as O   # the module itself: its struct mirrors and _params helper
from ref_build import build_and_load


class GtRef(ctypes.Structure):
    _fields_ = [("base", O.OracleRc1pass), ("light_forward", ctypes.c_float * 3),
                ("light_up", ctypes.c_float * 3), ("light_right", ctypes.c_float * 3),
                ("light_gap", ctypes.c_float), ("light_step", ctypes.c_float),
                ("apply_occlusion", ctypes.c_int32), ("apply_shadow", ctypes.c_int32),
                ("shadow_type", ctypes.c_int32), ("occ_distance", ctypes.c_float),
                ("sdw_distance", ctypes.c_float), ("n_occ", ctypes.c_int32), ("n_sdw", ctypes.c_int32),
                ("occ_rays", ctypes.c_void_p), ("sdw_rays", ctypes.c_void_p)]


def _bind(L):
    P, I = ctypes.c_void_p, ctypes.c_int
    L.gtref_render_rows.argtypes = [ctypes.POINTER(GtRef), I, I, P, P, I]
    L.gtref_render_rows.restype = ctypes.c_uint64


def lib():
    return build_and_load("crtgt_ref", _bind)


def half_rays(rays) -> np.ndarray:
    """A ray table as the renderer stores it: (n, 3) float32 of binary16-rounded values."""
    a = np.asarray(rays, np.float32).reshape(-1, 3)
    return np.ascontiguousarray(a.astype(np.float16).astype(np.float32))


def render(vol16, scale, tf_rgbt, camera, W, H, step, light, occ_rays=None, sdw_rays=None,
           apply_occlusion=False, apply_shadow=False, shadow_type=0, light_gap=1.0, light_step=0.5,
           occ_distance=0.0, sdw_distance=0.0, grad=None, phong=False,
           shading=(0.5, 0.5, 0.8, 30.0), filter_bits=0, threads: int = 0):
    """The converged ground-truth frame.  occ_rays / sdw_rays: (n, 3) floats (rounded to
    binary16 here, as the renderer stores them); the distances are explicit (> 0).
    Returns (rgba HxWx4, counts HxW, total)."""
    vol16 = np.ascontiguousarray(vol16, np.float32)
    tf = O._q16_array(tf_rgbt)
    if grad is not None:
        grad = np.ascontiguousarray(grad, np.float32)
    ka, kd, ks, shininess = shading
    Q = GtRef()
    Q.base = O._params(vol16, scale, tf, grad, camera, W, H, step, phong, ka, kd, ks, shininess,
                       (1.0, 1.0, 1.0), light["position"])
    Q.base.filter_bits = int(filter_bits)
    Q.light_forward[:] = [float(v) for v in light["forward"]]
    Q.light_up[:] = [float(v) for v in light["up"]]
    Q.light_right[:] = [float(v) for v in light["right"]]
    Q.light_gap, Q.light_step = float(light_gap), float(light_step)
    Q.apply_occlusion, Q.apply_shadow, Q.shadow_type = int(apply_occlusion), int(apply_shadow), int(shadow_type)
    Q.occ_distance, Q.sdw_distance = float(occ_distance), float(sdw_distance)
    occ = half_rays(occ_rays) if apply_occlusion else np.zeros((0, 3), np.float32)
    sdw = half_rays(sdw_rays) if apply_shadow else np.zeros((0, 3), np.float32)
    Q.n_occ, Q.n_sdw = occ.shape[0], sdw.shape[0]
    Q.occ_rays, Q.sdw_rays = occ.ctypes.data, sdw.ctypes.data
    rgba = np.zeros((H, W, 4), np.float32)
    cnt = np.zeros((H, W), np.uint32)
    S = lib().gtref_render_rows(ctypes.byref(Q), 0, H, rgba.ctypes.data, cnt.ctypes.data, int(threads))
    return rgba, cnt, int(S)
