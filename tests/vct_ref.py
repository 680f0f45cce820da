"""CPU reference of the voxel cone tracing renderer (tests only; not a conftest).

Builds tests/support/vct_ref.cpp -- which includes the oracle's translation unit, so Tex,
tf_lookup, the camera and slab code, cvr_expf / cvr_logf / cvr_powf and oracle_tf_get are the
pinned oracle's own -- with oracle/Makefile's flags into tests/support/build/ and binds it:

    pyramid(vol)            -> (levels: list of (d, h, w, 2) float32, max_stddev)
    table(vol, tf_table)    -> (ceil(max_stddev), 255) float32
    render(...)             -> (rgba, counts, total); render.stats holds the last frame's
                               cone statistics (see VctRef.stats in the source)
"""
from __future__ import annotations

import ctypes
import math

import numpy as np

from oracle import oracle as O   # the module itself: its struct mirrors and _params helper
from ref_build import build_and_load

MAX_LEVELS = 16
STATS = ("cones", "cut", "full", "level0_only", "top_only", "pair_mask", "fetches")


class VctRef(ctypes.Structure):
    _fields_ = [("base", O.OracleRc1pass), ("pyr", ctypes.c_void_p), ("nl", ctypes.c_int32),
                ("dims", (ctypes.c_int32 * 3) * MAX_LEVELS), ("table", ctypes.c_void_p),
                ("tab_h", ctypes.c_int32), ("max_stddev", ctypes.c_double),
                ("apply_occlusion", ctypes.c_int32), ("apply_shadow", ctypes.c_int32),
                ("cone_step", ctypes.c_float), ("cone_rate", ctypes.c_float),
                ("cone_initial", ctypes.c_float), ("cone_angle_deg", ctypes.c_float),
                ("apply_correction", ctypes.c_int32), ("correction_factor", ctypes.c_float),
                ("samples", ctypes.c_int32), ("stats", ctypes.c_uint64 * 8)]


def _bind(L):
    P, I = ctypes.c_void_p, ctypes.c_int
    L.vctref_pyramid.argtypes = [P, I, I, I, P, P, P]
    L.vctref_pyramid.restype = I
    L.vctref_table.argtypes = [P, ctypes.c_double, P]
    L.vctref_table.restype = I
    L.vctref_render_rows.argtypes = [ctypes.POINTER(VctRef), I, I, P, P, I]
    L.vctref_render_rows.restype = ctypes.c_uint64


def lib():
    return build_and_load("vct_ref", _bind)


def level_dims(shape):
    """The level chain of a (d, h, w) volume: halve (floor) until a dimension reaches 0."""
    d, h, w = shape
    out = []
    while w >= 1 and h >= 1 and d >= 1:
        out.append((d, h, w))
        d, h, w = d // 2, h // 2, w // 2
    return out


def pyramid(vol):
    """(levels, max_stddev): level i as a (d, h, w, 2) float32 array of binary16-rounded
    (mean, stddev), and maximum_standard_deviation (a double)."""
    vol = np.ascontiguousarray(vol, np.uint8)
    d, h, w = vol.shape
    dims_want = level_dims(vol.shape)
    flat = np.zeros((sum(a * b * c for a, b, c in dims_want), 2), np.float32)
    dims = np.zeros((MAX_LEVELS, 3), np.int32)
    mx = ctypes.c_double()
    nl = lib().vctref_pyramid(vol.ctypes.data, w, h, d, flat.ctypes.data, dims.ctypes.data, ctypes.byref(mx))
    levels, off = [], 0
    for L in range(nl):
        lw, lh, ld = (int(v) for v in dims[L])
        n = lw * lh * ld
        levels.append(flat[off:off + n].reshape(ld, lh, lw, 2).copy())
        off += n
    assert off == flat.shape[0]
    return levels, mx.value


def table(vol, tf_table, max_stddev=None):
    """The pre-integration table of (volume, double TF table of 256 entries)."""
    if max_stddev is None:
        max_stddev = pyramid(vol)[1]
    t = np.ascontiguousarray(tf_table, np.float64)
    assert t.shape == (256, 4)
    h = math.ceil(max_stddev)
    out = np.zeros((h, 255), np.float32)
    assert lib().vctref_table(t.ctypes.data, float(max_stddev), out.ctypes.data) == h
    return out


def render(vol16, scale, tf_rgbt, camera, W, H, step, light, pyr, tab, cone, apply_occlusion=True,
           apply_shadow=True, grad=None, phong=False, shading=(0.5, 0.5, 0.8, 30.0), filter_bits=0,
           threads: int = 0):
    """One frame.  pyr: pyramid(vol); tab: table(vol, tf_table); cone: dict with step, rate,
    initial, angle_deg, correction (bool), factor, samples.  Returns (rgba HxWx4, counts HxW,
    total, stats dict)."""
    vol16 = np.ascontiguousarray(vol16, np.float32)
    tf = O._q16_array(tf_rgbt)
    if grad is not None:
        grad = np.ascontiguousarray(grad, np.float32)
    levels, max_sd = pyr
    flat = np.ascontiguousarray(np.concatenate([l.reshape(-1, 2) for l in levels]), np.float32)
    tab = np.ascontiguousarray(tab, np.float32)
    ka, kd, ks, shininess = shading
    Q = VctRef()
    Q.base = O._params(vol16, scale, tf, grad, camera, W, H, step, phong, ka, kd, ks, shininess,
                       (1.0, 1.0, 1.0), light["position"])
    Q.base.filter_bits = int(filter_bits)
    Q.pyr, Q.nl = flat.ctypes.data, len(levels)
    for i, l in enumerate(levels):
        Q.dims[i][:] = [l.shape[2], l.shape[1], l.shape[0]]
    Q.table, Q.tab_h, Q.max_stddev = tab.ctypes.data, tab.shape[0], float(max_sd)
    Q.apply_occlusion, Q.apply_shadow = int(apply_occlusion), int(apply_shadow)
    Q.cone_step, Q.cone_rate = float(cone["step"]), float(cone["rate"])
    Q.cone_initial, Q.cone_angle_deg = float(cone["initial"]), float(cone["angle_deg"])
    Q.apply_correction, Q.correction_factor = int(cone["correction"]), float(cone["factor"])
    Q.samples = int(cone["samples"])
    rgba = np.zeros((H, W, 4), np.float32)
    cnt = np.zeros((H, W), np.uint32)
    S = lib().vctref_render_rows(ctypes.byref(Q), 0, H, rgba.ctypes.data, cnt.ctypes.data, int(threads))
    return rgba, cnt, int(S), dict(zip(STATS, (int(v) for v in Q.stats)))
