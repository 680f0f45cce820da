"""CPU reference of the slice-based directional occlusion renderer (tests only; not a
conftest).

Builds tests/support/sbtm_ref.cpp -- which includes the oracle's translation unit, so Tex,
tf_lookup, the camera code, cvr_expf and the half rounding are the pinned oracle's own --
with oracle/Makefile's flags into tests/support/build/ and binds it:

    slices(...)  -> dict(pos, depth, drawn, rx, ry): one entry per pass of the frame
    render(...)  -> Frame(rgba, counts, total, occ (2, H, W), stats, src, occ_hist, reach)
    fmaf, expf   -> libm's fmaf and the oracle's expf over float32 arrays
"""
from __future__ import annotations

import ctypes
from types import SimpleNamespace

import numpy as np

from oracle import oracle as O   # the module itself: its struct mirrors and _params helper
from ref_build import build_and_load

STATS = ("passes", "drawn", "stale_reads", "quad_only")
DEFAULTS = dict(angle=50.0, grid=(2, 2), attenuation=1.0, max_passes=90000, z_near=1.0, z_far=5000.0)


class SbtmRef(ctypes.Structure):
    _fields_ = [("base", O.OracleRc1pass), ("cone_half_angle_deg", ctypes.c_float),
                ("grid_x", ctypes.c_int32), ("grid_y", ctypes.c_int32), ("attenuation", ctypes.c_float),
                ("max_passes", ctypes.c_int32), ("z_near", ctypes.c_float), ("z_far", ctypes.c_float),
                ("stats", ctypes.c_uint64 * 4)]


def _bind(L):
    P, I = ctypes.c_void_p, ctypes.c_int
    L.sbtmref_slices.argtypes = [ctypes.POINTER(SbtmRef), P, P, P, P, P, I]
    L.sbtmref_slices.restype = I
    L.sbtmref_render.argtypes = [ctypes.POINTER(SbtmRef), P, P, P, P, P, P, I]
    L.sbtmref_render.restype = ctypes.c_uint64
    L.sbtmref_fmaf_n.argtypes = [P, P, P, P, ctypes.c_int64]
    L.sbtmref_fmaf_n.restype = None
    L.sbtmref_expf_n.argtypes = [P, P, ctypes.c_int64]
    L.sbtmref_expf_n.restype = None


def lib():
    return build_and_load("sbtm_ref", _bind)


def _query(vol16, scale, tf_rgbt, camera, W, H, step, par, filter_bits):
    """(SbtmRef, the arrays it points into)."""
    vol16 = np.ascontiguousarray(vol16, np.float32)
    tf = O._q16_array(tf_rgbt)
    p = dict(DEFAULTS, **par)
    Q = SbtmRef()
    Q.base = O._params(vol16, scale, tf, None, camera, W, H, step, False, 0.5, 0.5, 0.8, 30.0,
                       (1.0, 1.0, 1.0), (0.0, 0.0, 0.0))
    Q.base.filter_bits = int(filter_bits)
    Q.cone_half_angle_deg = float(p["angle"])
    Q.grid_x, Q.grid_y = (int(v) for v in p["grid"])
    Q.attenuation = float(p["attenuation"])
    Q.max_passes = int(p["max_passes"])
    Q.z_near, Q.z_far = float(p["z_near"]), float(p["z_far"])
    return Q, (vol16, tf)


def slices(vol16, scale, tf_rgbt, camera, W, H, step, par=None, filter_bits=0):
    Q, keep = _query(vol16, scale, tf_rgbt, camera, W, H, step, par or {}, filter_bits)
    n = lib().sbtmref_slices(ctypes.byref(Q), None, None, None, None, None, 0)
    pos, depth = np.zeros(n, np.float32), np.zeros(n, np.float32)
    drawn, rx, ry = (np.zeros(n, np.int32) for _ in range(3))
    lib().sbtmref_slices(ctypes.byref(Q), pos.ctypes.data, depth.ctypes.data, drawn.ctypes.data,
                         rx.ctypes.data, ry.ctypes.data, n)
    return dict(pos=pos, depth=depth, drawn=drawn.astype(bool), rx=rx, ry=ry)


def render(vol16, scale, tf_rgbt, camera, W, H, step, par=None, filter_bits=0, history=False, threads=0):
    """One frame.  par: angle, grid, attenuation, max_passes, z_near, z_far (DEFAULTS).  With
    history: src (passes, H, W, 4) and occ_hist (passes, H, W), NaN where discarded."""
    Q, keep = _query(vol16, scale, tf_rgbt, camera, W, H, step, par or {}, filter_bits)
    sl = slices(vol16, scale, tf_rgbt, camera, W, H, step, par, filter_bits)
    n = len(sl["pos"])
    rgba = np.zeros((H, W, 4), np.float32)
    cnt = np.zeros((H, W), np.uint32)
    occ = np.zeros((2, H, W), np.float32)
    reach = np.zeros((max(n, 1), 2), np.int32)
    src = np.zeros((n, H, W, 4), np.float32) if history else None
    hocc = np.zeros((n, H, W), np.float32) if history else None
    total = lib().sbtmref_render(ctypes.byref(Q), rgba.ctypes.data, cnt.ctypes.data, occ.ctypes.data,
                                 src.ctypes.data if history else None, hocc.ctypes.data if history else None,
                                 reach.ctypes.data, int(threads))
    out = SimpleNamespace(rgba=rgba, counts=cnt, total=int(total), occ=occ, slices=sl, reach=reach[:n],
                          stats=dict(zip(STATS, (int(v) for v in Q.stats))), src=src, occ_hist=hocc)
    for a in (rgba, cnt, occ):
        a.setflags(write=False)
    return out


def fmaf(a, b, c):
    a, b, c = (np.ascontiguousarray(np.broadcast_to(np.asarray(v, np.float32), np.broadcast(a, b, c).shape))
               for v in (a, b, c))
    out = np.empty(a.shape, np.float32)
    lib().sbtmref_fmaf_n(a.ctypes.data, b.ctypes.data, c.ctypes.data, out.ctypes.data, a.size)
    return out


def expf(x):
    x = np.ascontiguousarray(x, np.float32)
    out = np.empty(x.shape, np.float32)
    lib().sbtmref_expf_n(x.ctypes.data, out.ctypes.data, x.size)
    return out
