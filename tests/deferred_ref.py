"""CPU reference of the deferred isosurface renderer (tests only; not a conftest).

Builds tests/support/deferred_ref.cpp -- which includes the oracle's translation unit, so
the trilinear fetch, the camera code, cvr_expf and cvr_powf are the pinned oracle's own --
with oracle/Makefile's flags into tests/support/build/ and binds it:

    render(...)     -> Frame(gpos, gnrm (H, W, 4), lit, rgba, unshifted, counts, total, stats)
    tone_map(...)   -> post_process.frag over an image
    edge_texel(p,s) -> the texel the lighting pass reads for pixel coordinate p
    density(...)    -> the trilinear density at texture-space positions
"""
from __future__ import annotations

import ctypes
from types import SimpleNamespace

import numpy as np

from oracle import oracle as O   # the module itself: its struct mirrors and _params helper
from ref_build import build_and_load

STATS = ("hits", "misses", "off_box", "skip_rays", "shifted")
LIGHT0 = (-206.873, -51.0699, 557.011)
# the reference's constructor, Update and Redraw values (cvr_deferred_params_default)
DEFAULTS = dict(isovalue=0.5, step_small=0.05, step_large=1.0, step_range=0.1, num_blocks=(4, 4, 4),
                color=(0.66, 0.6, 0.05, 1.0), ka=0.5, kd=0.5, ks=0.8, shininess=30.0,
                light_color=(1.0, 1.0, 1.0), light_pos=LIGHT0, exposure=1.0, gamma=2.2,
                gbuffer_clear=(1.0, 1.0, 1.0, 0.0))


class DeferredRef(ctypes.Structure):
    _fields_ = [("base", O.OracleRc1pass), ("nb", ctypes.c_int32 * 3),
                ("bmin", ctypes.c_void_p), ("bmax", ctypes.c_void_p),
                ("iso", ctypes.c_float), ("step_small", ctypes.c_float), ("step_large", ctypes.c_float),
                ("step_range", ctypes.c_float), ("color", ctypes.c_float * 4),
                ("ka", ctypes.c_float), ("kd", ctypes.c_float), ("ks", ctypes.c_float),
                ("shininess", ctypes.c_float), ("light_color", ctypes.c_float * 3),
                ("light", ctypes.c_float * 3), ("exposure", ctypes.c_float), ("gamma", ctypes.c_float),
                ("clear", ctypes.c_float * 4), ("stats", ctypes.c_uint64 * 5)]


def _bind(L):
    P, I = ctypes.c_void_p, ctypes.c_int
    L.deferredref_render.argtypes = [ctypes.POINTER(DeferredRef), P, P, P, P, P, P, I]
    L.deferredref_render.restype = ctypes.c_uint64
    L.deferredref_tone_map.argtypes = [P, P, ctypes.c_int64, ctypes.c_float, ctypes.c_float]
    L.deferredref_tone_map.restype = None
    L.deferredref_edge_texel.argtypes = [I, I]
    L.deferredref_edge_texel.restype = I
    L.deferredref_density.argtypes = [ctypes.POINTER(DeferredRef), P, P, ctypes.c_int64]
    L.deferredref_density.restype = None


def lib():
    return build_and_load("deferred_ref", _bind)


def _query(vol16, vox, scale, camera, W, H, par):
    """(DeferredRef, the arrays it points into)."""
    vol16 = np.ascontiguousarray(vol16, np.float32)
    p = dict(DEFAULTS, **par)
    bmin, bmax = O.iso_blocks(vox, p["num_blocks"])
    dummy_tf = np.zeros((2, 4), np.float32)
    Q = DeferredRef()
    Q.base = O._params(vol16, scale, dummy_tf, None, camera, W, H, 1.0, False, 0.0, 0.0, 0.0, 0.0,
                       (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), aspect=camera.get("aspect", 0.0))
    Q.nb[:] = [int(b) for b in p["num_blocks"]]
    Q.bmin, Q.bmax = bmin.ctypes.data, bmax.ctypes.data
    Q.iso, Q.step_small = p["isovalue"], p["step_small"]
    Q.step_large, Q.step_range = p["step_large"], p["step_range"]
    Q.color[:] = p["color"]
    Q.ka, Q.kd, Q.ks, Q.shininess = p["ka"], p["kd"], p["ks"], p["shininess"]
    Q.light_color[:] = p["light_color"]
    Q.light[:] = p["light_pos"]
    Q.exposure, Q.gamma = p["exposure"], p["gamma"]
    Q.clear[:] = p["gbuffer_clear"]
    return Q, (vol16, bmin, bmax, dummy_tf)


def render(vol16, vox, scale, camera, W, H, par=None, threads=0):
    """One frame.  vol16: the R16F volume as float; vox: the raw voxels (block table); par
    overrides DEFAULTS.  Arrays come back read-only."""
    Q, keep = _query(vol16, vox, scale, camera, W, H, par or {})
    gpos, gnrm, lit, rgba, unshifted = (np.zeros((H, W, 4), np.float32) for _ in range(5))
    cnt = np.zeros((H, W), np.uint32)
    total = lib().deferredref_render(ctypes.byref(Q), gpos.ctypes.data, gnrm.ctypes.data, lit.ctypes.data,
                                     rgba.ctypes.data, cnt.ctypes.data, unshifted.ctypes.data, int(threads))
    for a in (gpos, gnrm, lit, rgba, unshifted, cnt):
        a.setflags(write=False)
    return SimpleNamespace(gpos=gpos, gnrm=gnrm, lit=lit, rgba=rgba, unshifted=unshifted, counts=cnt,
                           total=int(total), stats=dict(zip(STATS, (int(v) for v in Q.stats))),
                           blocks=keep[1:3])


def tone_map(lit, exposure, gamma):
    lit = np.ascontiguousarray(lit, np.float32)
    out = np.empty_like(lit)
    lib().deferredref_tone_map(lit.ctypes.data, out.ctypes.data, lit.size // 4, exposure, gamma)
    return out


def edge_texel(p, s):
    return int(lib().deferredref_edge_texel(int(p), int(s)))


def density(vol16, scale, tex):
    """The trilinear density at texture-space positions tex (n, 3)."""
    vol16 = np.ascontiguousarray(vol16, np.float32)
    Q = DeferredRef()
    dummy = np.zeros((2, 4), np.float32)
    cam = dict(eye=(0.0, 0.0, 1.0), center=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0))
    Q.base = O._params(vol16, scale, dummy, None, cam, 1, 1, 1.0, False, 0.0, 0.0, 0.0, 0.0,
                       (0.0, 0.0, 0.0), (0.0, 0.0, 0.0))
    tex = np.ascontiguousarray(tex, np.float32)
    out = np.empty(len(tex), np.float32)
    lib().deferredref_density(ctypes.byref(Q), tex.ctypes.data, out.ctypes.data, len(tex))
    return out
