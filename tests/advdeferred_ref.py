"""CPU reference of the advanced deferred isosurface renderer (tests only; not a conftest).

Builds tests/support/advdeferred_ref.cpp -- which includes deferred_ref.cpp and through it
the oracle's translation unit, so the geometry pass is DeferredShading's restatement and
dot, normalize, cvr_expf and cvr_powf are the pinned oracle's own -- and binds it:

    render(...)     -> Frame(gpos, gnrm, curv (H, W, 4), k1, k2 (H, W), dir (H, W, 2), lit, rgba,
                             flags (bit 0 ridge, bit 1 valley, before the toggles), counts,
                             total, stats, projection)
    curvature(...)  -> the curvature pass over a normal plane
    shade(...)      -> the lighting pass and the tone map over given planes
    tables(s, v)    -> the colour map (256, 4) and the ridge map's red channel (256, 256)
    wrap_texel(u,n) -> the texel a GL_NEAREST, GL_REPEAT fetch at coordinate u reads
"""
from __future__ import annotations

import ctypes
from types import SimpleNamespace

import numpy as np

import deferred_ref as DR
from ref_build import build_and_load

STATS = ("surface", "nan_curvature", "finite_curvature", "ridges", "valleys", "featured")
# cvr_advdeferred_params_default: the reference's constructor, Init, LightingPass and Redraw
# values and lighting_pass.comp's constants
DEFAULTS = dict(DR.DEFAULTS, ka=0.1, kd=0.7, ks=0.2, shininess=32.0, gbuffer_clear=(1.0, 1.0, 1.0, 1.0),
                flow_speed=1.0, flow_scale=10.0, time=0.0, show_ridges=True, show_valleys=True,
                accessibility_strength=0.5, screen_size=(0.0, 0.0), colormap_s=0.6, colormap_v=0.2)


class AdvRef(ctypes.Structure):
    _fields_ = [("d", DR.DeferredRef), ("flow_speed", ctypes.c_float), ("flow_scale", ctypes.c_float),
                ("time", ctypes.c_float), ("show_ridges", ctypes.c_int32), ("show_valleys", ctypes.c_int32),
                ("accessibility", ctypes.c_float), ("screen", ctypes.c_float * 2),
                ("cmap_s", ctypes.c_float), ("cmap_v", ctypes.c_float), ("stats", ctypes.c_uint64 * 6)]


def _bind(L):
    P, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    L.advref_tables.argtypes = [F, F, P, P]
    L.advref_tables.restype = None
    L.advref_curvature.argtypes = [P, I, I, F, F, P]
    L.advref_curvature.restype = None
    L.advref_shade.argtypes = [ctypes.POINTER(AdvRef), P, P, P, P, I, I, P, P, P]
    L.advref_shade.restype = None
    L.advref_render.argtypes = [ctypes.POINTER(AdvRef), P, P, P, P, P, P, P, I]
    L.advref_render.restype = ctypes.c_uint64
    L.advref_projection.argtypes = [ctypes.POINTER(AdvRef), P]
    L.advref_projection.restype = None
    L.advref_wrap_texel.argtypes = [F, I]
    L.advref_wrap_texel.restype = I


def lib():
    return build_and_load("advdeferred_ref", _bind)


def _fill(Q, p):
    Q.flow_speed, Q.flow_scale, Q.time = p["flow_speed"], p["flow_scale"], p["time"]
    Q.show_ridges, Q.show_valleys = int(bool(p["show_ridges"])), int(bool(p["show_valleys"]))
    Q.accessibility = p["accessibility_strength"]
    Q.screen[:] = p["screen_size"]
    Q.cmap_s, Q.cmap_v = p["colormap_s"], p["colormap_v"]


def _query(vol16, vox, scale, camera, W, H, par):
    p = dict(DEFAULTS, **par)
    d, keep = DR._query(vol16, vox, scale, camera, W, H, {k: p[k] for k in DR.DEFAULTS})
    Q = AdvRef()
    Q.d = d
    _fill(Q, p)
    return Q, keep


def _frame(Q, gpos, gnrm, curv, lit, rgba, flags, cnt, total):
    for a in (gpos, gnrm, curv, lit, rgba, flags, cnt):
        if a is not None:
            a.setflags(write=False)
    proj = np.zeros(2, np.float32)
    lib().advref_projection(ctypes.byref(Q), proj.ctypes.data)
    return SimpleNamespace(gpos=gpos, gnrm=gnrm, curv=curv, k1=curv[..., 0], k2=curv[..., 1], dir=curv[..., 2:4],
                           lit=lit, rgba=rgba, flags=flags, counts=cnt, total=total,
                           stats=dict(zip(STATS, (int(v) for v in Q.stats))), projection=(proj[0], proj[1]))


def render(vol16, vox, scale, camera, W, H, par=None, threads=0):
    """One frame.  vol16: the R16F volume as float; vox: the raw voxels (block table); par
    overrides DEFAULTS.  Arrays come back read-only."""
    Q, keep = _query(vol16, vox, scale, camera, W, H, par or {})
    gpos, gnrm, curv, lit, rgba = (np.zeros((H, W, 4), np.float32) for _ in range(5))
    cnt = np.zeros((H, W), np.uint32)
    flags = np.zeros((H, W), np.uint8)
    total = lib().advref_render(ctypes.byref(Q), gpos.ctypes.data, gnrm.ctypes.data, curv.ctypes.data,
                                lit.ctypes.data, rgba.ctypes.data, cnt.ctypes.data, flags.ctypes.data, int(threads))
    return _frame(Q, gpos, gnrm, curv, lit, rgba, flags, cnt, int(total))


def curvature(gnrm, p00, p11):
    """The curvature pass over a normal plane (H, W, 4): (H, W, 4) as (k1, k2, dir.x, dir.y)."""
    gnrm = np.ascontiguousarray(gnrm, np.float32)
    H, W = gnrm.shape[:2]
    curv = np.zeros((H, W, 4), np.float32)
    lib().advref_curvature(gnrm.ctypes.data, W, H, p00, p11, curv.ctypes.data)
    return curv


def shade(gpos, gnrm, curv, eye, par=None):
    """The lighting pass and the tone map over given planes: lit, rgba, flags, stats."""
    p = dict(DEFAULTS, **(par or {}))
    gpos, gnrm, curv = (np.ascontiguousarray(a, np.float32) for a in (gpos, gnrm, curv))
    H, W = gnrm.shape[:2]
    Q = AdvRef()
    Q.d.color[:] = p["color"]
    Q.d.ka, Q.d.kd, Q.d.ks, Q.d.shininess = p["ka"], p["kd"], p["ks"], p["shininess"]
    Q.d.light_color[:] = p["light_color"]
    Q.d.light[:] = p["light_pos"]
    Q.d.exposure, Q.d.gamma = p["exposure"], p["gamma"]
    _fill(Q, p)
    e = np.asarray(eye, np.float32)
    lit, rgba = np.zeros((H, W, 4), np.float32), np.zeros((H, W, 4), np.float32)
    flags = np.zeros((H, W), np.uint8)
    lib().advref_shade(ctypes.byref(Q), e.ctypes.data, gpos.ctypes.data, gnrm.ctypes.data, curv.ctypes.data, W, H,
                       lit.ctypes.data, rgba.ctypes.data, flags.ctypes.data)
    return SimpleNamespace(lit=lit, rgba=rgba, flags=flags, stats=dict(zip(STATS, (int(v) for v in Q.stats))))


def tables(s=0.6, v=0.2):
    cmap, ridge = np.zeros((256, 4), np.float32), np.zeros((256, 256), np.float32)
    lib().advref_tables(s, v, cmap.ctypes.data, ridge.ctypes.data)
    return cmap, ridge


def wrap_texel(u, size):
    return int(lib().advref_wrap_texel(float(u), int(size)))
