"""One awkward scene for the shaded renderers, shared by tests/test_aniso_gpu.py (GPU,
bit for bit) and tests/test_axis_rotation.py (CPU, the references against themselves
under a relabelling of the axes); a plain module, not a conftest.

Every other shaded case renders Marschner-Lobb n^3 with D.voxel_scale(n) and a cubic
pyramid: nx = ny = nz, sx = sy = sz, every pyramid level and the box are cubes, and an
axis taken for another changes no pixel.  Here nothing is equal:

    volume   marschner_lobb_u8(48)[:44, :40, :33]   (z, y, x) = (44, 40, 33)
    scale    (9.0, 11.5, 7.25)                      box 297 x 460 x 319
    pyramid  (40, 32, 24); light caches (20, 12, 9) (DOS) and (10, 7, 5) (EBS)

`twin` selects the scene (0) or its relabelled twin under R: v -> (v_y, v_z, v_x), a
cyclic relabelling of the axes and so a proper rotation: 1 relabels everything (volume
transpose(2, 0, 1), scale, camera, light, pyramid and cache sizes), 2 relabels
everything but the scale (the negative control: a different scene).  References are
computed once per session (functools.lru_cache) and shared read-only."""
import ctypes
import functools
import math
from types import SimpleNamespace

import numpy as np

import crtgt_cases as G
import ebs_preillum_cases as E
import preillum_cases as P
from cpp_volume_rendering_amd import _native as N
from cpp_volume_rendering_amd import datasets as D
from cpp_volume_rendering_amd.renderer import default_cone_params

SCALE = (9.0, 11.5, 7.25)
EXT_RES = (40, 32, 24)
DOS_DIMS = (20, 12, 9)
EBS_DIMS = (10, 7, 5)
FRAMES = ((96, 80), (77, 53))          # the second is ragged against the 8x8 tiles
OUTSIDE = dict(eye=(-300.0, 120.0, 420.0), center=(10.0, -5.0, 20.0), up=(0.0, 1.0, 0.0))
INSIDE = P.INSIDE                      # (10, -20, 30): inside the half box (148.5, 230, 159.5)
CAMS = {"outside": OUTSIDE, "inside": INSIDE}
LIGHT0 = P.LIGHT0                      # outside the box, 28 degree spot
LIGHT_INSIDE = dict(LIGHT0, position=E.LIGHT_INSIDE)
LIGHTS = {"light0": LIGHT0, "inside": LIGHT_INSIDE}


def R(v):
    """The relabelling of a world vector (or of an (x, y, z) size)."""
    return (v[1], v[2], v[0])


def back(a):
    """A twin's (z', y', x', ...) array in the scene's (z, y, x, ...) order."""
    return np.ascontiguousarray(np.moveaxis(a, (0, 1, 2), (2, 0, 1)))


def camera(key, twin=0):
    c = CAMS[key]
    return {k: R(v) for k, v in c.items()} if twin else c


def light(key, twin=0):
    l = LIGHTS[key]
    if not twin:
        return l
    return dict(l, **{k: R(l[k]) for k in ("position", "forward", "up", "right")})


def dims(d, twin=0):
    return R(d) if twin else d


def volume(bits=8):
    vol = D.marschner_lobb_u8(48)[:44, :40, :33].copy()
    return vol if bits == 8 else vol.astype(np.uint16) * 257 + 3


@functools.lru_cache(maxsize=None)
def scene(bits=8, twin=0):
    """vol, scale, vol16, tf, tf_rgba, grad (FD), step, n_xyz and the box diagonal."""
    import oracle as O
    vol = volume(bits)
    if twin:
        vol = np.ascontiguousarray(vol.transpose(2, 0, 1))
    scale = R(SCALE) if twin == 1 else SCALE
    table = O.tf_table_double(D.BONSAI_TF_RGB, D.BONSAI_TF_ALPHA)
    n_xyz = vol.shape[::-1]
    diag = math.sqrt(sum((n * float(s)) ** 2 for n, s in zip(n_xyz, scale)))
    return SimpleNamespace(vol=vol, scale=scale, vol16=O.volume_r16f(vol), tf=O.tf_rgbt(table),
                           tf_rgba=O.tf_rgbt(table, extinction_input=True), grad=O.gradient(vol, "fd"),
                           step=O.default_step(scale), n_xyz=n_xyz, diag=diag, bits=bits)


@functools.lru_cache(maxsize=None)
def pyramid(bits=8, twin=0):
    """The extinction pyramid's levels at EXT_RES (relabelled for a twin), read-only."""
    import oracle as O
    s = scene(bits, twin)
    levels = O.ext_volume(s.vol16, s.scale, s.tf_rgba, dims(EXT_RES, twin))
    for l in levels:
        l.setflags(write=False)
    return levels


@functools.lru_cache(maxsize=None)
def sat(bits=8, twin=0):
    """(ext lut, float SAT) as the EBS renderer builds them, read-only."""
    import oracle as O
    from test_ebs import lib_ext_lut
    lut = lib_ext_lut(bits // 8)
    t = O.sat_build(scene(bits, twin).vol, lut).astype(np.float32)
    t.setflags(write=False)
    return lut, t


def cone_tables(params, diag, frac):
    """cvr_build_cone_tables with the covered distance the library derives for a box of
    diagonal `diag`: (float)(diag * 0.50f | 0.75f), the product in double."""
    p = N.ConeParams.from_buffer_copy(params)
    if p.covered_distance <= 0:
        p.covered_distance = float(np.float32(np.float64(diag) * np.float64(np.float32(frac))))
    t = N.ConeTables()
    N.check(N.lib().cvr_build_cone_tables(ctypes.byref(p), 1.0, ctypes.byref(t)), "cones")
    return t


def occ1():
    """A single-ray occlusion cone (no 3- or 7-ray sections): it reads nothing but its axis."""
    c = default_cone_params(True)
    c.max_packing = 0
    return c


OCC = {"default": lambda: default_cone_params(True), "occ7": P.occ7, "occ1": occ1}

# ---------------------------------------------------------------------------------------
# rc1pass: the frames the shaded ones are compared with
# ---------------------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def plain(cam="outside", W=96, H=80, phong=False, bits=8, twin=0, fb=0):
    import oracle as O
    s = scene(bits, twin)
    out = O.render_rc1pass(s.vol16, s.scale, s.tf, camera(cam, twin), W, H, s.step,
                           grad=s.grad if phong else None, phong=phong,
                           light=light("light0", twin)["position"], filter_bits=fb)
    for a in out[:2]:
        a.setflags(write=False)
    return out


def assert_visible(rgba, cam="outside", W=96, H=80, bits=8, fb=0, shaded=True):
    """The conditions every reference frame meets (crtgt_cases.assert_shading_visible's,
    and for the outside view a frame that is mostly composited): checked on the reference."""
    base = plain(cam, W, H, False, bits, 0, fb)[0]
    comp = base[..., 3] > 0
    if cam == "outside":
        assert rgba[..., 3].max() > 0.5
        assert comp.mean() >= 0.5
    if shaded:
        diff = np.abs(rgba[..., :3] - base[..., :3]).max(axis=-1) > 1e-3
        assert comp.any() and (diff & comp).sum() >= 0.05 * comp.sum()


# ---------------------------------------------------------------------------------------
# DOS: the on-the-fly frame, the light cache, the cached frame
# ---------------------------------------------------------------------------------------

#            occlusion, shadow, shadow type, Phong, camera, occlusion cone
DOS_CASES = {
    "occlusion": (True, False, 0, False, "outside", "default"),
    "both_point": (True, True, 0, False, "outside", "default"),
    "both_spot": (True, True, 1, False, "outside", "default"),
    "both_dir": (True, True, 2, False, "outside", "default"),
    "phong_fd": (True, True, 0, True, "outside", "default"),
    "inside": (True, True, 0, False, "inside", "default"),
    "occ7": (True, False, 0, False, "outside", "occ7"),
    # every term of these reads world-space inputs only (see test_axis_rotation.py)
    "occ1_point": (True, True, 0, False, "outside", "occ1"),
    "occ1_dir": (True, True, 2, False, "outside", "occ1"),
    "occ1_phong": (True, True, 0, True, "outside", "occ1"),
    "shadow_only": (False, True, 0, False, "outside", "default"),
}


def dos_tables(name, bits=8, twin=0):
    s = scene(bits, twin)
    return (cone_tables(OCC[DOS_CASES[name][5]](), s.diag, 0.50),
            cone_tables(default_cone_params(False), s.diag, 0.75))


def _ro(out):
    for a in out[:2]:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def dos_frame(name, W=96, H=80, bits=8, twin=0, fb=0):
    """oracle.render_dos of a DOS_CASES entry: (rgba, counts, total), read-only."""
    import oracle as O
    occ_on, sdw_on, stype, phong, cam, _ = DOS_CASES[name]
    s = scene(bits, twin)
    occ, sdw = dos_tables(name, bits, twin)
    return _ro(O.render_dos(s.vol16, s.scale, s.tf, pyramid(bits, twin), camera(cam, twin), W, H, s.step,
                            occ, sdw, apply_occlusion=occ_on, apply_shadow=sdw_on, shadow_type=stype,
                            light=light("light0", twin), grad=s.grad if phong else None, phong=phong,
                            filter_bits=fb))


@functools.lru_cache(maxsize=None)
def dos_cache(name, twin=0):
    """lightcache_ref.dos_cache of a DOS_CASES entry at DOS_DIMS: (dz, dy, dx, 2) uint16."""
    import lightcache_ref as L
    occ_on, sdw_on, stype, _, cam, _ = DOS_CASES[name]
    s = scene(8, twin)
    occ, sdw = dos_tables(name, 8, twin)
    c = L.dos_cache(s.vol16, s.scale, pyramid(8, twin), camera(cam, twin), dims(DOS_DIMS, twin), occ, sdw,
                    light("light0", twin), apply_occlusion=occ_on, apply_shadow=sdw_on, shadow_type=stype)
    c.setflags(write=False)
    return c


def cached_frame(cache, cam, W, H, occ_on, sdw_on, phong, lpos, twin=0):
    """lightcache_ref.render (obj_ray_marching.comp, one shader for both renderers)."""
    import lightcache_ref as L
    s = scene(8, twin)
    lt = dict(light("light0", twin), position=lpos)
    return _ro(L.render(s.vol16, s.scale, s.tf, cache, camera(cam, twin), W, H, s.step, lt,
                        apply_occlusion=occ_on, apply_shadow=sdw_on, grad=s.grad if phong else None,
                        phong=phong))


@functools.lru_cache(maxsize=None)
def dos_cached_frame(name, W=96, H=80, twin=0):
    occ_on, sdw_on, _, phong, cam, _ = DOS_CASES[name]
    return cached_frame(dos_cache(name, twin), cam, W, H, occ_on, sdw_on, phong,
                        light("light0", twin)["position"], twin)


# ---------------------------------------------------------------------------------------
# EBS: the on-the-fly frame, the light cache, the cached frame
# ---------------------------------------------------------------------------------------

# keyword arguments of ebs_preillum_cases.ebs_params; `lkey` names the light, `cam` the camera
EBS_CASES = {
    "defaults_point": dict(),
    "occlusion_only": dict(apply_shadow=False),
    "shadow_only": dict(apply_occlusion=False),
    "directional": dict(shadow_type=1),
    "shadow_dir_only": dict(shadow_type=1, apply_occlusion=False),
    "phong": dict(phong=True),
    "wide_cone": E.CASES["wide_cone"],
    "cone_60": E.CASES["cone_60"],
    "inside": dict(cam="inside"),
    "light_inside": dict(lkey="inside"),
}


def ebs_params(name, step, twin=0):
    """cvr_ebs_params of an EBS_CASES entry."""
    c = dict(EBS_CASES[name])
    c.pop("cam", None)
    lt = light(c.pop("lkey", "light0"), twin)
    return E.ebs_params(step=step, light=lt["position"], light_forward=lt["forward"], **c)


def _ebs_kw(p):
    return dict(apply_occlusion=p.apply_occlusion, occ_shells=p.occlusion_shells, occ_radius=p.occlusion_radius,
                apply_shadow=p.apply_shadow, shadow_type=p.shadow_type, cone_angle_deg=p.shadow_cone_angle_deg,
                interval=p.shadow_sample_interval, initial_step=p.shadow_initial_step,
                ui_weight=p.shadow_ui_weight,
                max_distance=(p.shadow_max_distance if p.shadow_max_distance > 0 else None))


@functools.lru_cache(maxsize=None)
def ebs_frame(name, W=96, H=80, bits=8, twin=0, fb=0):
    """oracle.render_ebs of an EBS_CASES entry: (rgba, counts, total), read-only."""
    import oracle as O
    s = scene(bits, twin)
    p = ebs_params(name, s.step, twin)
    phong = bool(p.apply_gradient_shading)
    return _ro(O.render_ebs(s.vol16, s.scale, s.tf, sat(bits, twin)[1], camera(EBS_CASES[name].get("cam", "outside"), twin),
                            W, H, s.step, light=tuple(p.light_pos), light_forward=tuple(p.light_forward),
                            grad=s.grad if phong else None, phong=phong, filter_bits=fb, **_ebs_kw(p)))


@functools.lru_cache(maxsize=None)
def ebs_cache(name, twin=0):
    """ebs_lightcache_ref.ebs_cache of an EBS_CASES entry at EBS_DIMS: (dz, dy, dx, 2) uint16."""
    import ebs_lightcache_ref as L
    s = scene(8, twin)
    p = ebs_params(name, s.step, twin)
    c = L.ebs_cache(s.n_xyz, s.scale, sat(8, twin)[1], dims(EBS_DIMS, twin), tuple(p.light_pos),
                    tuple(p.light_forward), **_ebs_kw(p))
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def ebs_cached_frame(name, W=96, H=80, twin=0):
    s = scene(8, twin)
    p = ebs_params(name, s.step, twin)
    return cached_frame(ebs_cache(name, twin), EBS_CASES[name].get("cam", "outside"), W, H,
                        bool(p.apply_occlusion), bool(p.apply_shadow), bool(p.apply_gradient_shading),
                        tuple(p.light_pos), twin)


# ---------------------------------------------------------------------------------------
# crtgt: the ray tables and distances of crtgt_cases.py (21 and 26 steps per ray here too)
# ---------------------------------------------------------------------------------------

#              occlusion, shadow, shadow type, Phong, camera, occlusion rays
CRTGT_CASES = {
    "both_point": (True, True, 0, False, "outside", G.N_OCC),
    "both_dir": (True, True, 2, False, "outside", G.N_OCC),
    "phong_fd": (True, True, 0, True, "outside", G.N_OCC),
    "inside": (True, True, 0, False, "inside", G.N_OCC),
    "occ70": (True, False, 0, False, "outside", G.N_OCC_WIDE),
    # the shadow bundles alone: world-space inputs only (see test_axis_rotation.py)
    "shadow_point": (False, True, 0, False, "outside", G.N_OCC),
    "shadow_dir": (False, True, 2, False, "outside", G.N_OCC),
}


@functools.lru_cache(maxsize=None)
def crtgt_frame(name, W=96, H=80, twin=0):
    """crtgt_ref.render of a CRTGT_CASES entry: (rgba, counts, total), read-only.  The
    ray tables are stored in the cone's own frame (z = its axis), not in world axes:
    a twin reads them unchanged."""
    import crtgt_ref as C
    occ_on, sdw_on, stype, phong, cam, n_occ = CRTGT_CASES[name]
    s = scene(8, twin)
    occ, sdw = G.rays(n_occ)
    return _ro(C.render(s.vol16, s.scale, s.tf, camera(cam, twin), W, H, s.step, light("light0", twin), occ, sdw,
                        apply_occlusion=occ_on, apply_shadow=sdw_on, shadow_type=stype, light_gap=G.LIGHT_GAP,
                        light_step=G.LIGHT_STEP, occ_distance=G.OCC_DISTANCE, sdw_distance=G.SDW_DISTANCE,
                        grad=s.grad if phong else None, phong=phong))
