"""Scenes and cases shared by tests/test_vct.py (CPU) and tests/test_vct_gpu.py; a plain
module, not a conftest.

    cubic      the scene of tests/crtgt_cases.py: Marschner-Lobb 48^3, D.voxel_scale(48) (a box
               512 wide, a voxel 10.67), the bonsai TF, LIGHT0; 6 pyramid levels
    aniso      the scene of tests/aniso_cases.py: voxels (33, 40, 44), scale (9.0, 11.5, 7.25);
               odd dimensions drop voxels at every halving; 6 levels

The cone parameters are chosen so that the CPU reference's own statistics (asserted in
tests/test_vct.py) cover every path of the quadrilinear fetch.  With lambda =
log2(2 xl tan(angle)):

    LEVEL0   angle 0.5 deg, xl <= 48: 2 xl tan <= 0.84, lambda <= 0 throughout (level 0 only);
             6 samples of step 8 stay inside the box for most cones (they run the full count)
    MULTI    angle 10 deg, step 2 growing by 1.5: xl = 3, 5.5, 9.25, 14.9, 23.3, 36, 55, 83.5,
             lambda = 0.08, 0.95, 1.70, 2.39, 3.04, 3.66, 4.27, 4.88: the pairs (0,1) .. (4,5)
    TOP      MULTI with 12 samples: xl = 126, 190, ... gives lambda >= 5 = nl - 1 (the last level
             alone), and cones leave the box before the 12th sample (cut)

References are computed once per session (functools.lru_cache) and shared read-only."""
import ctypes
import functools

import numpy as np

import aniso_cases as A
import crtgt_cases as G
from cpp_volume_rendering_amd import _native as N
from cpp_volume_rendering_amd import datasets as D

INITIAL, INSIDE, MOVED, LIGHT0 = G.INITIAL, G.INSIDE, G.MOVED, G.LIGHT0
FRAMES = G.FRAMES                        # (96, 80) and (77, 53), ragged against the 8x8 tiles
ANISO_FRAME = (77, 53)

DEFAULT = dict(step=2.0, rate=1.0, initial=2.0, angle_deg=2.0, correction=True, factor=2.0, samples=50)
LEVEL0 = dict(step=8.0, rate=1.0, initial=4.0, angle_deg=0.5, correction=True, factor=2.0, samples=6)
MULTI = dict(step=2.0, rate=1.5, initial=2.0, angle_deg=10.0, correction=True, factor=2.0, samples=8)
TOP = dict(MULTI, samples=12)

#        scene, cone, occlusion, shadow, Phong, camera, filter_bits
CASES = {
    "defaults": ("cubic", DEFAULT, True, True, False, INITIAL, 0),
    "level0_only": ("cubic", LEVEL0, True, True, False, INITIAL, 0),
    "multi_level": ("cubic", MULTI, True, True, False, INITIAL, 0),
    "clamped_top": ("cubic", TOP, True, True, False, INITIAL, 0),
    "shadow_only": ("cubic", TOP, False, True, False, INITIAL, 0),
    "occlusion_only": ("cubic", MULTI, True, False, False, INITIAL, 0),
    "correction_off": ("cubic", dict(MULTI, correction=False), True, True, False, INITIAL, 0),
    "samples0": ("cubic", dict(MULTI, samples=0), True, True, False, INITIAL, 0),
    "phong_fd": ("cubic", MULTI, True, True, True, MOVED, 0),
    "inside": ("cubic", TOP, True, True, False, INSIDE, 0),
    "filter8": ("cubic", MULTI, True, True, False, INITIAL, 8),
    "both_off": ("cubic", MULTI, False, False, False, INITIAL, 0),
    "aniso_outside": ("aniso", MULTI, True, True, False, A.OUTSIDE, 0),
    "aniso_inside": ("aniso", TOP, True, True, False, A.INSIDE, 0),
}
# the frames a case is rendered at: both for the cubic scene, one for the other
SHADOWED = ("defaults", "level0_only", "multi_level", "clamped_top", "shadow_only", "phong_fd", "inside",
            "filter8")


def frames(name):
    return FRAMES if CASES[name][0] == "cubic" else (ANISO_FRAME,)


def tf_table():
    """The bonsai TF as TransferFunction1D's double table (256 x 4)."""
    import oracle as O
    return O.tf_table_double(D.BONSAI_TF_RGB, D.BONSAI_TF_ALPHA)


@functools.lru_cache(maxsize=None)
def opacity_lut():
    """GetOpc(i, 255), i < 255, as the library builds it from the control points."""
    rgb = np.ascontiguousarray(np.asarray(D.BONSAI_TF_RGB, np.float64).reshape(-1, 4))
    a = np.ascontiguousarray(np.asarray(D.BONSAI_TF_ALPHA, np.float64).reshape(-1, 2))
    out = np.zeros(255, np.float32)
    N.check(N.lib().cvr_tf1d_opacity_lut(N.dptr(rgb), rgb.shape[0], N.dptr(a), a.shape[0], 255, 255,
                                         N.fptr(out)), "cvr_tf1d_opacity_lut")
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def scene(which, twin=0):
    """(vol u8, scale, vol16, tf_rgbt, FD gradient, default step) of "cubic" or "aniso"."""
    if which == "cubic":
        assert twin == 0
        return G.scene()
    s = A.scene(8, twin)
    return s.vol, s.scale, s.vol16, s.tf, s.grad, s.step


@functools.lru_cache(maxsize=None)
def precomputed(which, twin=0):
    """((levels, max_stddev), table) of a scene by the CPU reference, read-only."""
    import vct_ref as R
    vol = scene(which, twin)[0]
    pyr = R.pyramid(vol)
    tab = R.table(vol, tf_table(), pyr[1])
    for l in pyr[0]:
        l.setflags(write=False)
    tab.setflags(write=False)
    return pyr, tab


def render_ref(which, cone, occ, sdw, phong, cam, fb, W, H, twin=0, light=None):
    import vct_ref as R
    _, scale, vol16, tf, grad, step = scene(which, twin)
    pyr, tab = precomputed(which, twin)
    out = R.render(vol16, scale, tf, cam, W, H, step, light or LIGHT0, pyr, tab, cone, apply_occlusion=occ,
                   apply_shadow=sdw, grad=grad if phong else None, phong=phong, filter_bits=fb)
    out[0].setflags(write=False)
    out[1].setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(name, W, H):
    """The CPU reference's frame of a case: (rgba, counts, total, stats), read-only."""
    which, cone, occ, sdw, phong, cam, fb = CASES[name]
    return render_ref(which, cone, occ, sdw, phong, cam, fb, W, H)


@functools.lru_cache(maxsize=None)
def plain(name, W, H):
    """Plain rc1pass (the oracle) of a case's frame: what the shading is compared with."""
    import oracle as O
    which, _, _, _, _, cam, fb = CASES[name]
    _, scale, vol16, tf, _, step = scene(which)
    rgba, cnt, total = O.render_rc1pass(vol16, scale, tf, cam, W, H, step, filter_bits=fb)
    rgba.setflags(write=False)
    cnt.setflags(write=False)
    return rgba, cnt, total


def assert_shading_visible(name, W, H):
    """The two conditions every shadowed case meets on the reference's own output: the frame
    is not empty, and the shading changes at least 5 % of the composited pixels."""
    rgba = reference(name, W, H)[0]
    base = plain(name, W, H)[0]
    assert rgba[..., 3].max() > 0.5
    comp = base[..., 3] > 0
    diff = np.abs(rgba[..., :3] - base[..., :3]).max(axis=-1) > 1e-3
    assert comp.any() and (diff & comp).sum() >= 0.05 * comp.sum()


def params(name):
    """cvr_vct_params of a case."""
    which, cone, occ, sdw, phong, _, _ = CASES[name]
    p = N.VctParams()
    N.lib().cvr_vct_params_default(ctypes.byref(p))
    p.step = scene(which)[5]
    p.apply_gradient_shading = int(phong)
    for k in ("position", "forward", "up", "right"):
        getattr(p.light, k)[:] = list(LIGHT0[k])
    p.light.spot_angle_deg = LIGHT0["spot_angle_deg"]
    p.apply_occlusion, p.apply_shadow = int(occ), int(sdw)
    p.cone_step, p.cone_step_increase_rate = cone["step"], cone["rate"]
    p.cone_initial_step, p.cone_apex_angle_deg = cone["initial"], cone["angle_deg"]
    p.apply_correction, p.correction_factor = int(cone["correction"]), cone["factor"]
    p.samples = cone["samples"]
    return p
