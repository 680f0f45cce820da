"""Scenes and cases shared by tests/test_deferred.py (CPU) and tests/test_deferred_gpu.py; a
plain module, not a conftest.

Scenes are those of tests/sbtm_cases.py: "small8" (Marschner-Lobb, 17 x 20 x 24 voxels as
(x, y, z), scale (1, 1.25, 0.75): the box 17 x 25 x 18), "small16" (its 16-bit twin), "aniso"
(33 x 40 x 44 voxels, scale (9, 11.5, 7.25)) and "mirror" (aniso with x and z swapped).

Frames: 41 x 37 (the lighting pass's fetch is shifted in six columns and four rows, and no
tile size divides it), 48 x 40 (no shift) and 96 x 80 (several 8 x 8 tiles a side; one case).

The cameras were picked on the CPU reference so that the conditions asserted in
tests/test_deferred.py hold: at least 20 % hits, an in-box miss and a background pixel in every
non-empty frame, and every hit within one step_small of a crossing of the trilinear density.
The last one is no property of the loop (a long step can cross the surface): under
sbtm_cases.FAR a few hits of a frame lay further, under the cameras below none does.  References are computed once per session
(functools.lru_cache) and shared read-only."""
import ctypes
import functools

import sbtm_cases as S
from cpp_volume_rendering_amd import _native as N

FRAMES = ((41, 37), (48, 40))
TILES = (96, 80)
SHIFTED_COLUMNS = {41: (1, 2, 4, 8, 16, 32), 37: (3, 6, 12, 24), 40: (), 48: (), 64: (), 80: (), 96: ()}

FRONT = dict(eye=(0.0, 5.6, 31.5), center=(0.5, -0.5, 1.0), up=(0.0, 1.0, 0.0))    # the whole box, background around it
BELOW = dict(eye=(0.0, -10.9, 30.1), center=(0.5, -0.5, 1.0), up=(0.0, 1.0, 0.0))
MOVED = S.MOVED
# inside the box (half sizes 8.5, 12.5, 9): tnear clamps to 0 and no ray misses the box
INSIDE = dict(eye=(-4.0, -6.0, 0.0), center=(-20.0, 2.0, 5.0), up=(0.0, 1.0, 0.0))
# nearer: the sparser surface of "high_iso" still fills 20 % of the frame
CLOSE = dict(eye=(15.0, 9.5, 25.0), center=(0.5, -0.5, 1.0), up=(0.0, 1.0, 0.0))
ANISO_CAM = dict(eye=(-300.0, 120.0, 420.0), center=(10.0, -5.0, 20.0), up=(0.0, 1.0, 0.0))

#        scene, camera, parameters (over deferred_ref.DEFAULTS)
CASES = {
    "defaults": ("small8", FRONT, {}),
    "u16": ("small16", FRONT, {}),
    "long_step": ("small8", MOVED, dict(step_large=3.0, step_range=0.3)),
    "blocks1": ("small8", FRONT, dict(num_blocks=(1, 1, 1))),
    "blocks8": ("small8", BELOW, dict(num_blocks=(8, 8, 8))),
    "high_iso": ("small8", CLOSE, dict(isovalue=0.8)),
    "empty": ("small8", FRONT, dict(isovalue=1.5)),
    "exposure0": ("small8", FRONT, dict(exposure=0.0)),
    "gamma0": ("small8", BELOW, dict(gamma=0.0)),
    "no_tone_map": ("small8", FRONT, dict(exposure=0.0, gamma=0.0)),
    "alpha": ("small8", FRONT, dict(color=(0.66, 0.6, 0.05, 0.5))),
    "inside": ("small8", INSIDE, {}),
    "clear": ("small8", FRONT, dict(gbuffer_clear=(0.25, 0.5, 0.125, 0.75))),
    "aniso": ("aniso", ANISO_CAM, dict(step_small=0.5, step_large=10.0, step_range=0.1)),
}
EMPTY = ("empty",)                           # every in-box ray misses by construction
NO_OFF_BOX = ("inside",)                     # from inside a convex box every ray is in it
NO_SKIP = ("blocks1",)                       # one block holds the whole range: nothing is skippable
# three light / material / tone-map settings for the relight path (over a case's parameters)
RELIGHT = (
    dict(light_pos=(40.0, 60.0, -20.0), ka=0.2, kd=0.9, ks=0.4, shininess=8.0),
    dict(color=(0.1, 0.7, 0.9, 0.75), light_color=(1.0, 0.5, 0.25), exposure=2.5, gamma=1.0),
    dict(light_pos=(-15.0, -30.0, 25.0), exposure=0.0, gamma=0.0, ks=0.0),
)


def frames(name):
    if name == "defaults":
        return FRAMES + (TILES,)
    return (FRAMES[1],) if CASES[name][0] == "aniso" else FRAMES


def all_frames():
    return [(n, W, H) for n in CASES for (W, H) in frames(n)]


scene = S.scene


def merged(name, extra=None):
    """A case's parameters over the defaults, `extra` over those."""
    import deferred_ref as R
    return {**R.DEFAULTS, **CASES[name][2], **(extra or {})}


@functools.lru_cache(maxsize=None)
def _reference(name, W, H, extra):
    import deferred_ref as R
    which, cam, par = CASES[name]
    s = scene(which)
    return R.render(s.vol16, s.vol, s.scale, cam, W, H, dict(par, **dict(extra)))


def reference(name, W, H, extra=None):
    """The CPU reference's frame of a case (deferred_ref.render's namespace), read-only."""
    return _reference(name, W, H, tuple(sorted((extra or {}).items())))


def params(name, extra=None):
    """cvr_deferred_params of a case."""
    q = merged(name, extra)
    p = N.DeferredParams()
    N.lib().cvr_deferred_params_default(ctypes.byref(p))
    p.isovalue, p.step_small, p.step_large, p.step_range = (q[k] for k in ("isovalue", "step_small", "step_large",
                                                                           "step_range"))
    p.num_blocks[:] = q["num_blocks"]
    p.color[:] = q["color"]
    p.ka, p.kd, p.ks, p.shininess = q["ka"], q["kd"], q["ks"], q["shininess"]
    p.light_color[:] = q["light_color"]
    p.light_pos[:] = q["light_pos"]
    p.exposure, p.gamma = q["exposure"], q["gamma"]
    p.gbuffer_clear[:] = q["gbuffer_clear"]
    return p
