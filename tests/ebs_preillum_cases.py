"""Scene and cases shared by tests/test_ebs_preillum.py (CPU) and
tests/test_ebs_preillum_gpu.py: test_ebs_gpu.py's own setup (Marschner-Lobb 40^3,
D.voxel_scale(40), the bonsai TF, oracle.sat_build), built once per session."""
import functools

import numpy as np

from cpp_volume_rendering_amd import _native as N
from cpp_volume_rendering_amd import datasets as D

N_VOX = 40
INITIAL = D.INITIAL_STATE_CAMERA
# EBS_CASES["ragged_inside"] of test_ebs_gpu.py: the eye inside the box
INSIDE = dict(eye=(10.0, -20.0, 30.0), center=(100.0, 50.0, -200.0), up=(0.0, 1.0, 0.0))
# test_ebs_gpu.py's light
LIGHT_POS = (-206.873, -51.0699, 557.011)
LIGHT_FWD = (-0.346883, -0.0856335, 0.933991)
# a point light inside the box (+-256) and off every voxel centre of both cache sizes:
# the voxels around it take all three chain axes, both signs, and unequal chain lengths
LIGHT_INSIDE = (5.3, 3.1, -4.7)
# ragged on every axis against any power-of-two block, and one whole number of 4^3 blocks
CACHE_DIMS = ((10, 7, 5), (16, 16, 16))

# keyword arguments of ebs_params below (test_ebs_gpu.ebs_params' names and values)
CASES = {
    "defaults_point": dict(),
    "occlusion_only": dict(apply_shadow=False),
    "shadow_only": dict(apply_occlusion=False),
    "directional": dict(shadow_type=1),
    "wide_cone": dict(angle=12.0, interval=3.0, initial=1.0, weight=0.7, shells=6, radius=1.5,
                      max_distance=150.0),
    # cone angles past 44 deg take the IEEE division for the cone edges (ebs_sat.h cone_div)
    "cone_60": dict(angle=60.0, max_distance=60.0),
    "cone_89": dict(angle=89.0, max_distance=40.0, apply_occlusion=False),
    "light_inside": dict(light=LIGHT_INSIDE),
}


def ebs_params(step=0.0, apply_occlusion=True, apply_shadow=True, shadow_type=0, phong=False,
               shells=15, radius=1.0, angle=1.0, interval=2.0, initial=2.0, weight=1.0,
               max_distance=0.0, light=LIGHT_POS, light_forward=LIGHT_FWD):
    p = N.EbsParams()
    p.step = step
    p.apply_gradient_shading = int(phong)
    p.ka, p.kd, p.ks, p.shininess = 0.5, 0.5, 0.8, 30.0
    p.ispecular[:] = [1.0, 1.0, 1.0]
    p.light_pos[:] = list(light)
    p.light_forward[:] = list(light_forward)
    p.apply_occlusion, p.occlusion_shells, p.occlusion_radius = int(apply_occlusion), shells, radius
    p.apply_shadow, p.shadow_type = int(apply_shadow), shadow_type
    p.shadow_cone_angle_deg, p.shadow_sample_interval = angle, interval
    p.shadow_initial_step, p.shadow_ui_weight, p.shadow_max_distance = initial, weight, max_distance
    return p


@functools.lru_cache(maxsize=None)
def scene():
    """(vol u8, scale, vol16, tf_rgbt, ext lut, float SAT, FD gradient): computed once."""
    import oracle as O
    from test_ebs import lib_ext_lut
    vol = D.marschner_lobb_u8(N_VOX)
    scale = D.voxel_scale(N_VOX)
    tf = O.tf_rgbt(O.tf_table_double(D.BONSAI_TF_RGB, D.BONSAI_TF_ALPHA))
    lut = lib_ext_lut(1)
    sat = O.sat_build(vol, lut).astype(np.float32)
    sat.setflags(write=False)
    return vol, scale, O.volume_r16f(vol), tf, lut, sat, O.gradient(vol, "fd")


@functools.lru_cache(maxsize=None)
def ref_cache(name, dims, filter_bits=0):
    """The reference light cache of a CASES entry: (dz, dy, dx, 2) uint16, read-only."""
    import ebs_lightcache_ref as R
    c = CASES[name]
    _, scale, _, _, _, sat, _ = scene()
    out = R.ebs_cache((N_VOX,) * 3, scale, sat, dims, c.get("light", LIGHT_POS), LIGHT_FWD,
                      apply_occlusion=c.get("apply_occlusion", True), occ_shells=c.get("shells", 15),
                      occ_radius=c.get("radius", 1.0), apply_shadow=c.get("apply_shadow", True),
                      shadow_type=c.get("shadow_type", 0), cone_angle_deg=c.get("angle", 1.0),
                      interval=c.get("interval", 2.0), initial_step=c.get("initial", 2.0),
                      ui_weight=c.get("weight", 1.0), max_distance=c.get("max_distance") or None,
                      filter_bits=filter_bits)
    out.setflags(write=False)
    return out
