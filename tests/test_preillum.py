"""Pre-illumination of the DOS renderer, CPU side: the reference restatement
(tests/support/lightcache_ref.cpp: lightcachecomputation.comp and obj_ray_marching.comp
over the oracle's own cone code) builds and has the properties the shaders have, and the
new C-ABI entry points exist and refuse a null context.  The GPU kernels are compared
with this reference bit for bit in tests/test_preillum_gpu.py."""
import ctypes

import numpy as np
import pytest

import lightcache_ref as R
import preillum_cases as C
from cpp_volume_rendering_amd import _native as N
from cpp_volume_rendering_amd.renderer import default_cone_params

ONE = 0x3C00   # binary16 1.0


def as_float(cache):
    return cache.view(np.float16).astype(np.float32)


def test_reference_builds():
    L = R.lib()
    assert hasattr(L, "lcref_dos_cache") and hasattr(L, "lcref_render_rows")


@pytest.mark.parametrize("dims", C.CACHE_DIMS)
def test_empty_pyramid_gives_full_visibility(dims):
    """No extinction anywhere: every cone sums to 0 and exp(-0) = 1, exactly."""
    _, scale, vol16, _, _, levels, _ = C.scene()
    zero = [np.zeros_like(l) for l in levels]
    for occ in (default_cone_params(True), C.occ7()):   # 3-ray and 7-ray averages
        c = R.dos_cache(vol16, scale, zero, C.INITIAL, dims, C.cone_tables(occ, 0.50),
                        C.cone_tables(default_cone_params(False), 0.75), C.LIGHT0,
                        apply_occlusion=True, apply_shadow=True, shadow_type=0)
        assert c.shape == (dims[2], dims[1], dims[0], 2)
        assert (c == ONE).all()


@pytest.mark.parametrize("dims", C.CACHE_DIMS)
def test_switched_off_terms_are_one(dims):
    occ_only = C.ref_cache("occlusion", dims)
    sdw_only = C.ref_cache("shadow_only", dims)
    assert (occ_only[..., 1] == ONE).all() and (sdw_only[..., 0] == ONE).all()
    assert (occ_only[..., 0] != ONE).any() and (sdw_only[..., 1] != ONE).any()


@pytest.mark.parametrize("dims", C.CACHE_DIMS)
def test_spot_light_cone(dims):
    """A voxel outside the spot cone stores exactly 0.0; inside it the spot cache is the
    point light's.  The chosen light leaves at least 5 % of the voxels on either side."""
    spot = C.ref_cache("both_spot", dims)[..., 1]
    point = C.ref_cache("both_point", dims)[..., 1]
    assert (spot == 0).mean() >= 0.05 and (spot != 0).mean() >= 0.05
    # the cone test in double, voxels within 1e-4 of the edge left to either side
    _, scale, *_ = C.scene()
    G = np.array([C.N_VOX * s for s in scale])
    idx = np.stack(np.meshgrid(*[np.arange(d) for d in dims[::-1]], indexing="ij"), -1)[..., ::-1]
    wp = (idx + 0.5) * (G / np.array(dims)) - G / 2
    k = np.array(C.LIGHT0["position"]) - wp
    k /= np.linalg.norm(k, axis=-1, keepdims=True)
    cos = k @ np.array(C.LIGHT0["forward"])
    edge = np.cos(np.pi * C.LIGHT0["spot_angle_deg"] / 180.0)
    outside, inside = cos < edge - 1e-4, cos > edge + 1e-4
    assert outside.mean() >= 0.05 and inside.mean() >= 0.05
    assert (spot[outside] == 0).all()
    assert (point[outside] != 0).any()          # the cut-off changes voxels the light reaches
    assert np.array_equal(spot[inside], point[inside])
    assert (spot[inside] != 0).any()


@pytest.mark.parametrize("name", sorted(C.CACHE_CASES))
def test_values_are_visibilities(name):
    for dims in C.CACHE_DIMS:
        f = as_float(C.ref_cache(name, dims))
        assert np.isfinite(f).all() and (f >= 0.0).all() and (f <= 1.0).all()


def test_more_weight_never_raises_visibility():
    """Doubling ui_weight doubles every cone's optical depth (exactly, a power of two):
    no voxel gets brighter."""
    dims = C.CACHE_DIMS[0]
    _, scale, vol16, _, _, levels, _ = C.scene()
    out = []
    for w in (1.0, 2.0):
        occ, sdw = default_cone_params(True), default_cone_params(False)
        occ.ui_weight *= w
        sdw.ui_weight *= w
        out.append(as_float(R.dos_cache(vol16, scale, levels, C.INITIAL, dims, C.cone_tables(occ, 0.50),
                                        C.cone_tables(sdw, 0.75), C.LIGHT0, apply_occlusion=True,
                                        apply_shadow=True, shadow_type=0)))
    assert (out[1] <= out[0]).all() and (out[1] < out[0]).any()


def test_march_without_shading_composites_nothing():
    """obj_ray_marching.comp:312 `src.a > 0 && Shade`: with occlusion and shadow off the
    frame stays (0, 0, 0, 0) and no ray terminates early, but every iteration counts."""
    _, scale, vol16, tf, _, _, _ = C.scene()
    import oracle as O
    step = O.default_step(scale)
    cache = C.ref_cache("both_point", C.CACHE_DIMS[0])
    W, H = 77, 53
    rgba, cnt, total = R.render(vol16, scale, tf, cache, C.INITIAL, W, H, step, C.LIGHT0,
                                apply_occlusion=False, apply_shadow=False)
    assert not rgba.any()
    assert total == int(cnt.sum()) > 0
    on = R.render(vol16, scale, tf, cache, C.INITIAL, W, H, step, C.LIGHT0, apply_occlusion=True,
                  apply_shadow=True)
    assert on[0][..., 3].max() > 0.5
    # shaded rays stop at the opacity threshold, unshaded ones run through the box
    assert (cnt >= on[1]).all() and total > on[2]
    # the plain march's counts without its early termination: a TF without opacity
    tf0 = tf.copy()
    tf0[:, 3] = 0.0
    _, c0, s0 = O.render_rc1pass(vol16, scale, tf0, C.INITIAL, W, H, step)
    assert np.array_equal(cnt, c0) and total == s0


def test_abi_null_context_and_symbols():
    L = N.lib()
    dims = (ctypes.c_int * 3)(32, 32, 32)
    assert L.cvr_compute_light_cache_dosct(None, None, None, dims) == N.CVR_ERR_ARG
    assert L.cvr_set_light_cache(None, None, dims) == N.CVR_ERR_ARG
    assert L.cvr_copy_light_cache(None, None, 0, dims) == N.CVR_ERR_ARG
    assert L.cvr_render_preillum(None, None, None, None) == N.CVR_ERR_ARG
    assert L.cvr_render_dosct_preillum(None, None, None, dims, None) == N.CVR_ERR_ARG
    assert L.cvr_get_option(None, b"light_cache_builds") == -1
