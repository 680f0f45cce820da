"""Properties of the EBS light cache's CPU reference alone (tests/support/
ebs_lightcache_ref.cpp over the pinned oracle's Sat / ebs_occlusion / cone_x|y|z), which
tests/test_ebs_preillum_gpu.py compares the GPU against as bit patterns: the reference
holds no NaN, every term that is on varies over the cache, the inside light exercises all
three chain axes, and a switched-off term is exactly 1.0."""
import numpy as np
import pytest

import ebs_preillum_cases as C

ONE = 0x3C00     # binary16 1.0


def halfs(cache):
    return cache.view(np.float16).astype(np.float32)


@pytest.mark.parametrize("dims", C.CACHE_DIMS, ids=lambda d: "x".join(map(str, d)))
@pytest.mark.parametrize("name", sorted(C.CASES))
def test_reference_cache_properties(name, dims):
    case = C.CASES[name]
    cache = C.ref_cache(name, dims)
    assert cache.shape == (dims[2], dims[1], dims[0], 2) and cache.dtype == np.uint16
    v = halfs(cache)
    assert not np.isnan(v).any()                      # bit patterns are compared: no NaN
    # (a value may exceed 1.0 by rounding: a box sum is a difference of eight float SAT
    # fetches and can come out slightly negative over empty space)
    assert np.isfinite(v).all() and (v >= 0.0).all()
    for ch, on in ((0, case.get("apply_occlusion", True)), (1, case.get("apply_shadow", True))):
        if on:
            share = ((v[..., ch] > 0.0) & (v[..., ch] < 1.0)).mean()
            print(f"{name} {dims} channel {ch}: {share:.3f} strictly inside (0, 1)")
            assert share >= 0.05
        else:
            assert (cache[..., ch] == ONE).all()      # a switched-off term is exactly 1.0


@pytest.mark.parametrize("dims", C.CACHE_DIMS, ids=lambda d: "x".join(map(str, d)))
def test_light_inside_takes_every_chain_axis(dims):
    """Per voxel, the dominant axis of light - realpos by the shader's own test
    (lightcachecomputation.comp:426-437): each axis is taken by >= 10 % of the voxels,
    so within the 4^3 voxels around the light one wave runs all three chains."""
    f = np.float32
    scale = C.scene()[1]
    idx = [np.arange(d, dtype=f) for d in dims]
    vs = [f(scale[i]) * (f(C.N_VOX) / f(dims[i])) for i in range(3)]
    half = [f(C.N_VOX) * f(scale[i]) * f(0.5) for i in range(3)]
    pos = [(idx[i] + f(0.5)) * vs[i] - half[i] for i in range(3)]
    z, y, x = np.meshgrid(pos[2], pos[1], pos[0], indexing="ij")
    ax, ay, az = (np.abs(f(C.LIGHT_INSIDE[i]) - p) for i, p in enumerate((x, y, z)))
    is_z = (az > ax) & (az > ay)
    is_y = ~is_z & (ay > ax)
    is_x = ~is_z & ~is_y
    for name, m in (("x", is_x), ("y", is_y), ("z", is_z)):
        print(f"light_inside {dims}: axis {name} {m.mean():.3f}")
        assert m.mean() >= 0.10
    # the light lies inside the volume box
    assert all(abs(C.LIGHT_INSIDE[i]) < float(half[i]) for i in range(3))


def test_reference_filter_bits_changes_the_cache():
    """CVR-SPEC-8 weights reach the SAT fetches of the cache (the GPU test compares both)."""
    a = C.ref_cache("defaults_point", C.CACHE_DIMS[0])
    b = C.ref_cache("defaults_point", C.CACHE_DIMS[0], 8)
    assert not np.isnan(halfs(b)).any()
    assert (a != b).any()
