"""Axis-rotation equivariance of the CPU references (no GPU).

"GPU == reference" compares two restatements that share their axis conventions: a
mix-up made the same way on both sides is bit-exact and wrong.  A symmetry of the scene
needs no second implementation.  R: v -> (v_y, v_z, v_x) is a cyclic relabelling of the
axes, a proper rotation, so the scene of tests/aniso_cases.py and its twin (volume
transpose(2, 0, 1); scale, camera, light, pyramid and cache sizes relabelled) must give
the same picture, the same per-pixel sample counts and, transposed back, the same
pyramid, SAT and light caches.  The scene is anisotropic and non-cubic, so an axis taken
for another moves the result far: every family has a negative control (the twin with the
scale left unrelabelled) that must miss the gate by a wide margin.

The gate is the project's own (tests/test_literal.py assert_gate): at most 0.1 % of
pixels over 2e-3, max at most 2e-2, SSIM at least 0.99.

Two constructions are not rotation-equivariant as the reference writes them, and are
checked for what remains:

  * rc1pdosct/ray_bbox_marching.comp:683  `v_right = normalize(cross(camera_dir, vec3(0, 1, 0)))`
    and rc1pcrtgt/gt_ray_marching.comp:398, the same line: the frame of the occlusion
    cones hangs on the fixed world axis y, which R does not map to itself.  The cone's own
    axis (eye - position) is equivariant, its roll about that axis is not: the 3- and 7-ray
    sections of a DOS occlusion cone and every off-axis ray of a crtgt occlusion bundle
    land elsewhere in the twin.  For those cases the counts and the alpha channel (which
    never read the shading) are held to the check, and the colour is asserted to differ,
    so that the exclusion cannot outlive its reason.  A single-ray occlusion cone
    (max_packing 0) reads its axis alone and is held to the whole gate, as are the shadow
    cones (frame from the light's own vectors), the DOS light cache
    (lightcachecomputation.comp:284 takes EyeCamUp, which rotates with the camera) and
    the crtgt shadow bundles.  The crtgt ray tables are stored in the cone's own frame
    (z = the axis; cvr_crtgt_build_rays rotates (0, 0, 1)), not in world axes, so the twin
    reads them unchanged.

  * the EBS box-chain shadow is equivariant but ill-conditioned to one ulp of its inputs
    (test_literal.py test_ebs_occlusion_and_shadow_conditioning): the relabelled light
    direction normalises with its sum in another order.  Counts, max and SSIM stay inside
    the gate; the share of pixels over 2e-3 is capped at twice what the oracle gives, the
    measurement written beside each cap below."""
import numpy as np
import pytest

import aniso_cases as A
from test_literal import assert_gate, gate


def check_counts(o, t, what):
    assert np.array_equal(o[1], t[1]), f"{what}: per-pixel counts differ"
    assert o[2] == t[2] == int(o[1].sum()) > 0


def check_frame(fn, name, share=None, **kw):
    """The frame of `name` against its twin's: counts identical and the gate (share: the
    cap on the pixels over 2e-3 instead of the gate's 0.1 %)."""
    o, t = fn(name, **kw), fn(name, twin=1, **kw)
    check_counts(o, t, name)
    r = gate(o[0], t[0])
    print(name, r)
    if share is None:
        assert_gate(r, name)
    else:
        assert r["frac_over"] <= share, (name, r)
        assert r["max"] <= 2e-2 and r["ssim"] >= 0.99, (name, r)


def check_alpha_only(fn, name):
    """A case whose colour hangs on the fixed helper axis (module docstring): counts and
    alpha as everywhere, and the colour does differ."""
    o, t = fn(name), fn(name, twin=1)
    check_counts(o, t, name)
    assert np.abs(o[0][..., 3] - t[0][..., 3]).max() <= 2e-3        # measured 2.8e-5
    assert gate(o[0], t[0])["frac_over"] > 0.05, name               # measured 0.27 .. 0.78


def check_control(fn, name, **kw):
    """The twin with the scale left unrelabelled is another scene: measured 0.66 .. 0.91."""
    assert gate(fn(name, **kw)[0], fn(name, twin=2, **kw)[0])["frac_over"] > 0.05, name


# ---------------------------------------------------------------------------------------
# the scene itself
# ---------------------------------------------------------------------------------------

def test_scene_meets_the_conditions_of_the_gpu_cases():
    for cam in A.CAMS:
        for W, H in A.FRAMES:
            A.assert_visible(A.plain(cam, W, H)[0], cam, W, H, shaded=False)
    comp = A.plain()[0][..., 3] > 0
    assert comp.mean() > 0.75                                       # measured 0.80
    half = np.array([n * s / 2 for n, s in zip(A.scene().n_xyz, A.SCALE)])
    assert (np.abs(A.INSIDE["eye"]) < half).all()
    assert (np.abs(A.LIGHT_INSIDE["position"]) < half).all()
    assert (np.abs(A.LIGHT0["position"]) > half).any()
    assert len(set(A.scene().n_xyz)) == len(set(A.SCALE)) == len(set(np.multiply(A.scene().n_xyz, A.SCALE))) == 3


# ---------------------------------------------------------------------------------------
# rc1pass
# ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("phong", [False, True], ids=["plain", "phong_fd"])
def test_rc1pass(phong):
    check_frame(lambda name, **kw: A.plain("outside", 96, 80, phong, **kw), f"rc1pass phong={phong}")


def test_rc1pass_control():
    check_control(lambda name, **kw: A.plain(**kw), "rc1pass")


# ---------------------------------------------------------------------------------------
# the extinction pyramid and the SAT
# ---------------------------------------------------------------------------------------

def test_extinction_pyramid():
    """A level's opacity is q16(sum(w c) / sum(w)) over 7^3 taps summed x outer, z inner
    (extcoefvolumegenerator.cpp:230-408): the twin sums in another order, the float sums
    differ by rounding and the binary16 result flips by at most one unit, 2^-11 below 1.
    tau = q16(-log(1 - o)) carries that as 2^-11 / (1 - o) = 2^-11 exp(tau), plus one
    unit of its own rounding (2^-10 below 2; the levels stay under 1.7).  The oracle
    gives: 0.042 % and 0.052 % of the texels of levels 0 and 1 differ (by 2^-9 at most),
    none on the coarser levels; the share is capped at twice that."""
    a, b = A.pyramid(), A.pyramid(twin=1)
    assert len(a) == len(b) == 6
    for L, (x, y) in enumerate(zip(a, b)):
        assert y.shape == tuple(A.R(x.shape[::-1]))[::-1]
        y = A.back(y)
        assert x.shape == y.shape and x.max() < 2.0
        d = np.abs(x - y)
        assert (d <= 2.0 ** -11 * np.exp(np.maximum(x, y).astype(np.float64)) + 2.0 ** -10).all(), L
        assert (d > 0).mean() <= 2 * 0.00052, (L, (d > 0).mean())
    # control: the twin's scale left alone filters another box
    c = A.back(A.pyramid(twin=2)[0])
    assert (np.abs(a[0] - c) > 2e-3).mean() > 0.05                  # measured 0.14


def test_sat():
    """BuildSAT sums lut[voxel] (floats) in double: with 58080 cells of 24-bit values
    the sums round little or not at all, so the order of the axes can move a double by a
    few of its units and the float SAT by one float unit at the most.  The oracle gives:
    identical, every cell."""
    (lut, a), (lut1, b) = A.sat(), A.sat(twin=1)
    assert np.array_equal(lut, lut1)
    b = A.back(b)
    assert a.shape == b.shape == (46, 42, 35)
    assert (np.abs(a - b) <= np.spacing(np.maximum(a, b))).all()
    assert a.max() > 5e4


# ---------------------------------------------------------------------------------------
# DOS
# ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["occ1_point", "occ1_dir", "occ1_phong", "shadow_only"])
def test_dos_frame(name):
    A.assert_visible(A.dos_frame(name)[0])
    check_frame(A.dos_frame, name)


@pytest.mark.parametrize("name", ["both_point", "occ7"])
def test_dos_frame_with_multi_ray_occlusion(name):
    check_alpha_only(A.dos_frame, name)


def test_dos_frame_control():
    check_control(A.dos_frame, "occ1_point")


def cache_diff(a, b):
    """Per channel, the share of voxels whose decoded binary16 differ by more than 2e-3."""
    d = np.abs(a.view(np.float16).astype(np.float64) - A.back(b).view(np.float16))
    return [(d[..., k] > 2e-3).mean() for k in (0, 1)]


@pytest.mark.parametrize("name", ["both_point", "both_spot", "both_dir", "inside"])
def test_dos_cache(name):
    """The occlusion cones of the cache take their frame from EyeCamUp
    (lightcachecomputation.comp:284), which rotates with the camera: 3-ray sections
    included, the whole cache is equivariant.  Measured: no voxel past 6e-8."""
    a, b = A.dos_cache(name), A.dos_cache(name, 1)
    assert b.shape == tuple(A.R(A.DOS_DIMS))[::-1] + (2,)
    for share in cache_diff(a, b):
        assert share <= 1e-3
    # the compared terms are not constant (from the inside eye every occlusion cone runs
    # its whole length through the volume: that channel alone is all 0.0)
    live = a[..., [1] if name == "inside" else [0, 1]]
    assert ((live != 0) & (live != 0x3C00)).mean() >= 0.05


def test_dos_cache_control():
    shares = cache_diff(A.dos_cache("both_point"), A.dos_cache("both_point", 2))
    assert min(shares) > 0.05                                       # measured 0.136, 0.063


@pytest.mark.parametrize("name", ["both_point", "both_dir", "inside"])
def test_dos_cached_frame(name):
    A.assert_visible(A.dos_cached_frame(name)[0], A.DOS_CASES[name][4])
    check_frame(A.dos_cached_frame, name)


def test_dos_cached_frame_control():
    check_control(A.dos_cached_frame, "both_point")


# ---------------------------------------------------------------------------------------
# EBS
# ---------------------------------------------------------------------------------------

# the share of pixels over 2e-3 the oracle gives for each case with the box-chain shadow
# on (of 7680 pixels), and the cap: twice that, or the gate's own 0.1 % where it is more
EBS_SHADOW_SHARE = {
    "defaults_point": 11 / 7680,      # 0.143 %  -> cap 0.286 %
    "directional": 11 / 7680,         # 0.143 %  -> cap 0.286 %
    "shadow_only": 37 / 7680,         # 0.482 %  -> cap 0.964 %
    "shadow_dir_only": 44 / 7680,     # 0.573 %  -> cap 1.146 %
    "wide_cone": 0.0,                 # none     -> the gate's 0.1 %
    "light_inside": 0.0,              # none     -> the gate's 0.1 %
}


@pytest.mark.parametrize("name", ["occlusion_only"])
def test_ebs_frame(name):
    A.assert_visible(A.ebs_frame(name)[0])
    check_frame(A.ebs_frame, name)


@pytest.mark.parametrize("name", sorted(EBS_SHADOW_SHARE))
def test_ebs_frame_with_shadow(name):
    A.assert_visible(A.ebs_frame(name)[0])
    check_frame(A.ebs_frame, name, share=max(1e-3, 2 * EBS_SHADOW_SHARE[name]))


def test_ebs_frame_control():
    check_control(A.ebs_frame, "occlusion_only")


# the share of the cache's 350 voxels whose shadow differs by more than 2e-3: the oracle
# gives one voxel for the directional light (0.0044 apart), none otherwise
EBS_CACHE_SHADOW_SHARE = {"defaults_point": 0.0, "directional": 1 / 350, "wide_cone": 0.0,
                          "light_inside": 0.0}


@pytest.mark.parametrize("name", sorted(EBS_CACHE_SHADOW_SHARE))
def test_ebs_cache(name):
    a, b = A.ebs_cache(name), A.ebs_cache(name, 1)
    assert b.shape == tuple(A.R(A.EBS_DIMS))[::-1] + (2,)
    occ, sdw = cache_diff(a, b)
    assert occ <= 1e-3                                              # measured: none past 4.9e-4
    assert sdw <= max(1e-3, 2 * EBS_CACHE_SHADOW_SHARE[name])
    assert ((a != 0) & (a != 0x3C00)).mean() >= 0.05


def test_ebs_cache_control():
    """The occlusion shells are sized in voxels and so do not read the scale; the shadow
    chain does."""
    _, sdw = cache_diff(A.ebs_cache("defaults_point"), A.ebs_cache("defaults_point", 2))
    assert sdw > 0.05                                               # measured 0.31


@pytest.mark.parametrize("name", ["defaults_point", "directional", "light_inside"])
def test_ebs_cached_frame(name):
    """The cache smooths the chain's jumps: the whole gate holds (measured: no pixel past
    2.2e-4)."""
    A.assert_visible(A.ebs_cached_frame(name)[0])
    check_frame(A.ebs_cached_frame, name)


def test_ebs_cached_frame_control():
    check_control(A.ebs_cached_frame, "defaults_point")


# ---------------------------------------------------------------------------------------
# crtgt
# ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["shadow_point", "shadow_dir"])
def test_crtgt_frame(name):
    A.assert_visible(A.crtgt_frame(name)[0])
    check_frame(A.crtgt_frame, name)


@pytest.mark.parametrize("name", ["both_point", "occ70"])
def test_crtgt_frame_with_occlusion(name):
    check_alpha_only(A.crtgt_frame, name)


def test_crtgt_frame_control():
    check_control(A.crtgt_frame, "shadow_point")
