"""What each state setter drops, through the C ABI alone.

One context carries every piece of state derived from (volume, TF): the gradient, the
DOS extinction pyramid, the EBS SAT, a DOS light cache, a ground-truth frame in
progress, the VCT opacities / pyramid / table and the isosurface block table.  Then:

                 new TF                                   new volume
    skip flags   invalid (cell_flags_valid 0)             invalid
    pyramid      kept (its own RGBA TF)                   freed
    SAT          kept (its own extinction LUT)            freed
    light cache  dropped                                  dropped
    gt frame     ended                                    ended
    VCT          opacities + table dropped, pyramid kept  everything dropped
    iso blocks   unaffected                               rebuilt, same picture

The smallest shapes that still build every structure: an 8 x 6 x 5 u8 volume with
scale (1, 1.5, 2), 16 x 16 frames, a 4^3 extinction pyramid, a 2^3 light cache."""
import ctypes

import numpy as np
import pytest

from cpp_volume_rendering_amd import _native as N
from cpp_volume_rendering_amd import datasets as D
from cpp_volume_rendering_amd.renderer import (Camera, Device, build_crtgt_rays, build_ext_lut,
                                               build_opacity_lut, build_tf_rgbt, default_cone_params,
                                               make_frame)

pytestmark = pytest.mark.gpu

W = H = 16
SCALE = (1.0, 1.5, 2.0)
EXT_RES = (4, 4, 4)
LC_DIMS = (2, 2, 2)
STATE = N.CVR_ERR_STATE


def volume():
    z, y, x = np.meshgrid(np.arange(5), np.arange(6), np.arange(8), indexing="ij")
    return ((x * 37 + y * 53 + z * 91) % 256).astype(np.uint8)      # (D, H, W) = (5, 6, 8)


def dos_params():
    p = N.DosParams()
    p.ka, p.kd, p.ks, p.shininess = 0.5, 0.5, 0.8, 30.0
    p.ispecular[:] = [1.0, 1.0, 1.0]
    p.light.position[:] = list(D.LIGHT_LIST0_POSITION)
    p.apply_occlusion, p.apply_shadow = 1, 1
    p.occlusion, p.shadow = default_cone_params(True), default_cone_params(False)
    return p


def ebs_params():
    p = N.EbsParams()
    p.ka, p.kd, p.ks, p.shininess = 0.5, 0.5, 0.8, 30.0
    p.ispecular[:] = [1.0, 1.0, 1.0]
    p.light_pos[:] = list(D.LIGHT_LIST0_POSITION)
    p.apply_occlusion, p.occlusion_shells, p.occlusion_radius = 1, 3, 1.0
    p.apply_shadow, p.shadow_type = 1, 0
    p.shadow_cone_angle_deg, p.shadow_sample_interval = 1.0, 2.0
    p.shadow_initial_step, p.shadow_ui_weight = 2.0, 1.0
    return p


def crtgt_params():
    p = N.CrtgtParams()
    N.lib().cvr_crtgt_params_default(ctypes.byref(p))
    p.apply_occlusion, p.apply_shadow = 1, 1
    return p


def vct_params():
    p = N.VctParams()
    N.lib().cvr_vct_params_default(ctypes.byref(p))
    p.samples = 4
    return p


def iso_params():
    p = N.IsoParams()
    N.lib().cvr_iso_params_default(0, ctypes.byref(p))
    return p


class Scene:
    """The context and what the calls below share."""

    def __init__(self, dev):
        self.dev, self.L = dev, N.lib()
        self.frame = make_frame(Camera(eye=(14.0, 11.0, 22.0)), W, H)
        self.lc_dims = (ctypes.c_int * 3)(*LC_DIMS)
        self.occ, self.sdw = build_crtgt_rays(90.0, 1, 1.0, 1)
        self.opacity = build_opacity_lut(D.BONSAI_TF_RGB, D.BONSAI_TF_ALPHA)

    def render(self, entry, p):
        """Status and image of one host-output frame."""
        rgba = np.zeros((H, W, 4), np.float32)
        out = N.Output(rgba.ctypes.data, None, None, 0, N.FORMAT_RGBA32F)
        st = getattr(self.L, entry)(self.dev.handle, ctypes.byref(self.frame), ctypes.byref(p),
                                    ctypes.byref(out))
        return st, rgba

    def advance(self):
        left = ctypes.c_ulonglong()
        return self.L.cvr_crtgt_advance(self.dev.handle, 1, None, ctypes.byref(left))

    def option(self, key):
        return self.L.cvr_get_option(self.dev.handle, key)

    def error(self):
        return (self.L.cvr_last_error(self.dev.handle) or b"").decode()

    def light_cache_and_gt_frame(self):
        """The two pieces both setters drop: (re)built before each of them."""
        self.dev.compute_light_cache(self.frame, dos_params(), LC_DIMS)
        self.dev.crtgt_begin(self.frame, crtgt_params(), self.occ, self.sdw)

    def copies(self):
        """Statuses of the three copy entry points (sizes only: no output buffer)."""
        h, dims, nl = self.dev.handle, (ctypes.c_int * 3)(), ctypes.c_int()
        return (self.L.cvr_copy_extinction_sat(h, None, 0, dims),
                self.L.cvr_copy_extinction_level(h, 0, None, dims, ctypes.byref(nl)),
                self.L.cvr_copy_light_cache(h, None, 0, dims))


def test_what_a_new_tf_and_a_new_volume_drop():
    vol = volume()
    tf = build_tf_rgbt(D.BONSAI_TF_RGB, D.BONSAI_TF_ALPHA)
    tf_rgba = build_tf_rgbt(D.BONSAI_TF_RGB, D.BONSAI_TF_ALPHA, extinction_input=True)
    assert tf.shape == (256, 4)
    ext_lut = build_ext_lut(D.BONSAI_TF_RGB, D.BONSAI_TF_ALPHA)
    dev = Device(0)
    try:
        s = Scene(dev)
        # every piece of derived state, on one context
        dev.set_volume(vol, SCALE)
        dev.set_transfer_function(tf)
        dev.set_gradient(N.GRADIENT_FINITE_DIFFERENCES)
        dev.set_extinction_volume(tf_rgba, EXT_RES, 1.0)
        dev.set_extinction_sat(ext_lut)
        dev.vct_set_opacity(s.opacity)
        dev.vct_precompute()
        s.light_cache_and_gt_frame()
        for entry, p in (("cvr_render_dosct", dos_params()), ("cvr_render_extbsd", ebs_params()),
                         ("cvr_render_preillum", dos_params()), ("cvr_render_vct", vct_params())):
            st, _ = s.render(entry, p)
            assert st == N.CVR_OK, (entry, s.error())
        st, iso_before = s.render("cvr_render_iso", iso_params())
        assert st == N.CVR_OK, s.error()
        assert (iso_before[..., 3] > 0).any()              # the isosurface is in view
        assert s.advance() == N.CVR_OK
        assert s.copies() == (N.CVR_OK, N.CVR_OK, N.CVR_OK)
        assert s.option(b"cell_flags_valid") == 1          # built by the frames above
        builds = s.option(b"vct_pyramid_builds")
        assert builds == 1

        # ---- a new transfer function
        dev.set_transfer_function(tf * np.float32(0.5))
        assert s.option(b"cell_flags_valid") == 0
        assert s.render("cvr_render_dosct", dos_params())[0] == N.CVR_OK, s.error()
        assert s.render("cvr_render_extbsd", ebs_params())[0] == N.CVR_OK, s.error()
        assert s.render("cvr_render_preillum", dos_params())[0] == STATE
        assert s.advance() == STATE
        assert s.render("cvr_render_vct", vct_params())[0] == STATE
        assert "cvr_vct_set_opacity" in s.error()
        assert s.option(b"vct_pyramid_builds") == builds
        sat, level, cache = s.copies()
        assert (sat, level, cache) == (N.CVR_OK, N.CVR_OK, STATE)

        # ---- a new volume (the same voxels), with the dropped pieces built again first
        dev.vct_set_opacity(s.opacity)
        s.light_cache_and_gt_frame()
        assert s.render("cvr_render_preillum", dos_params())[0] == N.CVR_OK, s.error()
        assert s.advance() == N.CVR_OK
        assert s.render("cvr_render_vct", vct_params())[0] == N.CVR_OK, s.error()
        assert s.option(b"vct_pyramid_builds") == builds   # the pyramid outlived the TF
        dev.set_volume(vol, SCALE)
        assert s.option(b"cell_flags_valid") == 0
        assert s.render("cvr_render_dosct", dos_params())[0] == STATE
        assert s.render("cvr_render_extbsd", ebs_params())[0] == STATE
        assert s.render("cvr_render_preillum", dos_params())[0] == STATE
        assert s.advance() == STATE
        assert s.copies() == (STATE, STATE, STATE)
        assert s.render("cvr_render_vct", vct_params())[0] == STATE
        assert "cvr_vct_set_opacity" in s.error()
        dev.vct_set_opacity(s.opacity)
        assert s.render("cvr_render_vct", vct_params())[0] == N.CVR_OK, s.error()
        assert s.option(b"vct_pyramid_builds") == builds + 1
        st, iso_after = s.render("cvr_render_iso", iso_params())
        assert st == N.CVR_OK, s.error()
        assert np.array_equal(iso_after.view(np.int32), iso_before.view(np.int32))
    finally:
        dev.close()                                        # cvr_destroy with all of it alive or dropped

    # a context that only ever took the SAT build's refusal
    dev = Device(0)
    try:
        dev.set_volume(vol, SCALE)
        L = N.lib()
        assert L.cvr_set_extinction_sat(dev.handle, N.fptr(ext_lut), 255) == N.CVR_ERR_ARG
        assert L.cvr_copy_extinction_sat(dev.handle, None, 0, (ctypes.c_int * 3)()) == STATE
    finally:
        dev.close()
