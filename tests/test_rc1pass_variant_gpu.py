"""Which rc1pass_tile_kernel<K, PHONG, SKIP, QUAD, XF, BUF, FB, CS> a frame launches
(read-only option "rc1pass_variant", include/cvr.h; raymarch.hip rc1_resolve_variant).

Every variant renders the same bits, so the parity suites pass whichever kernel the
options resolve to; a slip in the choice would only show as a slower frame.  Each row
here renders a small scene, decodes the variant the launch recorded from its own
template arguments, and compares it with what the if-ladder this table replaced
launched for the same options (the expected values were read from that ladder on the
GPU before it was removed).  Each row also compares its frame, bit for bit, with the
same scene rendered with cell_skip 0, macro 0, quad 0, so that a row cannot pass by
reporting a variant it did not run.  One row cannot: native_exp at the defaults (XF 2)
is the tolerance mode, whose frame differs from the exact one by design; it must differ
from it and meet the gate of test_tolerance_gpu.py instead.

The scene is a 24^3 blobs_u8 volume at 32x32 unless a row says otherwise.  BUF 1 needs
16 * pitch_z >= 2^23: the cell grid has N + 1 cells per axis, so a 724x724 slab is the
first ((724 + 1)^2 * 16 = 8410000 >= 8388608 > (723 + 1)^2 * 16 = 8386816); both sides
of that threshold and the 728x728x2 slab run here.  BUF 0 needs a cell grid of 4 GiB or
more, which is no few-second test: it is covered by reading rc1_resolve_variant only.
"""
import numpy as np
import pytest

from cpp_volume_rendering_amd import _native as N
from cpp_volume_rendering_amd import datasets as D
from cpp_volume_rendering_amd.renderer import Device

from test_rc1pass_gpu import INITIAL, assert_bitexact, gpu_render
from test_tolerance_gpu import GATE_FRAC, GATE_MAX, GATE_SSIM, _gate

pytestmark = pytest.mark.gpu

W = H = 32
PHONG = dict(phong=True, gmode=1, light=D.LIGHT_LIST0_POSITION)
PLAIN = dict(cell_skip=0, macro=0, quad=0)      # the options of every reference frame


def decode(v):
    assert v >= 0, "no rc1pass kernel was launched"
    return dict(K=v & 15, PHONG=(v >> 4) & 1, SKIP=(v >> 5) & 1, QUAD=(v >> 6) & 1, XF=(v >> 8) & 3,
                BUF=(v >> 10) & 3, FB=(v >> 12) & 15, CS=(v >> 16) & 7)


def variant(d):
    return N.lib().cvr_get_option(d.handle, b"rc1pass_variant")


def set_options(d, opts):
    for k, v in opts.items():
        N.check(N.lib().cvr_set_option(d.handle, k.encode(), v), k, d.handle)


def _slab(n):
    """n x n x 2 voxels: the middle two planes of the blobs volume, tiled."""
    return np.ascontiguousarray(np.tile(D.blobs_u8(24)[11:13], (1, n // 24 + 1, n // 24 + 1))[:, :n, :n])


def _scene(name):
    if name.startswith("slab"):
        n = int(name[4:])
        return _slab(n), D.voxel_scale(n), 16, 16
    return D.blobs_u8(24), D.voxel_scale(24), W, H


_refs = {}


def reference(bonsai_tf, scene="blobs", tf_scale=1.0, step=0.0, phong=False, filter_bits=0):
    """The frame of the scene under PLAIN (+ filter_bits, which changes the image):
    rendered once per distinct scene, never modified."""
    key = (scene, tf_scale, step, phong, filter_bits)
    if key not in _refs:
        vol, sc, w, h = _scene(scene)
        tf = bonsai_tf.copy()
        tf[:, 3] *= tf_scale
        d = Device(0)
        try:
            set_options(d, dict(PLAIN, filter_bits=filter_bits))
            rgba, cnt, total = gpu_render(d, vol, sc, tf, INITIAL, w, h, step=step, **(PHONG if phong else {}))
            v = decode(variant(d))
        finally:
            d.close()
        assert (v["SKIP"], v["QUAD"], v["CS"], v["FB"], v["PHONG"]) == (0, 0, 0, filter_bits, int(phong)), v
        rgba.setflags(write=False)
        cnt.setflags(write=False)
        _refs[key] = (rgba, cnt, total)
    return _refs[key]


def run(bonsai_tf, opts, frames=1, scene="blobs", tf_scale=1.0, step=0.0, phong=False, exact=True):
    """Renders `frames` frames of the scene under `opts`; every frame must equal the
    reference.  Returns the decoded variant of each frame and the last frame."""
    vol, sc, w, h = _scene(scene)
    tf = bonsai_tf.copy()
    tf[:, 3] *= tf_scale
    ref = reference(bonsai_tf, scene, tf_scale, step, phong, opts.get("filter_bits", 0))
    out, last = [], None
    d = Device(0)
    try:
        set_options(d, opts)
        for f in range(frames):
            last = gpu_render(d, vol, sc, tf, INITIAL, w, h, step=step, set_data=(f == 0),
                              **(PHONG if phong else {}))
            out.append(decode(variant(d)))
            if exact:
                assert_bitexact(last[1], ref[1], f"{opts} frame {f} counts")
                assert_bitexact(last[0], ref[0], f"{opts} frame {f} rgba")
                assert last[2] == ref[2]
    finally:
        d.close()
    return out, last


def V(K=4, PHONG=0, SKIP=0, QUAD=0, XF=1, BUF=2, FB=0, CS=3):
    """A variant, as the defaults' (row 1) with the named fields changed."""
    return dict(K=K, PHONG=PHONG, SKIP=SKIP, QUAD=QUAD, XF=XF, BUF=BUF, FB=FB, CS=CS)


def test_before_the_first_render():                                           # row 16
    d = Device(0)
    try:
        assert variant(d) == -1
        d.set_volume(D.blobs_u8(24), D.voxel_scale(24))
        assert variant(d) == -1
    finally:
        d.close()


@pytest.mark.parametrize("opts,phong,want", [
    (dict(), False, V()),                                                     # row 1
    (dict(), True, V(K=2, PHONG=1)),                                          # row 2
    (dict(batch=2), False, V(K=2)),                                           # row 3
    (dict(batch=4), True, V(K=4, PHONG=1)),                                   # row 4
    (dict(cell_skip=1), False, V(CS=1)),                                      # row 5
    (dict(cell_skip=2), False, V(CS=2)),
    (dict(cell_skip=4), False, V(CS=4)),
    (dict(cell_skip=0, macro=3, skip_min_pct=0), False, V(SKIP=1, CS=0)),     # row 6
    (dict(cell_skip=0, macro=0), False, V(SKIP=0, CS=0)),                     # row 7
    (dict(filter_bits=8), False, V(FB=8, CS=0, QUAD=0)),                      # row 8
    (dict(filter_bits=8, native_exp=1), False, V(FB=8, CS=0, QUAD=0)),        # row 10: XF stays 1
], ids=["defaults", "defaults_phong", "batch2", "batch4_phong", "cell_skip1", "cell_skip2", "cell_skip4",
        "macro_skip", "no_skip", "filter8", "filter8_native_exp"])
def test_variant_of_one_frame(bonsai_tf, opts, phong, want):
    got, _ = run(bonsai_tf, opts, phong=phong)
    assert got == [want]


def test_filter_bits_8_never_takes_the_quad_march(bonsai_tf):                 # row 9
    got, _ = run(bonsai_tf, dict(filter_bits=8, tile_order=1, quad=50), frames=5)
    assert got == [V(FB=8, CS=0, QUAD=0)] * 5


def test_quad_march_once_the_learned_order_is_in_use(bonsai_tf):              # row 11
    """The first frame has no launch order yet and runs the defaults' kernel; its
    epilogue builds the order, so frame 1 and every later one take the quad kernel
    (64-bit addressing, no per-cell skip)."""
    got, _ = run(bonsai_tf, dict(tile_order=1, quad=50), frames=5)
    assert got[0] == V()
    assert got[1:] == [V(QUAD=1, BUF=0, CS=0)] * 4


def test_native_exp_at_the_defaults(bonsai_tf):                               # row 12
    got, fast = run(bonsai_tf, dict(native_exp=1), exact=False)
    assert got == [V(XF=2)]
    ref = reference(bonsai_tf)
    assert not np.array_equal(fast[0].view(np.uint32), ref[0].view(np.uint32)), "the variant ran"
    within, mx, ssim = _gate(fast[0], ref[0])
    print(f"native_exp vs exact: within {within}, max {mx}, ssim {ssim}, samples {fast[2]} vs {ref[2]}")
    assert within >= GATE_FRAC and mx <= GATE_MAX and ssim >= GATE_SSIM, (within, mx, ssim)


def test_native_exp_is_ignored_off_the_headline_variant(bonsai_tf):           # row 13
    got0, f0 = run(bonsai_tf, dict(cell_skip=2, native_exp=0))
    got1, f1 = run(bonsai_tf, dict(cell_skip=2, native_exp=1))
    assert got0 == got1 == [V(CS=2)]
    assert_bitexact(f1[0], f0[0], "native_exp 1 vs 0 at cell_skip 2")
    assert_bitexact(f1[1], f0[1], "native_exp 1 vs 0 at cell_skip 2, counts")


def test_range_checked_exp_past_the_fast_range(bonsai_tf):                    # row 14
    tf_scale, step = 100.0, 2.0
    assert float(bonsai_tf[:, 3].max()) * tf_scale * step * (1.0 + 1.0 / 1024.0) > 86.0
    got, _ = run(bonsai_tf, dict(), tf_scale=tf_scale, step=step)
    assert got == [V(XF=0)]


@pytest.mark.parametrize("n,buf", [(723, 2), (724, 1), (728, 1)])            # row 15
def test_buffer_addressing_by_the_z_pitch(bonsai_tf, n, buf):
    assert ((n + 1) ** 2 * 16 < 2 ** 23) == (buf == 2)
    got, _ = run(bonsai_tf, dict(), scene=f"slab{n}")
    assert got == [V(BUF=buf)]
