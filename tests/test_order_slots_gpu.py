"""The life cycle of rc1pass's learned launch order (cvr_rc1pass.cpp, Ctx::OrderSlot):
when a frame marches under an order, when a stale order is dropped, when it is
rebuilt, and that every render stream has a slot of its own.  The order never
changes a pixel, so it is read off the tile_stats diagnostics: entry [4 t + 3] >> 32
is the block slot b that marched wave tile t.  Without an order (tile_order 1)
the kernel takes t = b; under an order every XCD band holds a contiguous run of
tiles dealt to the slots band, band + 8, ..., which cannot be the identity once
a band holds two tiles (t and t + 1 differ mod 8)."""
import ctypes
import math

import numpy as np
import pytest

from cpp_volume_rendering_amd import _native as N
from cpp_volume_rendering_amd import datasets as D
from cpp_volume_rendering_amd.renderer import Camera, Device, make_frame

pytestmark = pytest.mark.gpu

NVOX = 32
W = H = 128
NTILES = (W // 8) * (H // 8)
OPTIONS = (("tile_order", 1), ("order_interval", 1), ("tile_stats", 1), ("quad", 0),
           ("async_order", 0), ("stale_deg", 10))


def _rotated_y(eye, deg):
    """eye turned by deg about the y axis through the volume centre (the origin)."""
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    x, y, z = eye
    return (c * x + s * z, y, -s * x + c * z)


VIEW_A = dict(D.INITIAL_STATE_CAMERA)
VIEW_B = dict(VIEW_A, eye=_rotated_y(VIEW_A["eye"], 45.0))


def _blob_u8():
    """One Gaussian blob off the centre of a 32^3 volume: the tiles' costs differ."""
    i = np.arange(NVOX, dtype=np.float64)
    z, y, x = np.meshgrid(i, i, i, indexing="ij")
    d2 = (x - 10.0) ** 2 + (y - 20.0) ** 2 + (z - 12.0) ** 2
    return np.clip(np.floor(255.0 * np.exp(-d2 / (2.0 * 6.0 ** 2))), 0, 255).astype(np.uint8)


def _device(bonsai_tf, options):
    d = Device(0)
    for k, v in options:
        N.check(N.lib().cvr_set_option(d.handle, k.encode(), v), k, d.handle)
    d.set_volume(_blob_u8(), D.voxel_scale(NVOX))
    d.set_transfer_function(bonsai_tf)
    return d


def _frame(d, cam):
    """One frame into device buffers; returns (rgba bits, counts, ordered)."""
    import torch
    rgba = torch.zeros((W * H, 4), dtype=torch.float32, device="cuda")
    cnt = torch.zeros((W * H,), dtype=torch.int32, device="cuda")
    frame = make_frame(Camera(**cam), W, H)
    p = N.Rc1passParams()
    out = N.Output(rgba.data_ptr(), cnt.data_ptr(), None, 1)
    N.check(N.lib().cvr_render_rc1pass(d.handle, ctypes.byref(frame), ctypes.byref(p), ctypes.byref(out)),
            "render", d.handle)
    torch.cuda.synchronize()
    ordered = None
    nt = ctypes.c_int()
    N.check(N.lib().cvr_copy_tile_stats(d.handle, None, 0, ctypes.byref(nt)), "stats", d.handle)
    if nt.value:
        assert nt.value == NTILES
        st = np.zeros(NTILES * 4, np.uint64)
        N.check(N.lib().cvr_copy_tile_stats(d.handle, st.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                                            NTILES, ctypes.byref(nt)), "stats", d.handle)
        slots = (st.reshape(-1, 4)[:, 3] >> np.uint64(32)).astype(np.int64)
        assert np.array_equal(np.sort(slots), np.unique(slots)), "a slot marched two tiles"
        ordered = not np.array_equal(slots, np.arange(NTILES))
    return rgba.view(torch.int32).cpu().numpy(), cnt.cpu().numpy(), ordered


@pytest.fixture(scope="module")
def unordered(bonsai_tf):
    """The tile_order 0 images of the two views."""
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    d = _device(bonsai_tf, (("tile_order", 0),))
    try:
        ref = {k: _frame(d, cam)[:2] for k, cam in (("A", VIEW_A), ("B", VIEW_B))}
    finally:
        d.close()
    assert ref["A"][1].max() > 0 and not np.array_equal(ref["A"][0], ref["B"][0])
    return ref


def _check_image(got, ref, what):
    assert np.array_equal(got[1], ref[1]), f"{what}: counts"
    assert np.array_equal(got[0], ref[0]), f"{what}: rgba"


def test_order_sequence_one_stream(bonsai_tf, unordered):
    """A, A, then B (45 degrees away) three times: the second frame of a view that
    holds still runs under the order the frame before it built; a jump to a stale
    view runs without one and builds none; the next, steady, frame rebuilds."""
    import torch
    cams = {"A": VIEW_A, "B": VIEW_B}
    d = _device(bonsai_tf, OPTIONS)
    s = torch.cuda.Stream()
    try:
        d.set_stream(s.cuda_stream)
        seq = [("A", False), ("A", True), ("B", False), ("B", False), ("B", True)]
        for i, (view, want) in enumerate(seq):
            rgba, cnt, ordered = _frame(d, cams[view])
            _check_image((rgba, cnt), unordered[view], f"frame {i + 1} (view {view})")
            assert ordered == want, f"frame {i + 1} (view {view}): ordered {ordered}, expected {want}"
    finally:
        d.close()


def test_order_slots_belong_to_streams(bonsai_tf, unordered):
    """An order learned on one render stream is not used by a frame on another,
    and stays in use on its own."""
    import torch
    d = _device(bonsai_tf, OPTIONS)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    try:
        d.set_stream(s1.cuda_stream)
        assert _frame(d, VIEW_A)[2] is False
        assert _frame(d, VIEW_A)[2] is True
        d.set_stream(s2.cuda_stream)
        rgba, cnt, ordered = _frame(d, VIEW_A)
        _check_image((rgba, cnt), unordered["A"], "first frame on the second stream")
        assert ordered is False, "a fresh stream used another stream's order"
        d.set_stream(s1.cuda_stream)
        rgba, cnt, ordered = _frame(d, VIEW_A)
        _check_image((rgba, cnt), unordered["A"], "third frame on the first stream")
        assert ordered is True, "the first stream lost its order"
    finally:
        d.close()


def test_async_order_images(bonsai_tf, unordered):
    """Orders sorted on the side stream (lag 3, see test_schedules_bitexact): every
    frame's image is the unordered one."""
    d = _device(bonsai_tf, tuple((k, 1 if k == "async_order" else v) for k, v in OPTIONS))
    try:
        for i in range(5):
            rgba, cnt, _ = _frame(d, VIEW_A)
            _check_image((rgba, cnt), unordered["A"], f"async frame {i + 1}")
    finally:
        d.close()
