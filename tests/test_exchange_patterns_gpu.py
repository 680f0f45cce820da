"""The multi-rank exchange on synthetic tiles: geometry, bit patterns, recovery.

tests/test_exchange_gpu.py drives cvr_gather_tiles_n with rendered frames of whole
tiles.  Here nothing is rendered: bare contexts joined by cvr_comm_init_local exchange
the bit patterns of tests/exchange_cases.py (every code width in every channel, sign
bits, infinities and NaNs, random, constant and special tiles) over images that cut
tiles on both edges, ranks without tiles, an idle root, 32- and 64-pixel tiles and
groups whose size changes from one exchange to the next.  The padding slots of every
packed buffer hold a poison pattern and every image starts as a sentinel; the
expected image is screen_tiles.unpack (numpy indexing) and every comparison is bit for
bit.

The last tests pin the recovery contract of include/cvr.h: a cvr_gather_tiles_n call
refused with CVR_ERR_STATE (rank 0 before its peers, or a peer ahead of rank 0) has
issued no exchange, so the rounds after it arrive intact."""
import ctypes

import numpy as np
import pytest

import exchange_cases as X
from cpp_volume_rendering_amd import _native as N
from cpp_volume_rendering_amd import datasets as D
from cpp_volume_rendering_amd.renderer import Camera, Device, make_frame

pytestmark = pytest.mark.gpu

FORMS = {"code": (N.FORMAT_RGBA16F, 1), "raw16": (N.FORMAT_RGBA16F, 0), "raw32": (N.FORMAT_RGBA32F, 1)}


class Round:
    """One exchange's buffers (kept alive until the contexts are closed) and its
    expected images."""

    def __init__(self, nframes):
        self.nframes = nframes
        self.packed = {}        # communicator rank -> device buffer (rank 0: the gather buffer)
        self.gathered = None
        self.images = []        # rank 0: one device image per frame
        self.want = []          # the expected image of every frame


class Exchange:
    """N bare contexts on device 0 (no volume, no TF) joined in process."""

    def __init__(self, geom, form, streams=1, sets=2, lag=None):
        import torch
        self.torch = torch
        self.world, self.idle, self.tile, self.W, self.H, self.ks = X.GEOMETRIES[geom]
        self.fmt, code = FORMS[form]
        self.half = self.fmt == N.FORMAT_RGBA16F
        self.sworld, self.tpr = X.split_world(geom)
        self.D, self.B = streams, sets
        self.dev = torch.device("cuda", 0)
        self.L = N.lib()
        self.rounds = []
        self.issued = [0] * self.world      # exchanges each rank has issued
        self.ctxs = []
        try:
            for _ in range(self.world):
                self.ctxs.append(Device(0))
            arr = (ctypes.c_void_p * self.world)(*[c.handle.value for c in self.ctxs])
            N.check(self.L.cvr_comm_init_local(arr, self.world), "cvr_comm_init_local")
            opts = [("split_streams", streams), ("gather_sets", sets), ("gather_root_idle", int(self.idle)),
                    ("exchange_code", code)] + ([("exchange_lag", lag)] if lag is not None else [])
            for c in self.ctxs:
                for k, v in opts:
                    N.check(self.L.cvr_set_option(c.handle, k.encode(), v), k, c.handle)
            self.streams = [[torch.cuda.Stream(self.dev) for _ in range(streams)] for _ in range(self.world)]
        except Exception:
            self.close()
            raise

    def close(self):
        for c in self.ctxs:
            c.close()

    def _to_device(self, a):
        signed = a.view(np.int16 if a.dtype == np.uint16 else np.int32)
        return self.torch.from_numpy(np.ascontiguousarray(signed)).to(self.dev)

    def sentinel_image(self):
        a = (np.full((self.H, self.W, 4), X.SENTINEL16, np.uint16) if self.half else
             np.full((self.H, self.W, 4), X.SENTINEL32, np.uint32))
        return self._to_device(a)

    def bits(self, t):
        return t.cpu().numpy().view(np.uint16 if self.half else np.uint32)

    def prepare(self, seed, nframes, images=None):
        """Patterns for every render rank, uploaded; `images` (per frame: an index into
        the round's own images, or None for a NULL pointer) defaults to one per frame."""
        rng = np.random.default_rng(seed)
        npx = self.tile * self.tile
        R = Round(nframes)
        poison = X.POISON16 if self.half else X.POISON32
        host = []
        for sr in range(self.sworld):
            k = self.ks[sr]
            make = X.mixed_tiles if self.half else X.mixed_words
            tiles = make(rng, k * nframes, npx, start=int(rng.integers(X.CYCLE)))
            host.append(X.rank_buffers(tiles, k, self.tpr, nframes, poison))
        R.want = X.expected_images(host, self.W, self.H, self.tile, self.sworld)
        # rank 0's gather buffer: world blocks of nframes * tpr tiles; a rendering root's
        # tiles lie in block 0 already (d_packed == d_gathered)
        g = np.full((self.world,) + host[0].shape, (~poison) & (0xffff if self.half else 0xffffffff),
                    host[0].dtype)
        if not self.idle:
            g[0] = host[0]
        R.gathered = self._to_device(g)
        for r in range(1, self.world):
            R.packed[r] = self._to_device(host[r - 1 if self.idle else r])
        R.packed[0] = None if self.idle else R.gathered
        R.image_index = list(range(nframes)) if images is None else images
        R.images = [self.sentinel_image() for _ in range(nframes)]
        self.torch.cuda.synchronize()
        self.rounds.append(R)
        return R

    def call(self, R, r):
        """Rank r's cvr_gather_tiles_n of round R; returns the status."""
        c = self.ctxs[r]
        srank = max(r - 1, 0) if self.idle else r
        s = self.streams[r][self.issued[r] % self.D]
        N.check(self.L.cvr_set_stream(c.handle, s.cuda_stream), "stream", c.handle)
        fr = make_frame(Camera(**D.INITIAL_STATE_CAMERA), self.W, self.H, self.tile, srank, self.sworld)
        imgs = None
        if r == 0:
            imgs = (ctypes.c_void_p * R.nframes)(*[None if i is None else R.images[i].data_ptr()
                                                   for i in R.image_index])
        buf = R.packed[r]
        st = self.L.cvr_gather_tiles_n(c.handle, ctypes.byref(fr), R.nframes,
                                       buf.data_ptr() if buf is not None else None, self.tpr, self.fmt,
                                       R.gathered.data_ptr() if r == 0 else None, imgs)
        if st == N.CVR_OK:
            self.issued[r] += 1
        return st

    def ordered(self, R):
        for r in list(range(1, self.world)) + [0]:
            st = self.call(R, r)
            assert st == N.CVR_OK, (r, self.L.cvr_last_error(self.ctxs[r].handle))

    def sync(self):
        """cvr_gather_sync on every rank (rank 0 first: it posts what still trails),
        then the device; returns the statuses."""
        cur = self.torch.cuda.current_stream(self.dev)
        sts = []
        for c in self.ctxs:
            N.check(self.L.cvr_set_stream(c.handle, cur.cuda_stream), "stream", c.handle)
            sts.append(self.L.cvr_gather_sync(c.handle))
        self.torch.cuda.synchronize()
        return sts

    def check(self, R, what):
        """Image i holds the last frame that names it, bit for bit; no sentinel is left."""
        last = {i: j for j, i in enumerate(R.image_index) if i is not None}
        sentinel = X.SENTINEL16 if self.half else X.SENTINEL32
        for i, j in last.items():
            got = self.bits(R.images[i])
            assert np.array_equal(got, R.want[j]), f"{what}: image {i} is not frame {j}"
            assert not (got == sentinel).all(axis=2).any(), f"{what}: image {i} keeps sentinel pixels"
        for i in set(range(R.nframes)) - set(last):
            assert (self.bits(R.images[i]) == sentinel).all(), f"{what}: unnamed image {i} was written"


CASES = [(g, f) for g in X.GEOMETRIES for f in ("code", "raw16")] + \
        [(g, "raw32") for g in ("w3_t16_odd", "w8_idle_t16_even")]


def _run_groups(x, name):
    # 3 frames, 1 frame (a smaller bound: the receive slot changes), 3 frames again;
    # then 3 frames on the set that so far held 1 (its buffers grow) and 1 frame on a
    # set that held 3 (the slot shrinks, the capacity stays)
    rounds = []
    for i, nframes in enumerate((3, 1, 3, 3, 1)):
        R = x.prepare(1000 * i + 7, nframes)
        x.ordered(R)
        rounds.append(R)
    assert x.sync() == [N.CVR_OK] * x.world
    for i, R in enumerate(rounds):
        x.check(R, f"{name} group {i}")


@pytest.mark.parametrize("geom,form", CASES)
def test_patterns_arrive_bit_exact(geom, form):
    """Five groups of 3, 1, 3, 3 and 1 frames (ranks 1..N-1 before rank 0), one render
    stream and two buffer sets: every image equals the host unpack of the ranks' first
    tiles_for_rank tiles; poison and sentinel never show."""
    x = Exchange(geom, form, streams=1, sets=2)
    try:
        _run_groups(x, f"{geom}/{form}")
    finally:
        x.close()


def test_patterns_trailing_data_phase():
    """Two render streams over four buffer sets, exchange_lag -1: the coded data phase
    trails by one exchange and the final cvr_gather_sync posts the last one."""
    x = Exchange("w3_t16_odd", "code", streams=2, sets=4, lag=-1)
    try:
        _run_groups(x, "w3_t16_odd/code/lag")
    finally:
        x.close()


@pytest.mark.parametrize("form", ["code", "raw16"])
@pytest.mark.parametrize("images", [(0, 1, 0), (0, 0, 2), (0, None, 2)],
                         ids=["frames02_share", "frames01_share", "frame1_null"])
def test_repeated_and_null_images(form, images):
    """One group of 3 frames: an image named by two frames ends up with the later
    frame's pixels (the decode is split into runs so that it sees them in order); a
    NULL image skips its frame and the others arrive intact."""
    x = Exchange("w3_t16_odd", form)
    try:
        R = x.prepare(77, 3, images=list(images))
        x.ordered(R)
        assert x.sync() == [N.CVR_OK] * 3
        x.check(R, f"{form} {images}")
    finally:
        x.close()


@pytest.mark.parametrize("form", ["code", "raw16"])
def test_recovery_rank0_called_first(form):
    """Rank 0 calls before its peers and is refused (CVR_ERR_STATE, naming rank 1).
    The refused call issued nothing: the next rounds, in order, arrive bit-exact,
    cvr_gather_sync succeeds everywhere and the refused call's image keeps its sentinel."""
    x = Exchange("w3_t16_odd", form)
    try:
        A = x.prepare(1, 1)
        x.ordered(A)
        refused = x.prepare(2, 1)
        assert x.call(refused, 0) == N.CVR_ERR_STATE
        assert b"rank 1" in x.L.cvr_last_error(x.ctxs[0].handle)
        B, C = x.prepare(3, 1), x.prepare(4, 1)
        for R in (B, C):
            for r in (1, 2, 0):
                st = x.call(R, r)
                assert st == N.CVR_OK, (r, x.L.cvr_last_error(x.ctxs[r].handle))
        assert x.sync() == [N.CVR_OK] * 3
        for R, what in ((A, "round A"), (B, "round B"), (C, "round C")):
            x.check(R, what)
        assert (x.bits(refused.images[0]) == X.SENTINEL16).all(), "the refused call's image was written"
    finally:
        x.close()


@pytest.mark.parametrize("form", ["code", "raw16"])
def test_recovery_peer_ran_ahead(form):
    """Rank 1 issues the next exchange before rank 0 has posted the one whose buffers it
    would reuse and is refused; ranks 2 and 0 complete the round, another follows in
    order, and both arrive bit-exact."""
    x = Exchange("w3_t16_odd", form)
    try:
        A, B, C = x.prepare(11, 1), x.prepare(12, 1), x.prepare(13, 1)
        x.ordered(A)
        assert x.call(B, 1) == N.CVR_OK
        assert x.call(C, 1) == N.CVR_ERR_STATE
        assert b"rank 0 has not posted" in x.L.cvr_last_error(x.ctxs[1].handle)
        for r in (2, 0):
            assert x.call(B, r) == N.CVR_OK, (r, x.L.cvr_last_error(x.ctxs[r].handle))
        x.ordered(C)
        assert x.sync() == [N.CVR_OK] * 3
        for R, what in ((A, "round A"), (B, "round B"), (C, "round C")):
            x.check(R, what)
    finally:
        x.close()
