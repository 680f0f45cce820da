"""Synthetic tiles and geometries shared by tests/test_codec.py and
tests/test_exchange_patterns_gpu.py; a plain module, not a conftest.

The exchange (cvr_gather_tiles_n, codec.hip's exchange kernels, unpack_tiles_kernel)
moves bit patterns: nothing here is rendered.  Tiles are (n, npx, 4) uint16 channel
patterns (pixel p = y * tile + x), built so that every code width 0..16 occurs in
every channel, with bases whose sign bit is set and bases inside the RGBA16F
infinity / NaN ranges.  The expected image of a frame is screen_tiles.unpack (numpy
indexing) over every rank's first tiles_for_rank tiles."""
import numpy as np

from cpp_volume_rendering_amd import screen_tiles as T

# name: (world, idle root, tile, W, H, tiles per render rank)
GEOMETRIES = {
    # odd W, ragged on both edges; 3 frames of 7 tiles leave a partial 8-wave workgroup
    "w3_t16_odd": (3, False, 16, 75, 53, (7, 7, 6)),
    # even W cutting a tile (the two-pixels-per-lane unpack branch); 7 render ranks
    "w8_idle_t16_even": (8, True, 16, 70, 50, (3, 3, 3, 3, 3, 3, 2)),
    # four ranks send the empty stream
    "w8_t32_empty": (8, False, 32, 45, 33, (1, 1, 1, 1, 0, 0, 0, 0)),
    # 2 tiles per encode workgroup against 3 frames of 3 tiles
    "w2_t32": (2, False, 32, 75, 53, (3, 3)),
    # only rank 0's raw block carries pixels
    "w3_one_tile": (3, False, 16, 16, 16, (1, 0, 0)),
    # 64-pixel tiles: exchange_code 1 falls back to raw tiles
    "w2_t64": (2, False, 64, 70, 50, (1, 1)),
}

SPECIALS = (0x0000, 0x8000, 0x0001, 0x03ff, 0x7bff, 0x7c00, 0xfc00, 0x7e00, 0xffff)
SPECIALS32 = (0x00000000, 0x80000000, 0x00000001, 0x007fffff, 0x7f7fffff, 0x7f800000, 0xff800000,
              0x7fc00000, 0xffffffff)
POISON16, POISON32 = 0xDEAD, 0xDEADBEEF      # padding slots: must never reach an image
SENTINEL16, SENTINEL32 = 0xABCD, 0xABCDABCD  # images before the exchange

# mixed_tiles' cycle: 17 width tiles, then a random, a constant and the specials tile
CYCLE = 20


def split_world(name):
    """The render split of a geometry: (ranks that render, tile slots per rank)."""
    world, idle, tile, W, H, _ = GEOMETRIES[name]
    sworld = world - 1 if idle else world
    return sworld, T.max_tiles_per_rank(W, H, tile, sworld)


def _base(rng, kind, hi):
    """A base in [0, hi]: uniform, or inside the range `kind` asks for when hi allows."""
    lo, top = ((0, hi), (0x8000, hi), (0x7c00, min(0x7fff, hi)), (0xfc00, hi))[kind]
    if lo > top:
        lo, top = 0, hi
    return int(rng.integers(lo, top + 1))


def tiles_with_widths(rng, n, npx, widths):
    """(n, npx, 4) uint16 tiles whose channel c of tile t codes at exactly widths[t][c]
    bits (0..16): differences in [0, 2^w - 1] with one pixel at 0 and another at
    2^w - 1, on a base from [0, 0xffff - (2^w - 1)] (w = 16 forces base 0).  The
    bases rotate over: anywhere, sign bit set, 0x7c00..0x7fff, 0xfc00..0xffff."""
    out = np.zeros((n, npx, 4), np.uint16)
    for t in range(n):
        for c in range(4):
            w = int(widths[t][c])
            assert 0 <= w <= 16
            span = (1 << w) - 1
            d = rng.integers(0, span + 1, npx)
            if w:
                p0, p1 = rng.choice(npx, 2, replace=False)
                d[p0], d[p1] = 0, span
            out[t, :, c] = _base(rng, (t + c) % 4, 0xffff - span) + d
    return out


def specials_tile(npx):
    """One tile of SPECIALS only: channel 0 cycles all nine; channel 1 the largest
    finite value, +inf and a NaN; channel 2 -0, -inf and the all-ones NaN; channel 3
    zero and the smallest and largest denormals."""
    p = np.arange(npx)
    sub = (SPECIALS, (0x7bff, 0x7c00, 0x7e00), (0x8000, 0xfc00, 0xffff), (0x0000, 0x0001, 0x03ff))
    return np.stack([np.array(s, np.uint16)[(p + c) % len(s)] for c, s in enumerate(sub)], axis=1)


def mixed_tiles(rng, n, npx, start=0):
    """n tiles cycling, from position `start` of a cycle of 20: 17 tiles whose widths
    rotate over the channels (position q, channel c: (q + 5c) % 17), a fully random
    tile, a constant tile and the specials tile.  From start 0, n >= 17 holds every
    width 0..16 in every channel; from any start, n >= 20 holds the whole cycle."""
    out = np.zeros((n, npx, 4), np.uint16)
    for t in range(n):
        q = (start + t) % CYCLE
        if q < 17:
            out[t] = tiles_with_widths(rng, 1, npx, [[(q + 5 * c) % 17 for c in range(4)]])[0]
        elif q == 17:
            out[t] = rng.integers(0, 65536, (npx, 4))
        elif q == 18:
            out[t] = [_base(rng, (t + c) % 4, 0xffff) for c in range(4)]
        else:
            out[t] = specials_tile(npx)
    return out


def mixed_words(rng, n, npx, start=0):
    """The RGBA32F form (raw transport only): (n, npx, 4) uint32 words cycling random
    bits, constant tiles and a tile of SPECIALS32."""
    out = np.zeros((n, npx, 4), np.uint32)
    for t in range(n):
        q = (start + t) % 3
        if q == 0:
            out[t] = rng.integers(0, 1 << 32, (npx, 4), dtype=np.uint64)
        elif q == 1:
            out[t] = rng.integers(0, 1 << 32, 4, dtype=np.uint64)
        else:
            out[t] = np.array(SPECIALS32, np.uint32)[(np.arange(npx)[:, None] + np.arange(4)) % 9]
    return out


def code_widths(tiles):
    """(n, 4) code widths of (n, npx, 4) uint16 tiles: bit_length(max - min)."""
    x = tiles.astype(np.int64)
    span = x.max(axis=1) - x.min(axis=1)
    return np.array([[int(s).bit_length() for s in row] for row in span])


def rank_buffers(tiles, k, tpr, nframes, poison):
    """One rank's packed buffer (nframes, tpr, npx, 4): frame j's k tiles are
    tiles[j * k : (j + 1) * k] in its first k slots, `poison` in the padding."""
    buf = np.full((nframes, tpr) + tiles.shape[1:], poison, tiles.dtype)
    buf[:, :k] = tiles[:nframes * k].reshape((nframes, k) + tiles.shape[1:])
    return buf


def expected_images(packed_all, W, H, tile, nranks):
    """packed_all[rank][frame]: (tpr, npx, 4) packed tiles of the split's ranks.  The
    image of every frame: screen_tiles.unpack over the tiles i < tiles_for_rank,
    clipped to W x H (padding slots are never read)."""
    images = []
    for j in range(len(packed_all[0])):
        stack = np.stack([np.asarray(packed_all[r][j]) for r in range(nranks)])
        stack = stack.reshape(nranks, stack.shape[1], tile, tile, 4)
        images.append(T.unpack(stack, W, H, tile, nranks))
    return images
