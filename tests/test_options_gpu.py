"""cvr_set_option / cvr_get_option against the documented table of options
(include/cvr.h; the defaults are those of a fresh context).

One context without a volume: every writable key reads its default after
cvr_create, accepts both ends of its range and reads them back, refuses one value
below and one above it with CVR_ERR_ARG (the stored value stays, the key's name is
in cvr_last_error); the read-only keys read and are refused by set; an unknown key
is CVR_ERR_ARG from set and -1 from get.  (The group rule -- the exchange's four
keys are refused on a group, the rest fan out -- is covered by test_exchange_gpu.py.)"""
import pytest

from cpp_volume_rendering_amd import _native as N
from cpp_volume_rendering_amd.renderer import Device

pytestmark = pytest.mark.gpu

MAX_GATHER_SETS = 64            # CVR_MAX_GATHER_SETS (include/cvr.h)
INT_MAX = 2**31 - 1

# key: (default, accepted values to set and read back, refused values)
RANGES = {
    "batch": (0, (0, 2, 4), (-1, 1, 3, 5)),
    "tile_order": (1, (0, 2), (-1, 3)),
    "stale_deg": (5, (0, 180), (-1, 181)),
    "quad": (0, (0, 100), (-1, 101)),
    "filter_bits": (0, (0, 8), (-1, 7, 9)),
    "sat_chunk": (32, (1, 64), (0, 65)),
    "sat_layout": (0, (0, 1), (-1, 2)),
    "sat_keep_scratch": (0, (0, 1), (-1, 2)),
    "shade_flat": (1, (0, 1), (-1, 2)),
    "flat_group": (8, (1, 4096), (0, 4097)),
    "debug_flat_limit": (0, (0, INT_MAX), (-1,)),
    "kernel_timing": (0, (0, 4096), (-1, 4097)),
    "macro": (3, (0, 2, 6), (-1, 1, 7)),
    "cell_skip": (3, (0, 4), (-1, 5)),
    "skip_min_pct": (15, (0, 101), (-1, 102)),
    "tile_cost": (0, (0, 1), (-1, 2)),
    "max_waves_cu": (0, (0, 32), (-1, 33)),
    "launch_interleave": (1, (0, 1), (-1, 2)),
    "gather_root_idle": (0, (0, 1), (-1, 2)),
    "native_exp": (0, (0, 1), (-1, 2)),
    "encode_onepass": (0, (0, 1), (-1, 2)),
    "debug_cell_flags_oom": (0, (0, 1), (-1, 2)),
    "exchange_code": (1, (0, 1), (-1, 2)),
    "gather_sets": (0, (0, MAX_GATHER_SETS), (-1, MAX_GATHER_SETS + 1)),
    "exchange_lag": (-1, (-1, MAX_GATHER_SETS - 1), (-2, MAX_GATHER_SETS)),
    "split_streams": (1, (1, 32), (0, 33)),
    "async_order": (0, (0, 1), (-1, 2)),
    "order_interval": (8, (1, 1000000), (0, 1000001)),
    "debug_epi_stop": (0, (-INT_MAX - 1, INT_MAX), ()),
    "debug_keep": (0, (0, INT_MAX), (-1,)),
    "boost": (5, (0, 100), (-1, 101)),
    "band_cap": (130, (100, 200), (99, 201)),
}
FLAGS = {"shade_counters": 0, "tile_stats": 0}     # any value, stored as 0 / 1
READ_ONLY = {"cell_flags_active": 0, "cell_flags_valid": 0, "sat_build_us": 0,
             "occ_empty_permille": -1,             # -1 until a render has built the occupancy
             "flat_cap_kjobs": 0, "light_cache_builds": 0,
             "rc1pass_variant": -1}                # -1 until cvr_render_rc1pass has launched its kernel


@pytest.fixture(scope="module")
def ctx():
    dev = Device(0)
    yield dev.handle
    dev.close()


def _set(ctx, key, value):
    return N.lib().cvr_set_option(ctx, key.encode(), value)


def _get(ctx, key):
    return N.lib().cvr_get_option(ctx, key.encode())


def test_defaults_right_after_create():
    dev = Device(0)
    try:
        for key, (default, _, _) in RANGES.items():
            assert _get(dev.handle, key) == default, key
        for key, default in FLAGS.items():
            assert _get(dev.handle, key) == default, key
    finally:
        dev.close()


@pytest.mark.parametrize("key", sorted(RANGES))
def test_range(ctx, key):
    default, accepted, refused = RANGES[key]
    try:
        for v in accepted:
            assert _set(ctx, key, v) == N.CVR_OK, (key, v)
            assert _get(ctx, key) == v, (key, v)
        kept = accepted[-1]
        for v in refused:
            assert _set(ctx, key, v) == N.CVR_ERR_ARG, (key, v)
            assert _get(ctx, key) == kept, (key, v)
            assert key.encode() in N.lib().cvr_last_error(ctx), (key, v)
    finally:
        assert _set(ctx, key, default) == N.CVR_OK
    assert _get(ctx, key) == default


@pytest.mark.parametrize("key", sorted(FLAGS))
def test_flag_stored_as_0_or_1(ctx, key):
    for v, stored in ((7, 1), (-3, 1), (0, 0)):
        assert _set(ctx, key, v) == N.CVR_OK
        assert _get(ctx, key) == stored


def test_kernel_timing_reads_the_ring_size(ctx):
    try:
        assert _set(ctx, "kernel_timing", 3) == N.CVR_OK
        assert _get(ctx, "kernel_timing") == 3
    finally:
        assert _set(ctx, "kernel_timing", 0) == N.CVR_OK
    assert _get(ctx, "kernel_timing") == 0


@pytest.mark.parametrize("key", sorted(READ_ONLY))
def test_read_only(ctx, key):
    assert _get(ctx, key) == READ_ONLY[key]
    assert _set(ctx, key, 0) == N.CVR_ERR_ARG
    assert b"unknown option" in N.lib().cvr_last_error(ctx)
    assert key.encode() in N.lib().cvr_last_error(ctx)
    assert _get(ctx, key) == READ_ONLY[key]


def test_unknown_key(ctx):
    assert _set(ctx, "no_such_option", 1) == N.CVR_ERR_ARG
    assert b"unknown option 'no_such_option'" in N.lib().cvr_last_error(ctx)
    assert _get(ctx, "no_such_option") == -1
