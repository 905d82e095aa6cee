"""The stable (u64 key, i32 value) pair sort and the device scan on their own (ll_debug_sort_pairs, ll_debug_exscan): every
algorithm the sort chooses by size -- one LDS workgroup up to 8192 pairs (its row count changes at every multiple of 1024), eight LDS
chunks and a merge by rank up to 65536, device-wide 8-bit radix passes in tiles of 4096 above -- on both sides of every border, with the
key patterns that matter to a radix sort: no varying bit, one varying byte, long runs of equal keys (stability), keys that tie with the
all-ones padding.  The reference is numpy's stable argsort; every comparison is exact."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SMALL = [0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 2049, 7167, 7168, 7169, 8191, 8192]           # k_rs_small
MERGE = [8193, 9216, 16384, 16385, 24577, 57345, 65535, 65536]                                # k_rs_small per chunk + k_rs_merge
WIDE = [65537, 69631, 69632, 69633, 131073]                                                   # k_rs_hist8 / scan / k_rs_scatter8
REGIMES = {"small": SMALL, "merge": MERGE, "wide": WIDE}
BORDERS = [8192, 8193, 65536, 65537]
ALL_SIZES = [pytest.param(n, id=f"{r}-{n}") for r, ns in REGIMES.items() for n in ns]
ONES = np.uint64(0xffffffffffffffff)
CONST = np.uint64(0x5aa5c33c9669a53c)                   # no byte of it is 0x00 or 0xff


@pytest.fixture(scope="module")
def ctx(api):
    c = api.Context(api.default_params(16, batch=1, max_points=4096))
    yield c
    c.close()


def _vals(rng, n):
    """distinct int32 in random order, a third of them negative (never arange: a sort that regenerated them would pass)"""
    return (rng.permutation(n).astype(np.int64) * 3 - n).astype(np.int32)


def _check(ctx, keys, vals, what):
    keys = np.ascontiguousarray(keys, np.uint64); vals = np.ascontiguousarray(vals, np.int32)
    k0, v0 = keys.copy(), vals.copy()
    gk, gv = ctx.debug_sort_pairs(keys, vals)
    assert (keys == k0).all() and (vals == v0).all()                  # the binding sorts copies
    order = np.argsort(keys, kind="stable")
    bad = np.flatnonzero(gk != keys[order])
    assert bad.size == 0, f"{what}: {bad.size} of {len(keys)} keys out of place, first at {bad[:5].tolist()}"
    bad = np.flatnonzero(gv != vals[order])
    assert bad.size == 0, f"{what}: {bad.size} of {len(keys)} values out of place (stability), first at {bad[:5].tolist()}"


def _one_byte(rng, n, pos, rest):
    """keys that differ in byte `pos` only; every other byte is that of `rest`"""
    mask = np.uint64(0xff) << np.uint64(8 * pos)
    return (rest & ~mask) | (rng.integers(0, 256, n, dtype=np.uint64) << np.uint64(8 * pos))


def _ties_with_padding(rng, n):
    """keys equal to ~0 among keys whose varying bytes (0, 3 and 7) are mostly 0xff: in every pass that runs, real pairs share
    the digit 0xff -- and some the whole key -- with k_rs_small's padding, which must stay behind them all the same"""
    k = np.full(n, ONES, np.uint64)
    for pos in (0, 3, 7):
        b = np.where(rng.random(n) < 0.6, 0xff, rng.integers(0, 256, n)).astype(np.uint64)
        k = (k & ~(np.uint64(0xff) << np.uint64(8 * pos))) | (b << np.uint64(8 * pos))
    k[rng.random(n) < 0.25] = ONES
    return k


FAMILIES = {
    "all_equal": lambda rng, n: np.full(n, CONST, np.uint64),
    "random64": lambda rng, n: rng.integers(0, 2**64, n, dtype=np.uint64),
    "distinct2": lambda rng, n: rng.integers(0, 2**64, 2, dtype=np.uint64)[rng.integers(0, 2, n)],
    "distinct3": lambda rng, n: rng.integers(0, 2**64, 3, dtype=np.uint64)[rng.integers(0, 3, n)],
    "distinct257": lambda rng, n: rng.integers(0, 2**64, 257, dtype=np.uint64)[rng.integers(0, 257, n)],
    "ascending": lambda rng, n: np.sort(rng.integers(0, 2**64, n, dtype=np.uint64)),
    "descending_dups": lambda rng, n: np.sort(rng.integers(0, max(n // 3, 1), n).astype(np.uint64) * np.uint64(0x0000010000000101))[::-1].copy(),
    "ties_with_padding": _ties_with_padding,
    "voxel_shaped": lambda rng, n: (np.sort(rng.integers(0, 75, n)).astype(np.uint64) << np.uint64(32)) | rng.integers(0, 2**20, n, dtype=np.uint64),
}
for _pos in range(8):
    FAMILIES[f"byte{_pos}_varies"] = lambda rng, n, p=_pos: _one_byte(rng, n, p, CONST)
    FAMILIES[f"byte{_pos}_varies_rest_ff"] = lambda rng, n, p=_pos: _one_byte(rng, n, p, ONES)
EVERYWHERE = ("random64", "distinct2", "distinct3", "distinct257")
AT_BORDERS = [f for f in FAMILIES if f not in EVERYWHERE]


@pytest.mark.parametrize("n", ALL_SIZES)
def test_random_and_few_distinct_keys_at_every_size(ctx, n):
    """full random keys (every pass runs) and 2 / 3 / 257 distinct keys (long runs: only a stable sort keeps the values' order; many
    equal digits in one wave row) at every size of every regime"""
    for f in EVERYWHERE:
        rng = np.random.default_rng(n)
        _check(ctx, FAMILIES[f](rng, n), _vals(rng, n), f"{f} n={n}")


@pytest.mark.parametrize("n", BORDERS)
@pytest.mark.parametrize("family", AT_BORDERS)
def test_every_key_family_on_both_sides_of_the_regime_borders(ctx, family, n):
    rng = np.random.default_rng(n)
    _check(ctx, FAMILIES[family](rng, n), _vals(rng, n), f"{family} n={n}")


@pytest.mark.parametrize("regime", list(REGIMES))
def test_ties_with_the_padding_where_the_last_row_is_partial(ctx, regime):
    """sizes that are no multiple of 1024 (k_rs_small pads the last row with all-ones keys) nor of 4096 (the device-wide tiles)"""
    for n in [n for n in REGIMES[regime] if n % 1024]:
        for f in ("ties_with_padding", "byte0_varies_rest_ff", "byte7_varies_rest_ff", "all_equal"):
            rng = np.random.default_rng(n)
            _check(ctx, FAMILIES[f](rng, n), _vals(rng, n), f"{f} n={n}")


# ------------------------------------------------------------------ one workgroup per segment
LENGTHS = np.array([0, 1, 63, 65, 1023, 1024, 1025, 8192])


def _segment_lengths(nseg):
    if nseg == 1:
        return [[int(l)] for l in LENGTHS]
    if nseg == 2:
        return [[0, 8192], [8192, 0], [1023, 1025], [0, 0], [1, 0], [65, 63]]
    rng = np.random.default_rng(nseg)
    lens = LENGTHS[rng.integers(0, len(LENGTHS), nseg)]
    lens[0] = 0; lens[-1] = 0; lens[10:14] = 0                        # empty first, empty last, four empty in a row
    lens[1] = 8192; lens[14] = 1; lens[nseg // 2] = 8192
    return [lens.tolist()]


@pytest.mark.parametrize("leading", [True, False], ids=["keys_lead_with_segment", "keys_ignore_segment"])
@pytest.mark.parametrize("nseg", [1, 2, 75, 300])
def test_segments_are_sorted_on_their_own(ctx, nseg, leading):
    for lens in _segment_lengths(nseg):
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        n = int(off[-1])
        rng = np.random.default_rng(n + nseg)
        if leading:
            keys = (np.repeat(np.arange(nseg, dtype=np.uint64), lens) << np.uint64(32)) | rng.integers(0, 2**20, n, dtype=np.uint64)
        else:                                                         # 257 values shared by all segments: long runs, no segment order
            keys = rng.integers(0, 2**64, 257, dtype=np.uint64)[rng.integers(0, 257, n)]
        vals = _vals(rng, n)
        gk, gv = ctx.debug_sort_pairs(keys, vals, off)
        wk, wv = keys.copy(), vals.copy()
        for s in range(nseg):
            a, b = off[s], off[s + 1]
            order = np.argsort(keys[a:b], kind="stable")
            wk[a:b] = keys[a:b][order]; wv[a:b] = vals[a:b][order]
        bad = np.flatnonzero((gk != wk) | (gv != wv))
        assert bad.size == 0, f"nseg={nseg} lengths={lens[:16]}...: {bad.size} of {n} pairs out of place, first at {bad[:5].tolist()}"


def test_sort_argument_errors(ctx, api):
    k = np.zeros(8193, np.uint64); v = np.zeros(8193, np.int32)
    for off in ([0, 8193], [0, 10, 5, 8193], [1, 8193], [0, 8192]):   # too long a segment, descending, not from 0, not up to n
        with pytest.raises(api.LightLoamError) as e:
            ctx.debug_sort_pairs(k, v, off)
        assert e.value.code == -2, off
    ctx.debug_sort_pairs(k, v, [0, 1, 8193])                          # 8192 pairs in one segment is the limit itself


# ------------------------------------------------------------------ ll_device_exscan
T = 4096
SCAN_SIZES = [1, 2, T - 1, T, T + 1, 2 * T, T * 1023, T * 1024 - 1, T * 1024, T * 1024 + 1, T * 1025, T * T - 1, T * T]


def _scan_data(n):
    rng = np.random.default_rng(n)
    last_tile = ((n - 1) // T) * T
    end_of_a_tile = min(n - 1, (((n - 1) // T) // 2) * T + T - 1)    # the last element of the middle tile (of the only one if partial)
    yield "ones", np.ones(n, np.int32)
    yield "random 0..3", rng.integers(0, 4, n).astype(np.int32)
    for name, at in (("a one that ends a tile", end_of_a_tile), ("a one that starts the last tile", last_tile)):
        d = np.zeros(n, np.int32); d[at] = 1
        yield f"{name} ({at})", d


@pytest.mark.parametrize("n", SCAN_SIZES)
def test_exclusive_scan(ctx, n):
    """two levels of 4096-element tiles; the totals kernel gives a thread 1 tile up to 1024 tiles, up to 4 above"""
    for name, d in _scan_data(n):
        incl = np.cumsum(d, dtype=np.int64)
        assert incl[-1] < 2**31
        want = np.concatenate([[0], incl[:-1]]).astype(np.int32)
        got = ctx.debug_exscan(d)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, f"n={n} {name}: {bad.size} wrong, first at {bad[:5].tolist()}: {got[bad[:5]].tolist()} vs {want[bad[:5]].tolist()}"


def test_scan_argument_errors(ctx, api):
    with pytest.raises(api.LightLoamError) as e:
        ctx.debug_exscan(np.zeros(T * T + 1, np.int32))
    assert e.value.code == -2
    assert len(ctx.debug_exscan(np.zeros(0, np.int32))) == 0
