"""pcl::VoxelGrid on whole clouds (laserMapping's downSizeFilterCorner / downSizeFilterSurf): ll_voxel_grid against the
oracle's restatement, bit for bit (voxel membership and order exact, f32 centroid sums in input order) -- and the form the
cube-map stages use, many clouds ("segments") per call (ll_debug_voxel_segments), against the oracle run per segment: at the
sizes where the sort (8192, 65536) and the finish (65536) change algorithm, with voxel runs across k_vx_finish's 256-point
workgroups, and with segment borders inside a wave, on a wave edge and on a workgroup edge of the bounding-box kernel."""
import numpy as np
import pytest

from conftest import assert_bit_equal

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(api):
    c = api.Context(api.default_params(16, batch=1, max_points=4096))
    yield c
    c.close()


def _cloud(rng, n, extent, lattice=None):
    p = np.zeros((n, 4), np.float32)
    p[:, :3] = rng.uniform(-1, 1, (n, 3)) * extent
    if lattice:
        p[:, :3] = np.round(p[:, :3] / lattice) * lattice           # points exactly on voxel boundaries, duplicates
    p[:, 3] = rng.uniform(0, 64, n)
    return p


@pytest.mark.parametrize("n,extent,leaf,lattice", [
    (1, (1, 1, 1), 0.4, None), (7, (0.1, 0.1, 0.1), 0.4, None), (5000, (30, 30, 3), 0.4, None),
    (60000, (60, 60, 8), 0.8, None), (300000, (120, 120, 10), 0.8, None), (20000, (20, 20, 2), 0.4, 0.2),
    (4097, (10, 10, 10), 0.2, 0.1),
])
def test_matches_oracle(ctx, orc, n, extent, leaf, lattice):
    rng = np.random.default_rng(n)
    pts = _cloud(rng, n, np.array(extent), lattice)
    want = orc.voxel_grid(pts, leaf)
    got = ctx.voxel_grid(pts, leaf)
    assert len(got) == len(want)
    assert_bit_equal(got, want, f"voxel grid n={n} leaf={leaf}")


def test_feature_clouds_of_a_scan(ctx, orc, synth):
    cfg = synth.default_cfg(64)
    f = orc.extract(synth.scan(cfg, 2), orc.params(64))
    for name, leaf in (("less_sharp", 0.4), ("less_flat", 0.8)):                   # laserMapping.cpp:2363-2369
        assert_bit_equal(ctx.voxel_grid(f[name], leaf), orc.voxel_grid(f[name], leaf), name)


def test_leaf_too_small_passes_the_cloud_through(ctx, orc):
    """more than INT_MAX voxels: PCL warns and returns the input unchanged"""
    pts = _cloud(np.random.default_rng(5), 1000, np.array([400, 400, 400]))
    pts[:, :3] = np.abs(pts[:, :3]) + 0.5                                             # no negative zero to lose its sign
    want = orc.voxel_grid(pts, 0.2)
    assert len(want) == len(pts)
    assert_bit_equal(ctx.voxel_grid(pts, 0.2), want, "too small")


def test_empty_and_capacity(ctx, api):
    assert len(ctx.voxel_grid(np.zeros((0, 4), np.float32), 0.4)) == 0
    with pytest.raises(api.LightLoamError):
        ctx.voxel_grid(np.zeros((4, 4), np.float32), 0.0)


# ------------------------------------------------------------------ the size borders through the public entry
def _runs_cloud(rng, n, leaf, origin=(-2, -1, -3)):
    """n points in the cells of a 3 x 3 x k block of voxels, every cell holding 100 .. 700 of them, in random order.  A cell's
    points form one run of the sorted keys: the first run is 256 long, so the second starts exactly on a workgroup of
    k_vx_finish, and the later runs straddle the multiples of 256.  -> (cloud, first sorted position of every run)"""
    counts = [256] if n > 256 else [n]
    while sum(counts) < n:
        counts.append(min(int(rng.integers(100, 701)), n - sum(counts)))
    cell = np.repeat(np.arange(len(counts)), counts)
    ijk = np.stack([cell % 3, (cell // 3) % 3, cell // 9], 1) + np.array(origin)
    p = np.zeros((n, 4), np.float32)
    p[:, :3] = (ijk + rng.uniform(0.1, 0.9, (n, 3))) * leaf           # well inside the cell: f32 rounding cannot move a point out
    p[:, 3] = rng.uniform(0, 64, n)
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]])
    return p[rng.permutation(n)], starts, np.array(counts)


@pytest.mark.parametrize("leaf", [0.4, 0.8])
@pytest.mark.parametrize("n", [8191, 8192, 8193, 65535, 65536, 65537])
def test_long_runs_at_the_sort_and_finish_borders(ctx, orc, n, leaf):
    pts, starts, counts = _runs_cloud(np.random.default_rng(n), n, leaf)
    ends = starts + counts - 1
    assert (starts[1:] % 256 == 0).any()                              # a run that begins a workgroup ...
    assert ((starts % 256 != 0) & (starts // 256 != ends // 256)).any()      # ... and runs that begin in one and end in a later one
    want = orc.voxel_grid(pts, leaf)
    assert len(want) == len(counts)
    assert_bit_equal(ctx.voxel_grid(pts, leaf), want, f"runs n={n} leaf={leaf}")


@pytest.mark.parametrize("n", [257, 65537])
def test_one_voxel(ctx, orc, n):
    """all keys equal (no sort pass runs) and one f32 sum over the whole cloud in input order"""
    rng = np.random.default_rng(n)
    p = np.zeros((n, 4), np.float32)
    p[:, :3] = np.array([-4.0, 8.0, 0.8]) + rng.uniform(0.05, 0.35, (n, 3))
    p[:, 3] = rng.uniform(0, 64, n)
    for leaf in (0.4, 0.8):
        want = orc.voxel_grid(p, leaf)
        assert len(want) == 1
        assert_bit_equal(ctx.voxel_grid(p, leaf), want, f"one voxel n={n} leaf={leaf}")


# ------------------------------------------------------------------ many clouds per call
def _box_cloud(rng, n, center=None, extent=None, lattice=None):
    """n points in a box of its own: centres up to a kilometre from the origin on either side, so a bounding box that leaked from
    one segment into the next would change every voxel index"""
    center = rng.uniform(100, 1000, 3) * rng.choice([-1, 1], 3) if center is None else np.asarray(center, float)
    extent = rng.uniform(1, 6, 3) if extent is None else np.asarray(extent, float)
    if lattice:
        center = np.round(center)                                     # the lattice points stay exact, many on voxel boundaries
    p = _cloud(rng, n, extent, lattice)
    p[:, :3] += center.astype(np.float32)
    p[p == 0] = 0                                                     # no negative zero (a one-point voxel's sum starts from +0)
    return p


def _segments(ctx, orc, clouds, leaf, max_seg_len, what):
    """the clouds as the segments of one call against the oracle per cloud: points bit for bit, seg_count, n_out"""
    off = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.int32)
    pts = np.concatenate(clouds) if len(clouds) else np.zeros((0, 4), np.float32)
    want = [orc.voxel_grid(c, leaf) if len(c) else np.zeros((0, 4), np.float32) for c in clouds]
    got, cnt = ctx.debug_voxel_segments(pts, off, leaf, max_seg_len)
    assert cnt.tolist() == [len(w) for w in want], what
    assert len(got) == sum(len(w) for w in want), what
    assert_bit_equal(got, np.concatenate(want), what)
    return got, cnt


def _longest(clouds):
    return max(len(c) for c in clouds)


@pytest.mark.parametrize("leaf", [0.4, 0.8])
@pytest.mark.parametrize("wave", range(4))
@pytest.mark.parametrize("lengths", [[0, 1, 0, 0, 63, 64, 65, 191, 1, 256, 257, 511, 0],       # borders inside a wave and on wave edges
                                     [256, 0, 256, 64, 192, 300, 0, 0]],                        # borders on workgroup edges
                         ids=["waves", "workgroups"])
def test_segment_borders(ctx, orc, lengths, wave, leaf):
    """The two corners of every segment's box are single points three voxels outside the rest, at the places 64 wave + 17 and
    64 wave + 40 of the segment: the box is right only if the bounding-box kernel keeps what that one wave (or, where a wave
    holds several segments, that one lane) contributes.  Without the low corner the point's voxel index turns negative and it
    sorts last; without the high one the rows of the index get too short and voxels run into each other."""
    rng = np.random.default_rng(len(lengths))
    clouds = [_box_cloud(rng, n, lattice=0.25 if s % 3 == 0 else None) for s, n in enumerate(lengths)]
    for c in clouds:
        if len(c) >= 2:
            hi, lo = (64 * wave + 17) % len(c), (64 * wave + 40) % len(c)
            lo = lo if lo != hi else (hi + 1) % len(c)
            top, bottom = c[:, :3].max(0) + np.float32(3 * leaf), c[:, :3].min(0) - np.float32(3 * leaf)
            c[hi, :3] = top; c[lo, :3] = bottom
    a, ca = _segments(ctx, orc, clouds, leaf, _longest(clouds), f"borders, sort per segment, leaf={leaf}")
    b, cb = _segments(ctx, orc, clouds, leaf, 0, f"borders, one sort, leaf={leaf}")
    assert a.tobytes() == b.tobytes() and (ca == cb).all()


@pytest.fixture(scope="module")
def too_small_clouds():
    rng = np.random.default_rng(5)
    wide = _cloud(rng, 1000, np.array([400, 400, 400]))              # 2001^3 voxels of 0.4 m: more than INT_MAX
    wide[wide == 0] = 0
    return [_box_cloud(rng, 3000), wide, _box_cloud(rng, 6000)]


@pytest.mark.parametrize("sort", ["per_segment", "global"])
def test_leaf_too_small_segment_between_ordinary_ones(ctx, orc, too_small_clouds, sort):
    clouds = too_small_clouds
    assert len(orc.voxel_grid(clouds[1], 0.4)) == len(clouds[1]) and len(orc.voxel_grid(clouds[0], 0.4)) < len(clouds[0])
    got, cnt = _segments(ctx, orc, clouds, 0.4, _longest(clouds) if sort == "per_segment" else 0, f"too small, {sort}")
    assert_bit_equal(got[cnt[0]:cnt[0] + cnt[1]], clouds[1], "the segment passes through")


def _many(rng, lengths):
    return [_box_cloud(rng, n, lattice=0.25 if s % 4 == 1 else None) for s, n in enumerate(lengths)]


COMBOS = {
    # name: (seed, leaf, segment lengths); the longest segment is handed on as max_seg_len, as the cube-map stages do
    "segmented_sort_unfused": (1, 0.4, lambda rng: rng.integers(1500, 2501, 40).tolist()),                    # ~80000 in 40 segments
    "chunk_merge_fused": (2, 0.8, lambda rng: [700, 9000, 0, 1300] + rng.integers(500, 3000, 8).tolist()),    # 8192 < total <= 65536
    "device_wide_unfused": (3, 0.4, lambda rng: [4000, 9000] + rng.integers(5000, 8000, 9).tolist()),         # total > 65536
    "total_65536": (4, 0.8, lambda rng: [30000, 8000, 27536]),                                                # chunk-merge, fused
    "total_65537": (4, 0.8, lambda rng: [30000, 8000, 27537]),                                                # device-wide, unfused
    "total_65536_short_segments": (5, 0.4, lambda rng: [8192] * 8),                                           # segmented, fused
    "total_65537_short_segments": (5, 0.4, lambda rng: [8192] * 7 + [8191, 2]),                               # segmented, unfused
}


@pytest.mark.parametrize("combo", list(COMBOS))
def test_sort_and_finish_combinations(ctx, orc, combo):
    seed, leaf, lengths = COMBOS[combo]
    rng = np.random.default_rng(seed)
    lengths = lengths(rng)
    total, longest = sum(lengths), max(lengths)
    if combo == "segmented_sort_unfused": assert total > 65536 and longest <= 8192
    if combo == "chunk_merge_fused": assert 8192 < total <= 65536 and longest > 8192
    if combo == "device_wide_unfused": assert total > 65536 and longest > 8192
    if combo.startswith("total_"): assert total == int(combo.split("_")[1]) and (longest <= 8192) == combo.endswith("short_segments")
    clouds = _many(rng, lengths)
    _segments(ctx, orc, clouds, leaf, longest, f"{combo} leaf={leaf}")


def test_position_independence(ctx, orc):
    """the same cloud first, in the middle and last in one call, and alone: the same bits every time"""
    rng = np.random.default_rng(11)
    c = _box_cloud(rng, 3001, lattice=0.25)
    others = [_box_cloud(rng, 1999), _box_cloud(rng, 2500)]
    want = orc.voxel_grid(c, 0.4)
    for msl in (3001, 0):
        got, cnt = _segments(ctx, orc, [c, others[0], c, others[1], c], 0.4, msl, f"position, max_seg_len={msl}")
        o = np.concatenate([[0], np.cumsum(cnt)])
        for s in (0, 2, 4):
            assert_bit_equal(got[o[s]:o[s + 1]], want, f"segment {s}")
    alone, cnt = ctx.debug_voxel_segments(c, [0, len(c)], 0.4, 0)
    assert cnt.tolist() == [len(want)]
    assert_bit_equal(alone, want, "alone, segmented entry")
    assert_bit_equal(ctx.voxel_grid(c, 0.4), want, "alone, public entry")


def test_segmented_errors(ctx, orc, api):
    rng = np.random.default_rng(3)
    clouds = [_box_cloud(rng, 300), _box_cloud(rng, 500)]
    pts = np.concatenate(clouds); off = [0, 300, 800]
    m = sum(len(orc.voxel_grid(c, 0.4)) for c in clouds)
    got, _ = ctx.debug_voxel_segments(pts, off, 0.4, 500, cap=m)     # exactly enough
    assert len(got) == m
    with pytest.raises(api.LightLoamError) as e:
        ctx.debug_voxel_segments(pts, off, 0.4, 500, cap=m - 1)
    assert e.value.code == -4 and e.value.n_out == m                  # LL_ERR_CAPACITY, the needed size still reported
    for leaf, bad_off, msl in ((0.0, off, 0), (-0.4, off, 0), (0.4, [0, 500, 300, 800], 0), (0.4, [0, 300, 799], 0), (0.4, off, 499)):
        with pytest.raises(api.LightLoamError) as e:
            ctx.debug_voxel_segments(pts, bad_off, leaf, msl)
        assert e.value.code == -2, (leaf, bad_off, msl)
