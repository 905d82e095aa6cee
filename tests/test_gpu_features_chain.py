"""k_ring_features' serial chain (ll_features.hip): the ring's points are requested before the lists and the pick bitmap are built, and a
voxel run that is open at the end of its thread's range goes on through the registers of the following lanes of its wave before it
goes to memory.  Nothing of either may show: the four published clouds against the oracle, bit for bit.  (`ring_nlf`, the rings' less-flat
counts, has no getter: the contiguous less-flat cloud the ABI hands out is assembled from it -- a wrong count moves or drops points.)

The crafted rings walk a straight line beside the sensor (x fixed, y falling) at EQUAL steps of 0.2 m / L: every 0.2 m voxel holds L
consecutive points and the 11-tap curvature is zero, so no point is picked as sharp or less-sharp and the ring's sorted records are
runs of exactly L.  `_runs` restates the kernel's bookkeeping (thread t owns sorted places [t perm, (t + 1) perm), perm =
ceil(m / 256); 64 threads to a wave) from the oracle's labels, and the tests assert that the runs they mean to exercise are there:
runs that end in their own thread, in lane +1, +2, +3 and beyond, begun in lane 0, in a middle lane, in lane 62 and in lane 63."""
import numpy as np
import pytest

from conftest import assert_bit_equal

pytestmark = pytest.mark.gpu

LEAF = 0.2                       # scanRegistration.cpp:370: the less-flat cloud's VoxelGrid
RANKS = [0, 1]                   # ll_params.voxel_sort_ranks: the sort's two rankings (k_ring_features<.., false / true>)


def _line_ring(elev_deg, n, per_voxel, first=0.0, x=1.05, bumps=(), bump=0.05):
    """n points on the line x = const, y falling from -0.4 in steps of LEAF / per_voxel (`first`: fraction of a voxel the walk starts
    into its first voxel), z at the ring's elevation.  bumps: local indices pushed `bump` outwards (curvature 0.25: picked)."""
    step = LEAF / per_voxel
    y = -(0.4 + LEAF * first + step * (np.arange(n) + 0.5))
    xs = np.full(n, x)
    xs[list(bumps)] += bump
    z = np.hypot(xs, y) * np.tan(np.deg2rad(elev_deg))
    return np.stack([xs, y, z], axis=1)


def _scan(rings):
    pts = np.concatenate(rings).astype(np.float32)
    return np.concatenate([pts, np.zeros((len(pts), 1), np.float32)], axis=1)


def _runs(scan, label, lengths):
    """Per ring of a ring-major scan: (perm, [(sorted place of the run's head, points)]) of the less-flat records as the kernel sorts
    them -- by voxel (z, y, x index, f32 as pcl::VoxelGrid computes them), input order inside a voxel."""
    out, off = [], 0
    for nr in lengths:
        idx = np.arange(off + 5, off + nr - 6) if nr - 11 >= 6 else np.zeros(0, np.int64)
        off += nr
        mem = idx[label[idx] <= 0]
        m = len(mem)
        if m == 0:
            out.append((0, []))
            continue
        ijk = np.floor(scan[mem, :3] * np.float32(1.0 / LEAF)).astype(np.int64)
        order = np.lexsort((np.arange(m), ijk[:, 0], ijk[:, 1], ijk[:, 2]))
        key = ijk[order]
        head = np.concatenate([[True], (key[1:] != key[:-1]).any(axis=1)])
        starts = np.flatnonzero(head)
        out.append(((m + 255) // 256, list(zip(starts.tolist(), np.diff(np.concatenate([starts, [m]])).tolist()))))
    return out


def _reach(perm, p, n):
    """how a run goes on: (lane of its head, threads beyond its own that hold its points, does it leave its wave)"""
    t0, t1 = p // perm, (p + n - 1) // perm
    return t0 % 64, t1 - t0, t0 // 64 != t1 // 64


def _extract_and_compare(api, orc, scan, rings, ranks, what, max_ring_points=2304):
    ref = orc.extract(scan, orc.params(rings, minimum_range=0.3))
    assert ref["rc"] == 0, what
    ctx = api.Context(api.default_params(rings, batch=1, max_points=len(scan) + 8, minimum_range=0.3, max_ring_points=max_ring_points,
                                         voxel_sort_ranks=ranks))
    try:
        ctx.upload_scan(0, scan)
        ctx.extract(0, 1)
        assert ctx.scan_info(0).status == 0
        f = ctx.features(0)
        for name in ("sharp", "less_sharp", "flat", "less_flat"):
            assert_bit_equal(f[name], ref[name], f"{what} {name}")
    finally:
        ctx.close()
    return ref


# ------------------------------------------------------------------ run lengths x head lanes
# perm = 4 (768 < m <= 1024).  Points per voxel: 2, perm, perm + 1, 2 perm + 1, 3 perm + 1 and > 4 perm; three rings of each, started
# 0, 1/3 and 2/3 of a voxel into their first one and a few points apart in length, so that the heads fall on different lanes.
# The line's z follows its range (one laser: one elevation), so a ring crosses a voxel border in z now and then and splits a run there:
# the longest lines (fewest points per voxel) take the flattest of the 64 lasers, and no ring splits more than a few of its runs.
RUN_LENGTHS = (2, 4, 5, 9, 13, 19)
RUN_LASERS = {2: (57, 58, 59), 4: (56, 60, 61), 5: (55, 62, 63), 9: (52, 53, 54), 13: (49, 50, 51), 19: (46, 47, 48)}


def _run_scan():
    spec = sorted((laser, per_voxel, j) for per_voxel in RUN_LENGTHS for j, laser in enumerate(RUN_LASERS[per_voxel]))
    rings, lengths = [], []
    for laser, per_voxel, j in spec:                     # ring-major: ascending laser
        n = 1013 if (per_voxel, j) == (19, 0) else 1011 + 4 * j + RUN_LENGTHS.index(per_voxel)      # m = n - 11; 1013: a run of 19 headed in lane 0
        rings.append(_line_ring(-24.9 + 26.9 * laser / 63.0, n, per_voxel, first=j / 3.0))
        lengths.append(n)
    return _scan(rings), lengths


@pytest.fixture(scope="module")
def run_case(orc):
    scan, lengths = _run_scan()
    ref = orc.extract(scan, orc.params(64, minimum_range=0.3))
    return scan, lengths, ref


def test_the_crafted_runs_are_the_ones_meant(run_case):
    """the construction, before anything runs on the device: no less-sharp pick, perm = 4, and for every run length heads in lane 0, in
    a middle lane, in lane 62 and in lane 63; runs ending in their own thread, in lane +1, +2, +3 and beyond; runs that leave
    their wave from lane 62 and 63 (the memory path)"""
    scan, lengths, ref = run_case
    assert ref["rc"] == 0 and len(ref["label"]) == len(scan)
    assert len(ref["less_sharp"]) == 0, "equal steps: no curvature above the pick's threshold"
    runs = _runs(scan, ref["label"], lengths)
    seen = {}
    for (perm, rr), nr in zip(runs, lengths):
        assert perm == 4
        for p, n in rr:
            lane, beyond, leaves = _reach(perm, p, n)
            seen.setdefault(n, set()).add((lane, beyond, leaves))
    for n in RUN_LENGTHS:
        lanes = {l for l, _, _ in seen[n]}
        assert {0, 62, 63} <= lanes and any(8 <= l <= 55 for l in lanes), (n, sorted(lanes))
    beyond = lambda n: {b for _, b, _ in seen[n]}
    assert 0 in beyond(2) and 0 in beyond(4) and 1 in beyond(5) and 2 in beyond(9) and 3 in beyond(13) and max(beyond(19)) >= 4
    for n in (5, 9, 13, 19):                             # from lane 63 every one of them leaves the wave, from lane 62 those beyond lane +1
        assert any(l == 63 and lv for l, _, lv in seen[n]) and any(l == 62 and lv == (n > 5) for l, _, lv in seen[n]), n
        assert any(l == 0 and not lv for l, _, lv in seen[n]), n


@pytest.mark.parametrize("ranks", RANKS)
def test_runs_of_every_length_from_every_lane(api, orc, run_case, ranks):
    scan, lengths, ref = run_case
    got = _extract_and_compare(api, orc, scan, 64, ranks, f"runs, ranks={ranks}")
    assert len(got["less_flat"]) == sum(len(rr) for _, rr in _runs(scan, ref["label"], lengths))


# ------------------------------------------------------------------ ring lengths: rows, the first and the last loaded row
def _length_scan():
    """nrec = ring length - 6 = 256 k - 1, 256 k, 256 k + 1 for k = 1 .. 3 (a wave's last row full, one short, one over), rings of 11, 16
    and 17 points (no segment / no segment / the shortest one) and empty rings (8, 12, 15: no point has their elevation).  Ring 7, the
    flattest, has bumps on its first and on its last segment point and every 60 points between: less-sharp picks in the first and
    in the last loaded row, and voxels whose equal keys a pick splits in input order.  -> scan, ring lengths, ring 7's place, bumps"""
    n = 700
    bumps = sorted({5, n - 7} | set(range(40, n - 20, 60)))
    spec = {i: (256 * k + d + 6, 3, ()) for i, (k, d) in zip((0, 1, 2, 3, 4, 5, 6, 9, 10), [(k, d) for k in (1, 2, 3) for d in (-1, 0, 1)])}
    spec.update({11: (11, 3, ()), 13: (16, 3, ()), 14: (17, 3, ()), 7: (n, 9, bumps)})
    order = sorted(spec)
    rings = [_line_ring(-15 + 2 * i, spec[i][0], spec[i][1], first=0.5 * (i % 2), bumps=spec[i][2]) for i in order]
    return _scan(rings), [spec[i][0] for i in order], order.index(7), bumps


@pytest.mark.parametrize("ranks", RANKS)
def test_ring_lengths_at_the_row_borders_and_picks_in_the_outer_rows(api, orc, ranks):
    scan, lengths, at, bumps = _length_scan()
    ref = _extract_and_compare(api, orc, scan, 16, ranks, f"lengths, ranks={ranks}")
    off = sum(lengths[:at])
    lab = ref["label"][off:off + lengths[at]]
    assert lab[5] > 0 and lab[lengths[at] - 7] > 0, "picks on the first and on the last segment point"
    assert (lab[bumps] > 0).all() and len(ref["less_sharp"]) >= len(bumps)
    perm, rr = _runs(scan, ref["label"], lengths)[at]
    assert sum(n == 8 for _, n in rr) >= len(bumps) // 2, "a pick inside a voxel of nine leaves one run of eight"


# ------------------------------------------------------------------ the tiers of long rings
@pytest.mark.parametrize("ranks", RANKS)
def test_runs_in_the_long_ring_tiers(api, orc, ranks):
    """max_ring_points 4608 (hdl64): rings of 2305 .. 3072 points go to the 12-row instantiation, longer ones to the 18-row one; perm
    is 9 .. 18 there.  Runs of 2, perm + 1, 2 perm + 1, 3 perm + 1 and > 4 perm points, and a short ring for the main launch."""
    spec = [(2600, 2), (2900, 12), (3000, 23), (3072, 37), (3500, 15), (3700, 29), (4100, 50), (4608, 80), (900, 5)]
    rings = [_line_ring(-15 + 2 * i, n, per_voxel, first=(i % 3) / 3.0) for i, (n, per_voxel) in enumerate(spec)]
    scan = _scan(rings)
    ref = _extract_and_compare(api, orc, scan, 16, ranks, f"tiers, ranks={ranks}", max_ring_points=4608)
    reach = set()
    for (perm, rr), (n, per_voxel) in zip(_runs(scan, ref["label"], [n for n, _ in spec]), spec):
        assert perm == (n - 11 + 255) // 256
        reach |= {min(_reach(perm, p, k)[1], 9) for p, k in rr}
    assert {0, 1, 2, 3} <= reach and max(reach) >= 4
