"""ll_cubemaps_merge: cube maps combined on the device under a rigid transform.  The expected value never comes from the code under
test: it is built here from per-cube reads taken BEFORE the merge, the CPU oracle's pointAssociateToMap, the cube arithmetic of
laserMapping.cpp:2108-2125 in numpy and the oracle's VoxelGrid.  Every comparison is bytewise.  Most maps are fabricated with
import_maps from seeded random points, so that the boundary cases cost milliseconds.

Synchronisations per call, as lightloam_hip.h and DESIGN.md state them: 3 (per-cube counts, filtered sizes, commit), plus one per
cloud type whose filter call is above 65 536 points and holds a cube above 8 192 points (or one cube only)."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_drives_localize import FIT_FIELDS, IDENT, fit_tuple, localize_chain, make_drives, map_state, step
from test_gpu_map_export import run_frames, same_bytes
from test_gpu_mapping_sequences import CAP, _ctx, _guesses
from test_gpu_sequences import drives

pytestmark = pytest.mark.gpu

ALL, NONE = 1, -1
W, H, D = 21, 21, 11
N = W * H * D
LEAF = (0.4, 0.8)
BASE_SYNCS = 3
EMPTY = np.zeros((0, 4), np.float32)


def yaw_pose(deg, t):
    a = np.deg2rad(deg) / 2
    return np.array([0.0, 0.0, np.sin(a), np.cos(a), t[0], t[1], t[2]])


def cubes_of(pts, cen):
    """:2108-2125 for float32 points: the cube index per point, -1 outside the array"""
    idx = []
    for k in range(3):
        v = pts[:, k].astype(np.float64) + 25.0
        c = np.trunc(v / 50.0).astype(np.int64) + int(cen[k])
        c[v < 0] -= 1
        idx.append(c)
    i, j, k = idx
    inside = (i >= 0) & (i < W) & (j >= 0) & (j < H) & (k >= 0) & (k < D)
    return np.where(inside, i + W * j + W * H * k, -1)


def box(rng, n, lo, hi, intensity=0.0):
    p = rng.uniform(lo, hi, size=(n, 3)).astype(np.float32)
    return np.concatenate([p, np.full((n, 1), intensity, np.float32) + rng.integers(0, 64, (n, 1)).astype(np.float32)], 1)


def make_map(corner, surf, cen=(10, 10, 5), valid=()):
    """world points -> (points in the LL_MAP_ALL layout, layout): binned with the map's centre, order kept inside a cube"""
    counts = np.zeros((2, N), np.int32)
    by_cube = [{}, {}]
    for w, pts in enumerate((corner, surf)):
        pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 4)
        c = cubes_of(pts, cen)
        assert (c >= 0).all(), "a fabricated point lies outside the cube array"
        order = np.argsort(c, kind="stable")
        for cube in np.unique(c):
            by_cube[w][int(cube)] = pts[order][c[order] == cube]
            counts[w, cube] = len(by_cube[w][int(cube)])
    parts = [by_cube[w][c] for c in sorted(set(by_cube[0]) | set(by_cube[1])) for w in (0, 1) if c in by_cube[w]]
    pts = np.concatenate(parts) if parts else EMPTY
    return pts, (np.array(cen, np.int32), counts, np.array(valid, np.int32))


def small_ctx(api):
    return api.Context(api.default_params(16, batch=1, max_points=4096))


def import_all(many, maps):
    """maps[q]: None (left alone) or (points, layout)"""
    off = np.zeros(many.n_seq + 1, np.int64)
    parts = []
    for q, m in enumerate(maps):
        off[q + 1] = off[q] + (0 if m is None else len(m[0]))
        if m is not None:
            parts.append(m[0])
    pts = np.concatenate(parts) if parts else EMPTY
    many.import_maps(pts, off, [None if m is None else m[1] for m in maps])


def cubes(many, q):
    """{(w, cube): cloud} of the non-empty cubes of map q, by per-cube reads"""
    _, counts, _ = many.layout(q)
    return {(w, int(c)): many.cube(q, w, int(c), cap=int(counts[w, c])) for w in (0, 1) for c in np.nonzero(counts[w])[0]}


def state(many):
    pts, off = many.export(ALL)
    lay = [many.layout(q) for q in range(many.n_seq)]
    return pts.tobytes(), off.tobytes(), [tuple(x.tobytes() for x in L) for L in lay], [many.info(q) for q in range(many.n_seq)]


def expected_merge(orc, many, dst, src, T):
    """-> ({(w, cube): cloud} of dst after the merge, added [2], dropped [2], {(w, cube): points that go into the cube's filter});
    call it BEFORE the merge"""
    cen = many.layout(dst)[0]
    want = cubes(many, dst)
    have = cubes(many, src)
    added, dropped, pre = [0, 0], [0, 0], {}
    for w in (0, 1):
        parts = [have[(w, c)] for c in range(N) if (w, c) in have]                  # cube index ascending, own order inside
        if not parts:
            continue
        tp = orc.point_associate_to_map(T[:4], T[4:], np.concatenate(parts))
        c = cubes_of(tp, cen)
        dropped[w] = int((c < 0).sum()); added[w] = int((c >= 0).sum())
        for cube in np.unique(c[c >= 0]):
            cloud = np.concatenate([want.get((w, int(cube)), EMPTY), tp[c == cube]])
            want[(w, int(cube))] = orc.voxel_grid(cloud, LEAF[w])
            pre[(w, int(cube))] = len(cloud)
            assert 0 < len(want[(w, int(cube))]) <= len(cloud)
    return want, added, dropped, pre


def check_map(many, q, want, cen, valid, what):
    """map q equals `want` cube by cube and as an LL_MAP_ALL export; layout counts = cube sizes; centre and valid list as given"""
    c2, counts, v2 = many.layout(q)
    assert tuple(c2) == tuple(cen) and list(v2) == list(valid), what
    size = np.zeros((2, N), np.int32)
    for (w, c), cloud in want.items():
        size[w, c] = len(cloud)
    assert (counts == size).all(), f"{what}: layout counts differ in cubes {np.argwhere(counts != size)[:5].tolist()}"
    for (w, c), cloud in want.items():
        same_bytes(many.cube(q, w, c, cap=max(len(cloud), 1)), cloud, f"{what}: type {w} cube {c}")
    parts = [want[(w, c)] for c in range(N) for w in (0, 1) if (w, c) in want]
    pts, off = many.export([ALL if s == q else NONE for s in range(many.n_seq)])
    same_bytes(pts[off[q]:off[q + 1]], np.concatenate(parts) if parts else EMPTY, f"{what}: whole map")


def scene(seed):
    """src: points in 6 cubes (one cloud of 2500 points: several tiles and chunks; wide boxes that straddle cube faces after T);
    dst: points in 4 cubes, two of them where T takes src's first two boxes; a third map"""
    rng = np.random.default_rng(seed)
    T = yaw_pose(30.0, (12.5, -7.0, 1.0))
    centres = [(-120.0, 40.0, 3.0), (60.0, 110.0, -8.0), (210.0, -160.0, 12.0), (-260.0, -90.0, 1.0), (5.0, 5.0, 0.0), (330.0, 220.0, -4.0)]
    sizes = [700, 2500, 300, 450, 900, 64]
    half = [20.0, 24.0, 6.0, 24.0, 24.0, 3.0]
    src = [np.concatenate([box(rng, n if w == 0 else n // 2 + 1, np.array(c) - h, np.array(c) + h, w) for c, n, h in zip(centres, sizes, half)]) for w in (0, 1)]
    rot = lambda p: np.array([np.cos(np.pi / 6) * p[0] - np.sin(np.pi / 6) * p[1] + 12.5, np.sin(np.pi / 6) * p[0] + np.cos(np.pi / 6) * p[1] - 7.0, p[2] + 1.0])
    dcentres = [rot(centres[0]), rot(centres[1]), (-400.0, 300.0, 20.0), (150.0, 420.0, -30.0)]
    dst = [np.concatenate([box(rng, 600 + 100 * k, np.array(c) - 15.0, np.array(c) + 15.0, w) for k, c in enumerate(dcentres)]) for w in (0, 1)]
    third = [box(rng, 200, (-20.0, -20.0, -5.0), (20.0, 20.0, 5.0), w) for w in (0, 1)]
    return T, make_map(*dst, valid=(2000, 2001, 2022)), make_map(*src), make_map(*third)


def test_general_transform(api, orc):
    T, dst, src, third = scene(1)
    ctx = small_ctx(api)
    many = api.CubeMaps(ctx, 3, 64, 64, pool_points=1 << 15)
    import_all(many, [dst, src, third])
    assert (dst[1][1] > 0).sum() >= 4 * 2 and (src[1][1][0] > 0).sum() >= 6
    before = cubes(many, 0)
    want, added, dropped, pre = expected_merge(orc, many, 0, 1, T)
    touched = {k for k in want if k not in before or want[k].tobytes() != before[k].tobytes()}
    assert len({c for w, c in touched if w == 0} & {c for w, c in before if w == 0}) >= 2      # src lands on cubes dst already holds
    assert len({c for w, c in touched if w == 0} - {c for w, c in before if w == 0}) >= 4      # ... and on empty ones
    s1, s2 = state_of(many, 1), state_of(many, 2)
    sy0, f0 = many.stats()
    got_added, got_dropped = many.merge([(0, 1, T)])
    assert many.stats() == (sy0 + BASE_SYNCS, f0)
    assert got_added.tolist() == [added] and got_dropped.tolist() == [dropped] and dropped == [0, 0]
    check_map(many, 0, want, dst[1][0], dst[1][2], "dst")
    for k in before:                                                                # untouched cubes byte for byte
        if k not in touched:
            same_bytes(many.cube(0, k[0], k[1], cap=len(before[k])), before[k], f"untouched cube {k}")
    assert state_of(many, 1) == s1 and state_of(many, 2) == s2
    ms, cnt = many.merge_timing()
    assert cnt[0] == len(src[0]) and cnt[1] == len(touched) and cnt[2] == sum(len(want[k]) for k in touched) and all(m >= 0 for m in ms)
    many.close(); ctx.close()


def state_of(many, q):
    pts, off = many.export([ALL if s == q else NONE for s in range(many.n_seq)])
    return pts.tobytes(), tuple(x.tobytes() for x in many.layout(q)), many.info(q)


def test_identity_into_a_reset_map(api, orc):
    T, dst, src, third = scene(2)
    ctx = small_ctx(api)
    many = api.CubeMaps(ctx, 2, 64, 64, pool_points=1 << 15)
    import_all(many, [dst, src])
    many.reset(0)
    have = cubes(many, 1)
    added, dropped = many.merge([(0, 1, IDENT)])
    want = {k: orc.voxel_grid(v, LEAF[k[0]]) for k, v in have.items()}
    assert added.tolist() == [[int(src[1][1][w].sum()) for w in (0, 1)]] and dropped.tolist() == [[0, 0]]
    check_map(many, 0, want, (10, 10, 5), (), "identity")
    many.close(); ctx.close()


def test_negative_coordinates_moved_centre_and_drops(api, orc):
    """dst's centre is (3, 17, 5): cube index 20 ends at x = (21 - 3) * 50 - 25 = 875; T (+380 on x, a small yaw) lays one box of
    src across that edge and another across x + 25 = 0, y and z negative"""
    rng = np.random.default_rng(3)
    src = [np.concatenate([box(rng, 1500, (440.0, -300.0, -60.0), (520.0, -250.0, -20.0), w),
                           box(rng, 500, (-420.0, -300.0, -60.0), (-390.0, -250.0, -20.0), w)]) for w in (0, 1)]
    dst = [box(rng, 800, (-40.0, -330.0, -50.0), (-10.0, -270.0, -30.0), w) for w in (0, 1)]
    T = yaw_pose(0.6, (380.0, 0.0, 0.0))
    ctx = small_ctx(api)
    many = api.CubeMaps(ctx, 2, 64, 64, pool_points=1 << 15)
    import_all(many, [make_map(*dst, cen=(3, 17, 5)), make_map(*src)])
    want, added, dropped, pre = expected_merge(orc, many, 0, 1, T)
    s1 = state_of(many, 1)
    got_added, got_dropped = many.merge([(0, 1, T)])
    assert got_added.tolist() == [added] and got_dropped.tolist() == [dropped]
    for w in (0, 1):
        assert 0.2 * 2000 <= dropped[w] <= 0.8 * 2000 and added[w] + dropped[w] == 2000, (added, dropped)
    xs = np.concatenate([v[:, 0] for k, v in want.items()])
    assert (xs < -25.0).any() and (xs > -25.0).any() and (xs > 850.0).any() and not (xs >= 875.0).any()
    check_map(many, 0, want, (3, 17, 5), (), "moved centre")
    assert state_of(many, 1) == s1
    many.close(); ctx.close()


def test_sizes_at_which_the_kernels_can_go_wrong(api, orc):
    """source clouds of 0, 1, 63, 64, 65, 255, 256, 257 points; a merged corner cube above 8 192 points (the filter call stays
    below 65 536: no read-back) and a merged surf cube above 65 536 (one read-back)"""
    rng = np.random.default_rng(4)
    sizes = [0, 1, 63, 64, 65, 255, 256, 257]
    at = lambda k: np.array([-200.0 + 50.0 * k, 100.0, 0.0])                        # one cube each along x, at its middle
    small = [np.concatenate([box(rng, n, at(k) - 20.0, at(k) + 20.0, w) for k, n in enumerate(sizes) if n]) for w in (0, 1)]
    big_c, big_s = np.array([0.0, -100.0, 0.0]), np.array([100.0, -100.0, 0.0])
    src = [np.concatenate([small[0], box(rng, 5000, big_c - 20.0, big_c + 20.0)]), np.concatenate([small[1], box(rng, 40000, big_s - 20.0, big_s + 20.0, 1)])]
    dst = [np.concatenate([box(rng, 4000, big_c - 20.0, big_c + 20.0), box(rng, 10, at(3) - 20.0, at(3) + 20.0)]),
           np.concatenate([box(rng, 30000, big_s - 20.0, big_s + 20.0, 1), box(rng, 10, at(5) - 20.0, at(5) + 20.0, 1)])]
    T = yaw_pose(0.0, (1.5, -2.0, 0.5))
    ctx = small_ctx(api)
    many = api.CubeMaps(ctx, 2, 64, 64, pool_points=1 << 17)
    import_all(many, [make_map(*dst), make_map(*src)])
    counts = many.layout(1)[1]
    assert sorted(set(counts[0][counts[0] > 0].tolist())) == [1, 63, 64, 65, 255, 256, 257, 5000]
    want, added, dropped, pre = expected_merge(orc, many, 0, 1, T)
    extra = 0
    for w in (0, 1):                                                                # the filter calls as the documentation describes them
        seg = [n for (t, c), n in pre.items() if t == w]
        extra += int(sum(seg) > 65536 and (len(seg) == 1 or max(seg) > 8192))
        assert max(seg) > (8192, 65536)[w] and len(seg) > 1
    assert extra == 1 and sum(n for (t, c), n in pre.items() if t == 0) < 65536
    sy0, f0 = many.stats()
    got_added, got_dropped = many.merge([(0, 1, T)])
    assert many.stats() == (sy0 + BASE_SYNCS + extra, f0)
    assert got_added.tolist() == [added] and got_dropped.tolist() == [dropped]
    check_map(many, 0, want, (10, 10, 5), (), "sizes")
    many.close(); ctx.close()


def five_maps(api, ctx, seed):
    rng = np.random.default_rng(seed)
    maps = []
    for q in range(5):
        c = np.array([40.0 * q - 80.0, 30.0 * q - 60.0, 0.0])
        maps.append(make_map(*[box(rng, 900 + 150 * q, c - 24.0, c + 24.0, w) for w in (0, 1)]))
    many = api.CubeMaps(ctx, 5, 64, 64, pool_points=1 << 15)
    import_all(many, maps)
    return many


def test_many_ops_equal_one_op_at_a_time(api, orc):
    ops = [(0, 3, yaw_pose(12.0, (20.0, 5.0, 0.0))), (1, 4, yaw_pose(-40.0, (-30.0, 10.0, 2.0))), (2, 3, yaw_pose(75.0, (0.0, -45.0, -1.0)))]
    ctx = small_ctx(api)
    a, b = five_maps(api, ctx, 5), five_maps(api, ctx, 5)
    assert state(a) == state(b)
    want = [expected_merge(orc, a, d, s, T)[:3] for d, s, T in ops]
    sa = a.stats()[0]
    added, dropped = a.merge(ops)
    d3 = a.stats()[0] - sa
    rows = []
    for op in ops:
        sb = b.stats()[0]
        rows.append(b.merge([op]))
        assert b.stats()[0] - sb == d3 == BASE_SYNCS                                # the same whatever the number of ops
    assert added.tolist() == [r[0][0].tolist() for r in rows] == [w[1] for w in want]
    assert dropped.tolist() == [r[1][0].tolist() for r in rows] == [w[2] for w in want]
    assert state(a) == state(b)
    for (d, s, T), w in zip(ops, want):
        check_map(a, d, w[0], (10, 10, 5), (), f"map {d}")
    a.close(); b.close(); ctx.close()


def test_determinism(api):
    T, dst, src, third = scene(6)
    ctx = small_ctx(api)
    out = []
    for _ in range(2):
        many = api.CubeMaps(ctx, 3, 64, 64, pool_points=1 << 15)
        import_all(many, [dst, src, third])
        many.merge([(0, 1, T), (2, 1, IDENT)])
        out.append(state(many))
        many.close()
    assert out[0] == out[1]
    ctx.close()


def test_tables_stay_sound(api, synth):
    """two real maps (16-ring synthetic drives, 3 frames each), map 1 merged into map 0, then map 0 runs frame 3; a second object whose
    map 0 is the post-merge export + layout runs the same frame"""
    S, n = 2, 4
    cfgs, scans, _ = drives(synth, 16, S, n)
    ctx = _ctx(api, 16, scans)
    c, s, pool = CAP[16]
    a = api.CubeMaps(ctx, S, c, s, pool_points=pool)
    for k in range(n - 1):
        a.process_slots(_guesses(synth, cfgs, k, [(0.0, 0.0, 0.0)] * S), [k * S + q for q in range(S)])
    before = state_of(a, 0)
    added, dropped = a.merge([(0, 1, yaw_pose(3.0, (0.5, -0.25, 0.0)))])
    assert added.min() > 0 and state_of(a, 0)[0] != before[0]
    pts, off = a.export([ALL, NONE])
    b = api.CubeMaps(ctx, S, c, s, pool_points=pool)
    b.import_maps(pts, off, [a.layout(0), None])
    guess = _guesses(synth, cfgs, n - 1, [(0.0, 0.0, 0.0)] * S)
    slots = [(n - 1) * S, -1]
    pa, ra = a.process_slots(guess, slots)
    pb, rb = b.process_slots(guess, slots)
    assert pa[0].tobytes() == pb[0].tobytes() and ra[0] and rb[0]
    for which in range(4):
        same_bytes(a.cloud(0, which), b.cloud(0, which), f"cloud {which}")
    assert state_of(a, 0) == state_of(b, 0)
    a.close(); b.close(); ctx.close()


def test_capacity(api):
    """dst holds 3000 corner points and receives 2000: pool_points 4999 is refused with nothing changed, 5000 is enough"""
    rng = np.random.default_rng(8)
    dst = make_map(box(rng, 3000, (-24.0, -24.0, -10.0), (24.0, 24.0, 10.0)), box(rng, 100, (-24.0, -24.0, -10.0), (24.0, 24.0, 10.0), 1))
    src = make_map(box(rng, 2000, (-20.0, -20.0, -8.0), (70.0, 20.0, 8.0)), box(rng, 100, (-20.0, -20.0, -8.0), (70.0, 20.0, 8.0), 1))
    ctx = small_ctx(api)
    for pool, ok in ((4999, False), (5000, True)):
        many = api.CubeMaps(ctx, 2, 64, 64, pool_points=pool)
        import_all(many, [dst, src])
        before = state(many)
        if ok:
            added, dropped = many.merge([(0, 1, IDENT)])
            assert added.tolist() == [[2000, 100]] and dropped.tolist() == [[0, 0]] and state(many) != before
            assert many.layout(0)[1][0].sum() <= 5000
        else:
            with pytest.raises(api.LightLoamError) as e:
                many.merge([(0, 1, IDENT)])
            assert e.value.code == -4 and "op 0" in str(e.value) and "corner" in str(e.value), e.value
            assert state(many) == before
        many.close()
    ctx.close()


def test_refusals(api):
    T, dst, src, third = scene(9)
    ctx = small_ctx(api)
    many = api.CubeMaps(ctx, 3, 64, 64, pool_points=1 << 15)
    import_all(many, [dst, src, third])
    before = state(many)
    bad_T = [np.r_[IDENT[:6], np.nan], np.r_[np.inf, IDENT[1:]]]
    cases = [[], [(0, 3, IDENT)], [(-1, 1, IDENT)], [(0, -1, IDENT)], [(3, 1, IDENT)], [(1, 1, IDENT)],
             [(0, 1, IDENT), (0, 2, IDENT)],                                       # dst of two ops
             [(0, 1, IDENT), (1, 2, IDENT)], [(0, 1, IDENT), (2, 0, IDENT)],       # dst of one op, src of another
             [(0, 1, bad_T[0])], [(2, 1, IDENT), (0, 1, bad_T[1])]]
    for ops in cases:
        with pytest.raises(api.LightLoamError) as e:
            many.merge(ops)
        assert e.value.code == -2, (ops, e.value)
    op = api.MergeOp(0, 1, (C.c_double * 7)(*IDENT))
    assert many.lib.ll_cubemaps_merge(None, C.addressof(op), 1, None, None) == -2
    assert many.lib.ll_cubemaps_merge(many.h, None, 1, None, None) == -2
    assert many.lib.ll_cubemaps_merge_timing(None, None, None) == -2
    assert state(many) == before
    sy = many.stats()
    assert many.lib.ll_cubemaps_merge(many.h, C.addressof(op), 1, None, None) == 0   # a map may be src of several ops; NULL outputs
    many.merge([(0, 1, IDENT), (2, 1, IDENT)])
    assert many.stats()[0] == sy[0] + 2 * BASE_SYNCS and state(many) != before
    many.close(); ctx.close()


def test_drives(api, synth):
    """lanes 0 and 1 map drives A and B and go idle; lane 1's map is merged into lane 0's through Drives.cubemaps between two
    steps; lane 2 then localises drive A against map 0: the single localising chain on the merged map imported into a plain
    CubeMap / CubeMaps (localize_chain asserts that CubeMaps.localize_slots agrees and returns its fit records)"""
    n_map, n_loc, J = 5, 3, 1
    _, scans, pose0 = drives(synth, 16, 2, n_map)
    ctx, dr = make_drives(api, scans)
    started, mapped0 = set(), []
    for k in range(n_map):
        _, mapped, _ = step(api, ctx, dr, {0: (0, k), 1: (1, k)}, scans, pose0, started)
        mapped0.append(mapped[0].copy())
    dr.step(np.zeros(3, np.int32))                                                  # both lanes go IDLE
    before = map_state(api, dr, 0)
    src = map_state(api, dr, 1)
    s0 = dr.stats()
    added, dropped = dr.cubemaps.merge([(0, 1, yaw_pose(2.0, (0.4, 0.3, 0.0)))])
    assert added.min() > 0 and dr.stats() == s0                                     # ll_drives_stats counts the steps' synchronisations only
    merged = map_state(api, dr, 0)
    assert merged[0].tobytes() != before[0].tobytes() and merged[1][0].tolist() == before[1][0].tolist()
    assert map_state(api, dr, 1)[0].tobytes() == src[0].tobytes()
    start = np.tile(IDENT, (3, 1)); start[2] = mapped0[J]
    dr.set_localize([-1, -1, 0], start)
    started, got = set(), []
    for t in range(n_loc):
        odom, mapped, ran = step(api, ctx, dr, {2: (0, J + t)}, scans, pose0, started)
        got.append((odom[2].copy(), mapped[2].copy(), bool(ran[2]), fit_tuple(dr.fit()[2])))
    assert map_state(api, dr, 0)[0].tobytes() == merged[0].tobytes()
    odom, mapped, ran, fits, _ = localize_chain(api, scans[0][J:J + n_loc], pose0[0], start[2], merged[0], merged[1])
    for k in range(n_loc):
        assert (got[k][0] == odom[k]).all() and (got[k][1] == mapped[k]).all(), f"frame {k} pose"
        assert got[k][2] == bool(ran[k]) and got[k][2], k
        assert got[k][3] == fits[k] and fits[k][0] > 10 and fits[k][1] > 50, (k, got[k][3], fits[k])
    assert len(FIT_FIELDS) == 5
    dr.close(); ctx.close()
