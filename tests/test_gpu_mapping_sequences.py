"""ll_cubemaps: laserMapping's cube map for S sequences side by side (laserMapping.cpp:1584-2165).  Sequence q must equal an
ll_cubemap created with the same parameters and driven with the same frames, bit for bit: pose, ran, cen, the four clouds and
every cube."""
import ctypes as C

import numpy as np
import pytest

from conftest import assert_bit_equal
from test_gpu_sequences import drives, max_points

pytestmark = pytest.mark.gpu

CAP = {16: (4096, 32768, 1 << 18), 64: (16384, 131072, 1 << 20)}


def _pose7(pose3, offset=(0.0, 0.0, 0.0)):
    x, y, yaw = pose3
    return np.array([0.0, 0.0, np.sin(yaw / 2), np.cos(yaw / 2), x + offset[0], y + offset[1], offset[2]])


def _ctx(api, rings, scans):
    """frame k of sequence q in slot k * S + q, all extracted"""
    S, n = len(scans), len(scans[0])
    ctx = api.Context(api.default_params(rings, batch=S * n, max_points=max_points(scans)))
    for k in range(n):
        for q in range(S):
            ctx.upload_scan(k * S + q, scans[q][k])
    ctx.extract(0, S * n)
    return ctx


def _nonempty(cube, q=None):
    args = (lambda s, i: (q, s, i)) if q is not None else (lambda s, i: (s, i))
    return [(s, i) for s in (0, 1) for i in range(4851) if len(cube(*args(s, i)))]


def _assert_same(many, q, one, what):
    assert many.info(q) == one.info(), what
    for which in range(4):
        assert_bit_equal(many.cloud(q, which), one.cloud(which), f"{what}: cloud {which}")
    cubes = _nonempty(one.cube)
    assert cubes == _nonempty(many.cube, q), what
    for s, i in cubes:
        assert_bit_equal(many.cube(q, s, i), one.cube(s, i), f"{what}: cube {s} {i}")


def _guesses(synth, cfgs, k, offsets):
    return np.array([_pose7(synth.pose(c, k), o) + np.array([0, 0, 0, 0, 0.05, -0.02, 0.01]) for c, o in zip(cfgs, offsets)])


def _run_pair(api, synth, rings, S, n, offsets):
    cfgs, scans, _ = drives(synth, rings, S, n)
    ctx = _ctx(api, rings, scans)
    c, s, pool = CAP[rings]
    many = api.CubeMaps(ctx, S, c, s, pool_points=pool)
    ones = [api.CubeMap(ctx, c, s, pool_points=pool) for _ in range(S)]
    for k in range(n):
        guess = _guesses(synth, cfgs, k, offsets)
        poses, ran = many.process_slots(guess, [k * S + q for q in range(S)])
        for q in range(S):
            p1, r1 = ones[q].process_slot(guess[q], k * S + q)
            assert ran[q] == r1 == (k > 0), (k, q)
            assert_bit_equal(poses[q], p1, f"frame {k} sequence {q} pose")
    for q in range(S):
        _assert_same(many, q, ones[q], f"sequence {q}")
    syncs, frames = many.stats()
    assert frames == n and syncs <= 5 * n + 4 * n, (syncs, frames)      # five per frame + the filters' own read-backs
    return ctx, many, ones


@pytest.mark.parametrize("rings,S,n", [(16, 5, 7), (64, 3, 5)])
def test_bit_identical_to_single_maps(api, synth, rings, S, n):
    ctx, many, ones = _run_pair(api, synth, rings, S, n, [(0.0, 0.0, 0.0)] * S)
    for o in ones:
        o.close()
    many.close(); ctx.close()


def test_shift_loops_and_negative_coordinates(api, synth):
    """sequences that start far apart: the first prepare shifts every axis for some sequences and none for others"""
    offsets = [(-431.0, 512.5, 30.0), (0.0, 0.0, 0.0), (260.0, -140.0, -60.0), (0.0, 0.0, 0.0)]
    ctx, many, ones = _run_pair(api, synth, 16, 4, 5, offsets)
    assert many.info(0)[0] != (10, 10, 5) and many.info(1)[0] == (10, 10, 5)
    for o in ones:
        o.close()
    many.close(); ctx.close()


def test_ragged_frames_and_a_late_start(api, synth):
    """sequence 1 sits out frames 2 and 4 (nothing of it changes); sequence 3 starts at frame 3 beside running ones"""
    S, n = 4, 6
    cfgs, scans, _ = drives(synth, 16, S, n)
    ctx = _ctx(api, 16, scans)
    c, s, pool = CAP[16]
    many = api.CubeMaps(ctx, S, c, s, pool_points=pool)
    ones = [api.CubeMap(ctx, c, s, pool_points=pool) for _ in range(S)]
    ran_prev = np.array([7, 7, 7, 7], np.int32)
    for k in range(n):
        guess = _guesses(synth, cfgs, k, [(0.0, 0.0, 0.0)] * S)
        slots = [k * S + q for q in range(S)]
        if k in (2, 4):
            slots[1] = -1
        if k < 3:
            slots[3] = -1
        before = {q: (many.info(q), [(s_, i, many.cube(q, s_, i)) for s_, i in _nonempty(many.cube, q)])
                  for q in range(S) if slots[q] < 0}
        # the raw call: the untouched rows of pose and ran must come back as they went in
        p = np.ascontiguousarray(guess, np.float64).copy(); p[1] = guess[1] if slots[1] >= 0 else 123.0
        ran = ran_prev.copy()
        sl = np.array(slots, np.int32)
        rc = many.lib.ll_cubemaps_process_slots(many.h, sl.ctypes.data_as(C.c_void_p), p.ctypes.data_as(C.c_void_p), ran.ctypes.data_as(C.c_void_p))
        assert rc == 0, many.lib.ll_cubemaps_last_error(many.h)
        for q in range(S):
            if slots[q] < 0:
                assert ran[q] == 7
                assert (p[q] == (123.0 if q == 1 else guess[q])).all()
                info, cubes = before[q]
                assert many.info(q) == info
                assert [(s_, i) for s_, i, _ in cubes] == _nonempty(many.cube, q)
                for s_, i, pts in cubes:
                    assert_bit_equal(many.cube(q, s_, i), pts, f"frame {k} idle sequence {q} cube {s_} {i}")
                continue
            p1, r1 = ones[q].process_slot(guess[q], slots[q])
            assert ran[q] == r1, (k, q)
            assert_bit_equal(p[q], p1, f"frame {k} sequence {q}")
            if q == 3 and k == 3:
                assert r1 is False                                              # a fresh map: the :1822 gate
    for q in range(S):
        _assert_same(many, q, ones[q], f"sequence {q}")
    for o in ones:
        o.close()
    many.close(); ctx.close()


def test_host_clouds_equal_slots(api, synth):
    S, n = 3, 4
    cfgs, scans, _ = drives(synth, 16, S, n)
    ctx = _ctx(api, 16, scans)
    c, s, pool = CAP[16]
    a = api.CubeMaps(ctx, S, c, s, pool_points=pool)
    b = api.CubeMaps(ctx, S, c, s, pool_points=pool)
    for k in range(n):
        guess = _guesses(synth, cfgs, k, [(0.0, 0.0, 0.0)] * S)
        feats = [ctx.features(k * S + q) for q in range(S)]
        pa, ra = a.process(guess, [f["less_sharp"] for f in feats], [f["less_flat"] for f in feats])
        pb, rb = b.process_slots(guess, [k * S + q for q in range(S)])
        assert (ra == rb).all()
        assert_bit_equal(pa, pb, f"frame {k}")
    for q in range(S):
        assert a.info(q) == b.info(q)
        for which in range(4):
            assert_bit_equal(a.cloud(q, which), b.cloud(q, which), f"sequence {q} cloud {which}")
    a.close(); b.close(); ctx.close()


def test_pool_overflow_names_the_sequence_and_changes_nothing(api, synth):
    """a pool just large enough for a scan; sequence 1 moves 60 m per frame, the others stand still"""
    S = 3
    cfgs, scans, _ = drives(synth, 16, S, 1)
    ctx = _ctx(api, 16, scans)
    feats = [ctx.features(q) for q in range(S)]
    c = max(len(f["less_sharp"]) for f in feats)
    s = max(len(f["less_flat"]) for f in feats)
    many = api.CubeMaps(ctx, S, c, s, pool_points=max(4096, c, s))
    err = None
    for k in range(12):
        guess = np.array([[0, 0, 0, 1.0, 60.0 * k if q == 1 else 0.0, 0.0, 0.0] for q in range(S)])
        snap = [[(s_, i, many.cube(q, s_, i)) for s_, i in _nonempty(many.cube, q)] for q in range(S)]
        try:
            many.process_slots(guess, [q for q in range(S)])
        except api.LightLoamError as e:
            err = e
            break
    assert err is not None and err.code == -4 and "sequence 1" in str(err), err
    for q in range(S):
        assert [(s_, i) for s_, i, _ in snap[q]] == _nonempty(many.cube, q)
        for s_, i, pts in snap[q]:
            assert_bit_equal(many.cube(q, s_, i), pts, f"sequence {q} cube {s_} {i}")
    with pytest.raises(api.LightLoamError) as again:
        many.process_slots(guess, [q for q in range(S)])
    assert again.value.code == -4
    poses, ran = many.process_slots(guess, [0, -1, 2])                          # the others map on
    assert ran[0] and ran[2]
    many.close(); ctx.close()


def test_argument_errors_change_nothing(api, synth):
    S = 3
    cfgs, scans, _ = drives(synth, 16, S, 2)
    ctx = api.Context(api.default_params(16, batch=8, max_points=max_points(scans)))
    for q in range(S):
        ctx.upload_scan(q, scans[q][0])
    ctx.extract(0, S)
    near = np.zeros((64, 4), np.float32); near[:, 0] = 0.01                    # nothing survives the minimum range: no scan in slot 5
    ctx.upload_scan(5, near)
    try:
        ctx.extract(5, 1)
    except api.LightLoamError:
        pass
    with pytest.raises(api.LightLoamError) as e:
        api.CubeMaps(ctx, 0, 4096, 32768, pool_points=1 << 16)
    assert e.value.code == -2
    many = api.CubeMaps(ctx, S, 4096, 32768, pool_points=1 << 18)
    guess = _guesses(synth, cfgs, 0, [(0.0, 0.0, 0.0)] * S)
    many.process_slots(guess, [0, 1, 2])
    state = [(many.info(q), [(s_, i, many.cube(q, s_, i)) for s_, i in _nonempty(many.cube, q)]) for q in range(S)]
    for slots, code in [([0, 1, 8], -2), ([0, -2, 1], -2), ([0, 1, 1], -2), ([0, 1, 5], -7)]:
        with pytest.raises(api.LightLoamError) as e:
            many.process_slots(guess, slots)
        assert e.value.code == code, (slots, e.value)
    for q in range(S):
        info, cubes = state[q]
        assert many.info(q)[0] == info[0]
        for s_, i, pts in cubes:
            assert_bit_equal(many.cube(q, s_, i), pts, f"sequence {q} cube {s_} {i}")
    many.close(); ctx.close()


def test_free_running_sequence_matches_oracle(api, orc, synth):
    """one sequence among three, each side mapping with its own optimised pose, agrees with the oracle's cube map"""
    S, n = 3, 6
    cfgs, scans, _ = drives(synth, 16, S, n)
    ctx = _ctx(api, 16, scans)
    many = api.CubeMaps(ctx, S, 4096, 32768, pool_points=1 << 18)
    oc = orc.CubeMap()
    P = orc.params(16)
    for k in range(n):
        guess = _guesses(synth, cfgs, k, [(0.0, 0.0, 0.0)] * S)
        poses, ran = many.process_slots(guess, [k * S + q for q in range(S)])
        f = orc.extract(scans[1][k], P)
        oc.prepare(guess[1, 4:], f["less_sharp"], f["less_flat"])
        qo, to, ran_o = oc.optimize(guess[1, :4], guess[1, 4:]); oc.update(qo, to)
        assert bool(ran[1]) == bool(ran_o) == (k > 0)
        assert np.abs(poses[1, :4] - qo).max() < 1e-6 and np.abs(poses[1, 4:] - to).max() < 1e-6, (k, poses[1], qo, to)
    for s_, i in _nonempty(oc.cube):
        a, b = many.cube(1, s_, i), oc.cube(s_, i)
        assert abs(len(a) - len(b)) <= max(2, len(b) // 500)
    many.close(); ctx.close(); oc.close()


def _qmul(a, b):
    ax, ay, az, aw = a; bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


def _qrot(q, v):
    ux, uy, uz, w = q
    uv = 2.0 * np.array([uy * v[2] - uz * v[1], uz * v[0] - ux * v[2], ux * v[1] - uy * v[0]])
    return v + w * uv + np.array([uy * uv[2] - uz * uv[1], uz * uv[0] - ux * uv[2], ux * uv[1] - uy * uv[0]])


class _Mapping:
    """LaserMapping's transformAssociateToMap / transformUpdate (laserMapping.cpp:113-123) for one sequence"""

    def __init__(self):
        self.q_wmap_wodom = np.array([0, 0, 0, 1.0]); self.t_wmap_wodom = np.zeros(3)

    def associate(self, q_odom, t_odom):
        return np.concatenate([_qmul(self.q_wmap_wodom, q_odom), _qrot(self.q_wmap_wodom, t_odom) + self.t_wmap_wodom])

    def update(self, p, q_odom, t_odom):
        inv = np.array([-q_odom[0], -q_odom[1], -q_odom[2], q_odom[3]]) / np.dot(q_odom, q_odom)
        self.q_wmap_wodom = _qmul(p[:4], inv); self.t_wmap_wodom = p[4:] - _qrot(self.q_wmap_wodom, t_odom)


def test_end_to_end_with_odometry_sequences(api, synth):
    """ll_odometry_sequences -> world odometry -> transformAssociateToMap -> process_slots -> transformUpdate, against the same
    loop one sequence at a time through CubeMap.process_slot"""
    S, n = 4, 10
    cfgs, scans, pose0 = drives(synth, 16, S, n)
    ctx = _ctx(api, 16, scans)                                                  # ring of n rows: row r = frame r, slot r * S + q
    rel = ctx.odometry_sequences(S, n, 1, n - 1, pose0=pose0)
    c, s, pool = CAP[16]
    many = api.CubeMaps(ctx, S, c, s, pool_points=pool)
    ones = [api.CubeMap(ctx, c, s, pool_points=pool) for _ in range(S)]
    side = {"many": [_Mapping() for _ in range(S)], "one": [_Mapping() for _ in range(S)]}
    q_w = [np.array([0, 0, 0, 1.0]) for _ in range(S)]; t_w = [np.zeros(3) for _ in range(S)]
    for k in range(n):
        if k > 0:                                                               # laserOdometry.cpp:841-842
            for q in range(S):
                t_w[q] = t_w[q] + _qrot(q_w[q], rel[k - 1, q, 4:]); q_w[q] = _qmul(q_w[q], rel[k - 1, q, :4])
        guess = np.array([side["many"][q].associate(q_w[q], t_w[q]) for q in range(S)])
        poses, ran = many.process_slots(guess, [k * S + q for q in range(S)])
        for q in range(S):
            side["many"][q].update(poses[q], q_w[q], t_w[q])
            g1 = side["one"][q].associate(q_w[q], t_w[q])
            p1, r1 = ones[q].process_slot(g1, k * S + q)
            side["one"][q].update(p1, q_w[q], t_w[q])
            assert ran[q] == r1
            assert_bit_equal(poses[q], p1, f"frame {k} sequence {q}")
    for o in ones:
        o.close()
    many.close(); ctx.close()


def test_far_cubes_ragged_lanes_and_a_merge_on_compacted_pools(api, orc):
    """cubes outside the valid set that receive points (test_gpu_cubemap.far_frame), in pools of 4096 that compact on the way:
    lane 0 maps the far points, lane 1 the same scans without them, lane 2 sits out the odd frames.  Every lane equals a single
    map fed the same frames, lane 0 the oracle as well; then lane 0 is merged into lane 1 -- onto a compacted pool, from grown cubes"""
    from test_gpu_cubemap import FAR_CUBES, FAR_POOL, ORIGIN, far_frame, far_oracle_frame
    from test_gpu_map_merge import BASE_SYNCS, check_map, expected_merge
    S, n = 3, 20
    ctx = api.Context(api.default_params(16, batch=1, max_points=4096))
    many = api.CubeMaps(ctx, S, 64, 512, pool_points=FAR_POOL)
    ones = [api.CubeMap(ctx, 64, 512, pool_points=FAR_POOL) for _ in range(S)]
    oc = orc.CubeMap()
    guess = np.tile(ORIGIN, (S, 1))
    appended = 0
    for k in range(n):
        scans = [far_frame(k), far_frame(k, far=False), far_frame(k) if k % 2 == 0 else (None, None)]
        poses, ran = many.process(guess, [c for c, _ in scans], [s for _, s in scans])
        appended += far_oracle_frame(oc, k)
        for q in range(S):
            if scans[q][0] is None:
                continue
            p1, r1 = ones[q].process(guess[q], *scans[q])
            assert not ran[q] and not r1, (k, q)
            assert_bit_equal(poses[q], p1, f"frame {k} sequence {q} pose")
            assert_bit_equal(poses[q], ORIGIN, f"frame {k} sequence {q}: the pose moved")
        for q in range(S):                                                      # the pair tables' view, then the clouds they point at
            cen, counts, valid = many.layout(q)
            cen1, counts1, valid1 = ones[q].layout()
            assert tuple(cen) == tuple(cen1) and (counts == counts1).all() and valid.tolist() == valid1.tolist(), (k, q)
            for s, i in np.argwhere(counts):
                assert_bit_equal(many.cube(q, s, i, cap=counts[s, i]), ones[q].cube(s, i, cap=counts[s, i]), f"frame {k} sequence {q} cube {s} {i}")
        for s, i in _nonempty(oc.cube):
            assert_bit_equal(many.cube(0, s, i), oc.cube(s, i), f"frame {k} lane 0 cube {s} {i}")
    assert appended > FAR_POOL * 3 // 4, appended
    assert _nonempty(oc.cube) == _nonempty(many.cube, 0)
    for q in range(S):
        _assert_same(many, q, ones[q], f"sequence {q}")
    for s in (0, 1):
        for c in FAR_CUBES[s]:
            assert len(many.cube(0, s, c)) >= n and len(many.cube(1, s, c)) == 0 and len(many.cube(2, s, c)) >= n // 2
    cen, _, valid = many.layout(1)
    want, added, dropped, _ = expected_merge(orc, many, 1, 0, ORIGIN)
    lane0, lane2 = [[(s, i, many.cube(q, s, i)) for s, i in _nonempty(many.cube, q)] for q in (0, 2)]
    sy0, f0 = many.stats()
    got_added, got_dropped = many.merge([(1, 0, ORIGIN)])
    assert many.stats() == (sy0 + BASE_SYNCS, f0)
    assert got_added.tolist() == [added] and got_dropped.tolist() == [dropped] and dropped == [0, 0]
    check_map(many, 1, want, cen, valid, "lane 1 <- lane 0")
    for q, cubes in ((0, lane0), (2, lane2)):
        assert [(s, i) for s, i, _ in cubes] == _nonempty(many.cube, q)
        for s, i, pts in cubes:
            assert_bit_equal(many.cube(q, s, i), pts, f"after the merge: lane {q} cube {s} {i}")
    for o in ones:
        o.close()
    many.close(); ctx.close(); oc.close()
