"""ll_keyframes, ll_cubemaps_insert_keyframes, ll_drives_set_keyframes and ll_drives_correct through the C ABI.  The expected maps
never come from the code under test: tests/rebuildcases.py restates the insert from the CPU oracle's pointAssociateToMap, the cube
arithmetic of laserMapping.cpp:2108-2125 and the oracle's VoxelGrid (tests/test_rebuild_cases.py checks the restatement itself).
Every comparison is bytewise except the last test's "still tracking" bound.

Synchronisations per insert that moves a point, as lightloam_hip.h states them: 3 (per-cube counts, filtered sizes, commit); the
sizes here stay below the voxel filter's read-back (65 536 points per filter call)."""
import ctypes as C

import numpy as np
import pytest

import rebuildcases as rc
from rebuildcases import EMPTY, IDENT, N, expected_insert, yaw_pose
from test_gpu_drives import NAN7, qmul, qrot
from test_gpu_drives_localize import make_drives, map_state, same_map, step
from test_gpu_map_export import same_bytes
from test_gpu_map_merge import BASE_SYNCS, box, check_map, cubes, import_all, make_map, small_ctx, state, state_of
from test_gpu_mapping_sequences import CAP, _ctx, _guesses
from test_gpu_sequences import drives

pytestmark = pytest.mark.gpu


def fill(ctx, frames, poses, spare=0):
    """a store that holds exactly these frames (plus `spare` frames / points of room)"""
    kf = ctx.keyframes(len(frames) + spare, sum(len(f[0]) for f in frames) + 1 + spare, sum(len(f[1]) for f in frames) + 1 + spare)
    for k, (f, P) in enumerate(zip(frames, poses)):
        assert kf.add_points(f[0], f[1], P) == k
    return kf


def store_state(kf):
    pts, off = kf.export()
    return len(kf), pts.tobytes(), off.tobytes(), [(i["lane"], i["frame_index"], i["n"], i["offset"], i["pose"].tobytes()) for i in map(kf.info, range(len(kf)))]


def all_layout(want):
    """{(w, cube): cloud} -> (points in the LL_MAP_ALL layout, counts [2, N])"""
    counts = np.zeros((2, N), np.int32)
    for (w, c), cloud in want.items():
        counts[w, c] = len(cloud)
    parts = [want[(w, c)] for c in sorted({c for _, c in want}) for w in (0, 1) if (w, c) in want]
    return (np.concatenate(parts) if parts else EMPTY), counts


def check_insert(api, orc, frames, poses, ids, dst=None, reset=0, cen=None, pool=1 << 15, stored=False, what="insert"):
    """frames[i] under poses[i] for i in ids into map 0 of a two-map object (map 1 must not change) against the restatement"""
    ctx = small_ctx(api)
    many = api.CubeMaps(ctx, 2, 64, 64, pool_points=pool)
    other = make_map(box(np.random.default_rng(99), 300, (-20.0, -20.0, -5.0), (20.0, 20.0, 5.0)), box(np.random.default_rng(98), 300, (-20.0, -20.0, -5.0), (20.0, 20.0, 5.0), 1))
    import_all(many, [dst, other])
    kf = fill(ctx, frames, poses)
    before = cubes(many, 0)
    cen0, _, valid0 = many.layout(0)
    use_cen, use_valid = (cen, ()) if reset else (tuple(cen0), valid0)
    pre = {}
    want, added, dropped = expected_insert(orc, {} if reset else before, use_cen, [frames[i] for i in ids], [poses[i] for i in ids], pre)
    for w in (0, 1):
        assert sum(n for (t, c), n in pre.items() if t == w) < 65536                # no filter read-back: exactly BASE_SYNCS
    s1, k0 = state_of(many, 1), store_state(kf)
    sy0, f0 = many.stats()
    got_added, got_dropped = many.insert_keyframes(kf, [(0, ids, None if stored else [poses[i] for i in ids], reset, cen)])
    moved = sum(len(frames[i][0]) + len(frames[i][1]) for i in ids) > 0
    assert many.stats() == (sy0 + (BASE_SYNCS if moved else 0), f0), what
    assert got_added.tolist() == [added] and got_dropped.tolist() == [dropped], (what, got_added, added, got_dropped, dropped)
    check_map(many, 0, want, use_cen, use_valid, what)
    if reset:
        assert many.info(0) == (tuple(cen), (0, 0, 0, 0)), what
    else:
        touched = {k for k in want if k not in before or want[k].tobytes() != before[k].tobytes()}
        for k in before:
            if k not in touched:
                same_bytes(many.cube(0, k[0], k[1], cap=len(before[k])), before[k], f"{what}: untouched cube {k}")
    assert state_of(many, 1) == s1 and store_state(kf) == k0, what
    ms, cnt = many.insert_timing()
    assert cnt[0] == sum(len(frames[i][0]) + len(frames[i][1]) for i in ids) and all(m >= 0 for m in ms), what
    out = state_of(many, 0)
    kf.close(); many.close(); ctx.close()
    return out, want, added, dropped


# ---------------------------------------------------------------- the store
def test_add_points_then_export_gives_the_same_bytes(api):
    frames, poses = rc.sizes_scene(11)
    ctx = small_ctx(api)
    kf = fill(ctx, frames, poses)
    assert len(kf) == len(frames) == kf.size()
    pts, off = kf.export()
    at = [0, 0]
    for k, (f, P) in enumerate(zip(frames, poses)):
        i = kf.info(k)
        assert (i["lane"], i["frame_index"], i["n"]) == (-1, -1, (len(f[0]), len(f[1]))) and i["pose"].tobytes() == P.tobytes()
        assert i["offset"] == tuple(at)
        for w in (0, 1):
            same_bytes(pts[off[2 * k + w]:off[2 * k + w + 1]], f[w], f"frame {k} type {w}")
            at[w] += len(f[w])
    assert off[-1] == sum(len(f[0]) + len(f[1]) for f in frames)
    # a range in the middle; and an export put back with add_points stores the same bytes
    p2, o2 = kf.export(3, 4)
    assert p2.tobytes() == pts[off[6]:off[14]].tobytes() and (o2 == off[6:15] - off[6]).all()
    twin = ctx.keyframes(len(frames), int(off[-1]) + 1, int(off[-1]) + 1)
    for k in range(len(frames)):
        twin.add_points(pts[off[2 * k]:off[2 * k + 1]], pts[off[2 * k + 1]:off[2 * k + 2]], kf.info(k)["pose"])
    assert store_state(twin) == store_state(kf)
    kf.reset()
    assert len(kf) == 0 and kf.export()[1].tolist() == [0]
    assert kf.add_points(frames[3][0], frames[3][1], poses[3]) == 0 and kf.info(0)["offset"] == (0, 0)
    twin.close(); kf.close(); ctx.close()


def test_add_cubemaps_captures_the_stack_clouds(api, synth):
    """two sequences; frame 0 runs both, frame 1 only sequence 0: a capture equals cloud(q, 2) / cloud(q, 3) byte for byte, holds the
    pose and the tags given, and costs no synchronisation; a sequence that has run no frame is refused"""
    S, n = 2, 2
    cfgs, scans, _ = drives(synth, 16, S, n)
    ctx = _ctx(api, 16, scans)
    c, s, pool = CAP[16]
    a = api.CubeMaps(ctx, S, c, s, pool_points=pool)
    kf = ctx.keyframes(8, 4 * c, 4 * s)
    with pytest.raises(api.LightLoamError) as e:
        kf.add_cubemaps(a, [1, 0], np.tile(IDENT, (S, 1)))
    assert e.value.code == -7 and len(kf) == 0
    poses, _ = a.process_slots(_guesses(synth, cfgs, 0, [(0.0, 0.0, 0.0)] * S), [0, 1])
    sy = a.stats()
    assert kf.add_cubemaps(a, [1, 1], poses) == 0 and len(kf) == 2
    assert a.stats() == sy
    seen = {q: (a.cloud(q, 2), a.cloud(q, 3)) for q in range(S)}
    p1, _ = a.process_slots(_guesses(synth, cfgs, 1, [(0.0, 0.0, 0.0)] * S), [S, -1])
    assert kf.add_cubemaps(a, [0, 0], p1) == -1 and len(kf) == 2                     # nobody selected: nothing added
    assert kf.add_cubemaps(a, [1, 0], p1, lane_tag=[7, 8], frame_tag=[1, 1]) == 2 and len(kf) == 3
    seen[2] = (a.cloud(0, 2), a.cloud(0, 3))
    pts, off = kf.export()
    for k, (lane, fi, pose) in enumerate([(0, -1, poses[0]), (1, -1, poses[1]), (7, 1, p1[0])]):
        i = kf.info(k)
        assert (i["lane"], i["frame_index"]) == (lane, fi) and i["pose"].tobytes() == pose.tobytes()
        for w in (0, 1):
            assert len(seen[k][w]) > 0
            same_bytes(pts[off[2 * k + w]:off[2 * k + w + 1]], seen[k][w], f"frame {k} type {w}")
    a.reset(1)
    with pytest.raises(api.LightLoamError) as e:
        kf.add_cubemaps(a, [1, 1], p1)
    assert e.value.code == -7 and len(kf) == 3
    kf.close(); a.close(); ctx.close()


def test_store_refusals_change_nothing(api):
    rng = np.random.default_rng(12)
    f = [rc.frame(rng, 100, 200), rc.frame(rng, 50, 60)]
    ctx = small_ctx(api)
    kf = ctx.keyframes(3, 200, 300)
    kf.add_points(*f[0], IDENT); kf.add_points(*f[1], yaw_pose(5.0, (1.0, 2.0, 3.0)))
    before = store_state(kf)
    for corner, surf, word in ((rc.frame(rng, 51, 1)[0], EMPTY, "corner"), (EMPTY, rc.frame(rng, 1, 41)[1], "surf")):
        with pytest.raises(api.LightLoamError) as e:
            kf.add_points(corner, surf, IDENT)
        assert e.value.code == -4 and word in str(e.value), e.value
    for bad in (np.r_[IDENT[:6], np.nan], np.r_[np.inf, IDENT[1:]]):
        with pytest.raises(api.LightLoamError) as e:
            kf.add_points(f[1][0], f[1][1], bad)
        assert e.value.code == -2
    lib, pose = kf.lib, (C.c_double * 7)(*IDENT)
    off = (C.c_longlong * 16)()
    assert lib.ll_keyframes_add_points(kf.h, None, 3, None, 0, pose, None) == -2
    assert lib.ll_keyframes_add_points(kf.h, None, 0, None, -1, pose, None) == -2
    assert lib.ll_keyframes_add_points(kf.h, None, 0, None, 0, None, None) == -2
    assert lib.ll_keyframes_add_points(None, None, 0, None, 0, pose, None) == -2
    assert lib.ll_keyframes_export(kf.h, 0, 2, None, None) == -2 and lib.ll_keyframes_export(kf.h, 1, 2, None, off) == -2
    assert lib.ll_keyframes_export(kf.h, -1, 1, None, off) == -2 and lib.ll_keyframes_info(kf.h, 2, C.byref(api.KeyframeInfo())) == -2
    assert lib.ll_keyframes_size(None) == -2 and lib.ll_keyframes_reset(None) == -2
    assert lib.ll_keyframes_add_cubemaps(kf.h, None, None, None, None, None, None) == -2
    assert store_state(kf) == before
    assert kf.add_points(EMPTY, EMPTY, IDENT) == 2                                   # an empty frame is a frame
    with pytest.raises(api.LightLoamError) as e:
        kf.add_points(EMPTY, EMPTY, IDENT)
    assert e.value.code == -4 and "frames" in str(e.value) and len(kf) == 3
    for bad in (dict(max_frames=0, cap_corner=1, cap_surf=1), dict(max_frames=1, cap_corner=0, cap_surf=1), dict(max_frames=1, cap_corner=1, cap_surf=(1 << 30) + 1)):
        with pytest.raises(api.LightLoamError) as e:
            ctx.keyframes(**bad)
        assert e.value.code == -2
    kf.close(); ctx.close()


# ---------------------------------------------------------------- insert against the restatement
def test_general_scene_into_a_non_empty_map(api, orc):
    frames, poses, dst = rc.general_scene(1)
    dst = make_map(*dst, valid=(2000, 2001, 2022))
    out, want, added, dropped = check_insert(api, orc, frames, poses, [0, 1, 2, 3, 4], dst=dst, what="general")
    assert dropped == [0, 0] and len({c for w, c in want if w == 0}) >= 6
    # poses = NULL: the stored poses, the same bytes
    out2, _, _, _ = check_insert(api, orc, frames, poses, [0, 1, 2, 3, 4], dst=dst, stored=True, what="stored poses")
    assert out2 == out


def test_reset_with_a_moved_centre_negative_coordinates_and_drops(api, orc):
    frames, poses, cen = rc.moved_centre_scene(2)
    rng = np.random.default_rng(20)
    dst = make_map(box(rng, 500, (-24.0, -24.0, -10.0), (24.0, 24.0, 10.0)), box(rng, 500, (-24.0, -24.0, -10.0), (24.0, 24.0, 10.0), 1), valid=(5, 6))
    _, want, added, dropped = check_insert(api, orc, frames, poses, [0, 1, 2], dst=dst, reset=1, cen=cen, what="moved centre")
    for w in (0, 1):
        assert dropped[w] > 200 and added[w] > 500


@pytest.mark.parametrize("case", ["sizes", "chunk", "one_cube", "spread", "repeated", "descending", "no_points"])
def test_sizes_at_which_the_kernels_can_go_wrong(api, orc, case):
    """frame clouds of 0 points (one type, both), 1, 63 / 64 / 65, 1023 / 1024 / 1025, 2047 / 2049; three frames of 700 (a chunk of the
    counting sort spans two frame boundaries); all frames into one cube; one frame over more than 8 cubes; a repeated id; ids descending;
    an op without points"""
    rng = np.random.default_rng(30)
    dst = make_map(box(rng, 400, (-24.0, -24.0, -10.0), (24.0, 24.0, 10.0)), box(rng, 400, (-24.0, -24.0, -10.0), (24.0, 24.0, 10.0), 1))
    if case == "sizes":
        frames, poses = rc.sizes_scene(3)
        assert sorted({len(f[w]) for f in frames for w in (0, 1)}) == [0, 1, 5, 7, 63, 64, 65, 1023, 1024, 1025, 2047, 2049]
        check_insert(api, orc, frames, poses, list(range(len(frames))), dst=dst, pool=1 << 16, what=case)
    elif case == "chunk":
        frames, poses = rc.chunk_scene(4)
        check_insert(api, orc, frames, poses, [0, 1, 2], dst=dst, what=case)
    elif case == "one_cube":
        frames, poses = rc.one_cube_scene(6)
        _, want, _, _ = check_insert(api, orc, frames, poses, [0, 1, 2, 3], dst=None, reset=1, cen=(10, 10, 5), what=case)
        assert len(want) == 2
    elif case == "spread":
        frames, poses = rc.spread_scene(5)
        _, want, _, _ = check_insert(api, orc, frames, poses, [0], dst=dst, what=case)
        assert len({c for w, c in want if w == 0}) > 8
    elif case == "repeated":
        frames, poses = rc.chunk_scene(7)
        check_insert(api, orc, frames, poses, [1, 0, 1, 1], dst=dst, what=case)
    elif case == "descending":
        frames, poses, _ = rc.general_scene(8)
        check_insert(api, orc, frames, poses, [4, 3, 2, 1, 0], dst=dst, what=case)
    else:
        frames, poses = [(EMPTY, EMPTY)] + rc.chunk_scene(9)[0][:1], [IDENT, IDENT]
        check_insert(api, orc, frames, poses, [0, 0], dst=dst, what="empty frames")
        check_insert(api, orc, frames, poses, [], dst=dst, what="empty list")
        check_insert(api, orc, frames, poses, [], dst=dst, reset=1, cen=(4, 5, 6), what="empty list with reset")


# ---------------------------------------------------------------- the merge is the same machine
def test_a_frame_in_map_order_equals_the_merge(api):
    """a frame whose clouds are map src's points in LL_MAP_ALL order, inserted under T, gives the bytes of merge([(dst, src, T)])"""
    rng = np.random.default_rng(40)
    T = yaw_pose(30.0, (12.5, -7.0, 1.0))
    centres = [(-120.0, 40.0, 3.0), (60.0, 110.0, -8.0), (5.0, 5.0, 0.0)]
    src_w = [np.concatenate([box(rng, n if w == 0 else n // 2 + 1, np.array(c) - 24.0, np.array(c) + 24.0, w) for c, n in zip(centres, (700, 2500, 900))]) for w in (0, 1)]
    dst = make_map(*[box(rng, 800, (-140.0, -50.0, -10.0), (-60.0, 20.0, 10.0), w) for w in (0, 1)], valid=(7, 8))
    src = make_map(*src_w)
    pts, (cen, counts, _) = src
    clouds, at = [[], []], 0
    for c in range(N):
        for w in (0, 1):
            clouds[w].append(pts[at:at + counts[w, c]]); at += counts[w, c]
    frame = tuple(np.concatenate(clouds[w]) for w in (0, 1))
    ctx = small_ctx(api)
    a, b = api.CubeMaps(ctx, 2, 64, 64, pool_points=1 << 15), api.CubeMaps(ctx, 2, 64, 64, pool_points=1 << 15)
    import_all(a, [dst, None]); import_all(b, [dst, src])
    kf = fill(ctx, [frame], [IDENT])
    ia = a.insert_keyframes(kf, [(0, [0], [T], 0, None)])
    ib = b.merge([(0, 1, T)])
    assert ia[0].tolist() == ib[0].tolist() and ia[1].tolist() == ib[1].tolist() and ia[0].min() > 0
    assert state_of(a, 0) == state_of(b, 0)
    assert a.insert_timing()[1] == b.merge_timing()[1]
    kf.close(); a.close(); b.close(); ctx.close()


# ---------------------------------------------------------------- batch independence, determinism, synchronisations
def four_maps(api, ctx, seed):
    rng = np.random.default_rng(seed)
    maps = []
    for q in range(4):
        c = np.array([40.0 * q - 60.0, 30.0 * q - 45.0, 0.0])
        maps.append(make_map(*[box(rng, 700 + 150 * q, c - 24.0, c + 24.0, w) for w in (0, 1)]))
    many = api.CubeMaps(ctx, 4, 64, 64, pool_points=1 << 15)
    import_all(many, maps)
    return many


def test_four_ops_equal_one_at_a_time_and_runs_repeat(api, orc):
    frames, poses, _ = rc.general_scene(50)
    shifted = [yaw_pose(-15.0 * k, (-30.0 + 20.0 * k, 10.0 * k, 1.0)) for k in range(5)]
    ops = [(0, [0, 1, 2], None, 0, None), (1, [4, 3], [shifted[4], shifted[3]], 1, (9, 11, 5)), (2, [], None, 0, None), (3, [2, 2, 0], [shifted[2], shifted[1], shifted[0]], 0, None)]
    ctx = small_ctx(api)
    kf = fill(ctx, frames, poses)
    a, b, c = four_maps(api, ctx, 51), four_maps(api, ctx, 51), four_maps(api, ctx, 51)
    assert state(a) == state(b)
    want1 = expected_insert(orc, {}, (9, 11, 5), [frames[4], frames[3]], [shifted[4], shifted[3]])
    sa = a.stats()[0]
    added, dropped = a.insert_keyframes(kf, ops)
    assert a.stats()[0] - sa == BASE_SYNCS                                          # whatever the number of ops
    rows = []
    for op in ops:
        sb = b.stats()[0]
        rows.append(b.insert_keyframes(kf, [op]))
        assert b.stats()[0] - sb == (BASE_SYNCS if len(op[1]) else 0)
    assert added.tolist() == [r[0][0].tolist() for r in rows] and dropped.tolist() == [r[1][0].tolist() for r in rows]
    assert added[1].tolist() == want1[1] and added[2].tolist() == [0, 0]
    assert state(a) == state(b)
    check_map(a, 1, want1[0], (9, 11, 5), (), "op 1")
    c.insert_keyframes(kf, ops)                                                     # a second run: the same bytes
    assert state(c) == state(a)
    kf.close(); a.close(); b.close(); c.close(); ctx.close()


# ---------------------------------------------------------------- the tables after an insert
def test_tables_stay_sound(api, orc, synth):
    """two real maps (16-ring synthetic drives, 3 frames each, every frame captured); sequence 1's keyframes go into map 0 under their
    own poses; map 0 then runs frame 3 and equals a second object whose map 0 was imported from the RESTATEMENT's result"""
    S, n = 2, 4
    cfgs, scans, _ = drives(synth, 16, S, n)
    ctx = _ctx(api, 16, scans)
    c, s, pool = CAP[16]
    a = api.CubeMaps(ctx, S, c, s, pool_points=pool)
    kf = ctx.keyframes(S * n, n * c, n * s)
    seen, seen_pose = [], []
    for k in range(n - 1):
        poses, _ = a.process_slots(_guesses(synth, cfgs, k, [(0.0, 0.0, 0.0)] * S), [k * S + q for q in range(S)])
        assert kf.add_cubemaps(a, [0, 1], poses, frame_tag=[k, k]) == k
        seen.append((a.cloud(1, 2), a.cloud(1, 3))); seen_pose.append(poses[1].copy())
    before = cubes(a, 0)
    cen, _, valid = a.layout(0)
    want, added, dropped = expected_insert(orc, before, cen, seen, seen_pose)
    got = a.insert_keyframes(kf, [(0, list(range(n - 1)), None, 0, None)])
    assert got[0].tolist() == [added] and got[1].tolist() == [dropped] and min(added) > 0
    check_map(a, 0, want, cen, valid, "map 0 after the insert")
    pts, counts = all_layout(want)
    b = api.CubeMaps(ctx, S, c, s, pool_points=pool)
    b.import_maps(pts, [0, len(pts), len(pts)], [(cen, counts, valid), None])
    guess = _guesses(synth, cfgs, n - 1, [(0.0, 0.0, 0.0)] * S)
    slots = [(n - 1) * S, -1]
    pa, ra = a.process_slots(guess, slots)
    pb, rb = b.process_slots(guess, slots)
    assert pa[0].tobytes() == pb[0].tobytes() and ra[0] and rb[0]
    for which in range(4):
        same_bytes(a.cloud(0, which), b.cloud(0, which), f"cloud {which}")
    assert state_of(a, 0) == state_of(b, 0)
    kf.close(); a.close(); b.close(); ctx.close()


# ---------------------------------------------------------------- refusals
def test_insert_refusals_change_nothing(api):
    frames, poses, dst = rc.general_scene(60)
    ctx = small_ctx(api)
    many = api.CubeMaps(ctx, 3, 64, 64, pool_points=4096)
    import_all(many, [make_map(*dst, valid=(3, 4)), make_map(*dst), None])
    kf = fill(ctx, frames, poses)
    before, k0 = state(many), store_state(kf)
    bad = [np.r_[IDENT[:6], np.nan], np.r_[np.inf, IDENT[1:]]]
    arg_cases = [[], [(3, [0], None, 0, None)], [(-1, [0], None, 0, None)], [(0, [5], None, 0, None)], [(0, [0, -1], None, 0, None)],
                 [(0, [0], None, 0, None), (0, [1], None, 0, None)],                # dst of two ops
                 [(2, [0], None, 0, None), (0, [0, 1], [IDENT, bad[0]], 0, None)], [(0, [1], [bad[1]], 1, (10, 10, 5))],
                 [(0, [0], None, 1, (10, 10, (1 << 24) + 1))], [(0, [0], None, 1, (-(1 << 24) - 1, 10, 5))], [(0, [0], None, 2, None)]]
    for ops in arg_cases:
        with pytest.raises(api.LightLoamError) as e:
            many.insert_keyframes(kf, ops)
        assert e.value.code == -2, (ops, e.value)
    lib = many.lib
    ids = (C.c_int * 1)(4)                                                            # frame 4 into map 0: 3000 + 1740 surf points, too many for 4096
    op = api.InsertOp(0, 1, C.addressof(ids), None, 0, (C.c_int * 3)(10, 10, 5))
    assert lib.ll_cubemaps_insert_keyframes(None, kf.h, C.addressof(op), 1, None, None) == -2
    assert lib.ll_cubemaps_insert_keyframes(many.h, None, C.addressof(op), 1, None, None) == -2
    assert lib.ll_cubemaps_insert_keyframes(many.h, kf.h, None, 1, None, None) == -2
    assert lib.ll_cubemaps_insert_keyframes(many.h, kf.h, C.addressof(op), 0, None, None) == -2
    op_neg = api.InsertOp(0, -1, C.addressof(ids), None, 0, (C.c_int * 3)(10, 10, 5))
    op_null = api.InsertOp(0, 1, None, None, 0, (C.c_int * 3)(10, 10, 5))
    assert lib.ll_cubemaps_insert_keyframes(many.h, kf.h, C.addressof(op_neg), 1, None, None) == -2
    assert lib.ll_cubemaps_insert_keyframes(many.h, kf.h, C.addressof(op_null), 1, None, None) == -2
    assert lib.ll_cubemaps_insert_timing(None, None, None) == -2
    assert state(many) == before
    # capacity: map 0 holds 4 x 600 .. 900 points per type and frame 4 brings 1020 corner points: 4096 cannot hold them; with reset it
    # is decided against the empty map and fits.  The refused call has not reset the other op's dst either
    with pytest.raises(api.LightLoamError) as e:
        many.insert_keyframes(kf, [(1, [0], None, 1, (9, 9, 5)), (0, [4, 3], None, 0, None)])
    assert e.value.code == -4 and "op 1" in str(e.value) and "corner" in str(e.value), e.value
    assert state(many) == before and store_state(kf) == k0
    sy = many.stats()[0]
    assert lib.ll_cubemaps_insert_keyframes(many.h, kf.h, C.addressof(op), 1, None, None) == -4      # NULL outputs; still too full
    assert state(many) == before
    added, _ = many.insert_keyframes(kf, [(0, [4, 3], None, 1, (10, 10, 5))])
    assert added.min() > 0 and state(many) != before
    with pytest.raises(api.LightLoamError) as e:                                    # against the empty map, and still too many
        many.insert_keyframes(kf, [(2, [0, 1, 2, 3, 4, 4, 4], None, 1, (10, 10, 5))])
    assert e.value.code == -4 and "op 0" in str(e.value)
    assert many.layout(2)[1].sum() == 0 and many.stats()[0] >= sy + 3
    kf.close(); many.close(); ctx.close()


# ---------------------------------------------------------------- drives: capture
N_CAP = 4


def run_lanes(api, synth, with_store, every=1):
    _, scans, pose0 = drives(synth, 16, 2, N_CAP)
    ctx, dr = make_drives(api, scans)
    c, s, _ = CAP[16]
    kf = ctx.keyframes(2 * N_CAP, N_CAP * 2 * c, N_CAP * 2 * s) if with_store else None
    if kf is not None:
        dr.set_keyframes(kf, every)
    started, outs, seen = set(), [], []
    for k in range(N_CAP):
        frames = {0: (0, k), 1: (1, k)} if k != 2 else {0: (0, k)}                 # lane 1 sits out step 2 and so ends its drive
        if k == 3:
            started.discard(1); frames = {0: (0, 3), 1: (1, 0)}                     # ... and starts again
        out = step(api, ctx, dr, frames, scans, pose0, started)
        outs.append(out)
        seen.append({q: (dr.cubemaps.cloud(q, 2), dr.cubemaps.cloud(q, 3), out[1][q].copy()) for q in frames})
    return ctx, dr, kf, outs, seen


def test_drives_capture_equals_the_stack_clouds_and_changes_nothing(api, synth):
    ctx, dr, kf, outs, seen = run_lanes(api, synth, True)
    ctx2, dr2, _, outs2, _ = run_lanes(api, synth, False)
    for a, b in zip(outs, outs2):
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()
    assert dr.stats() == dr2.stats() and dr.cubemaps.stats() == dr2.cubemaps.stats()
    for q in range(2):
        assert same_map(map_state(api, dr, q), map_state(api, dr2, q))
    assert dr.save([1, 1, 0]) == dr2.save([1, 1, 0])
    fidx = {0: [0, 1, 2, 3], 1: [0, 1, None, 0]}
    want = [(q, fidx[q][k], seen[k][q]) for k in range(N_CAP) for q in sorted(seen[k])]
    assert len(kf) == len(want) == 7
    pts, off = kf.export()
    for i, (q, fi, (corner, surf, pose)) in enumerate(want):
        e = kf.info(i)
        assert (e["lane"], e["frame_index"]) == (q, fi) and e["pose"].tobytes() == pose.tobytes(), i
        same_bytes(pts[off[2 * i]:off[2 * i + 1]], corner, f"keyframe {i} corner")
        same_bytes(pts[off[2 * i + 1]:off[2 * i + 2]], surf, f"keyframe {i} surf")
        assert len(corner) > 0 and len(surf) > 0
    dr.close(); ctx.close(); dr2.close(); ctx2.close()


def test_a_full_store_refuses_the_step_before_it_runs(api, synth):
    """every = 2, room for 3 frames: step 0 captures both lanes, step 1 captures nothing and runs although only one frame of room is
    left, step 2 needs two: LL_ERR_CAPACITY, the lanes' blobs and the counters are as before, and after a reset of the store the same
    commands run"""
    _, scans, pose0 = drives(synth, 16, 2, 3)
    ctx, dr = make_drives(api, scans)
    c, s, _ = CAP[16]
    kf = ctx.keyframes(3, 8 * c, 8 * s)
    dr.set_keyframes(kf, every=2)
    with pytest.raises(api.LightLoamError) as e:
        dr.set_keyframes(kf, every=0)
    assert e.value.code == -2
    started = set()
    step(api, ctx, dr, {0: (0, 0), 1: (1, 0)}, scans, pose0, started)
    assert len(kf) == 2
    step(api, ctx, dr, {0: (0, 1), 1: (1, 1)}, scans, pose0, started)
    assert len(kf) == 2
    blob, stats, cstats, slots = dr.save([1, 1, 0]), dr.stats(), dr.cubemaps.stats(), dr.slots().tolist()
    with pytest.raises(api.LightLoamError) as e:
        step(api, ctx, dr, {0: (0, 2), 1: (1, 2)}, scans, pose0, started)
    assert e.value.code == -4 and "frames" in str(e.value), e.value
    assert len(kf) == 2 and dr.stats() == stats and dr.cubemaps.stats() == cstats and dr.slots().tolist() == slots
    assert dr.save([1, 1, 0]) == blob
    kf.reset()
    _, mapped, ran = step(api, ctx, dr, {0: (0, 2), 1: (1, 2)}, scans, pose0, started)
    assert ran[:2].all() and len(kf) == 2 and [kf.info(i)["frame_index"] for i in range(2)] == [2, 2]
    assert kf.info(1)["pose"].tobytes() == mapped[1].tobytes()
    # a pool without room for one more scan refuses too, and names the type
    small = ctx.keyframes(8, c, 8 * s)
    dr.set_keyframes(small, every=1)
    dr.step(np.zeros(3, np.int32))
    started = set()
    step(api, ctx, dr, {0: (0, 0)}, scans, pose0, started)
    assert len(small) == 1 and small.info(0)["n"][0] > 0
    with pytest.raises(api.LightLoamError) as e:
        step(api, ctx, dr, {0: (0, 1)}, scans, pose0, started)
    assert e.value.code == -4 and "corner" in str(e.value)
    dr.set_keyframes(None)
    step(api, ctx, dr, {0: (0, 1)}, scans, pose0, started)
    assert len(small) == 1
    small.close(); kf.close(); dr.close(); ctx.close()


# ---------------------------------------------------------------- drives: correct
def compose7(A, B):
    """A o B as ll_drives_correct spells it: q = qmul(q_A, q_B), t = qrot(q_A, t_B) + t_A, in f64"""
    r = qrot(list(A[:4]), list(B[4:]))
    return np.array(qmul(list(A[:4]), list(B[:4])) + [r[k] + A[4 + k] for k in range(3)])


def inverse7(A):
    q = np.array([-A[0], -A[1], -A[2], A[3]]) / float(A[:4] @ A[:4])
    return np.r_[q, -np.array(qrot(list(q), list(A[4:])))]


M2O_AT = 176 - 112         # the map-to-odom pose lies 64 bytes before the end of a record's payload ("The blob")


def test_correct(api, synth):
    """lane 0 maps 5 frames and goes idle; lane 1 localises frames 2, 3 against its map.  The identity leaves lane 1's checkpoint
    byte-identical.  Then a general C: lane 2 is lane 1's twin, restored from lane 1's checkpoint with the map-to-odom pose replaced by
    the restated f64 product C o M (M: the seven doubles of the checkpoint); both run frame 4 in one step and must agree bit for bit"""
    n_map, J = 5, 2
    _, scans, pose0 = drives(synth, 16, 1, n_map)
    ctx, dr = make_drives(api, scans)
    started, mapped0 = set(), []
    for k in range(n_map):
        mapped0.append(step(api, ctx, dr, {0: (0, k)}, scans, pose0, started)[1][0].copy())
    dr.step(np.zeros(3, np.int32))
    start = np.tile(IDENT, (3, 1)); start[1] = mapped0[J]
    dr.set_localize([-1, 0, 0], start)
    started = set()
    for k in (J, J + 1):
        _, _, ran = step(api, ctx, dr, {1: (0, k)}, scans, pose0, started)
    assert ran[1]
    blob = dr.save([0, 1, 0])
    ident = np.tile(IDENT, (3, 1))
    dr.correct([0, 1, 0], ident)
    assert dr.save([0, 1, 0]) == blob
    Cs = np.tile(NAN7, (3, 1)); Cs[1] = yaw_pose(0.4, (0.03, -0.02, 0.01)); Cs[1, :4] += [1e-3, -2e-3, 0.0, 0.0]   # not normalised, and used so
    for bad, code in (([0, 2, 0], -2), ([1, 1, 0], -7), ([0, 0, 1], -7)):
        with pytest.raises(api.LightLoamError) as e:
            dr.correct(bad, np.tile(Cs[1], (3, 1)))
        assert e.value.code == code
    with pytest.raises(api.LightLoamError) as e:
        dr.correct([0, 1, 0], np.tile(np.r_[IDENT[:6], np.inf], (3, 1)))
    assert e.value.code == -2 and dr.save([0, 1, 0]) == blob
    rec = api.describe_checkpoint(blob)["records"][0]
    end = int(rec["offset"] + rec["bytes"])
    raw = np.frombuffer(blob, np.uint8).copy()
    M = raw[end - M2O_AT:end - M2O_AT + 56].view(np.float64).copy()
    assert np.isfinite(M).all() and abs(M[:4] @ M[:4] - 1.0) < 1e-6
    raw[end - M2O_AT:end - M2O_AT + 56] = compose7(Cs[1], M).view(np.uint8)
    s0 = dr.stats()
    dr.correct([0, 1, 0], Cs)                                                        # rows of lanes that are not selected are not read
    assert dr.stats() == s0 and dr.save([0, 1, 0]) == raw.tobytes()                 # the device's product is the restated one, bit for bit
    dr.restore(raw.tobytes(), [2])
    started.add(2)
    _, mapped, ran = step(api, ctx, dr, {1: (0, J + 2), 2: (0, J + 2)}, scans, pose0, started)
    assert ran[1] and ran[2] and mapped[1].tobytes() == mapped[2].tobytes()
    assert np.linalg.norm(mapped[1][4:] - mapped0[J + 2][4:]) < 0.2                 # and the small C has not thrown the lane off the map
    dr.close(); ctx.close()


# ---------------------------------------------------------------- end to end
def test_a_rebuilt_map_keeps_the_lane_tracking(api, synth):
    """Lanes 0 (A) and 1 (B) drive the same 12 synthetic frames.  After frame 8 B's map is rebuilt from its 9 keyframes under G o P_f
    (G: 30 degrees of yaw and (12.5, -7, 1)), reset = 1, cen = (10, 10, 5), and B is corrected by G; B then runs frames 9 - 11.
    Required: ran = 1 on those frames and |t(G^-1 o mapped_B) - t(mapped_A)| < line_res = 0.4 m, a "still tracking" condition, not an
    accuracy claim: two voxel-centroid maps of the same points differ by less than a leaf.
    Measured on an MI355X (the 16-ring synthetic drive): 0.0031, 0.0025 and 0.0068 m on frames 9, 10 and 11."""
    n, cut = 12, 9
    _, scans, pose0 = drives(synth, 16, 1, n)
    ctx, dr = make_drives(api, scans)
    c, s, _ = CAP[16]
    kf = ctx.keyframes(2 * n, 2 * n * c, 2 * n * s)
    dr.set_keyframes(kf, 1)
    G = yaw_pose(30.0, (12.5, -7.0, 1.0))
    started = set()
    for k in range(cut):
        step(api, ctx, dr, {0: (0, k), 1: (0, k)}, scans, pose0, started)
    ids = [i for i in range(len(kf)) if kf.info(i)["lane"] == 1]
    assert [kf.info(i)["frame_index"] for i in ids] == list(range(cut))
    poses = [compose7(G, kf.info(i)["pose"]) for i in ids]
    a_before = map_state(api, dr, 0)
    added, dropped = dr.cubemaps.insert_keyframes(kf, [(1, ids, poses, 1, (10, 10, 5))])
    assert added.min() > 0 and dropped.tolist() == [[0, 0]]
    assert same_map(map_state(api, dr, 0), a_before)
    sel = np.tile(NAN7, (3, 1)); sel[1] = G
    dr.correct([0, 1, 0], sel)
    Ginv, worst = inverse7(G), 0.0
    for k in range(cut, n):
        _, mapped, ran = step(api, ctx, dr, {0: (0, k), 1: (0, k)}, scans, pose0, started)
        assert ran[0] and ran[1], k
        dev = float(np.linalg.norm(compose7(Ginv, mapped[1])[4:] - mapped[0][4:]))
        worst = max(worst, dev)
        print(f"frame {k}: |t(G^-1 o mapped_B) - t(mapped_A)| = {dev:.4f} m")
    print(f"worst deviation {worst:.4f} m")
    assert worst < 0.4, worst
    kf.close(); dr.close(); ctx.close()
