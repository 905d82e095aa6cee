"""ll_bev through the C ABI against the numpy restatement of tests/bevcases.py (tests/test_bev_cases.py checks the crafted inputs and
the yard scene on the restatement alone).  Grids are compared as bytes, volumes and result integers as integers, yaw and D_w7 as
doubles: every comparison is exact.  No expected value comes from the library."""
import ctypes as C
import math

import numpy as np
import pytest

import bevcases as bc
from test_gpu_map_merge import small_ctx

pytestmark = pytest.mark.gpu


def store(ctx, cases, spare=0):
    """one Keyframes store with the frames of all cases back to back -> (kf, the first id of every case)"""
    frames = [f for k in cases for f in k["frames"]]
    poses = [p for k in cases for p in k["poses"]]
    kf = ctx.keyframes(len(frames) + spare, sum(len(f[0]) for f in frames) + 1 + spare, sum(len(f[1]) for f in frames) + 1 + spare)
    for i, (f, P) in enumerate(zip(frames, poses)):
        assert kf.add_points(f[0], f[1], P) == i
    first = np.cumsum([0] + [len(k["frames"]) for k in cases])[:-1]
    return kf, [int(x) for x in first]


def op_of(case, first=0):
    return ([first + i for i in case["target"]], case["target_poses"], [first + i for i in case["query"]], case["query_poses"], case["yaw0"], case["yaw_step"],
            case["n_yaws"])


def record(r):
    return (r.score, r.second, r.iyaw, r.sx, r.sy, r.n_query, r.yaw, tuple(r.D_w7))


def wanted(res):
    return (res["score"], res["second"], res["iyaw"], res["sx"], res["sy"], res["n_query"], res["yaw"], tuple(float(v) for v in res["D"]))


def compare(bev, i, got, want, name):
    """op i of the last match against (grid, volume, result) of the restatement -> a list of what differs"""
    grid, vol, res = want
    bad = []
    g = bev.grid(i)
    if g.tobytes() != grid.tobytes():
        bad.append(f"{name}: grid differs in {int((g != grid).sum())} cells, first {np.argwhere(g != grid)[:3].tolist()}")
    v = bev.volume(i)
    if v.shape != vol.shape or (v != vol).any():
        bad.append(f"{name}: volume differs in {int((v != vol).sum()) if v.shape == vol.shape else v.shape} entries"
                   + (f", first {np.argwhere(v != vol)[:3].tolist()}: {v[v != vol][:3].tolist()} vs {vol[v != vol][:3].tolist()}" if v.shape == vol.shape else ""))
    if record(got) != wanted(res):
        bad.append(f"{name}: result {record(got)} vs {wanted(res)}")
    return bad


# ---------------------------------------------------------------- the crafted cases
def test_crafted_cases_exactly(api):
    c = bc.cfg(max_ops=32, **bc.SMALL)
    cases = list(bc.crafted_cases(c).values())
    ctx = small_ctx(api)
    kf, first = store(ctx, cases)
    bev = ctx.bev(kf, **bc.lib_params(c))
    got = bev.match([op_of(k, f) for k, f in zip(cases, first)])
    bad = []
    for i, k in enumerate(cases):
        bad += compare(bev, i, got[i], bc.np_match(k, c), k["name"])
    assert not bad, "\n".join(bad)
    ms, cnt = bev.timing()
    listed = sum(len(a) + len(b) for k in cases for i in k["target"] + k["query"] for a, b in [k["frames"][i]])
    assert cnt == (len(cases), listed, sum(k["n_yaws"] for k in cases) * 64) and all(m >= 0 for m in ms)
    bev.close(); kf.close(); ctx.close()


@pytest.mark.parametrize("which", ["shift_half_1", "shift_half_16", "window"])
def test_limits_of_the_search(api, which):
    c, case = bc.window_case() if which == "window" else bc.shift_limit_cases()[0 if which == "shift_half_1" else 1]
    ctx = small_ctx(api)
    kf, _ = store(ctx, [case])
    bev = ctx.bev(kf, **bc.lib_params(c))
    got = bev.match([op_of(case)])
    want = bc.np_match(case, c)
    bad = compare(bev, 0, got[0], want, case["name"])
    assert not bad, "\n".join(bad)
    if which == "window":
        assert got[0].second == -1
    bev.close(); kf.close(); ctx.close()


# ---------------------------------------------------------------- the yard scene at the default parameters
def test_yard_scene_exactly(api):
    c = bc.cfg()
    n = len(bc.DISPLACEMENTS)
    cases = [bc.yard_case(k) for k in range(n)]
    ctx = small_ctx(api)
    kf, _ = store(ctx, cases[:1])                                        # the cases share the four frames
    bev = ctx.bev(kf)
    got = bev.match([op_of(k) for k in cases])
    bad = []
    for k in range(n):
        bad += compare(bev, k, got[k], bc.yard_reference(k), f"yard {bc.DISPLACEMENTS[k]}")
    assert not bad, "\n".join(bad)
    for k in range(n):
        res = dict(yaw=got[k].yaw, D=list(got[k].D_w7))
        assert bc.yard_found(res, k, c) and got[k].score > got[k].second > 0
    bev.close(); kf.close(); ctx.close()


# ---------------------------------------------------------------- batches, positions, repetition
def test_alone_in_a_batch_reversed_repeated(api):
    c = bc.cfg(max_ops=8, **bc.SMALL)
    all_cases = bc.crafted_cases(c)
    cases = [all_cases[n] for n in ("chunk_2049", "multi_frame_stored", "cell_edges", "bad_values", "max_yaws", "square_edges")]
    ctx = small_ctx(api)
    kf, first = store(ctx, cases)
    bev = ctx.bev(kf, **bc.lib_params(c))
    ops = [op_of(k, f) for k, f in zip(cases, first)]

    def bits(order):
        got = bev.match([ops[i] for i in order])
        return {i: (record(got[pos]), bev.volume(pos).tobytes(), bev.grid(pos).tobytes()) for pos, i in enumerate(order)}

    together = bits(range(6))
    assert together[0][0] == wanted(bc.np_match(cases[0], c)[2])
    assert bits(range(6)) == together                                    # a second identical call
    assert bits(range(5, -1, -1)) == together                            # reversed: op 0 is now op 5 of 6
    for i in (0, 3, 5):
        assert bits([i])[i] == together[i], cases[i]["name"]             # alone
    assert bits([0, 0, 1, 0])[0] == together[0]                          # the same op three times in one call
    bev.close(); kf.close(); ctx.close()


# ---------------------------------------------------------------- refusals
def test_refusals_launch_nothing(api):
    c = bc.cfg(max_ops=4, max_yaws=4, **bc.SMALL)
    cases = bc.crafted_cases(bc.cfg(**bc.SMALL))
    a, b = cases["cell_edges"], cases["chunk_1025"]
    ctx = small_ctx(api)
    kf, first = store(ctx, [a, b], spare=8)
    bev = ctx.bev(kf, **bc.lib_params(c))
    good = [op_of(a, first[0]), op_of(b, first[1])]
    bev.match(good)
    before = (bev.timing()[1], bev.volume(0).tobytes(), bev.volume(1).tobytes(), bev.grid(1).tobytes())
    lib = api.load_library()

    def refused(code, call, *args):
        if isinstance(call, list):
            with pytest.raises(api.LightLoamError) as e:
                bev.match(call)
            assert e.value.code == code, (e.value, code)
        else:
            assert call(*args) == code
        assert (bev.timing()[1], bev.volume(0).tobytes(), bev.volume(1).tobytes(), bev.grid(1).tobytes()) == before

    t, tp, q, qp, yaw0, step, n = good[0]
    out = (api.BevResult * 4)()
    rec = api.BevOp(1, None, None, 1, None, None, 0.0, 0.1, 1)
    refused(-2, lib.ll_bev_match, None, C.addressof(rec), 1, C.addressof(out))            # NULL handle, ops, out
    refused(-2, lib.ll_bev_match, bev.h, None, 1, C.addressof(out))
    refused(-2, lib.ll_bev_match, bev.h, C.addressof(rec), 1, None)
    refused(-2, lib.ll_bev_match, bev.h, C.addressof(rec), 1, C.addressof(out))           # lists NULL with frames to read
    refused(-2, [])                                                                        # n_ops outside 1 .. max_ops
    refused(-2, [good[0]] * 5)
    refused(-2, [([], tp, q, qp, yaw0, step, n)])                                          # a side with no frame
    refused(-2, [good[1], (t, tp, [], qp, yaw0, step, n)])
    size = len(kf)
    refused(-2, [(t, tp, [size], qp, yaw0, step, n)])                                      # an id outside the store
    refused(-2, [([-1], tp, q, qp, yaw0, step, n)])
    nan_pose = np.tile(bc.IDENTITY, (len(q), 1)); nan_pose[0, 5] = np.nan
    inf_pose = np.tile(bc.IDENTITY, (len(t), 1)); inf_pose[0, 0] = np.inf
    refused(-2, [(t, tp, q, nan_pose, yaw0, step, n)])                                     # a non-finite pose
    refused(-2, [(t, inf_pose, q, qp, yaw0, step, n)])
    refused(-2, [(t, tp, q, qp, math.nan, step, n)])                                       # a non-finite yaw
    refused(-2, [(t, tp, q, qp, yaw0, math.inf, n)])
    refused(-2, [(t, tp, q, qp, 1e308, 1e308, 3)])                                         # yaw_2 overflows
    refused(-2, [(t, tp, q, qp, yaw0, step, 0)])                                           # n_yaws outside 1 .. max_yaws
    refused(-2, [(t, tp, q, qp, yaw0, step, 5)])
    with pytest.raises(api.LightLoamError) as e:                                           # a volume the last call did not have
        bev.volume(2)
    assert e.value.code == -2
    # more listed points than max_points: 1025 query points and the target's 900
    tight = ctx.bev(kf, **dict(bc.lib_params(c), max_points=1500))
    with pytest.raises(api.LightLoamError) as e:
        tight.match([good[1]])
    assert e.value.code == -4 and tight.timing()[1] == (0, 0, 0)
    tight.match([good[0]])
    tight.close()
    # create: parameters outside their ranges, and a grid that does not fit LDS (the error text is the store's)
    for bad in (dict(half=184, shift_half=16), dict(half=0), dict(half=513), dict(shift_half=0), dict(shift_half=17), dict(cell=0.0), dict(cell=math.inf),
                dict(z_layer=-1.0), dict(z_min=math.nan), dict(excl_yaw=-1), dict(excl_shift=-1), dict(max_ops=0), dict(max_ops=4097), dict(max_yaws=0),
                dict(max_yaws=65), dict(max_points=0)):
        with pytest.raises(api.LightLoamError) as e:
            ctx.bev(kf, **bad)
        assert e.value.code == -2, bad
    ctx.bev(kf, half=183, shift_half=16).close()                                           # (366 + 32)^2 + 4096 = 162 500 bytes: the largest that fits
    assert (bev.timing()[1], bev.volume(0).tobytes(), bev.volume(1).tobytes(), bev.grid(1).tobytes()) == before
    # the store is reset: LL_ERR_STATE until ll_bev_reset
    kf.reset()
    for k in (a, b):
        for f, P in zip(k["frames"], k["poses"]):
            kf.add_points(f[0], f[1], P)
    for call, args in ((bev.match, (good,)), (bev.volume, (0,)), (bev.grid, (0,))):
        with pytest.raises(api.LightLoamError) as e:
            call(*args)
        assert e.value.code == -7
    assert bev.timing()[1] == before[0]
    bev.reset()
    assert bev.timing()[1] == (0, 0, 0)
    with pytest.raises(api.LightLoamError) as e:                                           # the last call is forgotten
        bev.volume(0)
    assert e.value.code == -2
    bev.match(good)
    assert (bev.timing()[1], bev.volume(0).tobytes(), bev.volume(1).tobytes(), bev.grid(1).tobytes()) == before
    bev.close(); kf.close(); ctx.close()


def test_the_store_is_only_read(api):
    import viscases as vc
    frames, poses = vc.random_drive()
    ctx = small_ctx(api)
    kf = ctx.keyframes(len(frames), sum(len(f[0]) for f in frames) + 1, sum(len(f[1]) for f in frames) + 1)
    for f, P in zip(frames, poses):
        kf.add_points(f[0], f[1], P)
    vis = ctx.visibility(kf, max_images=8, width=48, height=12)
    ids = list(range(len(frames)))
    vis.run([(ids, None)])
    counts = [b"".join(x.tobytes() for x in vis.counts(k)) for k in ids]
    pts, off = kf.export()
    before = (pts.tobytes(), off.tobytes(), [kf.info(k)["pose"].tobytes() for k in ids])
    bev = ctx.bev(kf, half=64, max_ops=2)
    got = bev.match([(ids[:3], None, ids[3:], None, 0.0, math.radians(2.0), 3), ([5], None, [0, 1], poses[:2], 1.0, 0.0, 1)])
    assert got[0].n_query > 0 and bev.grid(0).any()
    pts, off = kf.export()
    assert (pts.tobytes(), off.tobytes(), [kf.info(k)["pose"].tobytes() for k in ids]) == before
    assert [b"".join(x.tobytes() for x in vis.counts(k)) for k in ids] == counts
    vis.run([(ids, None)])
    assert [b"".join(x.tobytes() for x in vis.counts(k)) for k in ids] == counts
    bev.close(); vis.close(); kf.close(); ctx.close()


# ---------------------------------------------------------------- from the match to an align guess
def _apply(T, p):
    import viscases as vc
    return vc.np_to_world(T, np.asarray(p, np.float32)).astype(np.float64)


def test_match_guess_align_on_the_yard(api):
    """Two cube maps rebuilt from the target scan and from the displaced query scan, each in its own world (the sensor at (0, 0, 1.8)
    under the identity); the truth that takes the query's map into the target's is the query sensor's pose in the yard.  Asserted is
    only what can be derived: the refinement from the coarse guess ends no farther from the truth than the guess was, by the mean
    distance of the query scan's points under the two transforms.  How far align ends from the Scan Context heading with ZERO
    translation is printed, not asserted."""
    k = 0
    frames, truth = bc.yard_scene()
    case = bc.yard_case(k)
    ctx = small_ctx(api)
    kf, _ = store(ctx, [case])
    bev = ctx.bev(kf)
    got = bev.match([op_of(case)])[0]
    D = np.array(got.D_w7[:])
    z = bc.YARD["sensor_z"]
    Pc = np.array([0, 0, 0, 1, 0, 0, z]); Pq = np.array([0, 0, 0, 1, 0, 0, z])
    many = api.CubeMaps(ctx, 2, 64, 64, pool_points=1 << 17)
    many.insert_keyframes(kf, [(0, [0], [Pc], 1, (10, 10, 5)), (1, [1 + k], [Pq], 1, (10, 10, 5))])
    T_true = bc.np_guess(truth[1 + k], bc.IDENTITY, Pq)                  # the query sensor's pose in the yard o P_q^-1
    T0 = api.bev_guess(Pc, D, Pq)
    sector = math.radians(6.0)
    yaw_sc = round(math.radians(bc.DISPLACEMENTS[k][2]) / sector) * sector
    T_sc = api.bev_guess(Pc, [0.0, 0.0, math.sin(yaw_sc / 2.0), math.cos(yaw_sc / 2.0), 0.0, 0.0, 0.0], Pq)
    pts = _apply(Pq, np.concatenate(frames[1 + k])[:, :3])               # the query scan in its map's world
    far = lambda T: float(np.linalg.norm(_apply(T, pts) - _apply(T_true, pts), axis=1).mean())    # noqa: E731
    T, ran, _ = many.align([(0, 1, T0), (0, 1, T_sc)], n_outer=4)
    print(f"\nmean distance from the truth over the query scan: coarse guess {far(T0):.3f} m -> aligned {far(T[0]):.3f} m (ran {bool(ran[0])}); "
          f"Scan Context heading with zero translation {far(T_sc):.3f} m -> aligned {far(T[1]):.3f} m (ran {bool(ran[1])})")
    reach = float(np.linalg.norm(pts[:, :2], axis=1).mean())
    assert far(T0) <= 0.5 * math.sqrt(2.0) + math.radians(1.0) * reach   # within one cell per axis and one degree about the sensor
    assert far(T[0]) <= far(T0)
    many.close(); bev.close(); kf.close(); ctx.close()
