"""The four places that take lists of frames of a Keyframes store -- Visibility.run, Entropy.run, Bev.match (target and query side)
and CubeMaps.insert_keyframes (plain and filtered) -- at one store of three frames with (5, 7), (0, 3) and (4, 0) points: a frame
with an empty corner cloud and one with an empty surf cloud.  Every refusal they share (an id outside the store, a non-finite given
pose, a duplicate where the site refuses one, the empty / NULL list) with its code AND its exact text; the duplicates a site allows;
the order of refusals inside a call; and after each refusal the object's timing and last-run readers as they were.  The expected
texts are literals, written down from the sources before the four sites shared csrc/ll_kf_list.h (tests/test_kf_list_host.py checks
that header alone); nothing here needs a reference."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_map_merge import small_ctx

pytestmark = pytest.mark.gpu

SIZES = ((5, 7), (0, 3), (4, 0))
ID = [0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]
ARG, CAPACITY, STATE = "LL_ERR_ARG: ", "LL_ERR_CAPACITY: ", "LL_ERR_STATE: "


def cloud(n, seed):
    rng = np.random.default_rng(seed)
    a = np.zeros((n, 4), np.float32)
    a[:, :3] = rng.uniform(-3.0, 3.0, (n, 3)) + [6.0, 0.0, 0.0]     # a few metres from the sensor: inside every range window
    return a


def add_frames(kf):
    for k, (nc, ns) in enumerate(SIZES):
        assert kf.add_points(cloud(nc, 10 + k), cloud(ns, 20 + k), [0.0, 0.0, 0.0, 1.0, 0.1 * k, 0.0, 0.0]) == k


def poses(n, bad=None, value=np.nan):
    p = np.tile(np.array(ID), (n, 1))
    if bad is not None:
        p[bad] = value
    return p


def refused(api, call, code, text):
    with pytest.raises(api.LightLoamError) as e:
        call()
    assert e.value.code == code, (e.value, code)
    assert str(e.value) == text


def raw_list(n_frames, null):
    """(n_frames, the frames pointer, what keeps it alive): the lists the Python wrappers cannot make"""
    f = np.zeros(max(n_frames, 1), np.int32)
    return n_frames, (None if null else f.ctypes.data), f


@pytest.fixture(scope="module")
def objects(api):
    ctx = small_ctx(api)
    kf = ctx.keyframes(8, 64, 64)
    add_frames(kf)
    o = {"ctx": ctx, "kf": kf, "vis": ctx.visibility(kf, max_images=2), "bev": ctx.bev(kf), "en": ctx.entropy(kf, max_points=16),
         "maps": api.CubeMaps(ctx, 1, 64, 64, pool_points=1 << 13)}
    yield o
    ctx.close()


def test_visibility_run(api, objects):
    vis = objects["vis"]
    assert list(vis.run([([0], None), ([1], None)])) == [0, 0]                                   # two ops, two frames: allowed
    vis.run([([0, 2], None)])
    before = lambda: (vis.timing()[1], [tuple(x.tobytes() for x in vis.counts(f)) for f in range(3)], [tuple(x.tobytes() for x in vis.images(k)) for k in range(2)])
    ms, state = vis.timing()[0], before()
    assert state[0] == (2, 5 + 7 + 4, 2)
    cases = [
        ([([0, 3], None)], "visibility: op 0: frame 3 is not in the store (size 3)"),
        ([([1], None), ([-1], None)], "visibility: op 1: frame -1 is not in the store (size 3)"),
        ([([0, 1], poses(2, (1, 2)))], "visibility: op 0: the pose of list entry 1 is not finite"),
        ([([0, 1], poses(2, (0, 6), np.inf))], "visibility: op 0: the pose of list entry 0 is not finite"),
        ([([0, 0], None)], "visibility: op 0: frame 0 is listed twice in this call"),
        ([([0], None), ([0], None)], "visibility: op 1: frame 0 is listed twice in this call"),
        ([([0, 0, 7], None)], "visibility: op 0: frame 0 is listed twice in this call"),              # the first error in list order
        ([([1, 7, 1], None)], "visibility: op 0: frame 7 is not in the store (size 3)"),
    ]
    for ops, text in cases:
        refused(api, lambda: vis.run(ops), -2, ARG + text)
        assert vis.timing()[0] == ms and before() == state, text
    for n, null in ((-1, False), (1, True)):
        n_frames, ptr, keep = raw_list(n, null)
        rec = api.VisibilityOp(n_frames, ptr, None)
        pairs = np.zeros(1, np.int64)
        refused(api, lambda: vis._ck(vis.lib.ll_visibility_run(vis.h, C.addressof(rec), 1, pairs.ctypes.data)), -2, ARG + "visibility: op 0: n_frames < 0 or frames is NULL")
        assert vis.timing()[0] == ms and before() == state
    out = np.zeros((16, 2), np.uint8)                                                            # Visibility.counts asks the store first: the library's own refusal
    for frame in (3, -1):
        refused(api, lambda: vis._ck(vis.lib.ll_visibility_counts(vis.h, frame, out.ctypes.data)), -2, ARG + f"visibility: frame {frame} is not in the store (size 3)")
    refused(api, lambda: vis.run([([0, 1, 2], None)]), -4, CAPACITY + "visibility: 3 listed frames, max_images is 2")
    refused(api, lambda: vis.run([([0, 1, 2, 3], None)]), -2, ARG + "visibility: op 0: frame 3 is not in the store (size 3)")   # arguments before capacity
    assert vis.timing()[0] == ms and before() == state


def test_entropy_run(api, objects):
    en = objects["en"]
    recs = en.run([([1], None), ([1, 2], None)])                                                # the same id in two ops: allowed
    assert [r.n_points for r in recs] == [3, 7]
    en.run([([0, 1], None)])
    before = lambda: (en.timing()[1], [tuple(x.tobytes() for x in en.values(k)) for k in range(2)])
    ms, state = en.timing()[0], before()
    assert state[0][:2] == (2, 15)
    cases = [
        ([([0, 3], None)], "entropy: op 0: frame 3 is not in the store (size 3)"),
        ([([1], None), ([-1], None)], "entropy: op 1: frame -1 is not in the store (size 3)"),
        ([([0, 1], poses(2, (1, 0)))], "entropy: op 0: the pose of list entry 1 is not finite"),
        ([([1], None), ([2], poses(1, (0, 6), -np.inf))], "entropy: op 1: the pose of list entry 0 is not finite"),
        ([([1, 1], None)], "entropy: op 0: frame 1 is listed twice in this op"),
        ([([1], None), ([2, 1, 2], None)], "entropy: op 1: frame 2 is listed twice in this op"),
        ([([0, 1, 2, 9], None)], "entropy: op 0: frame 9 is not in the store (size 3)"),             # a bad id AND over max_points: the argument
    ]
    for ops, text in cases:
        refused(api, lambda: en.run(ops), -2, ARG + text)
        assert en.timing()[0] == ms and before() == state, text
    for n, null in ((-1, False), (1, True)):
        n_frames, ptr, keep = raw_list(n, null)
        rec = api.EntropyOp(n_frames, ptr, None)
        out = (api.EntropyRec * 1)()
        refused(api, lambda: en._ck(en.lib.ll_entropy_run(en.h, C.addressof(rec), 1, C.addressof(out))), -2, ARG + "entropy: op 0: n_frames < 0 or frames is NULL")
    refused(api, lambda: en.run([([0, 1, 2], None)]), -4, CAPACITY + "entropy: 19 listed points, max_points is 16")
    assert en.timing()[0] == ms and before() == state


def test_bev_match(api, objects):
    bev = objects["bev"]
    op = lambda target, tposes, query, qposes: [(target, tposes, query, qposes, 0.0, 0.1, 2)]
    out = bev.match(op([0, 0], None, [1, 1, 0], None))                                          # ids repeat inside a side and across the sides
    assert out[0].n_query >= 0
    bev.match(op([0], None, [1, 2], None))
    before = lambda: (bev.timing()[1], bev.volume(0).tobytes(), bev.grid(0).tobytes())
    ms, state = bev.timing()[0], before()
    assert state[0][:2] == (1, 12 + 3 + 4)
    cases = [
        (op([0, 3], None, [1], None), "bev: op 0: target frame 3 is not in the store (size 3)"),
        (op([0], None, [1, 7], None), "bev: op 0: query frame 7 is not in the store (size 3)"),
        (op([0], None, [1], None) + op([-1], None, [7], None), "bev: op 1: target frame -1 is not in the store (size 3)"),   # the target side first
        (op([0, 1], poses(2, (1, 3)), [1], None), "bev: op 0: the pose of target list entry 1 is not finite"),
        (op([0], None, [1, 2], poses(2, (0, 4), np.inf)), "bev: op 0: the pose of query list entry 0 is not finite"),
        (op([], None, [1], None), "bev: op 0: the target side has no frame or its list is NULL"),
        (op([0], None, [], None), "bev: op 0: the query side has no frame or its list is NULL"),
        ([([0], None, [7], None, 0.0, 0.1, 0)], "bev: op 0: n_yaws = 0 is outside 1 .. max_yaws = 16"),   # the op's own checks before its lists
    ]
    for ops, text in cases:
        refused(api, lambda: bev.match(ops), -2, ARG + text)
        assert bev.timing()[0] == ms and before() == state, text


def test_insert_keyframes(api, objects):
    kf, vis, maps = objects["kf"], objects["vis"], objects["maps"]
    vis.run([([0, 2], None)])
    added, dropped = maps.insert_keyframes(kf, [(0, [0, 0, 1], None, 1, None)])                 # ids may repeat: every listing counts
    assert (added[0] + dropped[0]).tolist() == [10, 17]
    added, dropped, removed = maps.insert_keyframes(kf, [(0, [2, 2], None, 1, None)], visibility=vis, rule=(256, 255))
    assert (added[0] + dropped[0]).tolist() == [8, 0] and removed.tolist() == [[0, 0]]
    before = lambda: (maps.insert_timing(), maps.export(api.MAP_ALL)[0].tobytes(), maps.layout(0)[1].tobytes())
    state = before()
    for kw, what in (({}, "keyframe insert: "), ({"visibility": vis}, "filtered keyframe insert: ")):
        cases = [
            ([(0, [0, 3], None, 0, None)], what + "op 0: frame 3 is not in the store (size 3)"),
            ([(0, [-1], None, 1, None)], what + "op 0: frame -1 is not in the store (size 3)"),
            ([(0, [0, 1], poses(2, (1, 5)), 0, None)], what + "op 0: the pose of list entry 1 is not finite"),
            ([(0, [2], poses(1, (0, 0), np.inf), 1, None)], what + "op 0: the pose of list entry 0 is not finite"),
            ([(1, [3], None, 0, None)], what + "op 0: dst is no map"),                           # the destination before the frames
            ([(0, [3], None, 2, None)], what + "op 0: reset must be 0 or 1"),                    # ... and the op's own fields
        ]
        for ops, text in cases:
            refused(api, lambda: maps.insert_keyframes(kf, ops, **kw), -2, ARG + text)
            assert before() == state, text
    for n, null in ((-1, False), (1, True)):
        n_frames, ptr, keep = raw_list(n, null)
        rec = api.InsertOp(0, n_frames, ptr, None, 0, (C.c_int * 3)(10, 10, 5))
        added = np.zeros((1, 2), np.int64); dropped = np.zeros((1, 2), np.int64)
        refused(api, lambda: maps._ck(maps.lib.ll_cubemaps_insert_keyframes(maps.h, kf.h, C.addressof(rec), 1, added.ctypes.data, dropped.ctypes.data)), -2,
                ARG + "keyframe insert: op 0: n_frames < 0 or frames is NULL")
        assert before() == state


def test_stale_store_comes_after_arguments_and_capacity(api, objects):
    """last: the store is reset and filled again, so every id is valid and every follower is stale"""
    kf, vis, bev, en, maps = (objects[k] for k in ("kf", "vis", "bev", "en", "maps"))
    vis.run([([0, 2], None)]); en.run([([0, 1], None)]); bev.match([([0], None, [1, 2], None, 0.0, 0.1, 2)])
    t_vis, t_en, t_bev, t_ins = vis.timing(), en.timing(), bev.timing(), maps.insert_timing()
    kf.reset()
    add_frames(kf)
    refused(api, lambda: vis.run([([0, 1, 2], None)]), -4, CAPACITY + "visibility: 3 listed frames, max_images is 2")       # over max_images AND stale
    refused(api, lambda: vis.run([([0, 3], None)]), -2, ARG + "visibility: op 0: frame 3 is not in the store (size 3)")
    refused(api, lambda: vis.run([([0, 1], None)]), -7, STATE + "visibility: the store was reset since the counters were made: call ll_visibility_reset")
    refused(api, lambda: en.run([([0, 1, 2], None)]), -4, CAPACITY + "entropy: 19 listed points, max_points is 16")
    refused(api, lambda: en.run([([0, 0], None)]), -2, ARG + "entropy: op 0: frame 0 is listed twice in this op")
    refused(api, lambda: en.run([([0, 1], None)]), -7, STATE + "entropy: the store was reset since the object followed it: call ll_entropy_reset")
    refused(api, lambda: bev.match([([0], None, [7], None, 0.0, 0.1, 2)]), -2, ARG + "bev: op 0: query frame 7 is not in the store (size 3)")
    refused(api, lambda: bev.match([([0], None, [1], None, 0.0, 0.1, 2)]), -7, STATE + "bev: the store was reset since the object was made: call ll_bev_reset")
    refused(api, lambda: maps.insert_keyframes(kf, [(0, [3], None, 0, None)], visibility=vis), -7,
            STATE + "filtered keyframe insert: the store was reset since the counters were made: call ll_visibility_reset")
    assert (vis.timing(), en.timing(), bev.timing(), maps.insert_timing()) == (t_vis, t_en, t_bev, t_ins)
    added, dropped = maps.insert_keyframes(kf, [(0, [1, 1], None, 1, None)])                     # the plain insert follows no epoch
    assert (added[0] + dropped[0]).tolist() == [0, 6]
    vis.reset(); en.reset(); bev.reset()
    assert list(vis.run([([0, 1], None)])) == [2] and en.run([([1, 2], None)])[0].n_points == 7
    assert bev.match([([0], None, [1], None, 0.0, 0.1, 2)])[0].n_query >= 0
