"""ll_visibility and ll_cubemaps_insert_keyframes_filtered through the C ABI against the numpy restatement of tests/viscases.py
(tests/test_vis_cases.py checks the crafted inputs on the restatement alone).  Images are compared as uint32, counters as bytes, maps
through their LL_MAP_ALL export and layout: every comparison is bitwise.  No expected value comes from the library."""
import ctypes as C

import numpy as np
import pytest

import viscases as vc
from test_gpu_map_merge import small_ctx, state_of

pytestmark = pytest.mark.gpu

SIZES = [dict(width=16, height=4), dict()]
COARSE = dict(width=48, height=12)


def fill(ctx, frames, poses, spare=0):
    kf = ctx.keyframes(len(frames) + spare, sum(len(f[0]) for f in frames) + 1 + spare, sum(len(f[1]) for f in frames) + 1 + spare)
    for k, (f, P) in enumerate(zip(frames, poses)):
        assert kf.add_points(f[0], f[1], P) == k
    return kf


def all_counts(vis, n):
    """the counters of frames 0 .. n - 1 as one bytes object per frame"""
    return [b"".join(x.tobytes() for x in vis.counts(k)) for k in range(n)]


def want_bytes(counts):
    return [b"".join(x.tobytes() for x in fc) for fc in counts]


def same_u32(got, want, what):
    got = np.ascontiguousarray(got, np.float32).view(np.uint32); want = np.ascontiguousarray(want, np.float32).view(np.uint32)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"{what}: {len(bad)} pixels differ, first {bad[:4].tolist()}: {got[tuple(bad[0])]:#x} vs {want[tuple(bad[0])]:#x}"


# ---------------------------------------------------------------- images
@pytest.mark.parametrize("size", SIZES, ids=["16x4", "default"])
def test_images_bit_for_bit(api, orc, size):
    c = vc.cfg(**size)
    cases = vc.image_cases(c)
    names = list(cases)
    ctx = small_ctx(api)
    kf = fill(ctx, [cases[n] for n in names], [vc.IDENTITY] * len(names))
    vis = ctx.visibility(kf, max_images=len(names), **vc.lib_params(c))
    half = len(names) // 2
    pairs = vis.run([(list(range(half)), None), (list(range(half, len(names))), None)])         # k counts across the ops
    assert pairs.tolist() == [half * (half - 1), (len(names) - half) * (len(names) - half - 1)]
    for k, n in enumerate(names):
        raw, img = vis.images(k)
        want_raw, want_img = vc.np_images(*cases[n], c)
        same_u32(raw, want_raw, f"{n}: raw"); same_u32(img, want_img, f"{n}: img")
    assert np.isinf(vis.images(names.index("empty"))[1]).all()
    with pytest.raises(api.LightLoamError) as e:
        vis.images(len(names))
    assert e.value.code == -2
    ms, cnt = vis.timing()
    assert cnt == (len(names), sum(len(a) + len(b) for a, b in cases.values()), int(pairs.sum())) and all(m >= 0 for m in ms)
    vis.close(); kf.close(); ctx.close()


# ---------------------------------------------------------------- counters
@pytest.mark.parametrize("stored", [False, True], ids=["given", "stored"])
@pytest.mark.parametrize("size", [COARSE, dict()], ids=["48x12", "default"])
def test_counters_exactly(api, orc, size, stored):
    """op 0: six random frames under random poses, two of them beyond the radius of the first ones; op 1: the margin case (one ulp
    either side of r + m and r - m, an occluded point, a point whose pixel is empty in its observer)"""
    c = vc.cfg(**size)
    f0, p0 = vc.random_drive()
    f1, p1, expect = vc.margin_case(c)
    frames = f0 + f1; poses = np.concatenate([p0, p1])
    ctx = small_ctx(api)
    kf = fill(ctx, frames, poses if stored else [vc.IDENTITY * 3.0] * len(frames))             # "given" must not read the stored poses
    vis = ctx.visibility(kf, max_images=8, **vc.lib_params(c))
    ops = [(list(range(6)), None if stored else p0), ([6, 7], None if stored else p1)]
    pairs = vis.run(ops)
    w0, n0 = vc.np_vote(f0, p0, c); w1, n1 = vc.np_vote(f1, p1, c)
    assert pairs.tolist() == [n0, n1] and 0 < n0 < 30 and n1 == 2
    got, want = all_counts(vis, 8), want_bytes(w0 + w1)
    for k in range(8):
        assert got[k] == want[k], f"frame {k}: counters differ from the restatement"
    both = np.concatenate([np.concatenate(x) for x in w0])
    assert (both[:, 0] > 0).any() and (both[:, 1] > 0).any()                                     # the comparison above saw both kinds
    if not size:
        assert [tuple(int(v) for v in r) for r in np.concatenate(vis.counts(6))] == expect
    vis.close(); kf.close(); ctx.close()


def test_saturation(api):
    """one point seen through by 300 single-point observer frames reads 255, not 300 mod 256 = 44; each observer point is hit by the
    299 others (255) and occluded in the subject's image"""
    n = 300
    frames = [(vc.pts4([[20, 0.5, 1]]), vc.pts4(np.zeros((0, 3))))] + [(vc.pts4(np.zeros((0, 3))), vc.pts4([[40, 1, 2]]))] * n
    ctx = small_ctx(api)
    kf = fill(ctx, frames, [vc.IDENTITY] * (n + 1))
    vis = ctx.visibility(kf, max_images=n + 1, width=64, height=16)
    assert vis.run([(list(range(n + 1)), None)]).tolist() == [(n + 1) * n]
    assert vis.counts(0)[0].tolist() == [[255, 0]]
    for k in (1, n // 2, n):
        assert vis.counts(k)[1].tolist() == [[0, 255]]
    vis.close(); kf.close(); ctx.close()


def test_batches_alone_together_reversed(api, orc):
    c = vc.cfg(**COARSE)
    fa, pa = vc.random_drive(seed=7); fb, pb = vc.random_drive(seed=8, n_frames=5, far=(1,))
    extra = (vc.random_cloud(np.random.default_rng(3), 40), vc.random_cloud(np.random.default_rng(4), 90))
    frames = fa + fb + [extra]; poses = np.concatenate([pa, pb, [vc.IDENTITY]])
    ctx = small_ctx(api)
    kf = fill(ctx, frames, poses)
    vis = ctx.visibility(kf, max_images=11, **vc.lib_params(c))
    A, B = (list(range(6)), None), (list(range(6, 11)), None)
    want = want_bytes(vc.np_vote(fa, pa, c)[0] + vc.np_vote(fb, pb, c)[0]) + [bytes(2 * 130)]     # a frame that never took part: zeros
    vis.run([A, B])
    together = all_counts(vis, 12)
    assert together == want
    vis.reset()
    assert all_counts(vis, 12) == [bytes(len(w)) for w in want]
    vis.run([A])
    assert all_counts(vis, 12)[6:] == [bytes(len(w)) for w in want[6:]]                          # B's frames were not listed: still zero
    vis.run([B])
    assert all_counts(vis, 12) == together
    vis.reset(); vis.run([B, A])
    assert all_counts(vis, 12) == together
    # a run that lists other frames leaves these bytes alone; a frame listed alone in its op has no observer: its counters become zero
    assert vis.run([([11], None), ([0], None)]).tolist() == [0, 0]
    now = all_counts(vis, 12)
    assert now[1:11] == together[1:11] and now[0] == bytes(len(want[0])) and now[11] == bytes(260)
    vis.close(); kf.close(); ctx.close()


# ---------------------------------------------------------------- the filtered insert
@pytest.fixture(scope="module")
def street(orc):
    frames, poses, is_box = vc.street_scene()
    counts, pairs = vc.np_vote(frames, poses, vc.cfg())
    return frames, poses, is_box, counts, pairs


def test_street_scene_end_to_end(api, street):
    frames, poses, is_box, counts, pairs = street
    n = len(frames)
    gone = [(vc.np_removed(cc), vc.np_removed(cs)) for cc, cs in counts]
    assert sum(int(g[0].sum() + g[1].sum()) for g in gone) >= 28                                  # there is something to remove (test_vis_cases)
    ctx = small_ctx(api)
    kf = fill(ctx, frames, poses)
    kept = fill(ctx, [(f[0][~g[0]], f[1][~g[1]]) for f, g in zip(frames, gone)], poses)          # the removed points deleted by hand
    many = api.CubeMaps(ctx, 2, 64, 64, pool_points=1 << 17)
    vis = ctx.visibility(kf, max_images=n)
    assert vis.run([(list(range(n)), None)]).tolist() == [pairs]
    assert all_counts(vis, n) == want_bytes(counts)
    ids = list(range(n))
    added, dropped, removed = many.insert_keyframes(kf, [(0, ids, None, 1, (10, 10, 5))], visibility=vis)
    added1, dropped1 = many.insert_keyframes(kept, [(1, ids, None, 1, (10, 10, 5))])
    assert removed.tolist() == [[sum(int(g[w].sum()) for g in gone) for w in (0, 1)]]
    listed = [sum(len(f[w]) for f in frames) for w in (0, 1)]
    assert (added + dropped + removed).tolist() == [listed]
    assert added.tolist() == added1.tolist() and dropped.tolist() == dropped1.tolist()
    assert state_of(many, 0) == state_of(many, 1)
    assert many.insert_timing()[1][0] == sum(listed) - int(removed.sum())                         # the last insert: the store without them
    vis.close(); many.close(); kept.close(); kf.close(); ctx.close()


def test_nothing_removed_nothing_changed(api, orc):
    c = vc.cfg(**COARSE)
    frames, poses = vc.random_drive()
    want, _ = vc.np_vote(frames, poses, c)
    assert vc.np_removed(np.concatenate([np.concatenate(x) for x in want])).sum() > 10          # the default rule would remove points here
    ctx = small_ctx(api)
    kf = fill(ctx, frames, poses)
    many = api.CubeMaps(ctx, 5, 64, 64, pool_points=1 << 13)
    vis = ctx.visibility(kf, max_images=8, **vc.lib_params(c))
    ids = list(range(6))
    op = lambda q: [(q, ids, None, 1, (10, 10, 5))]                                                # noqa: E731
    a0, d0 = many.insert_keyframes(kf, op(0))
    vis.run([(ids, None)])
    a1, d1 = many.insert_keyframes(kf, op(1))                                                     # the plain insert, before and after a run
    assert state_of(many, 1) == state_of(many, 0) and a1.tolist() == a0.tolist() and d1.tolist() == d0.tolist()
    a2, d2, r2 = many.insert_keyframes(kf, op(2), visibility=vis, rule=(256, 255))                # 256 never removes
    assert state_of(many, 2) == state_of(many, 0) and a2.tolist() == a0.tolist() and d2.tolist() == d0.tolist() and r2.tolist() == [[0, 0]]
    a3, d3, r3 = many.insert_keyframes(kf, op(3), visibility=vis)                                 # the default rule does remove
    assert r3.sum() == vc.np_removed(np.concatenate([np.concatenate(x) for x in want])).sum() and state_of(many, 3) != state_of(many, 0)
    assert (a3 + d3 + r3).tolist() == (a0 + d0).tolist()
    vis.reset()                                                                                   # counters all zero
    a4, d4, r4 = many.insert_keyframes(kf, op(4), visibility=vis)
    assert state_of(many, 4) == state_of(many, 0) and a4.tolist() == a0.tolist() and d4.tolist() == d0.tolist() and r4.tolist() == [[0, 0]]
    vis.close(); many.close(); kf.close(); ctx.close()


# ---------------------------------------------------------------- refusals
def test_refusals_change_nothing(api, orc):
    c = vc.cfg(**COARSE)
    frames, poses = vc.random_drive()
    ctx = small_ctx(api)
    kf = fill(ctx, frames, poses, spare=400)
    other = fill(ctx, frames[:2], poses[:2])
    many = api.CubeMaps(ctx, 1, 64, 64, pool_points=1 << 13)
    vis = ctx.visibility(kf, max_images=6, **vc.lib_params(c))
    vis_other = ctx.visibility(other, max_images=2, **vc.lib_params(c))
    ids = list(range(6))
    vis.run([(ids, None)])
    many.insert_keyframes(kf, [(0, ids, None, 1, None)])
    before = (all_counts(vis, 6), state_of(many, 0))

    def refused(code, call, *a, **k):
        with pytest.raises(api.LightLoamError) as e:
            call(*a, **k)
        assert e.value.code == code, (e.value, code)
        assert (all_counts(vis, 6), state_of(many, 0)) == before

    bad_pose = poses.copy(); bad_pose[2, 5] = np.nan
    refused(-2, vis.run, [])                                                                       # n_ops < 1
    refused(-2, vis.run, [([0, 1, 1], None)])                                                      # twice in one op
    refused(-2, vis.run, [([0, 1], None), ([2, 0], None)])                                         # twice across ops
    refused(-2, vis.run, [([0, 6], None)]); refused(-2, vis.run, [([-1, 0], None)])                # outside the store
    refused(-2, vis.run, [(ids, bad_pose)])
    kf.add_points(frames[0][0], frames[0][1], poses[0])                                            # a seventh frame: one too many for max_images
    refused(-4, vis.run, [(ids[:3], None), (ids[3:] + [6], None)])
    lib = api.load_library()
    rec = api.VisibilityOp(0, None, None)
    assert lib.ll_visibility_run(None, C.addressof(rec), 1, None) == -2 and lib.ll_visibility_run(vis.h, None, 1, None) == -2
    rec = api.VisibilityOp(2, None, None)
    assert lib.ll_visibility_run(vis.h, C.addressof(rec), 1, None) == -2                           # frames NULL with frames to read
    rec = api.VisibilityOp(-1, None, None)
    assert lib.ll_visibility_run(vis.h, C.addressof(rec), 1, None) == -2
    assert lib.ll_visibility_counts(None, 0, None) == -2 and lib.ll_visibility_reset(None) == -2
    refused(-2, vis.counts, 7)
    op = [(0, ids, None, 0, None)]
    for rule in [(0, 255), (257, 255), (2, -1), (2, 256)]:
        refused(-2, many.insert_keyframes, kf, op, visibility=vis, rule=rule)
    refused(-2, many.insert_keyframes, kf, op, visibility=vis_other)                               # a visibility object of another store
    refused(-2, many.insert_keyframes, other, op, visibility=vis)
    refused(-2, many.insert_keyframes, kf, [(0, [9], None, 0, None)], visibility=vis)
    assert (all_counts(vis, 6), state_of(many, 0)) == before
    # an op with fewer than two frames, or with no pair within the radius, succeeds and zeroes its frames' counters
    far = poses[:2].copy(); far[1, 4:] = far[0, 4:] + [0.0, 41.0, 0.0]
    assert vis.run([([3], None), ([0, 1], far), ([], None)]).tolist() == [0, 0, 0]
    now = all_counts(vis, 6)
    assert [now[k] == bytes(len(now[k])) for k in range(6)] == [True, True, False, True, False, False] and now[2] == before[0][2]
    # the store is reset: the counters mean nothing until ll_visibility_reset
    map_before = state_of(many, 0)
    kf.reset()
    for k, (f, P) in enumerate(zip(frames, poses)):
        kf.add_points(f[0], f[1], P)
    for call, a, k in [(vis.run, ([(ids, None)],), {}), (vis.counts, (0,), {}), (many.insert_keyframes, (kf, op), dict(visibility=vis))]:
        with pytest.raises(api.LightLoamError) as e:
            call(*a, **k)
        assert e.value.code == -7
    assert state_of(many, 0) == map_before
    vis.reset()
    assert all_counts(vis, 6) == [bytes(len(x)) for x in before[0]]
    vis.run([(ids, None)])
    assert all_counts(vis, 6) == before[0]
    vis_other.close(); vis.close(); many.close(); other.close(); kf.close(); ctx.close()
