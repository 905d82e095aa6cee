"""ll_places on the GPU against the numpy restatement of tests/placecases.py: descriptor bits at crafted points and of resident
slots, exact (distance, shift) on one-hot descriptors -- which also pins the MFMA operand and accumulator lane maps: a swapped A and B,
or rows and columns, answers 60 - s --, float64 agreement on random descriptors, batch independence, the K-best selection, a lap of
the synthetic circle end to end, and ll_drives' slots.  No expected value comes from the library."""
import numpy as np
import pytest

import placecases as pc
from conftest import assert_bit_equal

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(api):
    c = api.Context(api.default_params(16, batch=2, max_points=4096))
    yield c
    c.close()


def _db(ctx, descs, capacity=None):
    db = ctx.places(capacity or len(descs))
    db.upload(0, np.stack(descs))
    return db


# ------------------------------------------------------------------------------------------------ the descriptor
@pytest.mark.parametrize("name", sorted(pc.describe_cases()))
def test_descriptor_bits_at_crafted_points(ctx, orc, name):
    pts, _ = pc.describe_cases()[name]
    db = ctx.places(2)
    assert db.add_points(pts) == 0 and db.add_points(pts[::-1]) == 1        # a maximum does not depend on the order
    got = db.download()
    want = pc.np_describe(pts)
    assert_bit_equal(got[0], want, name); assert_bit_equal(got[1], want, name + " reversed")
    db.close()


def test_descriptor_with_other_parameters(ctx, orc):
    pts = pc._inside(np.random.default_rng(5), 3000, max_radius=50.0)
    pts = np.concatenate([pts, pc.describe_cases()["n4097"][0]])             # points beyond 50 m are dropped
    db = ctx.places(1, max_radius=50.0, z_offset=1.25)
    db.add_points(pts)
    assert_bit_equal(db.download()[0], pc.np_describe(pts, 50.0, 1.25), "max_radius 50")
    db.close()


def test_slots_equal_the_description_of_their_downloaded_cloud(api, synth, orc):
    cfg = synth.default_cfg(16)
    thin = synth.default_cfg(16, drop_prob=0.3)                              # ring lengths differ
    scans = [synth.scan(cfg, 0), synth.scan(thin, 5), synth.scan(cfg, 9), np.zeros((0, 4), np.float32), np.full((300, 4), np.nan, np.float32)]
    c = api.Context(api.default_params(16, batch=len(scans), max_points=max(map(len, scans))))
    for k, s in enumerate(scans):
        c.upload_scan(k, s)
    c.extract(0, len(scans))
    assert [c.scan_info(k).status for k in range(5)] == [0, 0, 0, -5, -5]
    assert len(set(np.diff(c.cloud(1)[1]).tolist())) > 1                     # scan_start differences: the rings' lengths
    db = c.places(8)
    order = [2, 3, 0, 4, 1, 0]                                               # any order, a slot twice: ids follow the list
    assert db.add_slots(order[:2]) == 0 and db.add_slots(order[2:]) == 2 and len(db) == 6
    got = db.download()
    for i, k in enumerate(order):
        if k in (3, 4):
            assert not got[i].any(), k                                       # an empty scan: the all-zero descriptor
        else:
            cloud = c.cloud(k)[0]
            assert len(cloud) > 10000
            assert_bit_equal(got[i], pc.np_describe(cloud), "slot %d" % k)
    assert got[2].any() and (got[2] != got[4]).any()
    db.close(); c.close()


def test_a_refused_slot_gives_zeros(api, synth):
    scan = synth.scan(synth.default_cfg(16), 0)
    c = api.Context(api.default_params(16, batch=1, max_points=len(scan), max_ring_points=1024))
    c.upload_scan(0, scan); c.extract(0, 1)
    assert c.scan_info(0).status == -4
    db = c.places(1)
    db.add_slots([0])
    assert not db.download().any()
    db.close(); c.close()


def test_upload_download_reset(ctx, api):
    rng = np.random.default_rng(3)
    d = np.stack([pc.random_descriptor(rng) for _ in range(5)])
    db = ctx.places(6)
    db.upload(0, d[:3]); db.upload(3, d[3:]); assert len(db) == 5
    db.upload(1, d[4:5])                                                     # overwrite: the match-ready form follows
    assert_bit_equal(db.download(), np.stack([d[0], d[4], d[2], d[3], d[4]]), "upload")
    dist, shift = db.distances(1, 1, 4, 1)
    assert dist[0, 0] < 1e-6 and shift[0, 0] == 0
    for bad in (lambda: db.upload(6, d[:1]), lambda: db.download(3, 3), lambda: db.upload(-1, d[:1])):
        with pytest.raises(api.LightLoamError) as e:
            bad()
        assert e.value.code == -2
    with pytest.raises(api.LightLoamError) as e:
        db.upload(4, d[:3])
    assert e.value.code == -4 and len(db) == 5
    t = db.timing()
    assert t["places"] == 1 and t["pairs"] == 1 and t["ms"][0] > 0 and t["ms"][1] > 0 and t["ms"][2] == 0
    db.reset(); assert len(db) == 0
    db.close()


# ------------------------------------------------------------------------------------------------ the distance
def test_onehot_pairs_are_exact(ctx):
    cases = pc.onehot_cases()
    names = sorted(cases)
    db = _db(ctx, [d for n in names for d in cases[n][:2]])
    dist, shift = db.distances(0, len(db), 0, len(db))
    for i, n in enumerate(names):
        want_d, want_s = pc.onehot_expected(*cases[n][:2])
        got = (dist[2 * i, 2 * i + 1], int(shift[2 * i, 2 * i + 1]))
        assert got[1] == want_s and got[0].tobytes() == np.float32(want_d).tobytes(), (n, got, want_d, want_s)
        back = pc.onehot_expected(cases[n][1], cases[n][0])                  # candidate against query: the other heading
        got = (dist[2 * i + 1, 2 * i], int(shift[2 * i + 1, 2 * i]))
        assert got[1] == back[1] and got[0].tobytes() == np.float32(back[0]).tobytes(), (n, "swapped", got, back)
    want = np.array([[pc.onehot_expected(db_q, db_c) for db_c in db.download()] for db_q in db.download()[:4]])
    assert (dist[:4] == want[:, :, 0].astype(np.float32)).all() and (shift[:4] == want[:, :, 1]).all()     # unrelated pairs, ties between shifts
    db.close()


@pytest.fixture(scope="module")
def random_cases():
    out = {}
    for nq, nc in pc.MATCH_SIZES:
        qs, cand, turned = pc.random_match_case(nq, nc)
        D = np.array([[pc.np_distances(q, c) for c in cand] for q in qs])   # [nq][nc][60], float64
        out[(nq, nc)] = (qs, cand, turned, D)
    return out


@pytest.mark.parametrize("nq,nc", pc.MATCH_SIZES)
def test_random_descriptors_agree_with_float64(ctx, random_cases, nq, nc):
    qs, cand, turned, D = random_cases[(nq, nc)]
    db = _db(ctx, qs + cand)
    dist, shift = db.distances(0, nq, nq, nc)
    best = D.min(axis=2)
    err = np.abs(dist.astype(np.float64) - best)
    at = np.take_along_axis(D, shift[:, :, None].astype(np.int64), axis=2)[:, :, 0]
    print("max |d - d64| = %.3g, max d64(shift) - min = %.3g" % (err.max(), (at - best).max()))
    assert (shift < 60).all()
    assert (err <= 1e-5).all()
    assert (at - best <= 2e-5).all()
    for i in range(nq):                                                      # the revisit's heading is unique by more than 1e-3
        assert shift[i, i % nc] == turned[i]
    db.close()


def test_a_pair_has_the_same_bits_alone_and_in_any_batch(ctx, random_cases):
    for (nq, nc), cs in (((33, 65), [0, 3, 4, 31, 63, 64]), ((2, 130), [0, 63, 64, 127, 128, 129])):
        qs, cand, _, _ = random_cases[(nq, nc)]
        db = _db(ctx, qs + cand)
        dist, shift = db.distances(0, nq, nq, nc)
        for q in (0, nq - 1):
            for c in cs:
                d1, s1 = db.distances(q, 1, nq + c, 1)
                assert d1[0, 0].tobytes() == dist[q, c].tobytes() and s1[0, 0] == shift[q, c], (nq, nc, q, c)
        d2, s2 = db.distances(nq - 1, 1, nq + 2, nc - 2)                     # another tiling of the same pairs
        assert d2.tobytes() == dist[nq - 1:, 2:].tobytes() and s2.tobytes() == shift[nq - 1:, 2:].tobytes()
        ids, dm, sm = db.match(0, nq, nq, nc, K=1)
        first = np.array([np.flatnonzero(dist[q] == dist[q].min())[0] for q in range(nq)])
        assert (ids[:, 0] == nq + first).all() and dm[:, 0].tobytes() == dist[np.arange(nq), first].tobytes()
        assert (sm[:, 0] == shift[np.arange(nq), first]).all()
        db.close()


# ------------------------------------------------------------------------------------------------ the K best
@pytest.fixture(scope="module")
def topk(ctx):
    qs, cand = pc.topk_case()
    db = _db(ctx, cand + qs)                                                 # candidates 0 .. 69, queries 70 .. 74
    yield db, pc.np_ranking(qs, cand)
    db.close()


@pytest.mark.parametrize("K", pc.MATCH_K)
def test_match_is_the_stable_sort_of_distances(topk, K):
    db, D64 = topk
    nq, nc = D64.shape
    dist, shift = db.distances(nc, nq, 0, nc)
    ids, dm, sm = db.match(nc, nq, 0, nc, K=K)
    for q in range(nq):
        order = np.argsort(dist[q], kind="stable")[:K]
        assert ids[q].tolist() == order.tolist(), q
        assert dm[q].tobytes() == dist[q, order].tobytes() and sm[q].tolist() == shift[q, order].tolist()
        assert ids[q].tolist() == np.argsort(D64[q], kind="stable")[:K].tolist(), q      # and the float64 ranking: the ranks are 1e-4 apart
    if K > 1:
        assert ids[0, 1:3].tolist() == [12, 41][:K - 1] and dm[0, 1] == dist[0, 41]       # the duplicate ties to the lower id


def test_match_c_end_hides_ids_at_and_above_it(topk):
    db, D64 = topk
    nq, nc = D64.shape
    dist, _ = db.distances(nc, nq, 0, nc)
    c_end = [13, 0, 70, 41, -5]
    ids, dm, sm = db.match(nc, nq, 0, nc, K=3, c_end=c_end)
    for q, e in enumerate(c_end):
        vis = max(0, min(e, nc))
        order = np.argsort(dist[q, :vis], kind="stable")[:3].tolist()
        assert ids[q].tolist() == order + [-1] * (3 - len(order)), q
        assert dm[q, :len(order)].tobytes() == dist[q, order].tobytes() and np.isposinf(dm[q, len(order):]).all() and not sm[q, len(order):].any()
    assert ids[0, 0] == 12                                                   # 12 is seen, its copy 41 is not
    ids, _, _ = db.match(nc, nq, 10, 40, K=2, c_end=[13, 11, 10, 200, 50])   # a window: ids are database ids, c_end compares with them
    assert ids[0].tolist() == (np.argsort(dist[0, 10:13], kind="stable")[:2] + 10).tolist()
    assert ids[1].tolist() == [10, -1] and ids[2].tolist() == [-1, -1] and (ids[3] >= 10).all() and (ids[3] < 50).all()


def test_match_pads_and_refuses(topk, api):
    db, D64 = topk
    nq, nc = D64.shape
    ids, dm, sm = db.match(nc, 2, 0, 3, K=8)                                 # nc < K
    dist, shift = db.distances(nc, 2, 0, 3)
    for q in range(2):
        order = np.argsort(dist[q], kind="stable").tolist()
        assert ids[q].tolist() == order + [-1] * 5 and np.isposinf(dm[q, 3:]).all() and not sm[q, 3:].any()
        assert dm[q, :3].tobytes() == dist[q, order].tobytes()
    ids, dm, sm = db.match(nc, 2, 0, 0, K=2)
    assert (ids == -1).all() and np.isposinf(dm).all() and not sm.any()
    n = len(db)
    for call in (lambda: db.match(nc, nq, 0, nc, K=0), lambda: db.match(nc, nq, 0, nc, K=9), lambda: db.match(nc, nq + 1, 0, nc),
                 lambda: db.match(-1, 1, 0, nc), lambda: db.distances(0, 1, n, 1), lambda: db.distances(0, n + 1, 0, 1)):
        with pytest.raises(api.LightLoamError) as e:
            call()
        assert e.value.code == -2
    full = db.ctx.places(2)
    full.add_points(np.zeros((1, 4), np.float32))
    with pytest.raises(api.LightLoamError) as e:
        full.add_slots([0, 1])                                               # 1 + 2 > 2: nothing is added
    assert e.value.code == -4 and len(full) == 1
    full.add_slots([0])
    for call in (lambda: full.add_points(np.zeros((1, 4), np.float32)), lambda: full.add_slots([1])):
        with pytest.raises(api.LightLoamError) as e:
            call()
        assert e.value.code == -4 and len(full) == 2
    full.reset()
    with pytest.raises(api.LightLoamError) as e:
        full.add_slots([2])                                                  # the context has two slots
    assert e.value.code == -2 and len(full) == 0
    full.close()


# ------------------------------------------------------------------------------------------------ end to end
def test_a_lap_is_recognised_with_its_heading(ctx, synth):
    scans, queries, want, want_shift = pc.lap_scans(synth)
    db = ctx.places(len(scans) + len(queries))
    for s in scans + queries:
        db.add_points(s)
    n = len(scans)
    ids, dm, sm = db.match(n, len(queries), 0, n, K=2)
    print("lap: best", dm[:, 0].tolist(), "second", dm[:, 1].tolist())
    assert ids[:, 0].tolist() == want and sm[:, 0].tolist() == want_shift
    assert (dm[:, 0] < 0.2).all() and (dm[:, 1] > 0.5).all()
    db.close()


def test_drives_slots_before_the_step_hold_the_steps_cloud(api, synth):
    cfg = synth.default_cfg(16)
    scans = [synth.scan(cfg, k) for k in range(3)]
    plain = api.Context(api.default_params(16, batch=3, max_points=max(map(len, scans))))
    for k, s in enumerate(scans):
        plain.upload_scan(k, s)
    plain.extract(0, 3)
    ref = plain.places(3)
    ref.add_slots([0, 1, 2])
    want = ref.download()
    ref.close(); plain.close()
    c = api.Context(api.default_params(16, batch=2, max_points=max(map(len, scans))))
    dr = api.Drives(c, 1, 4096, 32768, pool_points=1 << 18)
    db = c.places(3)
    for k, s in enumerate(scans):
        slots = dr.slots()                                                   # BEFORE the step: where the scan goes and its cloud stays
        c.upload_scan(int(slots[0]), s)
        dr.step(np.array([api.START if k == 0 else api.RUN], np.int32), np.array([[0, 0, 0, 1.0, cfg.speed * cfg.period, 0, 0]]))
        assert db.add_slots(slots) == k
    got = db.download()
    assert want.any(axis=(1, 2)).all()
    assert_bit_equal(got, want, "drive lane")
    db.close(); dr.close(); c.close()
