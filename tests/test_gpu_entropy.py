"""ll_entropy through the C ABI against the brute-force numpy restatement of tests/entropycases.py (tests/test_entropy_cases.py checks
the restatement and the crafted inputs without a GPU).  Neighbour counts are compared exactly, h and pv within a bound derived below,
records and repeated runs bytewise.  No expected value comes from the library.

THE BOUND on a point with n neighbours, u = 2^-53, r = radius.  The f32 differences d are the same floats on both sides and their
products are exact in f64, so only the sums and what follows differ.  A sum of n terms of size <= r^2 in any order carries at most
n u times the sum of their sizes, after the division by n at most n u r^2; the mean's square the same again; with the roundings of the
divisions and the subtraction every entry of Sigma carries at most 4 (n + 8) u r^2.  By Weyl an eigenvalue of a symmetric 3 x 3 moves
by at most the perturbation's norm <= 3 times the entry bound; the Jacobi rotations add at most 64 u r^2.  h = 0.5 sum ln max(l, floor)
moves by at most 0.5 * 3 * (eigenvalue bound) / floor.  The store adds half an f32 ulp.  numpy.linalg.eigvalsh and the sums of the
restatement have errors of the same kind: twice the bound is allowed.  The largest error / bound ratio is printed.

EN_CHUNK, the LDS staging chunk of k_en_moments, is 256 candidates (entropycases.CHUNK): the 300-point cell is longer."""
import ctypes as C
import math

import numpy as np
import pytest

import entropycases as ec
import viscases as vc
from test_gpu_map_merge import small_ctx

pytestmark = pytest.mark.gpu

F = np.float32
REC_FIELDS = ("n_points", "n_valid", "n_sparse", "n_outside", "n_pairs", "sum_h", "sum_pv", "mme", "mpv")


def fill(ctx, frames, poses, spare=0):
    kf = ctx.keyframes(len(frames) + spare, sum(len(f[0]) for f in frames) + 1 + spare, sum(len(f[1]) for f in frames) + 1 + spare)
    for k, (f, P) in enumerate(zip(frames, poses)):
        assert kf.add_points(f[0], f[1], P) == k
    return kf


def n_points(frames):
    return sum(len(a) + len(b) for a, b in frames)


def all_values(en, L):
    return [tuple(x.tobytes() for x in en.values(k)) for k in range(L)]


def rec_dict(r):
    return {k: getattr(r, k) for k in REC_FIELDS}


def op_values(en, k0, n_frames):
    """the values of list positions k0 .. k0 + n_frames - 1, concatenated in list order"""
    parts = [en.values(k) for k in range(k0, k0 + n_frames)]
    return tuple(np.concatenate([p[j] for p in parts]) if parts else np.zeros(0) for j in range(3))


def check_values(got, want, c, what):
    """got: (h, pv, nn) of the library; want: entropycases.np_op.  nn exactly, the NaNs where they belong, h and pv within twice the
    derived bound -> (largest pv ratio, largest h ratio)"""
    h, pv, nn = got
    assert len(nn) == len(want["nn"]), what
    bad = np.nonzero(nn.astype(np.int64) != np.minimum(want["nn"], 65535))[0]
    assert len(bad) == 0, f"{what}: nn differs at {bad[:8].tolist()}: {nn[bad[:8]].tolist()} vs {want['nn'][bad[:8]].tolist()}"
    valid = want["nn"] >= c["min_neighbours"]
    assert (np.isnan(h) == ~valid).all() and (np.isnan(pv) == ~valid).all(), what
    if not valid.any():
        return 0.0, 0.0
    be, bh = ec.bounds(want["nn"][valid], c)
    r_pv = np.abs(pv[valid].astype(np.float64) - want["pv64"][valid]) / (be + ec.half_ulp32(want["pv64"][valid]))
    r_h = np.abs(h[valid].astype(np.float64) - want["h64"][valid]) / (bh + ec.half_ulp32(want["h64"][valid]))
    print(f"{what}: {int(valid.sum())} valid points, largest error / bound: pv {r_pv.max():.3g}, h {r_h.max():.3g}")
    assert r_pv.max() <= 2.0 and r_h.max() <= 2.0, (what, r_pv.max(), r_h.max())
    return float(r_pv.max()), float(r_h.max())


def check_rec(rec, got, want, c, what):
    """counts against the restatement exactly; the sums against math.fsum of the library's own stored values within n u sum|v|"""
    r = rec_dict(rec)
    for k in ("n_points", "n_valid", "n_sparse", "n_outside", "n_pairs"):
        assert r[k] == want["rec"][k], (what, k, r[k], want["rec"][k])
    assert r["n_points"] == r["n_valid"] + r["n_sparse"] + r["n_outside"]
    h, pv, nn = got
    valid = ~np.isnan(h)
    assert int(valid.sum()) == r["n_valid"]
    for name, v in (("sum_h", h), ("sum_pv", pv)):
        v = v[valid].astype(np.float64)
        assert abs(r[name] - math.fsum(v)) <= max(len(v), 1) * ec.U * float(np.abs(v).sum()), (what, name)
    nv = r["n_valid"]
    assert r["mme"] == (r["sum_h"] / nv if nv else 0.0) and r["mpv"] == (r["sum_pv"] / nv if nv else 0.0)


# ---------------------------------------------------------------- the crafted clouds
def crafted(c):
    """-> (frames of the store, ops as (name, ids, poses))"""
    rng = np.random.default_rng(20261020)
    frames, ops = [], []

    def add(*clouds):
        ids = []
        for x in clouds:
            frames.append(x if isinstance(x, tuple) else ec.one_frame(x)); ids.append(len(frames) - 1)
        return ids

    rnd = add(*[ec.random_box(rng, 1500, 3.0) for _ in range(3)])
    rp = np.array([np.concatenate([vc.quat(rng.uniform(-np.pi, np.pi), rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2)), rng.uniform(-0.3, 0.3, 3)]) for _ in rnd])
    ops.append(("random", rnd, rp))
    edge = add(ec.edge_pairs(c), ec.face_points(c))
    ops.append(("edges and faces", edge, [ec.IDENTITY] * 2))
    ops.append(("edges and faces near 1e4", edge, [ec.shift_pose([1e4, -1e4, 1e4])] * 2))
    near = float(F(ec.HALF) * c["cell"]) - 12.0
    ops.append(("edges and faces near the range's end", edge, [ec.shift_pose([near, -near, near])] * 2))
    clusters, _ = ec.cell_clusters(c)
    misc = add(ec.range_edge(c), ec.BAD_POINTS, ec.min_edge_clusters(c), clusters)
    ops.append(("range end, bad points, min_neighbours, cell sizes", misc, [ec.IDENTITY] * 4))
    ops.append(("one point", add(np.array([[1.0, 2.0, 3.0]])), [ec.IDENTITY]))
    ops.append(("no corner cloud", add((ec.pts4(np.zeros((0, 3))), ec.pts4(ec.random_box(rng, 200, 1.0)))), [ec.IDENTITY]))
    flat, line = ec.flat_and_line()
    ops.append(("flat and line", add((ec.pts4(flat[:10]), ec.pts4(flat[10:])), (ec.pts4(line[:3]), ec.pts4(line[3:]))), [ec.IDENTITY] * 2))
    return frames, ops


@pytest.fixture(scope="module")
def crafted_case():
    c = ec.cfg()
    frames, ops = crafted(c)
    want = [ec.np_op([frames[i] for i in ids], poses, c) for _, ids, poses in ops]
    return c, frames, ops, want


def test_crafted_clouds_against_brute_force(api, crafted_case):
    c, frames, ops, want = crafted_case
    ctx = small_ctx(api)
    kf = fill(ctx, frames, [ec.IDENTITY * 3.0] * len(frames))                                   # given poses must not read the stored ones
    total = sum(n_points([frames[i] for i in ids]) for _, ids, _ in ops)
    en = ctx.entropy(kf, max_points=total, **ec.lib_params(c))
    recs = en.run([(ids, np.array(poses)) for _, ids, poses in ops])
    k0, worst = 0, [0.0, 0.0]
    for (name, ids, _), w, rec in zip(ops, want, recs):
        got = op_values(en, k0, len(ids))
        r = check_values(got, w, c, name)
        worst = [max(a, b) for a, b in zip(worst, r)]
        check_rec(rec, got, w, c, name)
        k0 += len(ids)
    print(f"crafted clouds: largest error / bound ratio: pv {worst[0]:.3g}, h {worst[1]:.3g}")
    by = {name: (w, rec) for (name, _, _), w, rec in zip(ops, want, recs)}
    assert by["one point"][1].n_sparse == 1 and by["one point"][0]["nn"].tolist() == [1]
    assert by["no corner cloud"][1].n_points == 200
    w, rec = by["range end, bad points, min_neighbours, cell sizes"]
    assert rec.n_outside >= len(ec.BAD_POINTS) + 4 and w["nn"].max() == 300 > ec.CHUNK and rec.n_sparse >= c["min_neighbours"] - 1
    # the translated copies: near 1e4 every point has a cell; 12 m from the range's end the seven points of entropycases.edge_pairs at
    # x = 30 lie beyond it (the counts were compared with the restatement's above)
    for name, n_out in (("edges and faces near 1e4", 0), ("edges and faces near the range's end", 7)):
        assert by[name][1].n_outside == n_out and by[name][1].n_valid > 1000
    # exactly planar and exactly collinear: finite h through the floor, pv exactly zero
    k_flat = sum(len(ids) for _, ids, _ in ops[:-1])
    for k in (k_flat, k_flat + 1):
        h, pv, nn = en.values(k)
        assert (nn >= c["min_neighbours"]).all() and np.isfinite(h).all() and (pv == 0.0).all()
    ms, cnt = en.timing()
    assert cnt[0] == sum(len(ids) for _, ids, _ in ops) and cnt[1] == total and cnt[3] == sum(r.n_pairs for r in recs) and cnt[2] > 100
    assert cnt[4] == 2 and all(m >= 0 for m in ms)                                              # two synchronisations, eight ops
    recs1 = en.run([(ops[0][1], ops[0][2])])
    assert en.timing()[1][4] == 2 and bytes(recs1[0]) == bytes(recs[0])                         # ... and one op
    en.close(); kf.close(); ctx.close()


# ---------------------------------------------------------------- bits
def test_same_bits_alone_in_batches_and_on_repetition(api, crafted_case):
    c, frames, ops, _ = crafted_case
    ctx = small_ctx(api)
    kf = fill(ctx, frames, [ec.IDENTITY] * len(frames))
    en = ctx.entropy(kf, max_points=3 * 4500 + 8000, **ec.lib_params(c))
    A = (ops[0][1], ops[0][2]); B = (ops[1][1], np.array(ops[2][2])); E = (ops[4][1], None)
    n = len(A[0])
    rec = en.run([A])
    alone = (all_values(en, n), bytes(rec[0]))
    assert (bytes(en.run([A])[0]), all_values(en, n)) == (alone[1], alone[0])                    # repetition
    rec = en.run([A, B, E])
    assert (all_values(en, n), bytes(rec[0])) == alone                                           # first in a batch
    nb = len(B[0]) + len(E[0])
    rec = en.run([E, B, A])
    assert (all_values(en, nb + n)[nb:], bytes(rec[2])) == alone                                 # last
    other = A[1].copy(); other[:, 4:] += [[0.11, 0.0, 0.0], [0.0, -0.07, 0.0], [0.0, 0.0, 0.05]]
    rec = en.run([A, (A[0], other), A])                                                          # the same ids in three ops of one call
    v = all_values(en, 3 * n)
    assert (v[:n], bytes(rec[0])) == alone and (v[2 * n:], bytes(rec[2])) == alone
    assert v[n:2 * n] != alone[0] and bytes(rec[1]) != alone[1] and rec[1].n_points == rec[0].n_points
    en.close(); kf.close(); ctx.close()


def test_stored_poses_equal_the_same_poses_given(api, crafted_case):
    c, frames, ops, want = crafted_case
    ids, poses = ops[0][1], ops[0][2]
    ctx = small_ctx(api)
    kf = fill(ctx, [frames[i] for i in ids], poses)
    en = ctx.entropy(kf, max_points=4500, **ec.lib_params(c))
    here = list(range(len(ids)))
    rec = en.run([(here, None)])
    stored = (all_values(en, len(ids)), bytes(rec[0]))
    check_values(op_values(en, 0, len(ids)), want[0], c, "stored poses")
    rec = en.run([(here, poses)])
    assert (all_values(en, len(ids)), bytes(rec[0])) == stored
    en.close(); kf.close(); ctx.close()


# ---------------------------------------------------------------- the street scene
def test_street_scene_under_drift(api):
    frames, poses, want = ec.street()
    c = ec.cfg()
    n = n_points(frames)
    ctx = small_ctx(api)
    kf = fill(ctx, frames, poses[0])
    en = ctx.entropy(kf, max_points=3 * n)
    ids = list(range(len(frames)))
    recs = en.run([(ids, P) for P in poses])
    for j, (rec, w) in enumerate(zip(recs, want)):
        got = op_values(en, j * len(ids), len(ids))
        check_values(got, w, c, f"street, drift {ec.DRIFTS[j]}")
        check_rec(rec, got, w, c, f"street, drift {ec.DRIFTS[j]}")
        valid = w["nn"] >= c["min_neighbours"]
        be, bh = ec.bounds(w["nn"][valid], c)
        nv = int(valid.sum())
        for name, b, ref in (("mme", bh, w["h64"][valid]), ("mpv", be, w["pv64"][valid])):
            allowed = 2.0 * float((b + ec.half_ulp32(ref)).sum()) / nv + nv * ec.U * float(np.abs(ref).sum()) / nv
            print(f"street, drift {ec.DRIFTS[j]}: {name} {getattr(rec, name):.9g}, restatement {w['rec'][name]:.9g}, allowed {allowed:.3g}")
            assert abs(getattr(rec, name) - w["rec"][name]) <= allowed
        assert rec.n_valid >= 0.95 * rec.n_points
    assert recs[0].mme < recs[1].mme < recs[2].mme and recs[0].mpv < recs[1].mpv < recs[2].mpv
    ms, cnt = en.timing()
    assert cnt[1] == 3 * n > 65536 and cnt[4] == 3                                               # the sort's read-back is the third
    print("street: ms (keys, sort + cells, rows, moments, sums)", [round(m, 3) for m in ms], "counts", cnt)
    en.close(); kf.close(); ctx.close()


# ---------------------------------------------------------------- more cells than one device scan takes
def test_more_points_than_one_scan_takes(api):
    """The scan of the cell heads goes in chunks of 2^24 entries with a carry between them: 257^3 > 2^24 points on a lattice of 2.2
    cells, each alone in its cell (nn = 1, sparse), and a cluster in the first and in the last cell of the sorted order, whose cell
    numbers a wrong carry would move.  Brute force is not needed: no two lattice points are neighbours by construction"""
    c = ec.cfg()
    G = 257
    cell = float(c["cell"])
    g = (np.arange(G, dtype=np.float64) * 2.2 + 0.5) * cell
    assert G ** 3 > 1 << 24 and (np.diff(np.floor(g.astype(F) / c["cell"])) >= 2).all()
    rng = np.random.default_rng(3)
    first = np.array([g[0]] * 3) + rng.uniform(-0.01, 0.01, (6, 3)); last = np.array([g[-1]] * 3) + rng.uniform(-0.01, 0.01, (9, 3))
    ctx = small_ctx(api)
    kf = ctx.keyframes(G + 1, 64, G ** 3 + 64)
    ident = ec.IDENTITY
    plane = np.empty((G * G, 4), F)
    plane[:, 0] = np.tile(g, G); plane[:, 1] = np.repeat(g, G); plane[:, 3] = 0.0
    for iz in range(G):                                                                          # one frame per lattice plane, z ascending
        plane[:, 2] = g[iz]
        kf.add_points(np.zeros((0, 4), F), plane, ident)
    kf.add_points(ec.pts4(first), ec.pts4(last), ident)
    n = G ** 3 + 15
    en = ctx.entropy(kf, max_points=n)
    rec = en.run([(list(range(G + 1)), None)])[0]
    assert (rec.n_points, rec.n_valid, rec.n_sparse, rec.n_outside, rec.n_pairs) == (n, 17, G ** 3 - 2, 0, G ** 3 - 2 + 49 + 100)
    ms, cnt = en.timing()
    assert cnt[2] == G ** 3 and cnt[3] == rec.n_pairs and cnt[4] == 3
    for iz in (0, 1, 255, 256):                                                                  # 2^24 / 257^2 = 254.01: the chunk ends in plane 254
        h, pv, nn = en.values(iz)
        want = np.ones(G * G, np.uint16)
        if iz == 0:
            want[0] = 7
        if iz == G - 1:
            want[-1] = 10
        assert (nn == want).all() and (np.isnan(h) == (want == 1)).all()
    h, pv, nn = en.values(254)
    assert (nn == 1).all() and np.isnan(h).all()
    # the two clusters against the restatement of each alone (nothing else is within a radius of them)
    hc, pvc, nnc = en.values(G)
    for pts, lattice, sl, where in ((first, g[0], slice(0, 6), (0, 0)), (last, g[-1], slice(6, 15), (G - 1, -1))):
        hl, pvl, nnl = en.values(where[0])
        cloud = np.concatenate([pts, [[lattice] * 3]])
        w = ec.np_op([(ec.pts4(cloud), ec.pts4(np.zeros((0, 3))))], [ident], c)
        check_values((np.r_[hc[sl], hl[where[1]]], np.r_[pvc[sl], pvl[where[1]]], np.r_[nnc[sl], nnl[where[1]]]), w, c, f"cluster of {len(cloud)}")
    print("257^3 lattice: ms (keys, sort + cells, rows, moments, sums)", [round(m, 3) for m in ms])
    en.close(); kf.close(); ctx.close()


# ---------------------------------------------------------------- refusals
def test_refusals_leave_the_last_run_readable(api, crafted_case):
    c, frames, ops, _ = crafted_case
    ids, poses = ops[0][1], ops[0][2]
    sub = [frames[i] for i in ids]
    ctx = small_ctx(api)
    kf = fill(ctx, sub, poses, spare=1600)
    n = n_points(sub)
    for bad in (dict(radius=0.0), dict(radius=-1.0), dict(radius=8.5), dict(radius=float("nan")), dict(radius=float("inf")), dict(radius=1e-20),
                dict(min_neighbours=3), dict(lambda_floor=0.0), dict(lambda_floor=-1e-6), dict(lambda_floor=float("nan")), dict(max_points=0),
                dict(max_points=(1 << 27) + 1)):
        with pytest.raises(api.LightLoamError) as e:
            ctx.entropy(kf, **bad)
        assert e.value.code == -2, bad
    ctx.entropy(kf, radius=8.0, min_neighbours=4, max_points=(1 << 10)).close()
    en = ctx.entropy(kf, max_points=2 * n, **ec.lib_params(c))                                   # room for the three frames twice
    here = [0, 1, 2]
    rec = en.run([(here, None)])
    before = (all_values(en, 3), en.timing())

    def refused(code, call, *a, **k):
        with pytest.raises(api.LightLoamError) as e:
            call(*a, **k)
        assert e.value.code == code, (e.value, code)
        assert (all_values(en, 3), en.timing()) == before

    bad_pose = np.array(poses).copy(); bad_pose[1, 2] = np.inf
    refused(-2, en.run, [])
    refused(-2, en.run, [([0, 1, 1], None)])                                                     # twice in one op
    refused(-2, en.run, [([0, 3], None)]); refused(-2, en.run, [([-1], None)])                   # outside the store
    refused(-2, en.run, [(here, bad_pose)])
    refused(-4, en.run, [([0], None)] * 1025)                                                    # more than 1024 ops
    refused(-4, en.run, [(here, None), (here, None), ([0], None)])                               # one cloud too many for max_points
    refused(-2, en.values, 3); refused(-2, en.values, -1)
    assert kf.add_points(sub[0][0], sub[0][1], poses[0]) == 3
    refused(-4, en.run, [([0, 1, 2, 3], None), (here, None)])
    lib = api.load_library()
    out = api.EntropyRec()
    op = api.EntropyOp(0, None, None)
    assert lib.ll_entropy_run(None, C.addressof(op), 1, C.addressof(out)) == -2 and lib.ll_entropy_run(en.h, None, 1, C.addressof(out)) == -2
    assert lib.ll_entropy_run(en.h, C.addressof(op), 1, None) == -2
    for nf in (2, -1):
        op = api.EntropyOp(nf, None, None)
        assert lib.ll_entropy_run(en.h, C.addressof(op), 1, C.addressof(out)) == -2             # frames NULL with frames to read; n_frames < 0
    assert lib.ll_entropy_values(None, 0, None, None, None) == -2 and lib.ll_entropy_reset(None) == -2 and lib.ll_entropy_timing(None, None, None) == -2
    assert (all_values(en, 3), en.timing()) == before
    # the same id in two ops is no refusal; an op without a frame gives a zero record
    two = en.run([(here, None), ([], None), (here, None)])
    assert bytes(two[0]) == bytes(rec[0]) == bytes(two[2]) and rec_dict(two[1]) == dict.fromkeys(REC_FIELDS, 0)
    assert all_values(en, 6) == before[0] * 2
    # the store is reset: the object means nothing until ll_entropy_reset
    kf.reset()
    for k, (f, P) in enumerate(zip(sub, poses)):
        kf.add_points(f[0], f[1], P)
    for call, a in [(en.run, ([(here, None)],)), (en.values, (0,))]:
        with pytest.raises(api.LightLoamError) as e:
            call(*a)
        assert e.value.code == -7
    en.reset()
    with pytest.raises(api.LightLoamError) as e:
        en.values(0)                                                                             # the last run is forgotten
    assert e.value.code == -2
    assert bytes(en.run([(here, None)])[0]) == bytes(rec[0]) and all_values(en, 3) == before[0]
    en.close(); kf.close(); ctx.close()


# ---------------------------------------------------------------- a store captured by ll_drives
def test_a_captured_store_equals_the_same_clouds_added(api, synth):
    from test_gpu_keyframes import run_lanes
    ctx, dr, kf, _, _ = run_lanes(api, synth, True)
    pts, off = kf.export()
    L = len(kf)
    assert L == 7
    clouds = [(pts[off[2 * i]:off[2 * i + 1]], pts[off[2 * i + 1]:off[2 * i + 2]]) for i in range(L)]
    poses = [kf.info(i)["pose"] for i in range(L)]
    kf2 = fill(ctx, clouds, poses)
    lanes = [[i for i in range(L) if kf.info(i)["lane"] == q] for q in (0, 1)]
    assert all(len(x) >= 3 for x in lanes)
    n = n_points(clouds)
    en, en2 = ctx.entropy(kf, max_points=n, radius=1.0), ctx.entropy(kf2, max_points=n, radius=1.0)
    ops = [(lanes[0], None), (lanes[1], None)]
    r, r2 = en.run(ops), en2.run(ops)
    assert [bytes(x) for x in r] == [bytes(x) for x in r2] and all_values(en, L) == all_values(en2, L)
    assert r[0].n_points + r[1].n_points == n and r[0].n_valid > 0 and r[1].n_valid > 0
    en.close(); en2.close(); kf2.close(); dr.close(); ctx.close()
