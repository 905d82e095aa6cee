"""The information record (ll_pose_info) of localisation, alignment and localising drive lanes.  No expected value comes from the code
under test: H, g and rows are Map.normal_equations at the final pose on a private imported copy of the map (localisation: the way
test_gpu_localize.py checks fit.cost) or the CPU oracle's map_normal_equations on the oracle's own blocks (alignment: the way
test_gpu_map_align.py checks cost); sigma2 is exact host arithmetic on the fit record; eig is numpy.linalg.eigvalsh of the record's H.
H and g agree within REL = 1e-9 of max|H| (the sums run in another order; g is a sum that cancels at the optimum, so its error is
measured against the terms' scale, not against itself).  Asking for the record changes no bit of poses, ran and fit, and a record is
the same bits alone and in a batch."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_drives import CAP as DRIVE_CAP, compose, qmul, qrot
from test_gpu_drives_localize import IDENT, RINGS, S as LANES, Base, fit_tuple, make_drives, step
from test_gpu_localize import FAR, REL, World, _one_frame
from test_gpu_map_align import clouds, maps_object, pair
from test_gpu_map_merge import make_map, small_ctx

pytestmark = pytest.mark.gpu


def raw(rec):
    return bytes(memoryview(rec))


def is_zero(rec):
    return not any(raw(rec))


def as_arrays(rec):
    return np.array(rec.H[:]).reshape(6, 6), np.array(rec.g[:]), np.array(rec.eig[:])


def check_record(rec, fit, H_ref, g_ref, what):
    """H, g against the reference within REL of max|H|; rows, sigma2, eig, flags from their definitions"""
    H, g, eig = as_arrays(rec)
    scale = np.abs(H_ref).max()
    eH, eg = np.abs(H - H_ref).max() / scale, np.abs(g - g_ref).max() / scale
    rows = 3 * fit.n_edge + fit.n_plane
    want_eig = np.linalg.eigvalsh(H)
    e_eig = np.abs(eig - want_eig).max() / eig[5]
    print(f"{what}: rows {rec.rows}, |dH| / max|H| {eH:.3g}, |dg| / max|H| {eg:.3g}, eig {eig[0]:.6g} .. {eig[5]:.6g} (error / eig[5] {e_eig:.3g}), "
          f"sigma2 {rec.sigma2!r}")
    assert rec.rows == rows and rows > 6, what
    assert eH <= REL and eg <= REL, (what, eH, eg)
    assert (H == H.T).all(), what
    assert rec.sigma2 == (fit.sq_edge + fit.sq_plane) / (rows - 6), what
    assert (np.diff(eig) >= 0.0).all() and e_eig <= 1e-9, (what, eig, want_eig)
    assert rec.flags == 0, what


# ------------------------------------------------------------------------------------------------ localisation
@pytest.fixture(scope="module")
def world(api, synth):
    w = World(api, synth, 16)
    yield w
    w.close()


def test_localize_slots_info_against_the_single_map(world):
    w = world
    S, n, many = w.S, w.n, w.many
    ones = [None] + [w.private() for _ in range(1, S)]
    for k in (0, 3):
        frames, guess, slots = w.call(k)
        sy0 = many.stats()[0]
        poses, ran, fit, info = many.localize_slots(guess, slots, [0] * S, info=True)
        assert many.stats()[0] - sy0 <= 3                            # headers, prepare, poses + fit + info: no synchronisation added
        bare, ran_bare, fit_bare = many.localize_slots(guess, slots, [0] * S)
        assert bare.tobytes() == poses.tobytes() and (ran == ran_bare).all() and raw(fit) == raw(fit_bare)
        only, _, none, info_only = many.localize_slots(guess, slots, [0] * S, fit=False, info=True)
        assert none is None and only.tobytes() == poses.tobytes() and raw(info_only) == raw(info)
        assert not ran[0] and is_zero(info[0])                      # a sequence that sits out
        for q in range(1, S):
            p1, r1 = _one_frame(ones[q], w.feats[frames[q]], guess[q])
            assert r1 and ran[q] and (p1 == poses[q]).all()
            m = ones[q].map()
            m.associate(p1)
            assert (fit[q].n_edge, fit[q].n_plane) == tuple(m.counts())
            H_ref, g_ref, _ = m.normal_equations(p1)
            check_record(info[q], fit[q], H_ref, g_ref, f"call {k} sequence {q}")
        # a record alone, and at another position of the batch (sequence 1 reads sequence 2's slot): the same bits
        alone = many.localize_slots(guess, [-1, -1, slots[2]] + [-1] * (S - 3), [0] * S, info=True)
        assert raw(alone[3][2]) == raw(info[2]) and alone[0][2].tobytes() == poses[2].tobytes()
        assert all(is_zero(alone[3][q]) for q in range(S) if q != 2)
        g2 = guess.copy(); g2[1] = guess[2]
        moved = many.localize_slots(g2, [-1, slots[2], -1] + [-1] * (S - 3), [0] * S, info=True)
        assert raw(moved[3][1]) == raw(info[2]) and moved[0][1].tobytes() == poses[2].tobytes()
    w.assert_map0_untouched()


def test_no_optimisation_no_record(world, api):
    w = world
    S, n, many = w.S, w.n, w.many
    guess = np.tile(w.guess(1, FAR), (S, 1))                        # off the map: the gate stays shut
    poses, ran, fit, info = many.localize_slots(guess, [-1, n + 1] + [-1] * (S - 2), [0] * S, info=True)
    assert not ran.any() and all(is_zero(r) for r in info)
    # the slot with the empty scan is refused (LL_ERR_STATE, as without info); the caller's records are zeros all the same
    recs = (api.PoseInfo * S)()
    for r in recs:
        r.rows = 7; r.sigma2 = 1.0
    g = np.ascontiguousarray(np.tile(w.guess(1), (S, 1)))
    slots = np.array([-1, S * n] + [-1] * (S - 2), np.int32); map_of = np.zeros(S, np.int32)
    rc = many.lib.ll_cubemaps_localize_slots_info(many.h, slots.ctypes.data, map_of.ctypes.data, g.ctypes.data, None, None, C.addressof(recs))
    assert rc == -7 and all(is_zero(r) for r in recs)
    w.assert_map0_untouched()


# ------------------------------------------------------------------------------------------------ alignment
def oracle_neq(orc, T, stk, mp):
    b = orc.map_associate(T[:4], T[4:], stk[0], mp[0], stk[1], mp[1])
    H, g, _ = orc.map_normal_equations(T[:4], T[4:], stk[0], b[0], b[1], b[2], stk[1], b[3], b[4], b[5])
    return H, g, len(b[0]), len(b[3])


def test_align_info_against_the_oracle(api, orc):
    """test_sizes_that_are_multiples_of_nothing's maps: the whole src gives more blocks than one chunk of 1024, the picked ones fewer"""
    centre = (6.0, -4.0, 1.0)
    dst, src, T0 = pair(6, centre)
    rng = np.random.default_rng(60)
    c_all, s_all = src[0][src[0][:, 3] == 0], src[0][src[0][:, 3] == 1]
    pick = lambda a, k: a[np.sort(rng.choice(len(a), k, replace=False))]
    maps = [dst, src, make_map(pick(c_all, 63), pick(s_all, 65)), make_map(pick(c_all, 257), pick(s_all, 300))]
    ctx = small_ctx(api)
    many = maps_object(api, ctx, maps)
    ops = [(0, q, T0) for q in range(1, len(maps))]
    mp = clouds(many, 0)
    for n_outer in (0, 2):
        sy0 = many.stats()[0]
        T, ran, fit, info = many.align(ops, n_outer=n_outer, info=True)
        assert many.stats()[0] - sy0 == 1                           # still ONE synchronisation
        Tb, ranb, fitb = many.align(ops, n_outer=n_outer)
        assert Tb.tobytes() == T.tobytes() and (ran == ranb).all() and [fit_tuple(f) for f in fit] == [fit_tuple(f) for f in fitb]
        To, _, none, info_only = many.align(ops, n_outer=n_outer, fit=False, info=True)
        assert none is None and To.tobytes() == T.tobytes() and raw(info_only) == raw(info)
        if n_outer == 0:
            assert T.tobytes() == np.tile(T0, (len(ops), 1)).tobytes()   # the information at T0
        blocks = []
        for i, (d, s, _) in enumerate(ops):
            H_ref, g_ref, ne, npl = oracle_neq(orc, T[i], clouds(many, s), mp)
            assert (fit[i].n_edge, fit[i].n_plane) == (ne, npl) and ran[i]
            blocks.append(ne + npl)
            check_record(info[i], fit[i], H_ref, g_ref, f"n_outer {n_outer} op {i}")
        assert blocks[0] > 1024 and all(0 < b < 1024 for b in blocks[1:]), blocks
        for i, op in enumerate(ops):                                # alone, and in the reversed batch: the same bits
            Ta, _, _, ia = many.align([op], n_outer=n_outer, info=True)
            assert raw(ia[0]) == raw(info[i]) and Ta.tobytes() == T[i:i + 1].tobytes(), (n_outer, i)
        back = many.align(ops[::-1], n_outer=n_outer, info=True)[3]
        assert [raw(r) for r in back][:len(ops)] == [raw(r) for r in info][:len(ops)][::-1]
    few = make_map(c_all[:10], s_all)                               # a dst whose gate is shut: an all-zero record
    many2 = maps_object(api, ctx, [few, src, dst])
    T, ran, fit, info = many2.align([(0, 1, T0), (2, 1, T0)], n_outer=0, info=True)
    assert ran.tolist() == [False, True] and is_zero(info[0]) and info[1].rows > 6
    many2.close(); many.close(); ctx.close()


# ------------------------------------------------------------------------------------------------ drive lanes
def chain_info(api, scans, pose0, start, map_pts, layout):
    """test_gpu_drives_localize.localize_chain with the information records: odometry, transformAssociateToMap, localize_slots(info=True)
    on a one-sequence CubeMaps holding the map, transformUpdate -> (mapped poses, fit tuples, info records as bytes)"""
    n = len(scans)
    ctx = api.Context(api.default_params(RINGS, batch=n, max_points=max(map(len, scans))))
    for k, s in enumerate(scans):
        ctx.upload_scan(k, s)
    ctx.extract(0, n)
    ctx.set_target_from_slot(0)
    rel = ctx.odometry_frames(1, n - 1, pose0=pose0, n_outer=3, first_frame_index=1)
    c, s_, pool = DRIVE_CAP[RINGS]
    cms = api.CubeMaps(ctx, 1, c, s_, pool_points=pool)
    cms.import_maps(map_pts, [0, len(map_pts)], [layout])
    qw, tw = [0.0, 0.0, 0.0, 1.0], [0.0, 0.0, 0.0]
    qm, tm = [float(x) for x in start[:4]], [float(x) for x in start[4:]]
    mapped, fits, infos = [], [], []
    for k in range(n):
        if k > 0:
            qw, tw = compose(qw, tw, list(rel[k - 1, :4]), list(rel[k - 1, 4:]))
        r = qrot(qm, tw)
        guess = np.array(qmul(qm, qw) + [r[i] + tm[i] for i in range(3)])          # transformAssociateToMap
        p, rn, fit, info = cms.localize_slots(guess[None, :], [k], info=True)
        p = p[0]
        n2 = qw[0] * qw[0] + qw[1] * qw[1] + qw[2] * qw[2] + qw[3] * qw[3]         # transformUpdate
        inv = [-qw[0] / n2, -qw[1] / n2, -qw[2] / n2, qw[3] / n2]
        qm = qmul(list(p[:4]), inv)
        r = qrot(qm, tw)
        tm = [p[4 + i] - r[i] for i in range(3)]
        mapped.append(p); fits.append(fit_tuple(fit[0])); infos.append(raw(info[0]))
    cms.close(); ctx.close()
    return mapped, fits, infos


def test_drives_info(api, synth):
    base = Base(api, synth)
    scans, pose0 = base.scans, base.pose0
    start = np.tile(IDENT, (LANES, 1)); start[1] = base.mapped0[1]
    n_loc = 3

    def run(mode):
        """lane 1 localises frames 1 .. n_loc of drive A in lane 0's restored map, lane 2 maps drive B; mode: None never hears of the
        records, True asks for them, False asks and switches them off again"""
        ctx, dr = make_drives(api, scans)
        dr.restore(base.blob, [0])
        dr.set_localize([-1, 0, -1], start)
        if mode is not None:
            dr.set_info(True)
            if not mode:
                dr.set_info(False)
        started, rows = set(), []
        for t in range(n_loc):
            sy0 = dr.stats()[0]
            odom, mapped, ran = step(api, ctx, dr, {1: (0, 1 + t), 2: (1, t)}, scans, pose0, started)
            rows.append((odom.tobytes(), mapped.tobytes(), ran.tobytes(), [fit_tuple(f) for f in dr.fit()], [raw(r) for r in dr.info()], dr.stats()[0] - sy0))
        dr.step(np.zeros(LANES, np.int32))
        assert all(is_zero(r) for r in dr.info())                   # nobody ran: zeros
        dr.close(); ctx.close()
        return rows

    plain, on, off = run(None), run(True), run(False)
    mapped, fits, infos = chain_info(api, scans[0][1:1 + n_loc], pose0[0], start[1], base.map0[0], base.map0[1])
    zero = bytes(len(infos[0]))
    for t in range(n_loc):
        assert plain[t][:4] == on[t][:4] == off[t][:4], t            # the step's outputs do not know about the records
        assert plain[t][5] == on[t][5] == off[t][5], t               # nor do its synchronisations
        assert plain[t][4] == off[t][4] == [zero] * LANES, t
        assert on[t][4][0] == zero and on[t][4][2] == zero, t        # the idle lane and the mapping lane
        assert on[t][3][1] == fits[t] and on[t][4][1] == infos[t], t # the localising lane: the single chain's record, bit for bit
        assert infos[t] != zero
    base.close()
