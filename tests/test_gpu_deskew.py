"""TransformToEnd on the device (ll_deskew.hip, ll_set_deskew, ll_deskew_slots): the stage alone against the numpy restatement of
tests/deskewcases.py (every f32 coordinate equal or adjacent, >= 99.9 % the same bits, intensities exact), the rebuilt search grids
against the oracle's association, the frame loop against the oracle's loop fed with restated targets, and the loops against
themselves bit for bit: loop = its parts, sequences = each alone, drive lanes = the single-drive chain, resume = uninterrupted,
off = never switched on.  16-ring synthetic scans throughout."""
import numpy as np
import pytest

import deskewcases as dc
from conftest import assert_bit_equal
from test_gpu_drives import CAP, NAN7, compose, qmul, qrot
from test_gpu_sequences import drives, max_points

pytestmark = pytest.mark.gpu
RINGS = 16
POSE0 = np.array([0, 0, 0, 1.0, 0.9, 0.0, 0.0])
NAMES = ("sharp", "less_sharp", "flat", "less_flat")


def make_ctx(api, scans, batch=None, extract=True, distortion=1, **kw):
    batch = len(scans) if batch is None else batch
    ctx = api.Context(api.default_params(RINGS, batch=batch, max_points=max(map(len, scans)) + 7, distortion=distortion, **kw))
    for k, s in enumerate(scans):
        ctx.upload_scan(k, s)
    if extract:
        ctx.extract(0, len(scans))
    return ctx


def feature_bytes(ctx, slot):
    f = ctx.features(slot)
    return tuple(f[n].tobytes() for n in NAMES)


def raises(api, code, fn, *a, **kw):
    with pytest.raises(api.LightLoamError) as e:
        fn(*a, **kw)
    assert e.value.code == code, e.value
    return str(e.value)


@pytest.fixture(scope="module")
def scans9(synth):
    cfg = synth.default_cfg(RINGS)
    return [synth.scan(cfg, k) for k in range(9)]


# ------------------------------------------------------------------ the stage alone
def test_stage_alone_on_the_crafted_clouds(api):
    """uploaded (contiguous) clouds in two slots, a pose per slot, every crafted pose; host poses and resident poses give the same
    bytes.  One less-flat cloud is longer than one pass of the launch over a contiguous cloud (16 rows x 9 blocks x 256 points)."""
    pts = dc.points()
    order = lambda a: a[np.argsort(np.trunc(a[:, 3]), kind="stable")]
    lf_small = order(np.concatenate([dc.points(6), dc.random_points(700, 8)]))       # three 256-point blocks, the last partial
    lf_big = order(dc.random_points(16 * 9 * 256 + 300, 12))
    sharp, flat = pts[::2], pts[1::3]
    ctx = api.Context(api.default_params(RINGS, batch=2, max_points=len(lf_big) + 5, distortion=1))
    poses = dc.poses()
    shares = []
    for i in range(0, len(poses), 2):
        (na, qa, ta), (nb, qb, tb) = poses[i], poses[i + 1]
        p2 = np.array([np.concatenate([qa, ta]), np.concatenate([qb, tb])])
        lfs = (lf_small, lf_big if i == 0 else lf_small[::-1][:500][::-1])
        got = {}
        for how in ("host", "resident"):
            for slot in (0, 1):
                ctx.upload_features(slot, sharp, pts, flat, lfs[slot])
            if how == "host":
                ctx.deskew_slots(0, 2, p2, 1)
            else:
                ctx.set_pose_guess(0, 2, p2)
                ctx.deskew_slots(0, 2, None, 1)
            got[how] = [ctx.features(slot) for slot in (0, 1)]
        for slot, (name, q, t) in enumerate(((na, qa, ta), (nb, qb, tb))):
            f = got["host"][slot]
            assert feature_bytes_of(f) == feature_bytes_of(got["resident"][slot]), name
            assert f["sharp"].tobytes() == sharp.tobytes() and f["flat"].tobytes() == flat.tobytes(), name
            shares.append(dc.check_close(f["less_sharp"], dc.deskew(pts, q, t), f"{name}: less sharp"))
            shares.append(dc.check_close(f["less_flat"], dc.deskew(lfs[slot], q, t), f"{name}: less flat"))
    print("bit-identical shares:", min(s for s, _ in shares), "worst distance:", max(w for _, w in shares))
    ctx.close()


def feature_bytes_of(f):
    return tuple(f[n].tobytes() for n in NAMES)


@pytest.fixture(scope="module")
def extracted(api, orc, scans9):
    """three extracted scans and an empty one, deskewed in mode 2 with a pose per slot; what the slots held before, and after"""
    scans = scans9[:3] + [np.zeros((0, 4), np.float32)]
    ctx = make_ctx(api, scans)
    q = np.array([0.02, -0.035, 0.06, 1.0]); q /= np.linalg.norm(q)
    poses = np.array([np.concatenate([q, [0.8, 0.05, -0.03]]), np.concatenate([-q, [0.7, -0.02, 0.01]]),
                      np.concatenate([[0.0, 0.0, 0.0, 1.0], [0.9, 0.0, 0.0]]), np.concatenate([q, [0.5, 0.5, 0.5]])])
    snap = lambda: [dict(feat=ctx.features(k), cloud=ctx.cloud(k), labels=ctx.labels(k), info=ctx.scan_info(k)) for k in range(4)]
    before = snap()
    ctx.deskew_slots(0, 4, poses, 2)
    after = snap()
    yield dict(ctx=ctx, poses=poses, before=before, after=after)
    ctx.close()


def test_stage_alone_on_extracted_scans(extracted):
    shares = []
    for k in range(3):
        b, a, p = extracted["before"][k], extracted["after"][k], extracted["poses"][k]
        assert b["info"].status == 0 and b["info"].n > 1000 and b["info"].n_less_flat > 256
        for name in ("less_sharp", "less_flat"):                                       # less flat: the ring-strided rows of an extracted slot
            shares.append(dc.check_close(a["feat"][name], dc.deskew(b["feat"][name], p[:4], p[4:]), f"slot {k} {name}"))
        shares.append(dc.check_close(a["cloud"][0], dc.deskew(b["cloud"][0], p[:4], p[4:]), f"slot {k} laserCloud"))
        for name in ("sharp", "flat"):
            assert a["feat"][name].tobytes() == b["feat"][name].tobytes(), (k, name)
        for f in ("status", "n", "n_sharp", "n_less_sharp", "n_flat", "n_less_flat", "max_ring"):
            assert getattr(a["info"], f) == getattr(b["info"], f), (k, f)
        assert (a["cloud"][1] == b["cloud"][1]).all() and (a["cloud"][2] == b["cloud"][2]).all()      # ring offsets
        assert a["labels"].tobytes() == b["labels"].tobytes()
        assert (np.abs(a["feat"]["less_flat"][:, :3] - b["feat"]["less_flat"][:, :3]).max(axis=1) > 1e-3).mean() > 0.5   # it did move them
    print("bit-identical shares:", min(s for s, _ in shares), "worst distance:", max(w for _, w in shares))


def test_a_refused_scan_is_left_alone(extracted):
    b, a = extracted["before"][3], extracted["after"][3]
    assert b["info"].status != 0 and a["info"].status == b["info"].status
    assert feature_bytes_of(a["feat"]) == feature_bytes_of(b["feat"])
    for f in ("n", "n_sharp", "n_less_sharp", "n_flat", "n_less_flat"):
        assert getattr(a["info"], f) == getattr(b["info"], f), f


def test_grids_are_rebuilt(extracted, orc):
    """the association of slot 1 against the carry copied from deskewed slot 0, and of slot 2 against slot 1's own rebuilt grids,
    names exactly the points the oracle's association names in the downloaded deskewed clouds"""
    ctx = extracted["ctx"]
    q = np.array([0.01, -0.02, 0.03, 1.0]); q /= np.linalg.norm(q)
    t = np.array([0.85, 0.03, -0.02])
    pose = np.concatenate([q, t])
    feat = [extracted["after"][k]["feat"] for k in range(3)]
    orc.set_distortion(1)
    try:
        ctx.set_target_from_slot(0)
        for first, count, pairs in ((1, 1, [(1, 0)]), (1, 2, [(1, 0), (2, 1)])):
            ctx.associate(first, count, pose); ctx.vote(first, count, True); ctx.synchronize()    # the vote compacts the correspondences
            for k, tgt in pairs:
                es, ea, eb = orc.associate_corner(q, t, feat[k]["sharp"], feat[tgt]["less_sharp"])
                ps, pa, pb, pc = orc.associate_plane(q, t, feat[k]["flat"], feat[tgt]["less_flat"])
                assert len(es) > 10 and len(ps) > 10
                for got, want, nm in zip(ctx.edge_corr(k) + ctx.plane_corr(k), (es, ea, eb, ps, pa, pb, pc),
                                         ("e_src", "e_a", "e_b", "p_src", "p_a", "p_b", "p_c")):
                    assert len(got) == len(want) and (got == want).all(), f"slot {k} against {tgt}: {nm}"
    finally:
        orc.set_distortion(0)


# ------------------------------------------------------------------ the frame loop
@pytest.fixture(scope="module")
def loop9(api, scans9):
    """the 9-frame loop with distortion = 1: never switched on, switched off, mode 1 -- poses and every slot's feature clouds"""
    out = {}
    for name, mode in (("never", None), ("off", 0), ("on", 1)):
        ctx = make_ctx(api, scans9)
        if mode is not None:
            ctx.set_deskew(mode)
        ctx.set_target_from_slot(0)
        rel = ctx.odometry_frames(1, 8, pose0=POSE0, n_outer=3, first_frame_index=1)
        out[name] = dict(rel=rel, feat=[feature_bytes(ctx, k) for k in range(9)])
        if name == "on":
            out["ctx"] = ctx
        else:
            ctx.close()
    yield out
    out["ctx"].close()


def test_frame_loop_against_the_oracle(loop9, orc, scans9):
    """the oracle's loop, its target of frame k being frame k - 1's less-sharp / less-flat clouds after the numpy restatement at the
    oracle's own pose of frame k - 1 (frame 0, which nobody solved, as it is)"""
    P = orc.params(RINGS)
    ex = [orc.extract(s, P) for s in scans9]
    orc.set_nn_mode(1); orc.set_distortion(1)
    try:
        q = POSE0[:4].copy(); t = POSE0[4:].copy(); rel_o = []
        prev = ex[0]
        for k in range(1, 9):
            q, t = orc.odometry_frame(q, t, ex[k], prev, vote=k > 5)
            rel_o.append(np.concatenate([q, t]))
            prev = dict(less_sharp=dc.deskew(ex[k]["less_sharp"], q, t), less_flat=dc.deskew(ex[k]["less_flat"], q, t))
    finally:
        orc.set_nn_mode(0); orc.set_distortion(0)
    rel_o = np.array(rel_o)
    err = np.abs(loop9["on"]["rel"] - rel_o).max(axis=1)
    print("per-frame pose error against the oracle:", err)
    assert err.max() < 1e-6, err
    assert np.abs(loop9["on"]["rel"] - loop9["off"]["rel"]).max() > 1e-4


def test_off_is_off(loop9):
    assert loop9["never"]["rel"].tobytes() == loop9["off"]["rel"].tobytes()
    assert loop9["never"]["feat"] == loop9["off"]["feat"]
    assert loop9["on"]["feat"][0] == loop9["off"]["feat"][0]                          # the first target: whatever the caller set
    for k in range(1, 9):
        assert loop9["on"]["feat"][k][0] == loop9["off"]["feat"][k][0] and loop9["on"]["feat"][k][2] == loop9["off"]["feat"][k][2]
        assert loop9["on"]["feat"][k][1] != loop9["off"]["feat"][k][1] and loop9["on"]["feat"][k][3] != loop9["off"]["feat"][k][3]


def test_loop_equals_its_parts(api, loop9, scans9):
    """mode 1 over 8 frames = per frame { the carry from the slot before, one mode-0 ll_odometry_frames(k, 1) warm-started with the
    previous pose, ll_deskew_slots(k, 1, NULL, 1) }"""
    ctx = make_ctx(api, scans9)
    pose = POSE0
    rel = []
    for k in range(1, 9):
        ctx.set_target_from_slot(k - 1)
        pose = ctx.odometry_frames(k, 1, pose0=pose, n_outer=3, first_frame_index=k)[0]
        ctx.deskew_slots(k, 1, None, 1)
        rel.append(pose)
    assert np.array(rel).tobytes() == loop9["on"]["rel"].tobytes()
    assert [feature_bytes(ctx, k) for k in range(9)] == loop9["on"]["feat"]
    ctx.close()


def test_a_slot_is_deskewed_once(api, loop9, scans9):
    ctx = loop9["ctx"]
    poses = [ctx.pose(k).tobytes() for k in range(9)]
    msg = raises(api, -7, ctx.odometry_frames, 1, 8, pose0=POSE0)                     # every slot it would solve is deskewed already
    assert "slot 1" in msg
    msg = raises(api, -7, ctx.odometry_frames, 0, 4, pose0=POSE0)                     # slot 0 is not, slot 1 is
    assert "slot 1" in msg
    msg = raises(api, -7, ctx.deskew_slots, 3, 2)
    assert "slot 3" in msg
    ctx.synchronize()
    assert [ctx.pose(k).tobytes() for k in range(9)] == poses                         # nothing was enqueued
    assert [feature_bytes(ctx, k) for k in range(9)] == loop9["on"]["feat"]
    ctx.deskew_slots(0, 1)                                                            # slot 0 was never deskewed: accepted once
    raises(api, -7, ctx.deskew_slots, 0, 1)
    ctx.extract(3, 1)                                                                 # re-extracted from its resident raw scan: accepted again
    assert feature_bytes(ctx, 3) == loop9["off"]["feat"][3]
    ctx.deskew_slots(3, 1)
    assert feature_bytes(ctx, 3) == loop9["on"]["feat"][3]                            # same clouds, same pose, same bytes
    raises(api, -7, ctx.deskew_slots, 3, 1)
    ctx.upload_features(4, *[np.frombuffer(b, np.float32).reshape(-1, 4) for b in loop9["off"]["feat"][4]])
    ctx.deskew_slots(4, 1)                                                            # an upload clears the mark as well


def test_argument_and_state_errors(api, scans9):
    ctx = make_ctx(api, scans9[:2], distortion=0)
    assert "distortion" in raises(api, -7, ctx.set_deskew, 1)
    raises(api, -7, ctx.deskew_slots, 0, 1)
    ctx.close()
    ctx = make_ctx(api, scans9[:2])
    for mode in (-1, 3):
        raises(api, -2, ctx.set_deskew, mode)
    for mode in (0, 3):
        raises(api, -2, ctx.deskew_slots, 0, 1, None, mode)
    raises(api, -2, ctx.deskew_slots, 1, 2)
    ctx.set_deskew(2); ctx.set_deskew(0)
    ctx.close()


# ------------------------------------------------------------------ sequences
def test_sequences_equal_each_alone(api, synth):
    S, lengths = 3, (3, 5, 8)
    n_frames = max(lengths)
    _, scans, pose0 = drives(synth, RINGS, S, n_frames)
    ctx = api.Context(api.default_params(RINGS, batch=S * n_frames, max_points=max_points(scans), distortion=1))
    L = api.SeqLayout(0, S, n_frames)
    for r in range(n_frames):
        for q in range(S):
            ctx.upload_scan(api.sequence_slot(L, r, q), scans[q][r])
    ctx.extract(0, S * n_frames)
    ctx.set_deskew(1)
    seq_rows = [n - 1 for n in lengths]
    not_run = [(r, q) for q in range(S) for r in range(1, n_frames) if r - 1 >= seq_rows[q]]
    state = lambda: {rq: (feature_bytes(ctx, api.sequence_slot(L, *rq)), ctx.pose(api.sequence_slot(L, *rq)).tobytes()) for rq in not_run}
    before = state()
    rel = ctx.odometry_sequences(S, n_frames, 1, n_frames - 1, seq_rows=seq_rows, pose0=pose0)
    assert state() == before and len(not_run) == 5 + 3                               # a sequence that sits out keeps its slots
    feats = {q: [feature_bytes(ctx, api.sequence_slot(L, r, q)) for r in range(lengths[q])] for q in range(S)}
    assert "is already deskewed" in raises(api, -7, ctx.odometry_sequences, S, n_frames, 1, 2, pose0=pose0)
    ctx.close()
    for q in range(S):
        one = make_ctx(api, scans[q][:lengths[q]])
        one.set_deskew(1)
        one.set_target_from_slot(0)
        ref = one.odometry_frames(1, lengths[q] - 1, pose0=pose0[q], n_outer=3, first_frame_index=1)
        assert rel[:seq_rows[q], q].tobytes() == ref.tobytes(), q
        assert np.isnan(rel[seq_rows[q]:, q]).all()
        assert feats[q] == [feature_bytes(one, k) for k in range(lengths[q])], q
        one.close()


# ------------------------------------------------------------------ drives
def single_chain(api, scans, pose0, mode):
    """test_gpu_drives.single_chain on a distortion = 1 context with the deskew mode set: (odom, mapped, registered clouds, map export)"""
    n = len(scans)
    ctx = make_ctx(api, scans)
    ctx.set_deskew(mode)
    ctx.set_target_from_slot(0)
    rel = ctx.odometry_frames(1, n - 1, pose0=pose0, n_outer=3, first_frame_index=1)
    c, s_, pool = CAP[RINGS]
    cm = api.CubeMap(ctx, c, s_, pool_points=pool)
    qw, tw = [0.0, 0.0, 0.0, 1.0], [0.0, 0.0, 0.0]
    qm, tm = [0.0, 0.0, 0.0, 1.0], [0.0, 0.0, 0.0]
    odom, mapped, reg = [], [], []
    for k in range(n):
        if k > 0:
            qw, tw = compose(qw, tw, list(rel[k - 1, :4]), list(rel[k - 1, 4:]))
        r = qrot(qm, tw)
        guess = np.array(qmul(qm, qw) + [r[i] + tm[i] for i in range(3)])              # transformAssociateToMap
        p, _ = cm.process_slot(guess, k)
        n2 = qw[0] * qw[0] + qw[1] * qw[1] + qw[2] * qw[2] + qw[3] * qw[3]             # transformUpdate
        inv = [-qw[0] / n2, -qw[1] / n2, -qw[2] / n2, qw[3] / n2]
        qm = qmul(list(p[:4]), inv)
        r = qrot(qm, tw)
        tm = [p[4 + i] - r[i] for i in range(3)]
        odom.append(np.array(qw + tw)); mapped.append(p)
        cloud = ctx.cloud(k)[0]                                                        # pointAssociateToMap of the (deskewed) laserCloud
        ux, uy, uz, w = p[:4]
        v = cloud[:, :3].astype(np.float64)
        uvx = uy * v[:, 2] - uz * v[:, 1]; uvy = uz * v[:, 0] - ux * v[:, 2]; uvz = ux * v[:, 1] - uy * v[:, 0]
        uvx = uvx + uvx; uvy = uvy + uvy; uvz = uvz + uvz
        x = ((v[:, 0] + w * uvx) + (uy * uvz - uz * uvy)) + p[4]
        y = ((v[:, 1] + w * uvy) + (uz * uvx - ux * uvz)) + p[5]
        z = ((v[:, 2] + w * uvz) + (ux * uvy - uy * uvx)) + p[6]
        reg.append(np.stack([x.astype(np.float32), y.astype(np.float32), z.astype(np.float32), cloud[:, 3]], axis=1))
    exported = cm.export(1)
    cm.close(); ctx.close()
    return np.array(odom), np.array(mapped), reg, exported


START_AT = (0, 1)                     # lane 1 starts a step later: its START frame shares a row with lane 0's first solved frame
N_FRAMES = 8


def drive_steps(api, dr, ctx, scans, pose0, t0, t1, rows, syncs):
    for t in range(t0, t1):
        cmd = np.zeros(2, np.int32); frame = {}
        for q in range(2):
            k = t - START_AT[q]
            if 0 <= k < N_FRAMES:
                cmd[q] = api.START if k == 0 else api.RUN; frame[q] = k
        slots = dr.slots()
        for q, k in frame.items():
            ctx.upload_scan(int(slots[q]), scans[q][k])
        s0 = dr.stats()[0]
        odom, mapped, ran = dr.step(cmd, np.array([pose0[q] if q in frame else NAN7 for q in range(2)]))
        syncs.append(dr.stats()[0] - s0)
        for q in frame:
            rows.setdefault(q, []).append((odom[q].copy(), mapped[q].copy(), dr.registered(q)))


def new_drives(api, scans, mode):
    ctx = api.Context(api.default_params(RINGS, batch=4, max_points=max_points(scans), distortion=1))
    if mode is not None:
        ctx.set_deskew(mode)
    c, s_, pool = CAP[RINGS]
    return ctx, api.Drives(ctx, 2, c, s_, pool_points=pool, keep_registered=True)


def test_drive_lanes_equal_the_single_drive_chain_and_resume(api, synth):
    _, scans, pose0 = drives(synth, RINGS, 2, N_FRAMES)
    T = N_FRAMES + max(START_AT)
    # the uninterrupted run, mode 2, with a checkpoint after step 4 (lane 0 at frame 4, lane 1 at frame 3)
    ctx, dr = new_drives(api, scans, 2)
    rows, syncs = {}, []
    drive_steps(api, dr, ctx, scans, pose0, 0, 5, rows, syncs)
    blob = dr.save([1, 1])
    drive_steps(api, dr, ctx, scans, pose0, 5, T, rows, syncs)
    exported = [dr.cubemaps.export(np.array([1 if q == lane else -1 for q in range(2)], np.int32))[0] for lane in range(2)]
    dr.close(); ctx.close()
    for q in range(2):
        odom, mapped, reg, exp1 = single_chain(api, scans[q], pose0[q], 2)
        assert len(rows[q]) == N_FRAMES
        for k in range(N_FRAMES):
            assert_bit_equal(rows[q][k][0], odom[k], f"lane {q} frame {k} odom")
            assert_bit_equal(rows[q][k][1], mapped[k], f"lane {q} frame {k} mapped")
            assert rows[q][k][0].tobytes() == odom[k].tobytes() and rows[q][k][1].tobytes() == mapped[k].tobytes(), (q, k)
            assert rows[q][k][2].tobytes() == reg[k].tobytes() and len(reg[k]) > 1000, (q, k)
        assert exported[q].tobytes() == np.ascontiguousarray(exp1).tobytes() and len(exported[q]) > 1000, q
    # the same schedule with the switch off: as many host synchronisations per step
    ctx, dr = new_drives(api, scans, 0)
    rows0, syncs0 = {}, []
    drive_steps(api, dr, ctx, scans, pose0, 0, T, rows0, syncs0)
    dr.close(); ctx.close()
    assert syncs == syncs0, (syncs, syncs0)
    assert rows0[0][3][1].tobytes() != rows[0][3][1].tobytes()                         # and it is another computation
    # resume: a fresh context and Drives with the mode on
    ctx, dr = new_drives(api, scans, 2)
    dr.restore(blob, [0, 1])
    cur = dr.slots()
    for q in range(2):                                                                 # the restored slots (the other row) count as deskewed
        assert "already deskewed" in raises(api, -7, ctx.deskew_slots, int(cur[q]) + 2 if cur[q] < 2 else int(cur[q]) - 2, 1)
    rows2, syncs2 = {}, []
    drive_steps(api, dr, ctx, scans, pose0, 5, T, rows2, syncs2)
    for q in range(2):
        want = rows[q][5 - START_AT[q]:]
        assert len(rows2[q]) == len(want) >= 3
        for i, (g, w) in enumerate(zip(rows2[q], want)):
            for j in range(3):
                assert np.ascontiguousarray(g[j]).tobytes() == np.ascontiguousarray(w[j]).tobytes(), (q, i, j)
    assert syncs2 == syncs[5:]
    dr.close(); ctx.close()
