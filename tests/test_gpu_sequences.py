"""ll_odometry_sequences: laserOdometry's frame loop for many sequences side by side, against the single-sequence loop
(ll_odometry_frames, bit for bit), the oracle, and its own contract (vote gate per sequence, ragged lengths, ring continuation,
argument checks, the C++ host mirror)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PERIOD = 0.1


def drives(synth, rings, n_seq, n_frames):
    """n_seq different synthetic drives: cfgs, scans[q][k], and a warm start near each one's first motion"""
    cfgs = [synth.default_cfg(rings, seed=11 + 7 * q, speed=7.0 + 1.5 * (q % 4), yaw_rate=0.04 * ((q % 3) - 1)) for q in range(n_seq)]
    scans = [[synth.scan(c, k) for k in range(n_frames)] for c in cfgs]
    pose0 = np.array([[0, 0, 0, 1.0, c.speed * PERIOD, 0.0, 0.0] for c in cfgs])
    return cfgs, scans, pose0


def max_points(scans):
    return max(len(s) for seq in scans for s in seq)


def lockstep_ctx(api, rings, scans, ring_rows, frames_of_row=None):
    """a context whose ring rows hold the frames (row r = frame r unless frames_of_row says otherwise), all extracted"""
    S = len(scans)
    ctx = api.Context(api.default_params(rings, batch=S * ring_rows, max_points=max_points(scans)))
    L = api.SeqLayout(0, S, ring_rows)
    rows = frames_of_row if frames_of_row is not None else {r: r for r in range(min(ring_rows, len(scans[0])))}
    for r, k in rows.items():
        for q in range(S):
            ctx.upload_scan(api.sequence_slot(L, r, q), scans[q][k])
    ctx.extract(0, S * (max(rows) + 1))
    return ctx, L


def alone(api, rings, seq, pose0, first_frame_index=1, n=None):
    """one sequence through set_target_from_slot + ll_odometry_frames: poses and (n_edge, n_plane, n_plane_selected) per frame"""
    n = len(seq) if n is None else n
    ctx = api.Context(api.default_params(rings, batch=n, max_points=max(len(s) for s in seq[:n])))
    for k in range(n):
        ctx.upload_scan(k, seq[k])
    ctx.extract(0, n)
    ctx.set_target_from_slot(0)
    rel = ctx.odometry_frames(1, n - 1, pose0=pose0, n_outer=3, first_frame_index=first_frame_index)
    pi = [ctx.pair_info(k) for k in range(1, n)]
    ctx.close()
    return rel, [(p.n_edge, p.n_plane, p.n_plane_selected) for p in pi]


def pair_counts(ctx, L, rows, q):
    out = []
    for r in rows:
        p = ctx.pair_info(L.base + (r % L.ring_rows) * L.n_seq + q)
        out.append((p.n_edge, p.n_plane, p.n_plane_selected))
    return out


@pytest.mark.parametrize("rings,n_seq,n_frames", [(16, 5, 14), (64, 3, 9)])
def test_bit_identical_to_the_single_sequence_loop(api, synth, rings, n_seq, n_frames):
    _, scans, pose0 = drives(synth, rings, n_seq, n_frames)
    ctx, L = lockstep_ctx(api, rings, scans, n_frames)
    rel = ctx.odometry_sequences(n_seq, n_frames, 1, n_frames - 1, pose0=pose0)
    counts = [pair_counts(ctx, L, range(1, n_frames), q) for q in range(n_seq)]
    ctx.close()
    assert rel.shape == (n_frames - 1, n_seq, 7)
    for q in range(n_seq):
        ref, ref_counts = alone(api, rings, scans[q], pose0[q])
        assert np.array_equal(rel[:, q], ref), (q, np.abs(rel[:, q] - ref).max())
        assert counts[q] == ref_counts, q


def test_two_sequences_match_the_oracle(api, orc, synth):
    rings, n_seq, n_frames = 16, 5, 14
    _, scans, pose0 = drives(synth, rings, n_seq, n_frames)
    ctx, _ = lockstep_ctx(api, rings, scans, n_frames)
    rel = ctx.odometry_sequences(n_seq, n_frames, 1, n_frames - 1, pose0=pose0)
    ctx.close()
    P = orc.params(rings)
    for q in (0, 3):
        ex = [orc.extract(s, P) for s in scans[q]]
        orc.set_nn_mode(1)
        qq, t = pose0[q, :4].copy(), pose0[q, 4:].copy(); rel_o = []
        for k in range(1, n_frames):
            qq, t = orc.odometry_frame(qq, t, ex[k], ex[k - 1], vote=k > 5)
            rel_o.append(np.concatenate([qq, t]))
        orc.set_nn_mode(0)
        d = np.abs(rel[:, q] - np.array(rel_o)).max(axis=1)
        assert d.max() < 1e-6, (q, d)


def test_vote_gate_per_sequence(api, synth):
    rings, n_frames = 16, 9
    _, scans, pose0 = drives(synth, rings, 2, n_frames)
    ctx, _ = lockstep_ctx(api, rings, scans, n_frames)
    rel = ctx.odometry_sequences(2, n_frames, 1, n_frames - 1, frame_index0=[1, 4], pose0=pose0)
    ctx.close()
    for q, f0 in ((0, 1), (1, 4)):
        ref, _ = alone(api, rings, scans[q], pose0[q], first_frame_index=f0)
        assert np.array_equal(rel[:, q], ref), q
    # the gate does change the result: sequence 1 votes from its third row on, sequence 0 only from its sixth
    ref_late, _ = alone(api, rings, scans[1], pose0[1], first_frame_index=1)
    assert not np.array_equal(rel[:, 1], ref_late)


def slot_state(ctx, slot):
    pi = ctx.pair_info(slot)
    return (ctx.pose(slot).tobytes(), (pi.n_edge, pi.n_plane, pi.n_plane_selected),
            b"".join(a.tobytes() for a in ctx.edge_corr(slot)), b"".join(a.tobytes() for a in ctx.plane_corr(slot)))


def test_ragged_lengths_leave_the_other_slots_alone(api, synth):
    rings, S, n_frames = 16, 4, 9
    n = n_frames - 1
    _, scans, pose0 = drives(synth, rings, S, n_frames)
    ctx, L = lockstep_ctx(api, rings, scans, n_frames)
    ctx.odometry_sequences(S, n_frames, 1, n, pose0=pose0)                  # every slot holds a solved frame now
    pose_b = pose0.copy(); pose_b[:, 4] *= 0.8                              # a different warm start: rewritten slots would differ
    seq_rows = [n, n - 3, 0, n]
    not_run = [(r, q) for q in range(S) for r in range(1, n_frames) if r - 1 >= seq_rows[q]]
    before = {rq: slot_state(ctx, api.sequence_slot(L, *rq)) for rq in not_run}
    rel = ctx.odometry_sequences(S, n_frames, 1, n, seq_rows=seq_rows, pose0=pose_b)
    after = {rq: slot_state(ctx, api.sequence_slot(L, *rq)) for rq in not_run}
    full = ctx.odometry_sequences(S, n_frames, 1, n, pose0=pose_b)
    ctx.close()
    assert before == after
    for q in range(S):
        k = seq_rows[q]
        assert np.isnan(rel[k:, q]).all(), q
        assert np.array_equal(rel[:k, q], full[:k, q]), q
    assert not np.isnan(full).any()


def test_ring_continuation_equals_one_long_ring(api, synth):
    rings, S, n_frames = 16, 2, 12
    _, scans, pose0 = drives(synth, rings, S, n_frames)
    ctx, _ = lockstep_ctx(api, rings, scans, 13)
    one = ctx.odometry_sequences(S, 13, 1, n_frames - 1, pose0=pose0)
    ctx.close()
    ctx, L = lockstep_ctx(api, rings, scans, 7)                             # frames 0..6 in rows 0..6
    a = ctx.odometry_sequences(S, 7, 1, 6, pose0=pose0)
    for k in range(7, n_frames):                                            # frames 7..11 into the rows 0..4 that are done
        for q in range(S):
            ctx.upload_scan(api.sequence_slot(L, k, q), scans[q][k])
    ctx.extract(api.sequence_slot(L, 7, 0), (n_frames - 7) * S)
    b = ctx.odometry_sequences(S, 7, 7, n_frames - 7, frame_index0=7,     # row 7 is frame 7: it votes
                               pose0=None)                                  # warm start from the poses on the device
    ctx.close()
    assert np.array_equal(np.concatenate([a, b]), one)


def test_argument_checks(api):
    ctx = api.Context(api.default_params(16, batch=12, max_points=4096))
    lib = ctx.lib
    good = dict(L=(0, 3, 4), row0=1, n_rows=3, seq_rows=None, n_outer=3, iters=4)

    def call(**kw):
        a = dict(good, **kw)
        L = api.SeqLayout(*a["L"])
        rows = None if a["seq_rows"] is None else np.asarray(a["seq_rows"], np.int32)
        o = api.LmOptions(); lib.ll_lm_default_options(C.byref(o)); o.max_num_iterations = a["iters"]
        return lib.ll_odometry_sequences(ctx.h, C.byref(L), a["row0"], a["n_rows"],
                                         None if rows is None else rows.ctypes.data_as(C.c_void_p), None, None, a["n_outer"], C.byref(o), None)

    bad = [dict(L=(0, 0, 4)), dict(L=(0, 3, 1)), dict(L=(-1, 3, 4)), dict(L=(1, 3, 4)), dict(L=(0, 4, 4)),
           dict(n_rows=0), dict(n_rows=4), dict(seq_rows=[3, -1, 0]), dict(seq_rows=[4, 0, 0]),
           dict(n_outer=0), dict(n_outer=17), dict(iters=-1), dict(iters=65)]
    for b in bad:
        assert call(**b) == -2, b
    assert lib.ll_odometry_sequences(ctx.h, None, 1, 1, None, None, None, 3, None, None) == -2
    ctx.synchronize()
    ctx.close()


def test_native_host_mirror(tmp_path, api, synth):
    from lightloam_amd import build
    rings, S, n_frames = 16, 2, 8
    _, scans, pose0 = drives(synth, rings, S, n_frames)
    for q in range(S):
        for k in range(n_frames):
            scans[q][k].astype("<f4").tofile(tmp_path / f"s{q}_f{k}.bin")
    pose0.astype("<f8").tofile(tmp_path / "pose0.bin")
    lib_dir = os.path.dirname(build.lib_path())
    exe = str(tmp_path / "sequences_host")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "native", "sequences_host.cpp"), "-o", exe,
                           "-L", lib_dir, "-llightloam_hip", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe, str(tmp_path), str(rings), str(S), str(n_frames)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    got = np.array([[float(x) for x in line.split()] for line in out.stdout.strip().splitlines()]).reshape(n_frames - 1, S, 7)
    ctx, _ = lockstep_ctx(api, rings, scans, n_frames)
    rel = ctx.odometry_sequences(S, n_frames, 1, n_frames - 1, pose0=pose0)
    ctx.close()
    assert np.array_equal(got, rel)
