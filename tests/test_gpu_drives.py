"""ll_drives: whole drives side by side (registration -> odometry -> mapping per lane).  Every lane, every frame, must equal its
drive run alone through the single-drive chain -- ll_odometry_frames(1, n - 1, pose0, first_frame_index = 1), the world pose of
WorldPose::compose, a fresh CubeMap driven by transformAssociateToMap -> process_slot -> transformUpdate -- bit for bit; the
Python glue below restates lightloam_host.hpp's operation order (Python floats are IEEE doubles, no FMA)."""
import os
import subprocess

import numpy as np
import pytest

from conftest import assert_bit_equal
from test_gpu_mapping_sequences import _assert_same
from test_gpu_sequences import drives, max_points

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = {16: (4096, 32768, 1 << 18), 64: (16384, 131072, 1 << 20)}
NAN7 = np.full(7, np.nan)


def qmul(a, b):                                   # LaserMapping::qmul
    ax, ay, az, aw = a; bx, by, bz, bw = b
    return [aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
            aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz]


def qrot(q, v):                                   # LaserMapping::qrot
    ux, uy, uz, w = q
    uvx = uy * v[2] - uz * v[1]; uvy = uz * v[0] - ux * v[2]; uvz = ux * v[1] - uy * v[0]
    uvx += uvx; uvy += uvy; uvz += uvz
    return [v[0] + w * uvx + (uy * uvz - uz * uvy), v[1] + w * uvy + (uz * uvx - ux * uvz), v[2] + w * uvz + (ux * uvy - uy * uvx)]


def compose(q, t, ql, tl):                        # WorldPose::compose
    ux, uy, uz, w = q
    uv = [uy * tl[2] - uz * tl[1], uz * tl[0] - ux * tl[2], ux * tl[1] - uy * tl[0]]
    uv = [x + x for x in uv]
    t = [t[0] + ((tl[0] + w * uv[0]) + (uy * uv[2] - uz * uv[1])), t[1] + ((tl[1] + w * uv[1]) + (uz * uv[0] - ux * uv[2])),
         t[2] + ((tl[2] + w * uv[2]) + (ux * uv[1] - uy * uv[0]))]
    ax, ay, az, aw = q; bx, by, bz, bw = ql
    q = [aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw,
         aw * bw - ax * bx - ay * by - az * bz]
    return q, t


def single_chain(api, rings, scans, pose0):
    """one drive alone: (odom [n, 7], mapped [n, 7], ran [n]) and its CubeMap (the caller closes ctx, cm)"""
    n = len(scans)
    ctx = api.Context(api.default_params(rings, batch=n, max_points=max(map(len, scans))))
    for k, s in enumerate(scans):
        ctx.upload_scan(k, s)
    ctx.extract(0, n)
    ctx.set_target_from_slot(0)
    rel = ctx.odometry_frames(1, n - 1, pose0=pose0, n_outer=3, first_frame_index=1)
    c, s_, pool = CAP[rings]
    cm = api.CubeMap(ctx, c, s_, pool_points=pool)
    qw, tw = [0.0, 0.0, 0.0, 1.0], [0.0, 0.0, 0.0]
    qm, tm = [0.0, 0.0, 0.0, 1.0], [0.0, 0.0, 0.0]
    odom, mapped, ran = [], [], []
    for k in range(n):
        if k > 0:
            qw, tw = compose(qw, tw, list(rel[k - 1, :4]), list(rel[k - 1, 4:]))
        r = qrot(qm, tw)
        guess = np.array(qmul(qm, qw) + [r[i] + tm[i] for i in range(3)])          # transformAssociateToMap
        p, rn = cm.process_slot(guess, k)
        n2 = qw[0] * qw[0] + qw[1] * qw[1] + qw[2] * qw[2] + qw[3] * qw[3]         # transformUpdate
        inv = [-qw[0] / n2, -qw[1] / n2, -qw[2] / n2, qw[3] / n2]
        qm = qmul(list(p[:4]), inv)
        r = qrot(qm, tw)
        tm = [p[4 + i] - r[i] for i in range(3)]
        odom.append(np.array(qw + tw)); mapped.append(p); ran.append(rn)
    return np.array(odom), np.array(mapped), np.array(ran), ctx, cm


def run_schedule(api, synth, rings, schedule, n_lanes, check_step=None, keep_registered=False):
    """schedule: per lane a list of (first step, drive index, frames); returns per (lane, run) the step outputs, and the Drives"""
    D = max(d for runs in schedule for _, d, _ in runs) + 1
    F = max(f for runs in schedule for _, _, f in runs)
    cfgs, scans, pose0 = drives(synth, rings, D, F)
    ctx = api.Context(api.default_params(rings, batch=2 * n_lanes, max_points=max_points(scans)))
    c, s_, pool = CAP[rings]
    dr = api.Drives(ctx, n_lanes, c, s_, pool_points=pool, keep_registered=keep_registered)
    T = max(s0 + f for runs in schedule for s0, _, f in runs)
    got = {}
    for t in range(T):
        cmd = np.zeros(n_lanes, np.int32); frame = {}
        for q, runs in enumerate(schedule):
            for i, (s0, d, f) in enumerate(runs):
                if s0 <= t < s0 + f:
                    cmd[q] = api.START if t == s0 else api.RUN
                    frame[q] = (i, d, t - s0)
        slots = dr.slots()
        for q, (_, d, k) in frame.items():
            ctx.upload_scan(int(slots[q]), scans[d][k])
        p0 = np.array([pose0[frame[q][1]] if q in frame else NAN7 for q in range(n_lanes)])
        before = (dr.stats()[0], dr.cubemaps.stats()[0])
        odom, mapped, ran = dr.step(cmd, p0)
        after = (dr.stats()[0], dr.cubemaps.stats()[0])
        assert after[0] - before[0] == after[1] - before[1], (t, before, after)   # no host sync beyond the cube-map frame's
        for q in range(n_lanes):
            if q not in frame:
                assert np.isnan(odom[q]).all() and np.isnan(mapped[q]).all() and not ran[q]
                continue
            got.setdefault((q, frame[q][0]), []).append((odom[q], mapped[q], ran[q]))
        if check_step:
            check_step(ctx, dr, slots, frame, mapped)
    return got, dr, ctx, scans, pose0


@pytest.mark.parametrize("rings", [16, 64])
def test_lanes_equal_the_single_drive_chain(api, synth, rings):
    """ragged drives: different lengths, staggered starts, a lane that ends and starts a second drive, a lane idle at first"""
    if rings == 16:
        schedule = [[(0, 0, 8)], [(2, 1, 6), (8, 2, 7)], [(3, 3, 10)], [(0, 4, 14)], [(1, 5, 6)]]
    else:
        schedule = [[(0, 0, 5), (5, 1, 4)], [(1, 2, 6)]]
    got, dr, ctx, scans, pose0 = run_schedule(api, synth, rings, schedule, len(schedule))
    keep = []
    for q, runs in enumerate(schedule):
        for i, (_, d, f) in enumerate(runs):
            odom, mapped, ran, c1, cm = single_chain(api, rings, scans[d][:f], pose0[d])
            rows = got[(q, i)]
            assert len(rows) == f
            for k in range(f):
                assert_bit_equal(rows[k][0], odom[k], f"lane {q} drive {d} frame {k} odom")
                assert_bit_equal(rows[k][1], mapped[k], f"lane {q} drive {d} frame {k} mapped")
                assert bool(rows[k][2]) == bool(ran[k]) == (k > 0), (q, d, k)
            if i == len(runs) - 1:                                                  # the lane's map ends as the last drive's alone
                _assert_same(dr.cubemaps, q, cm, f"lane {q} drive {d}")
            keep.append((c1, cm))
    for c1, cm in keep:
        cm.close(); c1.close()
    syncs, frames = dr.stats()
    assert frames == max(s0 + f for runs in schedule for s0, _, f in runs) and syncs == dr.cubemaps.stats()[0]
    dr.close(); ctx.close()


@pytest.mark.parametrize("rings", [16, 64])
def test_registered_clouds(api, synth, rings):
    """keep_registered: laserCloud of the step's slot moved by the mapped pose (LaserMapping::qrot + t in f64, stored as f32)"""
    seen = []

    def check(ctx, dr, slots, frame, mapped):
        for q in frame:
            cloud = ctx.cloud(int(slots[q]))[0]
            reg = dr.registered(q)
            assert len(reg) == len(cloud) == ctx.scan_info(int(slots[q])).n
            ux, uy, uz, w = mapped[q, :4]
            v = cloud[:, :3].astype(np.float64)
            uvx = uy * v[:, 2] - uz * v[:, 1]; uvy = uz * v[:, 0] - ux * v[:, 2]; uvz = ux * v[:, 1] - uy * v[:, 0]
            uvx = uvx + uvx; uvy = uvy + uvy; uvz = uvz + uvz
            x = ((v[:, 0] + w * uvx) + (uy * uvz - uz * uvy)) + mapped[q, 4]
            y = ((v[:, 1] + w * uvy) + (uz * uvx - ux * uvz)) + mapped[q, 5]
            z = ((v[:, 2] + w * uvz) + (ux * uvy - uy * uvx)) + mapped[q, 6]
            want = np.stack([x.astype(np.float32), y.astype(np.float32), z.astype(np.float32), cloud[:, 3]], axis=1)
            assert_bit_equal(reg, want, f"lane {q} registered")
            seen.append(len(reg))
        for q in range(dr.n_lanes):
            if q not in frame:
                assert len(dr.registered(q)) == 0
    schedule = [[(0, 0, 4)], [(1, 1, 3)], [(0, 2, 2)]]
    _, dr, ctx, _, _ = run_schedule(api, synth, rings, schedule, 3, check_step=check, keep_registered=True)
    assert len(seen) == 9 and min(seen) > 1000
    dr.close(); ctx.close()


def test_argument_errors_enqueue_nothing(api, synth):
    """every LL_ERR_ARG case leaves the stats as they were, and the next valid step gives what a run without the bad calls gives"""
    rings, S = 16, 3
    cfgs, scans, pose0 = drives(synth, rings, S, 4)
    c, s_, pool = CAP[rings]
    plan = [[2, 2, 0], [1, 1, 2], [1, 0, 1], [1, 2, 1]]
    runs = []
    for bad in (False, True):
        ctx = api.Context(api.default_params(rings, batch=2 * S, max_points=max_points(scans)))
        dr = api.Drives(ctx, S, c, s_, pool_points=pool)
        frame = [-1] * S
        out = []
        for k, cmd in enumerate(plan):
            if bad and k == 3:                                                      # lane 1 sat out step 2
                stats = (dr.stats(), dr.cubemaps.stats())
                p_inf = np.array(pose0); p_inf[1, 2] = np.inf
                for c_bad, p_bad in [([1, 3, 1], pose0), ([1, 1, 1], pose0), ([1, 2, 1], p_inf), ([-1, 0, 1], pose0)]:
                    with pytest.raises(api.LightLoamError) as e:
                        dr.step(c_bad, p_bad)
                    assert e.value.code == -2 and "lane" in str(e.value), (c_bad, e.value)
                assert (dr.stats(), dr.cubemaps.stats()) == stats
            sl = dr.slots()
            for q in range(S):
                frame[q] = 0 if cmd[q] == 2 else frame[q] + 1 if cmd[q] == 1 else -1
                if cmd[q]:
                    ctx.upload_scan(int(sl[q]), scans[q][frame[q]])
            out.append(dr.step(cmd, pose0))
        runs.append(out)
        dr.close(); ctx.close()
    for (o1, m1, r1), (o2, m2, r2) in zip(*runs):
        assert_bit_equal(o1, o2, "odom"); assert_bit_equal(m1, m2, "mapped"); assert (r1 == r2).all()


def test_pool_overflow_stops_the_lanes(api, synth):
    """a pool just large enough for a scan: LL_ERR_CAPACITY names a lane; RUN on the lanes that ran is then LL_ERR_ARG, START works"""
    rings, S = 16, 2
    cfgs, scans, pose0 = drives(synth, rings, S, 20)
    probe = api.Context(api.default_params(rings, batch=1, max_points=max_points(scans)))
    c = s_ = 0
    for seq in scans:
        for sc in seq:
            probe.upload_scan(0, sc); probe.extract(0, 1); f = probe.features(0)
            c = max(c, len(f["less_sharp"])); s_ = max(s_, len(f["less_flat"]))
    probe.close()
    ctx = api.Context(api.default_params(rings, batch=2 * S, max_points=max_points(scans)))
    dr = api.Drives(ctx, S, c, s_, pool_points=max(4096, c, s_))
    err = None
    for k in range(20):
        sl = dr.slots()
        for q in range(S):
            ctx.upload_scan(int(sl[q]), scans[q][k])
        try:
            dr.step([api.START if k == 0 else api.RUN] * S, pose0)
        except api.LightLoamError as e:
            err = e
            break
    assert err is not None and err.code == -4 and "lane" in str(err), err
    with pytest.raises(api.LightLoamError) as e:
        dr.step([api.RUN, api.IDLE], pose0)
    assert e.value.code == -2
    sl = dr.slots()
    ctx.upload_scan(int(sl[0]), scans[0][0])
    odom, mapped, ran = dr.step([api.START, api.IDLE], pose0)
    assert (odom[0] == [0, 0, 0, 1, 0, 0, 0]).all() and not ran[0] and np.isnan(mapped[1]).all()
    assert dr.cubemaps.info(0)[1][2] > 0
    dr.close(); ctx.close()


def test_cubemaps_reset_leaves_the_others(api, synth):
    from test_gpu_mapping_sequences import _ctx, _guesses, _nonempty
    S, n = 3, 4
    cfgs, scans, _ = drives(synth, 16, S, n)
    ctx = _ctx(api, 16, scans)
    c, s_, pool = CAP[16]
    many = api.CubeMaps(ctx, S, c, s_, pool_points=pool)
    for k in range(n - 1):
        many.process_slots(_guesses(synth, cfgs, k, [(0.0, 0.0, 0.0)] * S), [k * S + q for q in range(S)])
    snap = {q: (many.info(q), [many.cloud(q, w) for w in range(4)], [(s, i, many.cube(q, s, i)) for s, i in _nonempty(many.cube, q)])
            for q in (0, 2)}
    many.reset(1)
    assert many.info(1) == ((10, 10, 5), (0, 0, 0, 0)) and _nonempty(many.cube, 1) == []
    for q, (info, clouds, cubes) in snap.items():
        assert many.info(q) == info
        for w in range(4):
            assert_bit_equal(many.cloud(q, w), clouds[w], f"sequence {q} cloud {w}")
        assert [(s, i) for s, i, _ in cubes] == _nonempty(many.cube, q)
        for s, i, pts in cubes:
            assert_bit_equal(many.cube(q, s, i), pts, f"sequence {q} cube {s} {i}")
    k = n - 1                                                                       # sequence 1 maps on as a fresh map would
    g = _guesses(synth, cfgs, k, [(0.0, 0.0, 0.0)] * S)
    fresh = api.CubeMap(ctx, c, s_, pool_points=pool)
    poses, ran = many.process_slots(g, [k * S + q for q in range(S)])
    p1, r1 = fresh.process_slot(g[1], k * S + 1)
    assert_bit_equal(poses[1], p1, "after reset"); assert ran[1] == r1 is False
    _assert_same(many, 1, fresh, "sequence 1 after reset")
    fresh.close(); many.close(); ctx.close()


def _build(tmp_path, name):
    from lightloam_amd import build
    lib_dir = os.path.dirname(build.lib_path())
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-pthread", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", name + ".cpp"),
                           "-o", exe, "-L", lib_dir, "-llightloam_hip", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_kitti_drives_tool_matches_the_single_drive_tool(tmp_path):
    """two copies of the KITTI-order HDL-64E drive (one truncated) over 2 lanes at ring capacity 4608: each result file is
    byte for byte what ll_odometry_kitti <dir> <out> 64 1.0 1 4608 writes"""
    import scangen
    many, one = _build(tmp_path, "ll_kitti_drives"), _build(tmp_path, "ll_odometry_kitti")
    scans = [scangen.hdl64_scan(k, order="kitti") for k in range(9)]
    dirs = []
    for i, n in enumerate((9, 5)):
        d = tmp_path / f"drive{i}"; d.mkdir()
        for k in range(n):
            scans[k].astype("<f4").tofile(d / f"{k:06d}.bin")
        dirs.append(str(d))
    res = tmp_path / "res"; res.mkdir()
    out = subprocess.run([many, str(res), "64", "1.0", "4608", "2"] + dirs, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    for i, d in enumerate(dirs):
        ref = tmp_path / f"ref{i}.txt"
        o = subprocess.run([one, d, str(ref), "64", "1.0", "1", "4608"], capture_output=True, text=True, timeout=600)
        assert o.returncode == 0, o.stdout + o.stderr
        assert (res / f"{i}.txt").read_bytes() == ref.read_bytes(), i
