"""End-to-end frames/s of whole drives side by side (ll_drives: upload + extract + odometry + mapping per step) against the same
drives run one after another through the single-drive chain, with the stages of a step timed on their own in the same run.

    python tools/bench_drives.py [--rings 64] [--lanes 1,8,32,128] [--frames 8] [--out profiles/r08_drives.json]

Lane q replays synthetic drive q % drives (the drives of tools/bench_mapping_sequences.py).  Step 0 starts every lane (frame 0:
no odometry, an empty map); steps 1 .. frames-1 are timed, each from the first upload to the end of ll_drives_step, device-
synchronised before and after.  In the same run, on a second context holding the same frames in the same slots, three stages are
timed per frame the same way:
  extract     ll_extract_batch over the row's S slots (uploads not included)
  odometry    ll_odometry_sequences, one row, every lane
  mapping     ll_cubemaps_process_slots, fed the poses the drives produced for that frame
and glue_ratio is (step - uploads) / (extract + odometry + mapping).  One after another: every distinct drive through upload,
extract, ll_odometry_frames of one frame, WorldPose and ll_cubemap_process_slot per frame.  Host synchronisations per step come
from ll_drives_stats, the cube maps' own from ll_cubemaps_stats.  Prints one JSON line and writes it to --out.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lightloam_amd  # noqa: E402,F401
from lightloam_amd import api, synth  # noqa: E402

CAP = {16: (4096, 32768), 64: (16384, 131072)}
PERIOD = 0.1


def make_drives(rings, n_drives, n_frames):
    cfgs = [synth.default_cfg(rings, seed=101 + 13 * d, speed=6.0 + 1.0 * (d % 5), yaw_rate=0.05 * ((d % 3) - 1)) for d in range(n_drives)]
    scans = [[synth.scan(c, k) for k in range(n_frames)] for c in cfgs]
    pose0 = np.array([[0, 0, 0, 1.0, c.speed * PERIOD, 0.0, 0.0] for c in cfgs])
    return scans, pose0


def timed(ctx, fn):
    ctx.synchronize()
    t0 = time.perf_counter()
    out = fn()
    ctx.synchronize()
    return time.perf_counter() - t0, out


def qmul(a, b):                                   # LaserMapping::qmul
    ax, ay, az, aw = a; bx, by, bz, bw = b
    return [aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw,
            aw * bw - ax * bx - ay * by - az * bz]


def qrot(q, v):                                   # LaserMapping::qrot
    ux, uy, uz, w = q
    uvx = uy * v[2] - uz * v[1]; uvy = uz * v[0] - ux * v[2]; uvz = ux * v[1] - uy * v[0]
    uvx += uvx; uvy += uvy; uvz += uvz
    return [v[0] + w * uvx + (uy * uvz - uz * uvy), v[1] + w * uvy + (uz * uvx - ux * uvz), v[2] + w * uvz + (ux * uvy - uy * uvx)]


def compose(q, t, ql, tl):                        # lightloam::WorldPose::compose
    ux, uy, uz, w = q
    uv = [uy * tl[2] - uz * tl[1], uz * tl[0] - ux * tl[2], ux * tl[1] - uy * tl[0]]
    uv = [x + x for x in uv]
    t = [t[0] + ((tl[0] + w * uv[0]) + (uy * uv[2] - uz * uv[1])), t[1] + ((tl[1] + w * uv[1]) + (uz * uv[0] - ux * uv[2])),
         t[2] + ((tl[2] + w * uv[2]) + (ux * uv[1] - uy * uv[0]))]
    return qmul(q, ql), t


def one_after_another(rings, scans, pose0, pool):
    D, F = len(scans), len(scans[0])
    ctx = api.Context(api.default_params(rings, batch=2, max_points=max(len(s) for d in scans for s in d)))
    tot = 0.0
    for d in range(D):
        cm = api.CubeMap(ctx, *CAP[rings], pool_points=pool)
        qw, tw, qm, tm = [0.0, 0.0, 0.0, 1.0], [0.0] * 3, [0.0, 0.0, 0.0, 1.0], [0.0] * 3
        for k in range(F):
            slot = k % 2
            ctx.synchronize()
            t0 = time.perf_counter()
            ctx.upload_scan(slot, scans[d][k])
            ctx.extract(slot, 1)
            if k > 0:                              # target: frame k - 1 as the carry; warm start: its solved pose
                rel = ctx.odometry_frames(slot, 1, pose0=pose0[d] if k == 1 else ctx.pose(1 - slot), first_frame_index=k)[0]
                qw, tw = compose(qw, tw, list(rel[:4]), list(rel[4:]))
            ctx.set_target_from_slot(slot)
            r = qrot(qm, tw)
            p, _ = cm.process_slot(np.array(qmul(qm, qw) + [r[i] + tm[i] for i in range(3)]), slot)
            n2 = qw[0] * qw[0] + qw[1] * qw[1] + qw[2] * qw[2] + qw[3] * qw[3]
            qm = qmul(list(p[:4]), [-qw[0] / n2, -qw[1] / n2, -qw[2] / n2, qw[3] / n2]); r = qrot(qm, tw)
            tm = [p[4 + i] - r[i] for i in range(3)]
            ctx.synchronize()
            if k:
                tot += time.perf_counter() - t0
        cm.close()
    ctx.close()
    return D * (F - 1) / tot


def side_by_side(rings, scans, pose0, S, pool):
    D, F = len(scans), len(scans[0])
    mp = max(len(s) for d in scans for s in d)
    ctx = api.Context(api.default_params(rings, batch=2 * S, max_points=mp))
    dr = api.Drives(ctx, S, *CAP[rings], pool_points=pool)
    p0 = pose0[np.arange(S) % D]
    ctx2 = api.Context(api.default_params(rings, batch=2 * S, max_points=mp))      # the stages on their own
    cms = api.CubeMaps(ctx2, S, *CAP[rings], pool_points=pool)
    L = api.SeqLayout(0, S, 2)
    t_step = t_up = t_ext = t_odo = t_map = 0.0
    s0 = c0 = 0
    for k in range(F):
        slots = dr.slots()
        ctx.synchronize()
        t0 = time.perf_counter()
        for q in range(S):
            ctx.upload_scan(int(slots[q]), scans[q % D][k])
        t1 = time.perf_counter()
        odom, mapped, ran = dr.step(np.full(S, api.RUN if k else api.START, np.int32), p0)
        ctx.synchronize()
        t2 = time.perf_counter()
        for q in range(S):
            ctx2.upload_scan(int(slots[q]), scans[q % D][k])
        first = int(slots[0]); row = first // S
        te, _ = timed(ctx2, lambda: ctx2.extract(first, S))
        to = 0.0
        if k == 0:
            ctx2.set_pose_guess(first, S, p0)                                         # the warm start of frame 1
        else:
            fidx = np.full(S, k, np.int32)
            to, _ = timed(ctx2, lambda: ctx2._ck(ctx2.lib.ll_odometry_sequences(ctx2.h, C.byref(L), row, 1, None, fidx.ctypes.data_as(C.c_void_p),
                                                                                None, 3, None, None)))
        tm, _ = timed(ctx2, lambda: cms.process_slots(mapped, [int(s) for s in slots]))
        if k == 0:
            s0, c0 = dr.stats()[0], dr.cubemaps.stats()[0]
        else:
            t_step += t2 - t0; t_up += t1 - t0; t_ext += te; t_odo += to; t_map += tm
    n = F - 1
    info = {"step_ms": 1e3 * t_step / n, "upload_ms": 1e3 * t_up / n, "extract_ms": 1e3 * t_ext / n, "odometry_ms": 1e3 * t_odo / n,
            "mapping_ms": 1e3 * t_map / n, "glue_ratio": (t_step - t_up) / (t_ext + t_odo + t_map),
            "host_syncs_per_step": (dr.stats()[0] - s0) / n, "cubemaps_host_syncs_per_step": (dr.cubemaps.stats()[0] - c0) / n}
    cms.close(); ctx2.close(); dr.close(); ctx.close()
    return S * n / t_step, info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rings", type=int, default=64)
    ap.add_argument("--lanes", default="1,8,32,128")
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--drives", type=int, default=8)
    ap.add_argument("--pool", type=int, default=1 << 19)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_drives.json"))
    a = ap.parse_args()
    scans, pose0 = make_drives(a.rings, a.drives, a.frames)
    seq_fps = one_after_another(a.rings, scans, pose0, a.pool)
    print(f"# one after another: {seq_fps:.1f} frames/s", file=sys.stderr, flush=True)
    res = {"tool": "tools/bench_drives.py", "rings": a.rings, "frames": a.frames, "timed_steps": a.frames - 1, "drives": a.drives,
           "pool_points": a.pool, "one_after_another_frames_per_s": seq_fps, "lanes": {}}
    for S in [int(x) for x in a.lanes.split(",")]:
        fps, info = side_by_side(a.rings, scans, pose0, S, a.pool)
        info["frames_per_s"] = fps
        info["x_one_after_another"] = fps / seq_fps
        res["lanes"][str(S)] = info
        print(f"# S {S}: {info}", file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
