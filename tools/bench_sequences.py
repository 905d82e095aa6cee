"""Frames/s of laserOdometry's frame loop for S sequences in lock-step (ll_odometry_sequences) against the same sequences run one
after another through ll_odometry_frames.

    python tools/bench_sequences.py [--rings 64 16] [--seqs 1,8,32,128,256,1024] [--rows 32] [--out profiles/r07_sequences.json]

Every sequence is one of --drives synthetic drives (synth.default_cfg with its own seed / speed / yaw_rate): sequence q replays drive
q % drives, so the chip sees S full frame loops while the host generates only a few drives.  Rows of the lock-step run sit in a ring
sized to the device memory; a drive longer than the ring streams through it -- the next frames are extracted into finished rows
between calls (not timed) and the call continues from the poses on the device (host_pose0 = NULL).  Times are device-synchronised
(ll_synchronize before and after every timed call) after one warm-up call; the one-after-another rate comes from the distinct
drives, each timed alone.  Prints one JSON line and writes it to --out.
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

PERIOD = 0.1


def make_drives(rings, n_drives, n_frames):
    cfgs = [synth.default_cfg(rings, seed=101 + 13 * d, speed=6.0 + 1.0 * (d % 5), yaw_rate=0.05 * ((d % 3) - 1)) for d in range(n_drives)]
    scans = [[synth.scan(c, k) for k in range(n_frames)] for c in cfgs]
    pose0 = np.array([[0, 0, 0, 1.0, c.speed * PERIOD, 0.0, 0.0] for c in cfgs])
    return scans, pose0


def free_bytes():
    """hipMemGetInfo of the current device (the HIP runtime the library already loaded)"""
    try:
        hip = C.CDLL("libamdhip64.so")
    except OSError:
        hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
    free, total = C.c_size_t(0), C.c_size_t(0)
    if hip.hipMemGetInfo(C.byref(free), C.byref(total)) != 0:
        raise RuntimeError("hipMemGetInfo failed")
    return free.value


def slot_bytes(rings, max_points):
    """device memory of one slot, measured on a small context"""
    f0 = free_bytes()
    ctx = api.Context(api.default_params(rings, batch=256, max_points=max_points))
    ctx.synchronize()
    f1 = free_bytes()
    ctx.close()
    return max(1, (f0 - f1) // 256)


def timed(ctx, fn):
    ctx.synchronize()
    t0 = time.perf_counter()
    fn()
    ctx.synchronize()
    return time.perf_counter() - t0


def sequential_rate(rings, scans, pose0, rows, reps):
    """each distinct drive alone through ll_odometry_frames: frames/s (median over reps of the total)"""
    mp = max(len(s) for d in scans for s in d)
    ctx = api.Context(api.default_params(rings, batch=rows + 1, max_points=mp))
    lib = ctx.lib
    totals = []
    for rep in range(reps + 1):                       # rep 0: warm-up
        tot = 0.0
        for d in range(len(scans)):
            for k in range(rows + 1):
                ctx.upload_scan(k, scans[d][k])
            ctx.extract(0, rows + 1)
            ctx.set_target_from_slot(0)
            p0 = np.ascontiguousarray(pose0[d])
            tot += timed(ctx, lambda: ctx._ck(lib.ll_odometry_frames(ctx.h, 1, rows, p0.ctypes.data_as(C.c_void_p), 3, 1, None, None)))
        if rep:
            totals.append(tot)
    ctx.close()
    return len(scans) * rows / float(np.median(totals))


def lockstep_rate(rings, scans, pose0, S, rows, reps, mem_frac):
    n_drives = len(scans)
    mp = max(len(s) for d in scans for s in d)
    per_slot = slot_bytes(rings, mp)
    fit_rows = int(mem_frac * free_bytes() // (per_slot * S))
    ring_rows = min(rows + 1, fit_rows)
    if ring_rows < 2:
        return None, {"skipped": f"{S} sequences x 2 rows do not fit"}
    ctx = api.Context(api.default_params(rings, batch=S * ring_rows, max_points=mp))
    lib = ctx.lib
    L = api.SeqLayout(0, S, ring_rows)
    p0 = np.ascontiguousarray(pose0[np.arange(S) % n_drives])

    def load(frames):
        for k in frames:
            for q in range(S):
                ctx.upload_scan(api.sequence_slot(L, k, q), scans[q % n_drives][k])
        rr = [k % ring_rows for k in frames]           # consecutive ring rows, wrapping at most once: one extract per piece
        cut = next((i for i in range(1, len(rr)) if rr[i] != rr[i - 1] + 1), len(rr))
        for piece in (rr[:cut], rr[cut:]):
            if piece:
                ctx.extract(piece[0] * S, len(piece) * S)

    def call(row0, n, pose):
        ptr = None if pose is None else pose.ctypes.data_as(C.c_void_p)
        ctx._ck(lib.ll_odometry_sequences(ctx.h, C.byref(L), row0, n, None, None, ptr, 3, None, None))

    load(list(range(ring_rows)))
    n1 = min(rows, ring_rows - 1)
    call(1, n1, p0)                                   # warm-up
    passes = []
    for rep in range(reps if ring_rows == rows + 1 else 1):
        if rep or ring_rows == rows + 1:
            t = timed(ctx, lambda: call(1, n1, p0))
        else:
            t = 0.0
            row = 1
            while row <= rows:
                n = min(ring_rows - 1, rows - row + 1)
                if row > 1:
                    load(list(range(row, row + n)))   # the next frames into the rows that are done (not timed)
                t += timed(ctx, lambda: call(row, n, p0 if row == 1 else None))
                row += n
        passes.append(t)
    ctx.close()
    t = float(np.median(passes))
    return S * rows / t, {"ring_rows": ring_rows, "row_ms": 1e3 * t / rows, "passes": len(passes)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rings", type=int, nargs="+", default=[64, 16])
    ap.add_argument("--seqs", default="1,8,32,128,256,1024")
    ap.add_argument("--rows", type=int, default=32)
    ap.add_argument("--drives", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--mem-frac", type=float, default=0.6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_sequences.json"))
    a = ap.parse_args()
    seqs = [int(x) for x in a.seqs.split(",")]
    res = {"tool": "tools/bench_sequences.py", "rows": a.rows, "n_outer": 3, "drives": a.drives, "curves": {}}
    for rings in a.rings:
        scans, pose0 = make_drives(rings, a.drives, a.rows + 1)
        seq_fps = sequential_rate(rings, scans, pose0, a.rows, a.reps)
        curve = {"one_after_another_frames_per_s": seq_fps, "lockstep": {}}
        for S in seqs:
            fps, info = lockstep_rate(rings, scans, pose0, S, a.rows, a.reps, a.mem_frac)
            info["frames_per_s"] = fps
            info["x_one_after_another"] = None if fps is None else fps / seq_fps
            curve["lockstep"][str(S)] = info
            print(f"# rings {rings} S {S}: {info}", file=sys.stderr, flush=True)
        res["curves"][str(rings)] = curve
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
