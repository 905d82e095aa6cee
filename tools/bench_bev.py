"""ll_bev: what a match costs per stage, and how close the score kernel comes to a derived LDS bound.

    python tools/bench_bev.py [--rings 64] [--ops 1,16,64] [--yaws 13] [--repeats 5] [--out profiles/bev.json]

Every figure is the median over `--repeats` FRESH processes, with the minimum and maximum beside it; device times are between HIP events
(ll_bev_timing: prepare, score, peak).  The keyframes are tools/bench_keyframes.py's: `--source-frames` frames of one synthetic
`rings`-ring drive, mapped and captured, fill a store round-robin, frame k under a pose 0.5 m further along a circle of 150 m radius.
Default parameters (cell 0.5, half 128, shift_half 16: 1024 shifts), `--yaws` yaws at 1 degree.
  single   every op matches ONE stored frame against ONE other (both under the identity, as after a place match); 1 / 16 / 64 ops per call
  triple   every op matches three consecutive frames against the next three under their stored poses (max_points raised to 2^23)
One untimed call, one timed, per shape and batch size.  Per stage the time and a rate:
  prepare  listed points per second
  score    point-hypothesis lookups per second: the sum over ops of (the op's query list entries) x n_yaws x (2 shift_half)^2 -- every
           staged entry is looked up by every thread of every (op, yaw) workgroup -- and that rate against the BOUND below
  peak     hypotheses per second
THE BOUND IS DERIVED, NOT MEASURED: 32 byte-lookups per clock per CU x 256 CUs x 2.4 GHz = 1.97 x 10^13 lookups/s.  It assumes that a
one-byte LDS read (ds_read_u8) costs what ds_read_b32 costs in the microarchitecture table (2 LDS cycles per 64-lane instruction), that
the broadcast reads of the staged entries are free, and that the chip holds its maximum clock.  Nobody has measured the first of these
on this part; the ratio says how far the kernel is from that assumption, not from a measured ceiling.  No time here is a pass criterion.
Prints one JSON line and writes it to --out.
"""
import argparse
import json
import math
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_keyframes import CAP, circle_pose, summary  # noqa: E402

BOUND = 32 * 256 * 2.4e9
IDENT = [0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]


def worker(a):
    sys.path.insert(0, a.root)
    import numpy as np
    import lightloam_amd  # noqa: F401
    from lightloam_amd import api
    from bench_mapping_sequences import make_drives
    from bench_visibility import make_store
    scans, guesses = make_drives(a.rings, 1, a.source_frames)
    ctx = api.Context(api.default_params(a.rings, batch=1, max_points=max(len(s) for s in scans[0])))
    clouds = make_store(a, api, ctx, scans, guesses)
    batches = [int(x) for x in a.ops.split(",")]
    K = 2 * max(batches) + 8
    kf = ctx.keyframes(K, sum(len(clouds[k % a.source_frames][0]) for k in range(K)) + 1, sum(len(clouds[k % a.source_frames][1]) for k in range(K)) + 1)
    for k in range(K):
        kf.add_points(*clouds[k % a.source_frames], circle_pose(k))
    n_of = [sum(len(clouds[k % a.source_frames][w]) for w in (0, 1)) for k in range(K)]
    step = math.radians(1.0)
    out = {}
    for shape in ("single", "triple"):
        bev = ctx.bev(kf, max_ops=max(batches), max_yaws=max(16, a.yaws), max_points=(1 << 21) if shape == "single" else (1 << 23))
        S2 = (2 * bev.params.shift_half) ** 2
        for n in batches:
            if shape == "single":
                ops = [([2 * i], [IDENT], [2 * i + 1], [IDENT], -6.0 * step, step, a.yaws) for i in range(n)]
            else:
                ops = [([i, i + 1, i + 2], None, [i + 3, i + 4, i + 5], None, -6.0 * step, step, a.yaws) for i in range(n)]
            bev.match(ops); ctx.synchronize()                                           # untimed
            t0 = time.perf_counter()
            res = bev.match(ops)
            wall = 1e3 * (time.perf_counter() - t0)
            ms, cnt = bev.timing()
            listed = sum(n_of[k] for o in ops for k in o[0] + o[2])
            lookups = sum(sum(n_of[k] for k in o[2]) for o in ops) * a.yaws * S2
            assert cnt == (n, listed, n * a.yaws * S2), (cnt, n, listed)
            out[f"{shape}_{n}"] = dict(ops=n, listed_points=listed, lookups=lookups, hypotheses=cnt[2], prepare_ms=ms[0], score_ms=ms[1], peak_ms=ms[2],
                                       device_ms=float(sum(ms)), wall_ms=wall, best_score=int(res[0].score), second=int(res[0].second), n_query=int(res[0].n_query))
        bev.close()
    kf.close(); ctx.close()
    print("RESULT " + json.dumps(out), flush=True)


def run_worker(a, rep):
    env = dict(os.environ); env.pop("LIGHTLOAM_HIP_LIB", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "1", "--root", ROOT, "--rings", str(a.rings), "--ops", a.ops, "--yaws", str(a.yaws),
           "--source-frames", str(a.source_frames)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    if p.returncode != 0 or not lines:
        sys.exit(f"worker failed (repeat {rep}): {p.stdout[-2000:]}{p.stderr[-2000:]}")
    print(f"# repeat {rep}: {lines[-1][7:]}", file=sys.stderr, flush=True)
    return json.loads(lines[-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rings", type=int, default=64)
    ap.add_argument("--ops", default="1,16,64")
    ap.add_argument("--yaws", type=int, default=13)
    ap.add_argument("--source-frames", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bev.json"))
    ap.add_argument("--worker", default="", help=argparse.SUPPRESS)
    ap.add_argument("--root", default=ROOT, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    got = {}
    for rep in range(a.repeats):
        for name, r in run_worker(a, rep).items():
            for key, val in r.items():
                got.setdefault(name, {}).setdefault(key, []).append(val)
    res = {"tool": "tools/bench_bev.py", "rings": a.rings, "source_frames": a.source_frames, "yaws": a.yaws, "repeats": a.repeats,
           "what": "medians over fresh processes; device ms between HIP events; default parameters (cell 0.5, half 128, shift_half 16)",
           "bound_lookups_per_s": BOUND,
           "bound_is": "DERIVED, not measured: 32 byte-lookups per clock per CU x 256 CUs x 2.4 GHz; assumes a one-byte LDS read costs what ds_read_b32 "
                       "costs in the microarchitecture table, free broadcast reads of the staged entries and the maximum clock; the cost of a byte read "
                       "has not been measured on this part",
           "shapes": {}}
    for name, r in got.items():
        e = {key: summary(v) for key, v in r.items()}
        e["prepare_points_per_s"] = e["listed_points"]["median"] / (e["prepare_ms"]["median"] * 1e-3)
        e["score_lookups_per_s"] = e["lookups"]["median"] / (e["score_ms"]["median"] * 1e-3)
        e["score_over_bound"] = e["score_lookups_per_s"] / BOUND
        e["peak_hypotheses_per_s"] = e["hypotheses"]["median"] / (e["peak_ms"]["median"] * 1e-3)
        res["shapes"][name] = e
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
