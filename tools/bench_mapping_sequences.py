"""Frames/s of laserMapping's per-frame body for S sequences side by side (ll_cubemaps_process_slots) against the same drives run
one after another through ll_cubemap_process_slot.

    python tools/bench_mapping_sequences.py [--rings 64] [--seqs 1,8,32,128] [--frames 8] [--out profiles/r07_mapping_sequences.json]

Sequence q replays synthetic drive q % drives (synth.default_cfg with its own seed / speed / yaw rate).  Per frame the S scans are
uploaded into slots 0 .. S-1 and extracted (not timed), then one process_slots call is timed, device-synchronised before and after.
Frame 0 (an empty map: the :1822 gate skips the solve) is a warm-up; frames 1 .. frames-1 are timed.  The one-after-another rate
times the distinct drives, each through its own ll_cubemap, the same way.  Host synchronisations per frame come from
ll_cubemaps_stats.  Prints one JSON line and writes it to --out.
"""
import argparse
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


def make_drives(rings, n_drives, n_frames):
    cfgs = [synth.default_cfg(rings, seed=101 + 13 * d, speed=6.0 + 1.0 * (d % 5), yaw_rate=0.05 * ((d % 3) - 1)) for d in range(n_drives)]
    scans = [[synth.scan(c, k) for k in range(n_frames)] for c in cfgs]
    guesses = [[np.array([0.0, 0.0, np.sin(p[2] / 2), np.cos(p[2] / 2), p[0] + 0.05, p[1] - 0.02, 0.01])
                for p in (synth.pose(c, k) for k in range(n_frames))] for c in cfgs]
    return scans, np.array(guesses)


def load(ctx, scans, S, k):
    for q in range(S):
        ctx.upload_scan(q, scans[q % len(scans)][k])
    ctx.extract(0, S)


def timed(ctx, fn):
    ctx.synchronize()
    t0 = time.perf_counter()
    out = fn()
    ctx.synchronize()
    return time.perf_counter() - t0, out


def one_after_another(rings, scans, guesses, pool):
    D, F = len(scans), len(scans[0])
    ctx = api.Context(api.default_params(rings, batch=1, max_points=max(len(s) for d in scans for s in d)))
    tot = 0.0
    for d in range(D):
        cm = api.CubeMap(ctx, *CAP[rings], pool_points=pool)
        for k in range(F):
            load(ctx, [scans[d]], 1, k)
            t, _ = timed(ctx, lambda: cm.process_slot(guesses[d, k], 0))
            if k:
                tot += t
        cm.close()
    ctx.close()
    return D * (F - 1) / tot


def side_by_side(rings, scans, guesses, S, pool):
    D, F = len(scans), len(scans[0])
    ctx = api.Context(api.default_params(rings, batch=S, max_points=max(len(s) for d in scans for s in d)))
    cms = api.CubeMaps(ctx, S, *CAP[rings], pool_points=pool)
    g = guesses[np.arange(S) % D]
    tot, syncs0 = 0.0, 0
    for k in range(F):
        load(ctx, scans, S, k)
        if k == 1:
            syncs0 = cms.stats()[0]
        t, (_, ran) = timed(ctx, lambda: cms.process_slots(g[:, k], list(range(S))))
        if k:
            tot += t
            assert ran.all()
    syncs = (cms.stats()[0] - syncs0) / (F - 1)
    cms.close(); ctx.close()
    return S * (F - 1) / tot, {"frame_ms": 1e3 * tot / (F - 1), "host_syncs_per_frame": syncs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rings", type=int, nargs="+", default=[64])
    ap.add_argument("--seqs", default="1,8,32,128")
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--drives", type=int, default=8)
    ap.add_argument("--pool", type=int, default=1 << 19)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_mapping_sequences.json"))
    a = ap.parse_args()
    seqs = [int(x) for x in a.seqs.split(",")]
    res = {"tool": "tools/bench_mapping_sequences.py", "frames": a.frames, "timed_frames": a.frames - 1, "drives": a.drives,
           "pool_points": a.pool, "launches_per_frame": "not measured", "curves": {}}
    for rings in a.rings:
        scans, guesses = make_drives(rings, a.drives, a.frames)
        seq_fps = one_after_another(rings, scans, guesses, a.pool)
        curve = {"one_after_another_frames_per_s": seq_fps, "side_by_side": {}}
        print(f"# rings {rings} one after another: {seq_fps:.1f} frames/s", file=sys.stderr, flush=True)
        for S in seqs:
            fps, info = side_by_side(rings, scans, guesses, S, a.pool)
            info["frames_per_s"] = fps
            info["x_one_after_another"] = fps / seq_fps
            curve["side_by_side"][str(S)] = info
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
