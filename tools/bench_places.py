"""Place recognition (ll_places): device time of describing resident slots and of the exhaustive match.

    python tools/bench_places.py [--rings 64] [--slots 64,1024] [--match 16x4096,256x65536] [--out profiles/places.json]

  describe   `--distinct` synthetic scans fill a context of max(--slots) slots round-robin and are extracted once; ll_places_add_slots of
             the first n slots into an empty database, `--warmup` untimed and `--repeats` timed calls.  Device time (events) of the
             describe launch plus the match-ready form, from ll_places_timing; slots and points per second.
  match      nq + nc random descriptors (non-negative heights, 30 % empty bins) are uploaded; ll_places_match with K = 1 of the first
             nq against the other nc.  Device time of the Gram matrices + diagonals and of the selection (events), wall time of the
             call, pairs per second of Gram time, and that rate as a fraction of the issue-rate bound.
The bound is derived, not measured: a pair is 40 v_mfma_f32_32x32x2_f32 of 64 cycles each on one SIMD, 1024 SIMDs at 2.4 GHz give
1024 * 2.4e9 / (40 * 64) = 9.6e8 pairs/s.  Prints one JSON line and writes it to --out.
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

BOUND_PAIRS_PER_S = 1024 * 2.4e9 / (40 * 64)


def med(x):
    return float(np.median(x))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rings", type=int, default=64)
    ap.add_argument("--slots", default="64,1024")
    ap.add_argument("--match", default="16x4096,256x65536")
    ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "places.json"))
    a = ap.parse_args()
    api.load_library()
    res = {"tool": "tools/bench_places.py", "rings": a.rings, "warmup": a.warmup, "repeats": a.repeats,
           "bound_pairs_per_s": BOUND_PAIRS_PER_S, "bound": "derived: 40 MFMA 32x32x2 f32 x 64 cycles per pair per SIMD, 1024 SIMDs, 2.4 GHz",
           "describe": {}, "match": {}}
    # ---- describe
    n_slots = [int(x) for x in a.slots.split(",") if x]
    if n_slots:
        cfg = synth.default_cfg(a.rings)
        scans = [synth.scan(cfg, 10 * k) for k in range(a.distinct)]
        B = max(n_slots)
        ctx = api.Context(api.default_params(a.rings, batch=B, max_points=max(map(len, scans))))
        for s in range(B):
            ctx.upload_scan(s, scans[s % len(scans)])
        ctx.extract(0, B)
        pts = [ctx.scan_info(s).n for s in range(len(scans))]
        db = ctx.places(B)
        for n in n_slots:
            ms = []
            for rep in range(a.warmup + a.repeats):
                db.reset()
                db.add_slots(np.arange(n))
                t = db.timing()["ms"][0]
                if rep >= a.warmup:
                    ms.append(t)
            points = sum(pts[s % len(pts)] for s in range(n))
            res["describe"][str(n)] = {"slots": n, "points": points, "device_ms": med(ms), "device_ms_min": min(ms), "device_ms_max": max(ms),
                                       "slots_per_s": n / (med(ms) * 1e-3), "points_per_s": points / (med(ms) * 1e-3)}
            print(f"# describe {n}: {res['describe'][str(n)]}", file=sys.stderr, flush=True)
        db.close(); ctx.close()
    # ---- match
    sizes = [tuple(int(v) for v in x.split("x")) for x in a.match.split(",") if x]
    if sizes:
        ctx = api.Context(api.default_params(16, batch=1, max_points=1024))
        rng = np.random.default_rng(1)
        total = max(nq + nc for nq, nc in sizes)
        db = ctx.places(total)
        step = 8192
        for first in range(0, total, step):                        # uploaded in pieces: the host array of all of them would be 300 MB
            n = min(step, total - first)
            d = rng.uniform(0.05, 6.0, (n, 20, 60)).astype(np.float32)
            d[rng.random(d.shape) < 0.3] = 0
            db.upload(first, d)
        for nq, nc in sizes:
            wall, gram, sel = [], [], []
            for rep in range(a.warmup + a.repeats):
                ctx.synchronize()
                t0 = time.perf_counter()
                ids, dist, shift = db.match(0, nq, nq, nc, K=1)
                t = 1e3 * (time.perf_counter() - t0)
                if rep >= a.warmup:
                    tm = db.timing()["ms"]
                    wall.append(t); gram.append(tm[1]); sel.append(tm[2])
            pairs = nq * nc
            rate = pairs / (med(gram) * 1e-3)
            res["match"]["%dx%d" % (nq, nc)] = {"nq": nq, "nc": nc, "pairs": pairs, "gram_ms": med(gram), "gram_ms_min": min(gram), "gram_ms_max": max(gram),
                                                "select_ms": med(sel), "wall_ms": med(wall), "pairs_per_s": rate,
                                                "fraction_of_issue_bound": rate / BOUND_PAIRS_PER_S,
                                                "best_distance_mean": float(dist.mean())}
            print(f"# match {nq}x{nc}: {res['match']['%dx%d' % (nq, nc)]}", file=sys.stderr, flush=True)
        db.close(); ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
