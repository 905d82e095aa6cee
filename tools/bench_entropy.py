"""Entropy: what ll_entropy_run costs per stage, and how many neighbour pairs a second it gets through.

    python tools/bench_entropy.py [--rings 64] [--frames 64,512,4096] [--repeats 5] [--out profiles/entropy.json]

Every figure is the median over `--repeats` FRESH processes, with the minimum and maximum beside it; device times are between HIP
events (ll_entropy_timing: keys, sort + cells, rows, moments, sums).  The keyframes are tools/bench_keyframes.py's: `--source-frames`
frames of one synthetic `rings`-ring drive, mapped and captured, fill a store of K keyframes round-robin, frame k under a pose 0.5 m
further along a circle of 150 m radius.
  run      one op that lists all K frames under the stored poses, default parameters (max_points = the listed points): one untimed
           run, one timed.  Device time per stage, wall time, the op's record, occupied cells, neighbour pairs and pairs per second of
           device time and of the moments kernel's time.
  derived  per neighbour pair that passes the test the moments kernel does 16 f64 operations (6 products, 10 additions, no
           contraction); per candidate it reads 16 bytes of LDS per wave (one broadcast address for 64 lanes).  `f64_gflops_passed` is
           16 x pairs / moments time: a LOWER bound of the kernel's f64 rate derived from the counts, not a counter reading -- the
           candidates that fail the test cost the f32 test only and are not counted by the library.
  host     if scipy imports, the 64-frame case through scipy.spatial.cKDTree on the host (float64 throughout, query_ball_point,
           numpy.linalg.eigvalsh), one run: wall time, mme and mpv beside the device's.  Otherwise "not run".
Prints one JSON line and writes it to --out.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_keyframes import summary  # noqa: E402
from bench_visibility import fill, make_store  # noqa: E402


def host_kdtree(kf, K, radius=0.5, min_nb=6, floor=1e-6):
    """the same measure on the host in float64 -> dict, or None without scipy"""
    try:
        from scipy.spatial import cKDTree
    except Exception:
        return None
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import viscases as vc
    pts, off = kf.export()
    w = np.concatenate([vc.np_to_world(kf.info(k)["pose"], pts[off[2 * k]:off[2 * k + 2]]) for k in range(K)]).astype(np.float64)
    t0 = time.perf_counter()
    tree = cKDTree(w)
    nb = tree.query_ball_point(w, radius, workers=-1)
    h = np.full(len(w), np.nan); pv = np.full(len(w), np.nan)
    for i, idx in enumerate(nb):
        if len(idx) < min_nb:
            continue
        lam = np.linalg.eigvalsh(np.cov(w[idx].T, bias=True))
        pv[i] = max(lam[0], 0.0); h[i] = 0.5 * (3.0 * (1.0 + np.log(2.0 * np.pi)) + np.log(np.maximum(lam, floor)).sum())
    return {"wall_ms": 1e3 * (time.perf_counter() - t0), "mme": float(np.nanmean(h)), "mpv": float(np.nanmean(pv)), "n_valid": int(np.isfinite(h).sum()),
            "pairs": int(sum(len(x) for x in nb))}


def worker(a):
    sys.path.insert(0, a.root); sys.path.insert(0, os.path.join(a.root, "tools"))
    import lightloam_amd  # noqa: F401
    from lightloam_amd import api
    from bench_mapping_sequences import make_drives
    scans, guesses = make_drives(a.rings, 1, a.source_frames)
    ctx = api.Context(api.default_params(a.rings, batch=1, max_points=max(len(s) for s in scans[0])))
    clouds = make_store(a, api, ctx, scans, guesses)
    out = {}
    for K in [int(x) for x in a.frames.split(",")]:
        kf, poses, n_pts = fill(a, ctx, clouds, K)
        en = ctx.entropy(kf, max_points=sum(n_pts))
        op = [(list(range(K)), None)]
        en.run(op)                                                                      # untimed
        t0 = time.perf_counter()
        rec = en.run(op)[0]
        r = {"run_wall_ms": 1e3 * (time.perf_counter() - t0)}
        ms, cnt = en.timing()
        assert cnt[1] == sum(n_pts) == rec.n_points and cnt[3] == rec.n_pairs, (cnt, rec.n_points, rec.n_pairs)
        r.update(keys_ms=ms[0], sort_cells_ms=ms[1], rows_ms=ms[2], moments_ms=ms[3], sums_ms=ms[4], run_device_ms=float(sum(ms)), points=cnt[1],
                 cells=cnt[2], pairs=cnt[3], syncs=cnt[4], n_valid=rec.n_valid, n_sparse=rec.n_sparse, n_outside=rec.n_outside, mme=rec.mme, mpv=rec.mpv)
        if a.host and K == 64:
            r["host"] = host_kdtree(kf, K)
        out[str(K)] = r
        en.close(); kf.close()
    ctx.close()
    print("RESULT " + json.dumps(out), flush=True)


def run_worker(a, rep):
    env = dict(os.environ); env.pop("LIGHTLOAM_HIP_LIB", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "1", "--rings", str(a.rings), "--frames", a.frames, "--source-frames", str(a.source_frames)]
    if rep == 0:
        cmd.append("--host")
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=1100, env=env, cwd=ROOT)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    if p.returncode != 0 or not lines:
        sys.exit(f"worker failed (repeat {rep}): {p.stdout[-2000:]}{p.stderr[-2000:]}")
    print(f"# repeat {rep}: {lines[-1][7:]}", file=sys.stderr, flush=True)
    return json.loads(lines[-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rings", type=int, default=64)
    ap.add_argument("--frames", default="64,512,4096")
    ap.add_argument("--source-frames", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "entropy.json"))
    ap.add_argument("--host", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--worker", default="", help=argparse.SUPPRESS)
    ap.add_argument("--root", default=ROOT, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    got, host = {}, "not run: scipy does not import on this machine"
    for rep in range(a.repeats):
        for K, r in run_worker(a, rep).items():
            h = r.pop("host", None)
            if h is not None:
                host = h
            for key, val in r.items():
                got.setdefault(K, {}).setdefault(key, []).append(val)
    res = {"tool": "tools/bench_entropy.py", "rings": a.rings, "source_frames": a.source_frames, "repeats": a.repeats,
           "what": "medians over fresh processes; device ms between HIP events; radius 0.5, min_neighbours 6, lambda_floor 1e-6",
           "derived": "f64_gflops_passed = 16 f64 operations x pairs / moments time: a lower bound derived from counts, not a counter reading",
           "run": {}, "host_ckdtree_64_frames": host}
    for K, r in got.items():
        e = {key: summary(v) for key, v in r.items()}
        e["pairs_per_s_device"] = e["pairs"]["median"] / (e["run_device_ms"]["median"] * 1e-3)
        e["pairs_per_s_moments"] = e["pairs"]["median"] / (e["moments_ms"]["median"] * 1e-3)
        e["f64_gflops_passed"] = 16e-9 * e["pairs_per_s_moments"]
        e["mean_neighbours"] = e["pairs"]["median"] / max(e["points"]["median"], 1.0)
        res["run"][K] = e
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
