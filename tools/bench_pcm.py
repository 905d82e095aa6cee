"""Pcm: what ll_pcm_run costs per stage, how many pairs and row-ANDs a second it gets through, and ll_pcm_host beside it.

    python tools/bench_pcm.py [--sizes 256,1024,4096] [--graphs 1,16] [--repeats 5] [--out profiles/pcm.json]

Every figure is the median over `--repeats` FRESH processes, with the minimum and maximum beside it; device times are between HIP
events (ll_pcm_timing: prepare, adjacency, order, clique, pick), wall times a host clock around the call, which ends in its one
synchronisation.  Per case one untimed call, then one timed.
  graphs   4541 poses, 0.82 m apart, twice round a circle; C candidates per graph between a pose of the first lap and one within five poses
           of the same place on the second, G graphs per call (the same poses, other candidates).
           kind "half": half the candidates measure the poses' own relative pose (plus 1 mrad, 2 cm of noise: mutually consistent),
           half are random; kind "all": every candidate is consistent with every other, the selection's worst case.
  host     ll_pcm_host for ONE graph of the case on one core (wall), taken in the first process only: compare it with the device's
           1-graph call.
  derived  pairs_per_s_adjacency = C * C * G / adjacency time (both triangles are evaluated); f64_ops_per_pair = 190 counted from
           ll_pcm_math.h (two compositions, the two norms, the thresholds, no contraction), so f64_gops_adjacency is derived from counts,
           not a counter reading.  row_ands_per_s = clique steps / clique time; a step reads one row of ceil(C / 64) * 8 bytes from L2.
           DERIVED bound, not measured here: the microarchitecture guide's chip-wide rate of rows served from the XCDs' L2, 16.8 TB/s,
           over 512-byte rows is 32.8e9 row-ANDs a second at C = 4096; the walk is a chain of dependent reads per wave, so its rate is
           set by latency and the waves in flight, not by that bound.
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

N_POSES = 4541
F64_OPS_PER_PAIR = 190
L2_ROW_BYTES_PER_S = 16.8e12


def lap():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import pcmcases as pc
    dth = 4.0 * np.pi / N_POSES                                       # two laps
    r = 3724.0 / (4.0 * np.pi)
    a = dth * np.arange(N_POSES)
    P = np.zeros((N_POSES, 7))
    P[:, 2] = np.sin(a / 2); P[:, 3] = np.cos(a / 2); P[:, 4] = r * np.sin(a); P[:, 5] = r * (1.0 - np.cos(a))
    return pc, P


def candidates(pc, P, C, kind, seed):
    """a PCM_CANDIDATE-shaped tuple of arrays (i, j, Z [C, 7])"""
    rng = np.random.default_rng(seed)
    i = rng.integers(5, N_POSES // 2 - 5, C); j = i + N_POSES // 2 + rng.integers(-5, 6, C)
    rv = rng.normal(0, 1e-3, (C, 3)); ang = np.linalg.norm(rv, axis=1, keepdims=True)
    noise = np.concatenate([np.sin(ang / 2) * rv / ang, np.cos(ang / 2), rng.normal(0, 0.02, (C, 3))], axis=1)
    Z = pc.compose(pc.relative(P[i], P[j]), noise)
    if kind == "half":
        bad = rng.permutation(C)[:C // 2]
        q = rng.normal(0, 1, (len(bad), 4)); q /= np.linalg.norm(q, axis=1, keepdims=True)
        Z[bad] = np.concatenate([q, rng.normal(0, 30.0, (len(bad), 3))], axis=1)
    return i, j, Z


def worker(a):
    sys.path.insert(0, a.root)
    import lightloam_amd  # noqa: F401
    from lightloam_amd import api
    pc, P = lap()
    sizes = [int(x) for x in a.sizes.split(",")]; counts = [int(x) for x in a.graphs.split(",")]
    ctx = api.Context(api.default_params(16, batch=1, max_points=4096))
    pcm = ctx.pcm(max(counts), max(counts) * N_POSES, max(counts) * max(sizes))
    out = {}
    for kind in ("half", "all"):
        for C in sizes:
            graphs = []
            for g in range(max(counts)):
                i, j, Z = candidates(pc, P, C, kind, 1000 * C + g)
                cd = np.zeros(C, api.PCM_CANDIDATE); cd["i"] = i; cd["j"] = j; cd["Z_w7"] = Z
                graphs.append((P, cd))
            host = None
            if a.host:
                t0 = time.perf_counter()
                hw, hsel, hdeg, hrec = api.pcm_host(*graphs[0])
                host = 1e3 * (time.perf_counter() - t0)
            for G in counts:
                pcm.run(graphs[:G])                                                     # untimed
                t0 = time.perf_counter()
                sel, deg, rec = pcm.run(graphs[:G])
                wall = 1e3 * (time.perf_counter() - t0)
                t = pcm.timing()
                want = C // 2 if kind == "half" else C
                assert all(r.n_selected == want for r in rec), [r.n_selected for r in rec]
                if host is not None:
                    assert sel[0].tobytes() == hsel.tobytes() and deg[0].tobytes() == hdeg.tobytes() and bytes(memoryview(rec[0])) == bytes(memoryview(hrec))
                ms = t["ms"]
                r = dict(run_wall_ms=wall, prepare_ms=ms[0], adjacency_ms=ms[1], order_ms=ms[2], clique_ms=ms[3], pick_ms=ms[4], run_device_ms=float(sum(ms)),
                         pairs=t["pairs"], clique_steps=t["clique_steps"], n_selected=rec[0].n_selected)
                if host is not None and G == 1:
                    r["host_one_graph_wall_ms"] = host
                out[f"{kind}/C{C}/G{G}"] = r
    pcm.close(); ctx.close()
    print("RESULT " + json.dumps(out), flush=True)


def run_worker(a, rep):
    env = dict(os.environ); env.pop("LIGHTLOAM_HIP_LIB", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "1", "--sizes", a.sizes, "--graphs", a.graphs]
    if rep == 0:
        cmd.append("--host")
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=500, env=env, cwd=ROOT)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    if p.returncode != 0 or not lines:
        sys.exit(f"worker failed (repeat {rep}): {p.stdout[-2000:]}{p.stderr[-2000:]}")
    print(f"# repeat {rep}: {lines[-1][7:]}", file=sys.stderr, flush=True)
    return json.loads(lines[-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,1024,4096")
    ap.add_argument("--graphs", default="1,16")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pcm.json"))
    ap.add_argument("--host", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--worker", default="", help=argparse.SUPPRESS)
    ap.add_argument("--root", default=ROOT, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    got = {}
    for rep in range(a.repeats):
        for case, r in run_worker(a, rep).items():
            for key, val in r.items():
                got.setdefault(case, {}).setdefault(key, []).append(val)
    res = {"tool": "tools/bench_pcm.py", "poses": N_POSES, "repeats": a.repeats,
           "what": "medians over fresh processes; device ms between HIP events; default thresholds; host = ll_pcm_host, one graph, one core, first process only",
           "derived": f"f64_gops_adjacency = {F64_OPS_PER_PAIR} f64 operations x pairs / adjacency time, from counts; l2_row_bound_per_s is DERIVED from the "
                      "microarchitecture guide's 16.8 TB/s of L2-served rows, not measured here",
           "run": {}}
    for case, r in got.items():
        e = {key: summary(v) for key, v in r.items()}
        C = int(case.split("/")[1][1:])
        e["pairs_per_s_adjacency"] = e["pairs"]["median"] / (e["adjacency_ms"]["median"] * 1e-3)
        e["f64_gops_adjacency"] = 1e-9 * F64_OPS_PER_PAIR * e["pairs_per_s_adjacency"]
        e["row_ands_per_s"] = e["clique_steps"]["median"] / (e["clique_ms"]["median"] * 1e-3)
        e["l2_row_bound_per_s"] = L2_ROW_BYTES_PER_S / (((C + 63) // 64) * 8)
        if "host_one_graph_wall_ms" in e:
            e["device_faster_than_host"] = bool(e["run_wall_ms"]["median"] < e["host_one_graph_wall_ms"]["median"])
        res["run"][case] = e
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
