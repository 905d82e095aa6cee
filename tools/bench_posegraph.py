"""Pose graphs (ll_posegraphs): device time of the batched solve on drifting laps with 1 % loop edges.

    python tools/bench_posegraph.py [--nodes 512,2048,4541] [--batches 1,16,256] [--processes 5] [--out profiles/posegraph.json]

  graph      a planar double lap of N poses (the second lap retraces the first), odometry edges from the truth with Gaussian noise and a
             constant yaw bias per step, N / 100 loop edges from the truth (with noise, Huber width 1) between a pose and the one a lap
             earlier.  The start is the odometry chained up from node 0, so it drifts; node 0 is fixed.  Every graph of a batch has its
             own noise.
  figures    per (N, batch): device time of ll_posegraphs_solve's one launch (events, ll_posegraphs_timing), LM and PCG iterations of
             graph 0, microseconds per PCG iteration (the launch's time over graph 0's PCG iterations: one workgroup per graph, so the
             batch runs side by side), and the bytes one PCG iteration touches per graph -- N nodes x (36 + 6 doubles of block and
             diagonal, 7 vectors of 6 read or written) + 2 (N + loops) incident blocks of 36 doubles -- as a fraction of what the L2 and
             HBM could move in that time (published and measured figures of the MI355X: HBM3E 8 TB/s peak, L2 about 34.5 TB/s over
             the chip, and 66 - 73 GB/s -- taken as 70 -- for what ONE CU reads from its XCD's L2).  A graph is one workgroup on one
             CU, so the last rate is the one a single large graph can meet; the chip-wide rates only matter to large batches.
  processes  every figure is the median over `--processes` fresh processes (each solves every configuration once after one warm-up
             solve of the smallest).
The capability is new, so there is no earlier figure to compare with.  `restatement` is the wall time of the numpy dense LM of
tests/posegraphcases.py on the 512-node graph: an independent restatement that the tests use as their reference, not a competitor.
Prints one JSON line and writes it to --out.

    python tools/bench_posegraph.py --preconditioner both [--parent-root DIR] [--out profiles/posegraph_chain.json]

  --preconditioner  jacobi (the default: everything above, unchanged), chain (the same figures under LL_PG_PRECOND_CHAIN), or both:
             the same graphs under each kind, every (kind, repeat) a fresh process as above, kinds alternating.  With --parent-root DIR
             (a built checkout of the parent commit, as tools/bench_info.py takes it) the parent's library solves them too, under its
             only preconditioner, and `default_bits_equal_parent` says per configuration whether this tree's block-Jacobi poses and
             records are byte for byte the parent's (a SHA-256 over graph 0 .. batch - 1 of every process).  The file holds, per kind
             and (N, batch): device ms (median, minimum, maximum), LM and PCG iterations, factorisations and fallbacks, the final cost
             and the largest lap gap, and `chain_over_jacobi`, the ratio of the median device times.
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# a child of --preconditioner both that measures the parent's library imports the parent's package
sys.path.insert(0, sys.argv[sys.argv.index("--root") + 1] if "--root" in sys.argv[:-1] else ROOT)
import lightloam_amd  # noqa: E402,F401
from lightloam_amd import api  # noqa: E402

HBM_BYTES_PER_S = 8.0e12
L2_BYTES_PER_S = 34.5e12
L2_ONE_CU_BYTES_PER_S = 70.0e9


def lap_graph(n, seed, yaw_bias=2e-4, sig_yaw=1e-3, sig_t=0.01, radius=50.0):
    """(start [n, 7], edges PG_EDGE [n - 1 + n // 100]) of a planar double lap"""
    rng = np.random.default_rng(seed)
    half = n // 2
    th = 2.0 * np.pi * np.arange(n) / half
    xy = radius * np.stack([np.sin(th), 1.0 - np.cos(th)], axis=1)
    loops = np.sort(rng.choice(np.arange(half, n), size=max(n // 100, 1), replace=False))
    ei = np.concatenate([np.arange(n - 1), loops]); ej = np.concatenate([np.arange(1, n), loops - half])
    dyaw = th[ej] - th[ei]
    d = xy[ej] - xy[ei]
    c, s = np.cos(th[ei]), np.sin(th[ei])
    rel = np.stack([c * d[:, 0] + s * d[:, 1], -s * d[:, 0] + c * d[:, 1], np.zeros(len(ei))], axis=1)     # R(yaw_i)^T (t_j - t_i)
    dyaw = dyaw + rng.normal(0.0, sig_yaw, len(ei)); dyaw[:n - 1] += yaw_bias
    rel = rel + rng.normal(0.0, sig_t, rel.shape)
    edges = np.zeros(len(ei), api.PG_EDGE)
    edges["i"] = ei; edges["j"] = ej
    edges["Z_w7"][:, 2] = np.sin(0.5 * dyaw); edges["Z_w7"][:, 3] = np.cos(0.5 * dyaw); edges["Z_w7"][:, 4:] = rel
    edges["sqrt_info"][:, :3] = 100.0; edges["sqrt_info"][:, 3:] = 20.0
    edges["huber"][n - 1:] = 1.0
    yaw = np.concatenate([[0.0], np.cumsum(dyaw[:n - 1])])         # the drifting chain
    step = np.stack([np.cos(yaw[:-1]) * rel[:n - 1, 0] - np.sin(yaw[:-1]) * rel[:n - 1, 1],
                     np.sin(yaw[:-1]) * rel[:n - 1, 0] + np.cos(yaw[:-1]) * rel[:n - 1, 1], rel[:n - 1, 2]], axis=1)
    start = np.zeros((n, 7))
    start[:, 2] = np.sin(0.5 * yaw); start[:, 3] = np.cos(0.5 * yaw)
    start[1:, 4:] = np.cumsum(step, axis=0)
    return start, edges


def pcg_bytes(n, n_edges):
    return 8 * (n * (36 + 6 + 7 * 6) + 2 * n_edges * 36)


def child(a):
    nodes = [int(x) for x in a.nodes.split(",")]; batches = [int(x) for x in a.batches.split(",")]
    ctx = api.Context(api.default_params(16, batch=1, max_points=1024))
    nmax, bmax = max(nodes), max(batches)
    pg = ctx.posegraphs(bmax, nmax * bmax, (nmax + nmax // 100) * bmax)
    if a.kind == "chain":
        pg.set_preconditioner(api.PG_PRECOND_CHAIN)
    pg.solve([lap_graph(min(nodes), 0)])
    out = {}
    for n in nodes:
        graphs = [lap_graph(n, 1000 + b) for b in range(bmax)]
        for b in batches:
            t0 = time.perf_counter()
            x, rec = pg.solve(graphs[:b])
            wall = 1e3 * (time.perf_counter() - t0)
            t = pg.timing()
            r = rec[0]
            drift0 = float(np.linalg.norm(graphs[0][0][n // 2:, 4:6] - graphs[0][0][:n - n // 2, 4:6], axis=1).max())
            drift1 = float(np.linalg.norm(x[0][n // 2:, 4:6] - x[0][:n - n // 2, 4:6], axis=1).max())
            out["%dx%d" % (n, b)] = {"nodes": n, "edges": len(graphs[0][1]), "batch": b, "device_ms": t["ms"][1], "wall_ms": wall,
                                     "lm_iterations": r.lm_iterations, "lm_successes": r.lm_successes, "pcg_iterations": r.pcg_iterations,
                                     "termination": r.termination, "cost0": r.cost0, "cost": r.cost,
                                     "lm_iterations_batch": t["lm_iterations"], "pcg_iterations_batch": t["pcg_iterations"],
                                     "lap_gap_before_m": drift0, "lap_gap_after_m": drift1}
            if a.kind:                                              # the comparison's extras; the parent's package has no precond_stats
                h = hashlib.sha256()
                for g in range(b):
                    h.update(x[g].tobytes()); h.update(bytes(memoryview(rec[g])))
                stats = pg.precond_stats() if hasattr(pg, "precond_stats") else {"factorisations": 0, "fallbacks": 0}
                out["%dx%d" % (n, b)].update({"sha256": h.hexdigest(), "factorisations_batch": stats["factorisations"],
                                              "fallbacks_batch": stats["fallbacks"]})
            print("# %dx%d: %s" % (n, b, out["%dx%d" % (n, b)]), file=sys.stderr, flush=True)
    pg.close(); ctx.close()
    print(json.dumps(out))


def restatement(n):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import posegraphcases as pc
    start, edges = lap_graph(n, 1000)
    el = [pc.edge(e["i"], e["j"], e["Z_w7"], e["sqrt_info"], e["huber"]) for e in edges]
    t0 = time.perf_counter()
    x, gmax, it = pc.dense_lm(start, el, max_iterations=30)
    return {"what": "numpy dense LM of tests/posegraphcases.py (central-difference Jacobians, numpy.linalg.solve): a restatement, not a competitor",
            "nodes": n, "wall_s": time.perf_counter() - t0, "iterations": it, "gradient_max": gmax}


def compare(a):
    """--preconditioner chain / both: per kind the children's figures side by side"""
    kinds = [("jacobi", ROOT), ("chain", ROOT)] if a.preconditioner == "both" else [("chain", ROOT)]
    if a.parent_root:
        if not os.path.exists(os.path.join(a.parent_root, "light-loam_amd", "liblightloam_hip.so")):
            sys.exit("--parent-root must name a built checkout of the parent commit (light-loam_amd/liblightloam_hip.so in it)")
        kinds.insert(0, ("parent", os.path.abspath(a.parent_root)))
    runs = {k: [] for k, _ in kinds}
    for p in range(a.processes):                                   # fresh processes, one after the other, the kinds alternating
        for kind, root in kinds:
            env = dict(os.environ); env.pop("LIGHTLOAM_HIP_LIB", None)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--nodes", a.nodes, "--batches", a.batches,
                                "--kind", "chain" if kind == "chain" else "jacobi", "--root", root],
                               stdout=subprocess.PIPE, check=True, timeout=1500, env=env, cwd=root)
            runs[kind].append(json.loads(r.stdout.decode().strip().splitlines()[-1]))
    keep = ("nodes", "edges", "batch", "lm_iterations", "lm_successes", "pcg_iterations", "termination", "cost0", "cost", "lm_iterations_batch",
            "pcg_iterations_batch", "factorisations_batch", "fallbacks_batch", "lap_gap_before_m", "lap_gap_after_m")
    res = {"tool": "tools/bench_posegraph.py", "preconditioner": a.preconditioner, "processes": a.processes,
           "what": "device ms of the solve's one launch (ll_posegraphs_timing), median over fresh processes; iterations, cost and lap gap of "
                   "graph 0, *_batch summed over the batch; parent = the parent commit's library (block-Jacobi only)",
           "kinds": {}}
    for kind, _ in kinds:
        res["kinds"][kind] = {}
        for key in runs[kind][0]:
            ms = [r[key]["device_ms"] for r in runs[kind]]
            e = {k: runs[kind][0][key][k] for k in keep}
            e.update({"device_ms": float(np.median(ms)), "device_ms_min": min(ms), "device_ms_max": max(ms),
                      "same_bits_in_every_process": len({r[key]["sha256"] for r in runs[kind]}) == 1})
            res["kinds"][kind][key] = e
    K = res["kinds"]
    if "jacobi" in K:
        res["chain_over_jacobi"] = {key: K["chain"][key]["device_ms"] / K["jacobi"][key]["device_ms"] for key in K["chain"]}
    if "parent" in K and "jacobi" in K:
        res["default_bits_equal_parent"] = {key: {r[key]["sha256"] for r in runs["jacobi"]} == {r[key]["sha256"] for r in runs["parent"]}
                                            and K["jacobi"][key]["same_bits_in_every_process"] for key in K["jacobi"]}
        res["jacobi_over_parent"] = {key: K["jacobi"][key]["device_ms"] / K["parent"][key]["device_ms"] for key in K["jacobi"]}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", default="512,2048,4541")
    ap.add_argument("--batches", default="1,16,256")
    ap.add_argument("--processes", type=int, default=5)
    ap.add_argument("--restatement-nodes", type=int, default=512)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default=None, help="profiles/posegraph.json; profiles/posegraph_chain.json for --preconditioner chain or both")
    ap.add_argument("--preconditioner", choices=["jacobi", "chain", "both"], default="jacobi")
    ap.add_argument("--parent-root", help="with --preconditioner both: a built checkout of the parent commit, measured beside this tree")
    ap.add_argument("--kind", default="", help=argparse.SUPPRESS)
    ap.add_argument("--root", default=ROOT, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "posegraph.json" if a.preconditioner == "jacobi" else "posegraph_chain.json")
    if a.preconditioner != "jacobi":
        return compare(a)
    runs = []
    for p in range(a.processes):                                   # fresh processes, one after the other
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--nodes", a.nodes, "--batches", a.batches],
                           stdout=subprocess.PIPE, check=True, timeout=1500)
        runs.append(json.loads(r.stdout.decode().strip().splitlines()[-1]))
    res = {"tool": "tools/bench_posegraph.py", "processes": a.processes, "hbm_bytes_per_s": HBM_BYTES_PER_S, "l2_bytes_per_s": L2_BYTES_PER_S,
           "l2_one_cu_bytes_per_s": L2_ONE_CU_BYTES_PER_S, "rates": "MI355X: HBM3E 8 TB/s peak; L2 34.5 TB/s chip-wide, 70 GB/s into one CU", "solve": {}}
    for key in runs[0]:
        ms = [r[key]["device_ms"] for r in runs]
        e = dict(runs[0][key])
        e.update({"device_ms": float(np.median(ms)), "device_ms_min": min(ms), "device_ms_max": max(ms),
                  "wall_ms": float(np.median([r[key]["wall_ms"] for r in runs]))})
        e["same_iterations_in_every_process"] = all(r[key]["pcg_iterations"] == e["pcg_iterations"] for r in runs)
        if e["pcg_iterations"] > 0:
            us = 1e3 * e["device_ms"] / e["pcg_iterations"]
            by = pcg_bytes(e["nodes"], e["edges"])
            e.update({"us_per_pcg_iteration": us, "bytes_per_pcg_iteration_per_graph": by,
                      "fraction_of_one_cu_l2_rate": by / (us * 1e-6) / L2_ONE_CU_BYTES_PER_S,
                      "fraction_of_l2_rate": by * e["batch"] / (us * 1e-6) / L2_BYTES_PER_S,
                      "fraction_of_hbm_rate": by * e["batch"] / (us * 1e-6) / HBM_BYTES_PER_S})
        res["solve"][key] = e
    if a.restatement_nodes > 0:
        res["restatement"] = restatement(a.restatement_nodes)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
