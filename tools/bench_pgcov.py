"""Pose-graph covariances (ll_posegraphs_covariances): device time of joint covariances of pose pairs on the laps of bench_posegraph.

    python tools/bench_pgcov.py [--nodes 512,2048,4541] [--queries 1,8,64] [--processes 3] [--out profiles/pgcov.json]

  graph      tools/bench_posegraph.py's drifting double lap of N poses with N / 100 loop edges, first solved (default options, the
             kind's preconditioner); the covariances are taken at the solved poses.
  queries    Q pairs (a, a - N / 2): a pose of the second lap and the one a lap earlier, what a loop candidate asks about; the a's are
             spread evenly over the second lap, so Q pairs are 2 Q sources and 12 Q columns.
  figures    per kind (jacobi, chain), N and Q: device ms of the call's prepare and columns launches (events, ll_posegraphs_cov_timing),
             their sum as the call, wall ms, the columns' time and PCG iterations per column, the records' statuses and largest
             residual; beside them the device ms and iterations of the ONE solve of the same graph under the same kind.
  processes  every figure is the median over `--processes` fresh processes per kind, kinds alternating.
  retry      where a call under the chain preconditioner ends with a status other than 0 at the default 1000 iterations per column and
             Q <= 8, it is repeated once with --retry-limit (20000) and reported beside as `with_a_higher_limit`: what convergence costs.
  dense      at --dense-nodes (512) the wall time of numpy.linalg.inv of the dense H (tests/pgcovcases.py builds it), and the largest
             difference between the device's blocks and that inverse's, per kind, for Q = 8.
There is no pass mark: the capability is new.  Prints one JSON line and writes it to --out.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lightloam_amd  # noqa: E402,F401
from lightloam_amd import api  # noqa: E402
from bench_posegraph import lap_graph  # noqa: E402


def pair_queries(n, q):
    half = n // 2
    a = half + (np.arange(q) * (n - half)) // q + (n - half) // (2 * q)
    return [(0, int(k), int(k - half)) for k in a]


def dense(x, edges, queries, joint):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import pgcovcases as cv
    import posegraphcases as pc
    el = [pc.edge(e["i"], e["j"], e["Z_w7"], e["sqrt_info"], e["huber"]) for e in edges]
    t0 = time.perf_counter()
    H, free = cv.dense_H(x, el)
    t1 = time.perf_counter()
    S = np.zeros_like(H)
    S[np.ix_(free, free)] = np.linalg.inv(H[np.ix_(free, free)])
    t2 = time.perf_counter()
    diff = max(float(np.abs(joint[k] - cv.joint(S, a, b)).max()) for k, (_, a, b) in enumerate(queries))
    return {"what": "numpy: the dense H of tests/pgcovcases.py, numpy.linalg.inv of its free part", "unknowns": int(free.sum()),
            "build_wall_s": t1 - t0, "inv_wall_s": t2 - t1, "max_abs_difference_from_device": diff,
            "largest_entry": float(np.abs(S).max())}


def child(a):
    nodes = [int(x) for x in a.nodes.split(",")]; counts = [int(x) for x in a.queries.split(",")]
    ctx = api.Context(api.default_params(16, batch=1, max_points=1024))
    nmax = max(nodes)
    pg = ctx.posegraphs(1, nmax, nmax + nmax // 100)
    pg.set_preconditioner(a.kind)
    warm = lap_graph(min(nodes), 0)
    pg.solve([warm]); pg.covariances([warm], pair_queries(min(nodes), 1))
    out = {}
    for n in nodes:
        start, edges = lap_graph(n, 1000)
        x, rec = pg.solve([(start, edges)])
        t = pg.timing()
        solve = {"device_ms": t["ms"][1], "lm_iterations": rec[0].lm_iterations, "pcg_iterations": rec[0].pcg_iterations,
                 "termination": rec[0].termination, "cost": rec[0].cost}
        for q in counts:
            queries = pair_queries(n, q)
            t0 = time.perf_counter()
            joint, crec = pg.covariances([(x[0], edges)], queries)
            wall = 1e3 * (time.perf_counter() - t0)
            ct = pg.cov_timing()
            cols = 6 * ct["sources"]
            e = {"nodes": n, "edges": len(edges), "queries": q, "sources": ct["sources"], "columns": cols, "prepare_ms": ct["ms"][0],
                 "columns_ms": ct["ms"][1], "device_ms": ct["ms"][0] + ct["ms"][1], "wall_ms": wall, "pcg_iterations": ct["pcg_iterations"],
                 "pcg_iterations_per_column": ct["pcg_iterations"] / cols, "most_pcg_iterations_of_a_query": max(r.pcg_iterations for r in crec),
                 "statuses": sorted({r.status for r in crec}), "largest_residual": max(r.residual for r in crec),
                 "all_finite": bool(np.isfinite(joint).all()), "solve": solve}
            if e["statuses"] != [0] and a.kind == "chain" and q <= 8:  # the default limit was too low: what convergence costs
                joint2, crec2 = pg.covariances([(x[0], edges)], queries, api.pg_cov_options(max_pcg_iterations=a.retry_limit))
                c2 = pg.cov_timing()
                e["with_a_higher_limit"] = {"max_pcg_iterations": a.retry_limit, "prepare_ms": c2["ms"][0], "columns_ms": c2["ms"][1],
                                            "device_ms": c2["ms"][0] + c2["ms"][1], "pcg_iterations_per_column": c2["pcg_iterations"] / cols,
                                            "most_pcg_iterations_of_a_column_at_least": max(r.pcg_iterations for r in crec2) / 12.0,
                                            "statuses": sorted({r.status for r in crec2}), "largest_residual": max(r.residual for r in crec2),
                                            "largest_change_of_an_entry": float(np.abs(joint2 - joint).max()), "largest_entry": float(np.abs(joint2).max())}
            if n == a.dense_nodes and q == 8:
                e["dense"] = dense(x[0], edges, queries, joint)
            out["%dx%d" % (n, q)] = e
            print("# %s %dx%d: %s" % (a.kind, n, q, e), file=sys.stderr, flush=True)
    pg.close(); ctx.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", default="512,2048,4541")
    ap.add_argument("--queries", default="1,8,64")
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--dense-nodes", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pgcov.json"))
    ap.add_argument("--retry-limit", type=int, default=20000)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--kind", default="jacobi", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    kinds = ["jacobi", "chain"]
    runs = {k: [] for k in kinds}
    for p in range(a.processes):                                    # fresh processes, one after the other, the kinds alternating
        for kind in kinds:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--nodes", a.nodes, "--queries", a.queries,
                                "--dense-nodes", str(a.dense_nodes if p == 0 else 0), "--retry-limit", str(a.retry_limit), "--kind", kind], stdout=subprocess.PIPE, check=True, timeout=1100)
            runs[kind].append(json.loads(r.stdout.decode().strip().splitlines()[-1]))
    res = {"tool": "tools/bench_pgcov.py", "processes": a.processes,
           "what": "ll_posegraphs_covariances on bench_posegraph's laps at the solved poses: device ms (events) of prepare and columns, medians over "
                   "fresh processes; Q pair queries = 2 Q sources = 12 Q columns, one workgroup per column; solve = the one solve of the same graph "
                   "under the same preconditioner", "kinds": {}}
    for kind in kinds:
        res["kinds"][kind] = {}
        for key in runs[kind][0]:
            e = dict(runs[kind][0][key])
            for f in ("prepare_ms", "columns_ms", "device_ms", "wall_ms"):
                v = [r[key][f] for r in runs[kind]]
                e[f] = float(np.median(v)); e[f + "_min"] = min(v); e[f + "_max"] = max(v)
            sv = [r[key]["solve"]["device_ms"] for r in runs[kind]]
            e["solve"] = dict(e["solve"], device_ms=float(np.median(sv)), device_ms_min=min(sv), device_ms_max=max(sv))
            if "with_a_higher_limit" in e:
                for f in ("prepare_ms", "columns_ms", "device_ms"):
                    e["with_a_higher_limit"][f] = float(np.median([r[key]["with_a_higher_limit"][f] for r in runs[kind]]))
            e["columns_ms_per_column"] = e["columns_ms"] / e["columns"]
            e["call_over_solve"] = e["device_ms"] / e["solve"]["device_ms"]
            e["same_iterations_in_every_process"] = all(r[key]["pcg_iterations"] == e["pcg_iterations"] for r in runs[kind])
            res["kinds"][kind][key] = e
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
