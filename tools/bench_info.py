"""What the measured information costs: ll_pose_info out of localisation and alignment, and full 6 x 6 edges in the pose graph, beside
the same calls of the parent commit in the same session.

    python tools/bench_info.py --parent-root DIR [--rings 64] [--seqs 1,16] [--frames 6] [--ops 1,4,16] [--calls 11] [--nodes 512] [--repeats 5]
                               [--out profiles/info.json]

DIR is a built checkout of the commit before ll_pose_info existed (git worktree add DIR <commit>; python DIR/__graft_entry__.py).
Every figure is DEVICE time: between two HIP events on the context's stream around the one call (localize, align), or the solve's own
events (ll_posegraphs_timing).
  localize  tools/bench_mapping_sequences.py's workload (sequence q replays synthetic drive q % 8): frames 0 .. `frames` - 1 are mapped
            into S maps, then frames 1 .. `frames` - 1 go through ll_cubemaps_localize_slots, every sequence against its own frozen map,
            the scans uploaded and extracted beforehand; ms per frame for S = 1 and 16, with the fit record (`fit`) and with fit and
            information (`fit_info`).  A frame holds the call's three host synchronisations.
  align     on the 16 maps left by that pass (sequences q and q + 8 hold the same drive's map): ops (q, q + 8) and (q + 8, q) from the
            identity, n_outer = 2; ms per call (the median of `calls` calls) for 1, 4 and 16 ops, `fit` and `fit_info`.
  solve6    tools/bench_posegraph.py's 512-pose double lap: ll_posegraphs_solve with its diagonal weights (`solve`) and
            ll_posegraphs_solve6 with the same weights given as full matrices diag(sqrt_info) (`solve6`): the cost of generality.  The two
            run the same arithmetic up to added zeros, so the LM and PCG iteration counts are reported beside the times.
Every repeat is a fresh process per library -- the parent's, then this tree's, alternating -- and a process measures its variants one
after another: `parent` (fit only; diagonal solve), and `fit` / `fit_info` / `solve` / `solve6` here.  Per figure the file holds the
repeats' values with their median, minimum and maximum.  `fit` and `solve` compute what the parent computes; `inside_parent_spread`
says per figure whether their median lies inside the parent's own minimum .. maximum.  No bar is set for `fit_info` and `solve6`.
Prints one JSON line and writes it to --out.
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = {16: (4096, 32768), 64: (16384, 131072)}
DRIVES = 8
IDENT = [0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]


class Events:
    """device time between two events on a stream (hipEventElapsedTime)"""

    def __init__(self, stream):
        self.hip = C.CDLL("libamdhip64.so")
        self.stream = C.c_void_p(stream)
        self.e = [C.c_void_p(), C.c_void_p()]
        for e in self.e:
            assert self.hip.hipEventCreate(C.byref(e)) == 0

    def start(self):
        assert self.hip.hipEventRecord(self.e[0], self.stream) == 0

    def stop_ms(self):
        assert self.hip.hipEventRecord(self.e[1], self.stream) == 0
        assert self.hip.hipEventSynchronize(self.e[1]) == 0
        ms = C.c_float(0)
        assert self.hip.hipEventElapsedTime(C.byref(ms), self.e[0], self.e[1]) == 0
        return float(ms.value)


def worker(a):
    """one process, one library (the package under a.root): every variant's figures as a JSON line"""
    sys.path.insert(0, a.root)
    import lightloam_amd  # noqa: F401
    from lightloam_amd import api, synth
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from bench_posegraph import lap_graph                           # uses the api imported above
    here = a.variants != "parent"
    variants = [("fit", {}), ("fit_info", {"info": True})] if here else [("parent", {})]
    out = {name: {} for name, _ in variants}
    cfgs = [synth.default_cfg(a.rings, seed=101 + 13 * d, speed=6.0 + 1.0 * (d % 5), yaw_rate=0.05 * ((d % 3) - 1)) for d in range(DRIVES)]
    scans = [[synth.scan(c, k) for k in range(a.frames)] for c in cfgs]
    guesses = np.array([[np.array([0.0, 0.0, np.sin(p[2] / 2), np.cos(p[2] / 2), p[0] + 0.05, p[1] - 0.02, 0.01])
                         for p in (synth.pose(c, k) for k in range(a.frames))] for c in cfgs])
    mp = max(len(s) for d in scans for s in d)
    for S in [int(x) for x in a.seqs.split(",")]:
        ctx = api.Context(api.default_params(a.rings, batch=S, max_points=mp))
        cms = api.CubeMaps(ctx, S, *CAP[a.rings], pool_points=a.pool)
        ev = Events(ctx.stream)
        g = guesses[np.arange(S) % DRIVES]
        slots = list(range(S))

        def load(k):
            for q in range(S):
                ctx.upload_scan(q, scans[q % DRIVES][k])
            ctx.extract(0, S); ctx.synchronize()

        for k in range(a.frames):                                   # the maps
            load(k)
            cms.process_slots(g[:, k], slots)
        # ---- ll_cubemaps_localize_slots
        for name, kw in variants:
            load(1)
            cms.localize_slots(g[:, 1], slots, None, **kw)          # warm-up: the variant's first launches
            ms, syncs0 = [], cms.stats()[0]
            for k in range(1, a.frames):
                load(k)
                ev.start()
                res = cms.localize_slots(g[:, k], slots, None, **kw)
                ms.append(ev.stop_ms())
                assert res[1].all()
            out[name][f"localize_S{S}_ms_per_frame"] = float(np.mean(ms))
            out[name][f"localize_S{S}_host_syncs_per_frame"] = (cms.stats()[0] - syncs0) / len(ms)
        # ---- ll_cubemaps_align, on the largest set of maps
        if S >= 2 * DRIVES:
            pairs = [(q, q + DRIVES) for q in range(DRIVES)] + [(q + DRIVES, q) for q in range(DRIVES)]
            for n_ops in [int(x) for x in a.ops.split(",")]:
                ops = [(d, s, IDENT) for d, s in pairs[:n_ops]]
                cms.align(ops, n_outer=2)                           # the workspace grows here, not in the timed calls
                for name, kw in variants:
                    ms = []
                    for _ in range(a.calls):
                        ev.start()
                        res = cms.align(ops, n_outer=2, **kw)
                        ms.append(ev.stop_ms())
                        assert res[1].all()
                    out[name][f"align_{n_ops}_ops_ms_per_call"] = float(np.median(ms))     # a call is a millisecond: one stall of the host is not a figure
                    out[name][f"align_{n_ops}_ops_blocks"] = int(sum(f.n_edge + f.n_plane for f in res[2][:n_ops]))
        cms.close(); ctx.close()
    # ---- ll_posegraphs_solve / _solve6
    ctx = api.Context(api.default_params(16, batch=1, max_points=1024))
    start, edges = lap_graph(a.nodes, 1000)
    pg = ctx.posegraphs(1, a.nodes, len(edges))
    pg.solve([lap_graph(64, 0)])
    for name, e in ([("solve", edges), ("solve6", api.pg_edges6(edges))] if here else [("parent", edges)]):
        key = "solve" if name == "parent" else name
        ms = []
        for _ in range(3):
            x, rec = pg.solve([(start, e)])
            ms.append(pg.timing()["ms"][1])
        out.setdefault(name, {})[f"{key}_{a.nodes}_ms"] = float(np.mean(ms))
        out[name][f"{key}_{a.nodes}_lm_iterations"] = rec[0].lm_iterations
        out[name][f"{key}_{a.nodes}_pcg_iterations"] = rec[0].pcg_iterations
    pg.close(); ctx.close()
    print("RESULT " + json.dumps(out), flush=True)


def summary(values):
    v = [float(x) for x in values]
    return {"values": v, "median": float(np.median(v)), "min": min(v), "max": max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", help="a built checkout of the parent commit")
    ap.add_argument("--rings", type=int, default=64)
    ap.add_argument("--seqs", default="1,16")
    ap.add_argument("--frames", type=int, default=6)
    ap.add_argument("--ops", default="1,4,16")
    ap.add_argument("--nodes", type=int, default=512)
    ap.add_argument("--calls", type=int, default=11, help="timed align calls per variant and process (their median is the process's figure)")
    ap.add_argument("--pool", type=int, default=1 << 19)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "info.json"))
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--root", default=ROOT, help=argparse.SUPPRESS)
    ap.add_argument("--variants", default="here", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    if not a.parent_root or not os.path.exists(os.path.join(a.parent_root, "light-loam_amd", "liblightloam_hip.so")):
        sys.exit("--parent-root must name a built checkout of the parent commit (light-loam_amd/liblightloam_hip.so in it)")
    if a.frames < 3:
        sys.exit("--frames >= 3")
    runs = {}
    for rep in range(a.repeats):
        for root, variants in ((os.path.abspath(a.parent_root), "parent"), (ROOT, "here")):
            env = dict(os.environ); env.pop("LIGHTLOAM_HIP_LIB", None)
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--root", root, "--variants", variants, "--rings", str(a.rings),
                   "--seqs", a.seqs, "--frames", str(a.frames), "--ops", a.ops, "--nodes", str(a.nodes), "--calls", str(a.calls), "--pool", str(a.pool)]
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=root)
            lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not lines:
                sys.exit(f"worker failed ({variants}, repeat {rep}, status {p.returncode}): {p.stdout[-2000:]}{p.stderr[-2000:]}")
            for name, r in json.loads(lines[-1][7:]).items():
                for key, val in r.items():
                    runs.setdefault(name, {}).setdefault(key, []).append(val)
            print(f"# repeat {rep} {variants}: {lines[-1][7:]}", file=sys.stderr, flush=True)
    res = {"tool": "tools/bench_info.py", "rings": a.rings, "seqs": a.seqs, "frames": a.frames, "timed_frames": a.frames - 1, "ops": a.ops,
           "align_calls": a.calls, "n_outer": 2, "nodes": a.nodes, "pool_points": a.pool, "repeats": a.repeats,
           "what": "device ms: two HIP events on the context's stream around the call (localize, align), ll_posegraphs_timing (solve); "
                   "one fresh process per library and repeat, alternating; medians over the repeats",
           "variants": {name: {key: summary(v) for key, v in r.items()} for name, r in runs.items()}}
    V = res["variants"]
    inside, over = {}, {}
    for key in sorted(k for k in V["parent"] if "_ms" in k):
        same = "solve" if key.startswith("solve") else "fit"
        more, more_key = ("solve6", key.replace("solve_", "solve6_")) if same == "solve" else ("fit_info", key)
        inside[key] = V["parent"][key]["min"] <= V[same][key]["median"] <= V["parent"][key]["max"]
        over[more_key] = {"over_" + same: V[more][more_key]["median"] / V[same][key]["median"],
                          "extra_ms": V[more][more_key]["median"] - V[same][key]["median"]}
    res["inside_parent_spread"] = inside
    res["cost_of_the_feature"] = over
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
