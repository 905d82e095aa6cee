"""What the mapping vote (ll_cubemaps_set_vote / ll_drives_set_map_vote) costs a frame, beside the same frames of the parent commit in
the same session.

    python tools/bench_map_vote.py --parent-root DIR [--rings 64] [--seqs 1,16] [--frames 8] [--lanes 16] [--steps 8] [--repeats 5]
                                   [--out profiles/map_vote.json]

DIR is a built checkout of the commit before ll_map_set_vote existed (git worktree add DIR <commit>; python DIR/__graft_entry__.py).
All figures are DEVICE time between two HIP events on the context's stream, on the workload of tools/bench_mapping_sequences.py
(sequence q replays synthetic drive q % 8):
  cubemaps  one ll_cubemaps_process_slots call per frame for S = 1 and 16 sequences, the scans uploaded and extracted beforehand;
            frame 0 (an empty map: the :1822 gate skips the solve) warms up, frames 1 .. `frames` - 1 are timed, per frame;
  drives    ll_drives_step of `lanes` lanes (mapping), the scans uploaded beforehand, per step: step 0 starts the lanes, step 1
            warms up, steps 2 .. `steps` - 1 are timed.
A frame holds the cube-map frame's host synchronisations, so this is the time the stream was busy or waiting for the host between
the two events.  Every repeat is a fresh process per library -- the parent's, then this tree's, alternating -- and a process
measures its variants one after another: `parent` (the parent has no switch), and `off` / `on` here (`on`: every sequence votes in
every frame; the drives vote from frame 1 on, from_frame = 0).  Per variant the file holds the repeats' values with their median,
minimum and maximum, the host synchronisations per frame, and with the vote on the share of the plane blocks it kept.  `off`
computes what the parent computes, so its median has to lie inside the parent's own minimum .. maximum over the repeats:
`off_inside_parent_spread`, and the exit status, say whether it does.  `on` is reported as it comes: no bar is set for it.
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
PERIOD = 0.1
DRIVES = 8


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
    variants = [("parent", None)] if a.variants == "parent" else [("off", 0), ("on", 1)]
    out = {name: {} for name, _ in variants}
    cfgs = [synth.default_cfg(a.rings, seed=101 + 13 * d, speed=6.0 + 1.0 * (d % 5), yaw_rate=0.05 * ((d % 3) - 1)) for d in range(DRIVES)]
    F = max(a.frames, a.steps)
    scans = [[synth.scan(c, k) for k in range(F)] for c in cfgs]
    guesses = np.array([[np.array([0.0, 0.0, np.sin(p[2] / 2), np.cos(p[2] / 2), p[0] + 0.05, p[1] - 0.02, 0.01])
                         for p in (synth.pose(c, k) for k in range(F))] for c in cfgs])
    mp = max(len(s) for d in scans for s in d)
    # ---- ll_cubemaps_process_slots
    for S in [int(x) for x in a.seqs.split(",")]:
        for name, vote in variants:
            ctx = api.Context(api.default_params(a.rings, batch=S, max_points=mp))
            cms = api.CubeMaps(ctx, S, *CAP[a.rings], pool_points=a.pool)
            if vote:
                cms.set_vote([1] * S)
            ev = Events(ctx.stream)
            g = guesses[np.arange(S) % DRIVES]
            ms, kept, cand, syncs0 = [], 0, 0, 0
            for k in range(a.frames):
                for q in range(S):
                    ctx.upload_scan(q, scans[q % DRIVES][k])
                ctx.extract(0, S); ctx.synchronize()
                if k == 1:
                    syncs0 = cms.stats()[0]
                ev.start()
                _, ran = cms.process_slots(g[:, k], list(range(S)))
                t = ev.stop_ms()
                if k:
                    ms.append(t)
                    assert ran.all()
            out[name][f"cubemaps_S{S}_ms_per_frame"] = float(np.mean(ms))
            out[name][f"cubemaps_S{S}_host_syncs_per_frame"] = (cms.stats()[0] - syncs0) / len(ms)
            cms.close(); ctx.close()
    # ---- ll_drives
    S = a.lanes
    p0 = np.array([[0, 0, 0, 1.0, cfgs[q % DRIVES].speed * PERIOD, 0.0, 0.0] for q in range(S)])
    for name, vote in variants:
        ctx = api.Context(api.default_params(a.rings, batch=2 * S, max_points=mp))
        dr = api.Drives(ctx, S, *CAP[a.rings], pool_points=a.pool)
        if vote:
            dr.set_map_vote(0)
        ev = Events(ctx.stream)
        ms, s_before = [], 0
        for k in range(a.steps):
            slots = dr.slots()
            for q in range(S):
                ctx.upload_scan(int(slots[q]), scans[q % DRIVES][k])
            ctx.synchronize()
            if k == 2:
                s_before = dr.stats()[0]
            ev.start()
            dr.step(np.full(S, api.RUN if k else api.START, np.int32), p0)
            t = ev.stop_ms()
            if k >= 2:
                ms.append(t)
        out[name]["drives_ms_per_step"] = float(np.mean(ms))
        out[name]["drives_host_syncs_per_step"] = (dr.stats()[0] - s_before) / len(ms)
        dr.close(); ctx.close()
    # ---- what the vote keeps on this workload (one sequence, the last timed frame's final association)
    if a.variants != "parent":
        ctx = api.Context(api.default_params(a.rings, batch=1, max_points=mp))
        cm = api.CubeMap(ctx, *CAP[a.rings], pool_points=a.pool)
        cm.set_vote(True)
        kept = cand = 0
        for k in range(a.frames):
            ctx.upload_scan(0, scans[0][k]); ctx.extract(0, 1)
            _, ran = cm.process_slot(guesses[0, k], 0)
            if ran:
                _, _, sel, _ = cm.map().download_vote()
                kept += int(sel.sum()); cand += len(sel)
        out["on"]["plane_blocks_kept_share"] = kept / max(cand, 1)
        out["on"]["plane_blocks_per_frame"] = cand / max(a.frames - 1, 1)
        cm.close(); ctx.close()
    print("RESULT " + json.dumps(out), flush=True)


def summary(values):
    v = [float(x) for x in values]
    return {"values": v, "median": float(np.median(v)), "min": min(v), "max": max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", help="a built checkout of the parent commit")
    ap.add_argument("--rings", type=int, default=64)
    ap.add_argument("--seqs", default="1,16")
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--lanes", type=int, default=16)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--pool", type=int, default=1 << 19)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_vote.json"))
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--root", default=ROOT, help=argparse.SUPPRESS)
    ap.add_argument("--variants", default="here", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    if not a.parent_root or not os.path.exists(os.path.join(a.parent_root, "light-loam_amd", "liblightloam_hip.so")):
        sys.exit("--parent-root must name a built checkout of the parent commit (light-loam_amd/liblightloam_hip.so in it)")
    if a.steps < 4 or a.frames < 3:
        sys.exit("--steps >= 4 and --frames >= 3")
    runs = {}
    for rep in range(a.repeats):
        for root, variants in ((os.path.abspath(a.parent_root), "parent"), (ROOT, "here")):
            env = dict(os.environ); env.pop("LIGHTLOAM_HIP_LIB", None)
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--root", root, "--variants", variants, "--rings", str(a.rings),
                   "--seqs", a.seqs, "--frames", str(a.frames), "--lanes", str(a.lanes), "--steps", str(a.steps), "--pool", str(a.pool)]
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=root)
            lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not lines:
                sys.exit(f"worker failed ({variants}, repeat {rep}): {p.stdout[-2000:]}{p.stderr[-2000:]}")
            for name, r in json.loads(lines[-1][7:]).items():
                for key, val in r.items():
                    runs.setdefault(name, {}).setdefault(key, []).append(val)
            print(f"# repeat {rep} {variants}: {lines[-1][7:]}", file=sys.stderr, flush=True)
    res = {"tool": "tools/bench_map_vote.py", "rings": a.rings, "seqs": a.seqs, "frames": a.frames, "timed_frames": a.frames - 1, "lanes": a.lanes,
           "steps": a.steps, "timed_steps": a.steps - 2, "pool_points": a.pool, "repeats": a.repeats,
           "what": "device ms between two HIP events on the context's stream; one fresh process per library and repeat, alternating",
           "variants": {name: {key: summary(v) for key, v in r.items()} for name, r in runs.items()}}
    inside = {}
    for key in sorted(k for k in res["variants"]["parent"] if "_ms_" in k):
        par, off, on = res["variants"]["parent"][key], res["variants"]["off"][key], res["variants"]["on"][key]
        inside[key] = par["min"] <= off["median"] <= par["max"]
        on["over_parent_median"] = on["median"] / par["median"]
    res["off_inside_parent_spread"] = inside
    if not all(inside.values()):
        res["note"] = "with the vote off a median lies outside the parent's own minimum .. maximum over its repeats: see the values"
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not all(inside.values()):
        sys.exit("the vote off lies outside the parent's own spread: " + json.dumps(inside))


if __name__ == "__main__":
    main()
