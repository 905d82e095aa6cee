"""What TransformToEnd (ll_set_deskew) costs the frame loops, beside the same loops of the parent commit in the same session.

    python tools/bench_deskew.py --parent-root DIR [--rings 64] [--frames 32] [--lanes 16] [--steps 8] [--repeats 5] [--out profiles/deskew.json]

DIR is a built checkout of the commit before ll_set_deskew existed (git worktree add DIR <commit>; python DIR/__graft_entry__.py).
Two figures, both DEVICE time between two HIP events on the context's stream, with distortion = 1 everywhere:
  frames   ll_odometry_frames over `frames` - 1 frames of one `rings`-ring drive (extracted beforehand, the carry set from slot 0),
           per frame;
  drives   ll_drives_step of `lanes` lanes (mapping, registered clouds kept), the scans uploaded beforehand, per step: step 0
           starts the lanes, step 1 warms up, steps 2 .. `steps` - 1 are timed.  A step holds the cube-map frame's host
           synchronisations, so this is the time the stream was busy or waiting for the host between the two events.
Every repeat is a fresh process per library -- the parent's, then this tree's, alternating -- and a process measures its variants
one after another after one untimed pass each: `parent` (the parent has no switch), and modes 0, 1, 2 here.  Per variant the file
holds the repeats' values with their median, minimum and maximum.  Mode 0 computes what the parent computes, so its median has to
lie inside the parent's own minimum .. maximum over the repeats: `mode0_inside_parent_spread`, and the exit status, say whether it
does.  Modes 1 and 2 are reported as they come.  Prints one JSON line and writes it to --out.
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
    """one process, one library (the package under a.root): every variant's two figures as a JSON line"""
    sys.path.insert(0, a.root)
    import lightloam_amd  # noqa: F401
    from lightloam_amd import api, synth
    variants = [("parent", None)] if a.variants == "parent" else [(f"mode{m}", m) for m in (0, 1, 2)]
    out = {}
    # ---- ll_odometry_frames
    cfg = synth.default_cfg(a.rings, seed=101, speed=8.0, yaw_rate=0.05)
    scans = [synth.scan(cfg, k) for k in range(a.frames)]
    pose0 = np.array([0, 0, 0, 1.0, cfg.speed * PERIOD, 0.0, 0.0])
    ctx = api.Context(api.default_params(a.rings, batch=a.frames, max_points=max(map(len, scans)), distortion=1))
    ev = Events(ctx.stream)
    for k, s in enumerate(scans):
        ctx.upload_scan(k, s)
    for name, mode in variants:
        if mode is not None:
            ctx.set_deskew(mode)
        ms = []
        for rep in range(2):                                   # an untimed pass, then the timed one; the slots extracted anew for each
            ctx.extract(0, a.frames); ctx.set_target_from_slot(0); ctx.synchronize()
            ev.start()
            rel = ctx.odometry_frames(1, a.frames - 1, pose0=pose0, n_outer=3, first_frame_index=1)
            ms.append(ev.stop_ms())
        assert np.isfinite(rel).all()
        out[name] = {"frames_ms_per_frame": ms[-1] / (a.frames - 1)}
    ctx.close()
    # ---- ll_drives
    S, D = a.lanes, 4
    cfgs = [synth.default_cfg(a.rings, seed=101 + 13 * d, speed=6.0 + 1.0 * (d % 5), yaw_rate=0.05 * ((d % 3) - 1)) for d in range(D)]
    dscans = [[synth.scan(c, k) for k in range(a.steps)] for c in cfgs]
    p0 = np.array([[0, 0, 0, 1.0, cfgs[q % D].speed * PERIOD, 0.0, 0.0] for q in range(S)])
    for name, mode in variants:
        ctx = api.Context(api.default_params(a.rings, batch=2 * S, max_points=max(len(s) for d in dscans for s in d), distortion=1))
        if mode is not None:
            ctx.set_deskew(mode)
        dr = api.Drives(ctx, S, *CAP[a.rings], pool_points=1 << 19, keep_registered=True)
        ev = Events(ctx.stream)
        ms = []
        s_before = 0
        for k in range(a.steps):
            slots = dr.slots()
            for q in range(S):
                ctx.upload_scan(int(slots[q]), dscans[q % D][k])
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
    print("RESULT " + json.dumps(out), flush=True)


def summary(values):
    v = [float(x) for x in values]
    return {"values": v, "median": float(np.median(v)), "min": min(v), "max": max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", help="a built checkout of the parent commit")
    ap.add_argument("--rings", type=int, default=64)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--lanes", type=int, default=16)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deskew.json"))
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--root", default=ROOT, help=argparse.SUPPRESS)
    ap.add_argument("--variants", default="modes", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    if not a.parent_root or not os.path.exists(os.path.join(a.parent_root, "light-loam_amd", "liblightloam_hip.so")):
        sys.exit("--parent-root must name a built checkout of the parent commit (light-loam_amd/liblightloam_hip.so in it)")
    if a.steps < 4 or a.frames < 3:
        sys.exit("--steps >= 4 and --frames >= 3")
    runs = {}
    for rep in range(a.repeats):
        for root, variants in ((os.path.abspath(a.parent_root), "parent"), (ROOT, "modes")):
            env = dict(os.environ); env.pop("LIGHTLOAM_HIP_LIB", None)
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--root", root, "--variants", variants, "--rings", str(a.rings),
                   "--frames", str(a.frames), "--lanes", str(a.lanes), "--steps", str(a.steps)]
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=root)
            lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not lines:
                sys.exit(f"worker failed ({variants}, repeat {rep}): {p.stdout[-2000:]}{p.stderr[-2000:]}")
            for name, r in json.loads(lines[-1][7:]).items():
                for key, val in r.items():
                    runs.setdefault(name, {}).setdefault(key, []).append(val)
            print(f"# repeat {rep} {variants}: {lines[-1][7:]}", file=sys.stderr, flush=True)
    res = {"tool": "tools/bench_deskew.py", "rings": a.rings, "frames": a.frames, "lanes": a.lanes, "steps": a.steps,
           "timed_steps": a.steps - 2, "repeats": a.repeats, "distortion": 1,
           "what": "device ms between two HIP events on the context's stream; one fresh process per library and repeat, alternating",
           "variants": {name: {key: summary(v) for key, v in r.items()} for name, r in runs.items()}}
    inside = {}
    for key in ("frames_ms_per_frame", "drives_ms_per_step"):
        par, m0 = res["variants"]["parent"][key], res["variants"]["mode0"][key]
        inside[key] = par["min"] <= m0["median"] <= par["max"]
        for m in ("mode1", "mode2"):
            res["variants"][m][key]["over_parent_median"] = res["variants"][m][key]["median"] / par["median"]
    res["mode0_inside_parent_spread"] = inside
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not all(inside.values()):
        sys.exit("mode 0 lies outside the parent's own spread: " + json.dumps(inside))


if __name__ == "__main__":
    main()
