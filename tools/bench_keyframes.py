"""Keyframes: what a map rebuild (ll_cubemaps_insert_keyframes) takes beside the same rebuild through the host, and what capturing
keyframes costs an ll_drives step beside the parent commit's library.

    python tools/bench_keyframes.py --parent-root DIR [--rings 64] [--frames 64,512,4096] [--lanes 16] [--steps 8] [--repeats 5]
                                    [--host-max-frames 512] [--out profiles/keyframes.json]

DIR is a built checkout of the commit before ll_keyframes existed (light-loam_amd/liblightloam_hip.so in it).  Every figure is the
median over `--repeats` FRESH processes, with the minimum and maximum beside it; device times are between HIP events.
  insert   `--source-frames` frames of one synthetic `rings`-ring drive are mapped and captured (ll_keyframes_add_cubemaps); their
           clouds, exported once, fill a store of K keyframes round-robin (ll_keyframes_add_points), frame k under a pose 0.5 m
           further along a circle of 150 m radius.  One map is rebuilt from all K (reset = 1; above 2^25 points of a type split over
           calls of at most that many, the later ones with reset = 0): one untimed rebuild, one timed.
           The library's device time per stage (ll_cubemaps_insert_timing: assign, sort + gather, filter, commit), wall time, source
           points per second, synchronisations.  The assign stage moves 16 B in and 20 B out per point; its rate is set beside the
           copy rate of profiles/r05_stream_rate.json (flat copy, the best of its rows).
  host     for K <= --host-max-frames the same rebuild without it: ll_keyframes_export, pointAssociateToMap and the cube arithmetic
           in numpy (the library's f64 operation order), ll_voxel_grid per touched cube, the layout by hand, ll_cubemaps_import.  Its
           bytes are compared with the insert's before it is timed.
  capture  ll_drives_step of `lanes` mapping lanes, the scans uploaded beforehand: step 0 starts the lanes, step 1 warms up, steps
           2 .. `steps` - 1 are timed between two events on the stream.  Variants: `parent` (the parent's library, which has no
           store), `off` (this tree, no store set), `on` (every = 1).  Processes alternate parent / this tree.  `off` computes what the
           parent computes: `off_inside_parent_spread` says whether its median lies inside the parent's own minimum .. maximum.
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
W, H, D = 21, 21, 11
N = W * H * D
LEAF = (0.4, 0.8)
CAP = {16: (4096, 32768), 64: (16384, 131072)}
PERIOD = 0.1


def circle_pose(k, radius=150.0, step=0.5):
    a = k * step / radius
    return np.array([0.0, 0.0, np.sin(a / 2), np.cos(a / 2), radius * np.sin(a), radius * (1.0 - np.cos(a)), 0.0])


def host_rebuild(ctx, cms, kf, poses, associate, cubes_of):
    """export, transform and bin on the host, ll_voxel_grid per touched cube, the layout by hand, import -> voxel grid calls"""
    pts, off = kf.export()
    counts = np.zeros((2, N), np.int32)
    clouds, calls = {}, 0
    for w in (0, 1):
        tp = np.concatenate([associate(poses[f], pts[off[2 * f + w]:off[2 * f + w + 1]]) for f in range(len(poses))])
        c = cubes_of(tp, (10, 10, 5))
        order = np.argsort(c, kind="stable")
        cs, first, n = np.unique(c[order], return_index=True, return_counts=True)
        for cube, f, k in zip(cs, first, n):
            if cube < 0:
                continue
            clouds[(w, int(cube))] = ctx.voxel_grid(tp[order[f:f + k]], LEAF[w]); calls += 1
            counts[w, cube] = len(clouds[(w, int(cube))])
    parts = [clouds[(w, c)] for c in range(N) for w in (0, 1) if (w, c) in clouds]
    allpts = np.concatenate(parts)
    cms.import_maps(allpts, [0, len(allpts)], [(np.array([10, 10, 5], np.int32), counts, np.zeros(0, np.int32))])
    return calls


def insert_worker(a):
    sys.path.insert(0, a.root); sys.path.insert(0, os.path.join(a.root, "tools"))
    import lightloam_amd  # noqa: F401
    from lightloam_amd import api
    from bench_map_merge import associate, cubes_of
    from bench_mapping_sequences import make_drives
    scans, guesses = make_drives(a.rings, 1, a.source_frames)
    ctx = api.Context(api.default_params(a.rings, batch=1, max_points=max(len(s) for s in scans[0])))
    c, s = CAP[a.rings]
    one = api.CubeMaps(ctx, 1, c, s, pool_points=1 << 21)
    src = ctx.keyframes(a.source_frames, a.source_frames * c, a.source_frames * s)
    for k in range(a.source_frames):
        ctx.upload_scan(0, scans[0][k]); ctx.extract(0, 1)
        pose, _ = one.process_slots(guesses[:1, k], [0])
        src.add_cubemaps(one, [1], pose)
    pts, off = src.export()
    src.close(); one.close()
    clouds = [(pts[off[2 * f]:off[2 * f + 1]], pts[off[2 * f + 1]:off[2 * f + 2]]) for f in range(a.source_frames)]
    out = {}
    for K in [int(x) for x in a.frames.split(",")]:
        n_pts = [sum(len(clouds[k % a.source_frames][w]) for k in range(K)) for w in (0, 1)]
        kf = ctx.keyframes(K, n_pts[0] + 1, n_pts[1] + 1)
        poses = [circle_pose(k) for k in range(K)]
        for k in range(K):
            kf.add_points(*clouds[k % a.source_frames], poses[k])
        # a pool holds at most 2^26 points of a type: a larger rebuild is split over calls (reset = 1, then reset = 0) of at most 2^25
        # points of a type each, as a caller would split it
        per = [max(len(clouds[k % a.source_frames][w]) for w in (0, 1)) for k in range(K)]
        calls, at = [], 0
        while at < K:
            end, room = at, 1 << 25
            while end < K and (end == at or per[end] <= room):
                room -= per[end]; end += 1
            calls.append((0, list(range(at, end)), None, int(at == 0), (10, 10, 5)))
            at = end
        pool = max(4096, s, max(n_pts) + 1) if len(calls) == 1 else 1 << 26
        cms = api.CubeMaps(ctx, 1, c, s, pool_points=pool)

        def rebuild():
            ms, cnt, dropped = np.zeros(4), np.zeros(3, np.int64), 0
            for op in calls:
                dropped += int(cms.insert_keyframes(kf, [op])[1].sum())
                m, n = cms.insert_timing()
                ms += m; cnt += n
            return ms, cnt, dropped

        rebuild(); ctx.synchronize()                                                # untimed
        s0 = cms.stats()[0]
        t0 = time.perf_counter()
        ms, cnt, dropped = rebuild()
        wall = 1e3 * (time.perf_counter() - t0)
        r = {"calls": len(calls), "points_in": int(cnt[0]), "corner_points_in": n_pts[0], "surf_points_in": n_pts[1], "touched_cubes": int(cnt[1]),
             "points_out": int(cnt[2]), "dropped": dropped, "wall_ms": wall, "assign_ms": ms[0], "sort_gather_ms": ms[1], "filter_ms": ms[2],
             "commit_ms": ms[3], "device_ms": float(sum(ms)), "host_syncs": cms.stats()[0] - s0, "store_MB": 16e-6 * sum(n_pts)}
        if K <= a.host_max_frames and len(calls) == 1:
            ref = cms.export(api.MAP_ALL)[0].tobytes()
            host_rebuild(ctx, cms, kf, poses, associate, cubes_of)
            assert cms.export(api.MAP_ALL)[0].tobytes() == ref, "the insert and the host leg differ"
            t0 = time.perf_counter()
            r["host_voxel_grid_calls"] = host_rebuild(ctx, cms, kf, poses, associate, cubes_of)
            r["host_wall_ms"] = 1e3 * (time.perf_counter() - t0)
        out[str(K)] = r
        cms.close(); kf.close()
    ctx.close()
    print("RESULT " + json.dumps(out), flush=True)


def capture_worker(a):
    sys.path.insert(0, a.root); sys.path.insert(0, os.path.join(a.root, "tools"))
    import lightloam_amd  # noqa: F401
    from lightloam_amd import api, synth
    from bench_deskew import Events
    S, Dn = a.lanes, 4
    cfgs = [synth.default_cfg(a.rings, seed=101 + 13 * d, speed=6.0 + 1.0 * (d % 5), yaw_rate=0.05 * ((d % 3) - 1)) for d in range(Dn)]
    dscans = [[synth.scan(c, k) for k in range(a.steps)] for c in cfgs]
    p0 = np.array([[0, 0, 0, 1.0, cfgs[q % Dn].speed * PERIOD, 0.0, 0.0] for q in range(S)])
    out = {}
    for name in (["parent"] if a.variants == "parent" else ["off", "on"]):
        ctx = api.Context(api.default_params(a.rings, batch=2 * S, max_points=max(len(s) for d in dscans for s in d)))
        dr = api.Drives(ctx, S, *CAP[a.rings], pool_points=1 << 19)
        kf = None
        if name == "on":
            kf = ctx.keyframes(S * a.steps, S * a.steps * CAP[a.rings][0], S * a.steps * CAP[a.rings][1])
            dr.set_keyframes(kf, 1)
        ev = Events(ctx.stream)
        ms, s_before = [], 0
        for k in range(a.steps):
            slots = dr.slots()
            for q in range(S):
                ctx.upload_scan(int(slots[q]), dscans[q % Dn][k])
            ctx.synchronize()
            if k == 2:
                s_before = dr.stats()[0]
            ev.start()
            dr.step(np.full(S, api.RUN if k else api.START, np.int32), p0)
            t = ev.stop_ms()
            if k >= 2:
                ms.append(t)
        out[name] = {"drives_ms_per_step": float(np.mean(ms)), "drives_host_syncs_per_step": (dr.stats()[0] - s_before) / len(ms)}
        if kf is not None:
            out[name]["keyframes"] = len(kf)
            out[name]["points_per_keyframe"] = float(np.mean([sum(kf.info(i)["n"]) for i in range(len(kf))]))
        dr.close(); ctx.close()
    print("RESULT " + json.dumps(out), flush=True)


def summary(values):
    v = [float(x) for x in values]
    return {"values": v, "median": float(np.median(v)), "min": min(v), "max": max(v)}


def run_worker(a, root, kind, variants, rep):
    env = dict(os.environ); env.pop("LIGHTLOAM_HIP_LIB", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", kind, "--root", root, "--variants", variants, "--rings", str(a.rings),
           "--frames", a.frames, "--lanes", str(a.lanes), "--steps", str(a.steps), "--source-frames", str(a.source_frames),
           "--host-max-frames", str(a.host_max_frames)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=root)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    if p.returncode != 0 or not lines:
        sys.exit(f"worker failed ({kind} {variants}, repeat {rep}): {p.stdout[-2000:]}{p.stderr[-2000:]}")
    print(f"# repeat {rep} {kind} {variants}: {lines[-1][7:]}", file=sys.stderr, flush=True)
    return json.loads(lines[-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", help="a built checkout of the parent commit")
    ap.add_argument("--rings", type=int, default=64)
    ap.add_argument("--frames", default="64,512,4096")
    ap.add_argument("--source-frames", type=int, default=8)
    ap.add_argument("--host-max-frames", type=int, default=512)
    ap.add_argument("--lanes", type=int, default=16)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "keyframes.json"))
    ap.add_argument("--worker", default="", help=argparse.SUPPRESS)
    ap.add_argument("--root", default=ROOT, help=argparse.SUPPRESS)
    ap.add_argument("--variants", default="here", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return insert_worker(a) if a.worker == "insert" else capture_worker(a)
    if not a.parent_root or not os.path.exists(os.path.join(a.parent_root, "light-loam_amd", "liblightloam_hip.so")):
        sys.exit("--parent-root must name a built checkout of the parent commit (light-loam_amd/liblightloam_hip.so in it)")
    if a.steps < 4:
        sys.exit("--steps >= 4")
    ins, cap = {}, {}
    for rep in range(a.repeats):
        for K, r in run_worker(a, ROOT, "insert", "here", rep).items():
            for key, val in r.items():
                ins.setdefault(K, {}).setdefault(key, []).append(val)
        for root, variants in ((os.path.abspath(a.parent_root), "parent"), (ROOT, "here")):
            for name, r in run_worker(a, root, "capture", variants, rep).items():
                for key, val in r.items():
                    cap.setdefault(name, {}).setdefault(key, []).append(val)
    with open(os.path.join(ROOT, "profiles", "r05_stream_rate.json")) as f:
        copy_GBps = max(r["GBps"] for r in json.load(f)["stream_rate"]["results"] if r["pattern"] == "flat" and r["mode"] == "copy")
    res = {"tool": "tools/bench_keyframes.py", "rings": a.rings, "source_frames": a.source_frames, "lanes": a.lanes, "steps": a.steps,
           "timed_steps": a.steps - 2, "repeats": a.repeats,
           "what": "medians over fresh processes; device ms between HIP events; capture: one process per library and repeat, alternating",
           "stream_copy_GBps": copy_GBps, "insert": {}, "capture": {name: {key: summary(v) for key, v in r.items()} for name, r in cap.items()}}
    for K, r in ins.items():
        e = {key: summary(v) for key, v in r.items()}
        pts = e["points_in"]["median"]
        e["points_per_s_device"] = pts / (e["device_ms"]["median"] * 1e-3)
        e["points_per_s_wall"] = pts / (e["wall_ms"]["median"] * 1e-3)
        e["assign_GBps"] = 36.0 * pts / (e["assign_ms"]["median"] * 1e-3) / 1e9         # 16 B read, 16 + 4 B written per point
        e["assign_fraction_of_copy_rate"] = e["assign_GBps"] / copy_GBps
        if "host_wall_ms" in e:
            e["host_over_insert"] = e["host_wall_ms"]["median"] / e["wall_ms"]["median"]
        res["insert"][K] = e
    par, off, on = (res["capture"][n]["drives_ms_per_step"] for n in ("parent", "off", "on"))
    res["off_inside_parent_spread"] = par["min"] <= off["median"] <= par["max"]
    res["capture_on_over_off"] = on["median"] / off["median"]
    res["capture_ms_per_step"] = on["median"] - off["median"]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
