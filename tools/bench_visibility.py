"""Visibility: what ll_visibility_run costs per stage, what the filtered rebuild (ll_cubemaps_insert_keyframes_filtered) takes beside
the plain one, and that the plain ll_cubemaps_insert_keyframes did not move against the parent commit's library.

    python tools/bench_visibility.py --parent-root DIR [--rings 64] [--frames 64,512,4096] [--repeats 5] [--out profiles/visibility.json]

DIR is a built checkout of the commit before ll_visibility existed (light-loam_amd/liblightloam_hip.so in it).  Every figure is the
median over `--repeats` FRESH processes, with the minimum and maximum beside it; device times are between HIP events.  The keyframes
are tools/bench_keyframes.py's: `--source-frames` frames of one synthetic `rings`-ring drive, mapped and captured, fill a store of K
keyframes round-robin, frame k under a pose 0.5 m further along a circle of 150 m radius.
  run      one op that lists all K frames under the stored poses, default parameters (max_images = K): one untimed run, one timed.
           Device time per stage (ll_visibility_timing: images, erode, vote), wall time, ordered frame pairs, point-observer
           evaluations (the sum over subject frames of points x observers) and both per second of device time.
  insert   in the same process: the plain rebuild (reset = 1) and the filtered rebuild with the default rule {2, 255}, one untimed and
           one timed each (ll_cubemaps_insert_timing), and what the rule removed.  The synthetic drive has no movers: this says what
           the filter costs, nothing about what it should remove.
  parent   the plain rebuild alone, one process per library and repeat, alternating parent / this tree: device and wall time and the
           SHA-256 of the rebuilt map's LL_MAP_ALL export, which must be the same in both.  `plain_inside_parent_spread` says whether
           this tree's median lies inside the parent's own minimum .. maximum.
Prints one JSON line and writes it to --out.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_keyframes import CAP, circle_pose, summary  # noqa: E402


def make_store(a, api, ctx, scans, guesses):
    """-> clouds of the source frames: [(corner, surf)]"""
    c, s = CAP[a.rings]
    one = api.CubeMaps(ctx, 1, c, s, pool_points=1 << 21)
    src = ctx.keyframes(a.source_frames, a.source_frames * c, a.source_frames * s)
    for k in range(a.source_frames):
        ctx.upload_scan(0, scans[0][k]); ctx.extract(0, 1)
        pose, _ = one.process_slots(guesses[:1, k], [0])
        src.add_cubemaps(one, [1], pose)
    pts, off = src.export()
    src.close(); one.close()
    return [(pts[off[2 * f]:off[2 * f + 1]], pts[off[2 * f + 1]:off[2 * f + 2]]) for f in range(a.source_frames)]


def fill(a, ctx, clouds, K):
    n_pts = [sum(len(clouds[k % a.source_frames][w]) for k in range(K)) for w in (0, 1)]
    kf = ctx.keyframes(K, n_pts[0] + 1, n_pts[1] + 1)
    poses = np.array([circle_pose(k) for k in range(K)])
    for k in range(K):
        kf.add_points(*clouds[k % a.source_frames], poses[k])
    return kf, poses, n_pts


def timed_insert(ctx, cms, kf, K, **kw):
    """one untimed and one timed rebuild of map 0 from all K frames -> (device ms [4], wall ms, the timed call's return)"""
    op = [(0, list(range(K)), None, 1, (10, 10, 5))]
    cms.insert_keyframes(kf, op, **kw); ctx.synchronize()
    t0 = time.perf_counter()
    ret = cms.insert_keyframes(kf, op, **kw)
    wall = 1e3 * (time.perf_counter() - t0)
    return cms.insert_timing()[0], wall, ret


def worker(a):
    sys.path.insert(0, a.root); sys.path.insert(0, os.path.join(a.root, "tools"))
    import lightloam_amd  # noqa: F401
    from lightloam_amd import api
    from bench_mapping_sequences import make_drives
    scans, guesses = make_drives(a.rings, 1, a.source_frames)
    ctx = api.Context(api.default_params(a.rings, batch=1, max_points=max(len(s) for s in scans[0])))
    clouds = make_store(a, api, ctx, scans, guesses)
    c, s = CAP[a.rings]
    out = {}
    for K in [int(x) for x in a.frames.split(",")]:
        kf, poses, n_pts = fill(a, ctx, clouds, K)
        cms = api.CubeMaps(ctx, 1, c, s, pool_points=max(4096, s, max(n_pts) + 1))
        r = {"points": sum(n_pts)}
        ms, wall, _ = timed_insert(ctx, cms, kf, K)
        r.update(plain_device_ms=float(sum(ms)), plain_assign_ms=float(ms[0]), plain_wall_ms=wall,
                 map_sha256=hashlib.sha256(cms.export(api.MAP_ALL)[0].tobytes()).hexdigest())
        if a.worker == "vis":
            vis = ctx.visibility(kf, max_images=K)
            op = [(list(range(K)), None)]
            vis.run(op)                                                                 # untimed
            t0 = time.perf_counter()
            pairs = int(vis.run(op)[0])
            r["run_wall_ms"] = 1e3 * (time.perf_counter() - t0)
            vms, cnt = vis.timing()
            t = poses[:, 4:]
            d2 = sum((t[:, None, k] - t[None, :, k]) ** 2 for k in range(3))            # x, y, z in that order, as the library sums them
            n_obs = (d2 <= 40.0 ** 2).sum(axis=1) - 1
            assert int(n_obs.sum()) == pairs == cnt[2] and cnt[1] == sum(n_pts), (int(n_obs.sum()), pairs, cnt)
            per_frame = np.array([sum(len(clouds[k % a.source_frames][w]) for w in (0, 1)) for k in range(K)])
            r.update(images_ms=vms[0], erode_ms=vms[1], vote_ms=vms[2], run_device_ms=float(sum(vms)), frame_pairs=pairs,
                     evaluations=int((per_frame * n_obs).sum()), image_MB=2 * 4e-6 * K * vis.params.width * vis.params.height)
            fms, fwall, (_, _, removed) = timed_insert(ctx, cms, kf, K, visibility=vis)
            r.update(filtered_device_ms=float(sum(fms)), filtered_assign_ms=float(fms[0]), filtered_wall_ms=fwall, removed=int(removed.sum()))
            vis.close()
        out[str(K)] = r
        cms.close(); kf.close()
    ctx.close()
    print("RESULT " + json.dumps(out), flush=True)


def run_worker(a, root, kind, rep):
    env = dict(os.environ); env.pop("LIGHTLOAM_HIP_LIB", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", kind, "--root", root, "--rings", str(a.rings), "--frames", a.frames,
           "--source-frames", str(a.source_frames)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=root)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    if p.returncode != 0 or not lines:
        sys.exit(f"worker failed ({kind} in {root}, repeat {rep}): {p.stdout[-2000:]}{p.stderr[-2000:]}")
    print(f"# repeat {rep} {kind} {root}: {lines[-1][7:]}", file=sys.stderr, flush=True)
    return json.loads(lines[-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", help="a built checkout of the parent commit")
    ap.add_argument("--rings", type=int, default=64)
    ap.add_argument("--frames", default="64,512,4096")
    ap.add_argument("--source-frames", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "visibility.json"))
    ap.add_argument("--worker", default="", help=argparse.SUPPRESS)
    ap.add_argument("--root", default=ROOT, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    if not a.parent_root or not os.path.exists(os.path.join(a.parent_root, "light-loam_amd", "liblightloam_hip.so")):
        sys.exit("--parent-root must name a built checkout of the parent commit (light-loam_amd/liblightloam_hip.so in it)")
    got = {"vis": {}, "parent": {}, "here": {}}
    for rep in range(a.repeats):
        for name, root, kind in (("vis", ROOT, "vis"), ("parent", os.path.abspath(a.parent_root), "plain"), ("here", ROOT, "plain")):
            for K, r in run_worker(a, root, kind, rep).items():
                for key, val in r.items():
                    got[name].setdefault(K, {}).setdefault(key, []).append(val)
    res = {"tool": "tools/bench_visibility.py", "rings": a.rings, "source_frames": a.source_frames, "repeats": a.repeats,
           "what": "medians over fresh processes; device ms between HIP events; parent / here: one process per library and repeat, alternating",
           "run": {}, "plain_insert": {}}
    for K, r in got["vis"].items():
        sha = set(r.pop("map_sha256"))
        e = {key: summary(v) for key, v in r.items()}
        e["frame_pairs_per_s_device"] = e["frame_pairs"]["median"] / (e["run_device_ms"]["median"] * 1e-3)
        e["evaluations_per_s_device"] = e["evaluations"]["median"] / (e["run_device_ms"]["median"] * 1e-3)
        e["evaluations_per_s_vote"] = e["evaluations"]["median"] / (e["vote_ms"]["median"] * 1e-3)
        e["filtered_over_plain_device"] = e["filtered_device_ms"]["median"] / e["plain_device_ms"]["median"]
        res["run"][K] = e
        shas = sha | set(got["parent"][K]["map_sha256"]) | set(got["here"][K]["map_sha256"])
        par, here = summary(got["parent"][K]["plain_device_ms"]), summary(got["here"][K]["plain_device_ms"])
        res["plain_insert"][K] = {"parent_device_ms": par, "here_device_ms": here, "parent_wall_ms": summary(got["parent"][K]["plain_wall_ms"]),
                                  "here_wall_ms": summary(got["here"][K]["plain_wall_ms"]), "maps_byte_identical": len(shas) == 1,
                                  "plain_inside_parent_spread": par["min"] <= here["median"] <= par["max"],
                                  "plain_not_above_parent_max": here["median"] <= par["max"]}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not all(v["maps_byte_identical"] for v in res["plain_insert"].values()):
        sys.exit("the plain insert's maps differ between the parent's library and this tree")


if __name__ == "__main__":
    main()
