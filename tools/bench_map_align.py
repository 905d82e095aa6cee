"""Map alignment (ll_cubemaps_align) against the only route there was before it, on the same maps in the same run.

    python tools/bench_map_align.py [--rings 64] [--frames 200] [--ops 1,4,16] [--n-outer 2] [--out profiles/map_align.json]

One map is built by running `--frames` frames of one synthetic drive through ll_cubemaps_process_slots; its LL_MAP_ALL export and
layout are then imported into every map of an ll_cubemaps with n_ops + 1 maps.  Op i registers map n_ops (the shared source) to
map i from its own guess, a few decimetres and half a degree off the identity that is the truth between two copies of one map.
  align      ll_cubemaps_align of all ops in one call: `--warmup` untimed calls, `--repeats` timed ones.  Wall time per call (it
             ends in its one synchronisation), the library's device time per stage (ll_cubemaps_align_timing: build, search +
             fit, evaluate + solve, fit record; events), stack_points_per_s_device = stack points x n_outer over the whole
             call's device time (build and fit record included: a rate of the call, not of a kernel), synchronisations per call.
  host       the route without it: export both maps, split them by type on the host, an ll_map created with capacities for them,
             ll_map_set_map, ll_map_set_scan, ll_map_optimize -- one pair at a time.  `--host-repeats` timed passes over all ops.
The poses of the two routes are compared first, at 1e-7 per component.  Prints one JSON line and writes it to --out.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import lightloam_amd  # noqa: E402,F401
from lightloam_amd import api  # noqa: E402
from bench_mapping_sequences import CAP, make_drives  # noqa: E402

N = 21 * 21 * 11
POSE_TOL = 1e-7


def by_type(pts, counts):
    """an LL_MAP_ALL cloud (per cube corner then surf) -> [corner, surf], each in cube order"""
    out, at = ([], []), 0
    for c in np.nonzero(counts.sum(0))[0]:
        for w in (0, 1):
            n = int(counts[w, c])
            out[w].append(pts[at:at + n]); at += n
    return [np.concatenate(o) if o else np.zeros((0, 4), np.float32) for o in out]


def host_route(ctx, cms, ops, n_outer):
    """export, split, ll_map with the maps' capacities, set_map, set_scan, optimize: per op"""
    poses = []
    for dst, src, T0 in ops:
        which = np.full(cms.n_seq, api.MAP_NONE, np.int32); which[dst] = which[src] = api.MAP_ALL
        pts, off = cms.export(which)
        mp = by_type(pts[off[dst]:off[dst + 1]], cms.layout(dst)[1])
        stk = by_type(pts[off[src]:off[src + 1]], cms.layout(src)[1])
        m = api.Map(ctx, len(mp[0]) + 8, len(mp[1]) + 8, len(stk[0]) + 8, len(stk[1]) + 8)
        m.set_map(mp[0], mp[1]); m.set_scan(stk[0], stk[1])
        pose, ran = m.optimize(T0, n_outer)
        assert ran
        poses.append(pose)
        m.close()
    return np.array(poses)


def med(x):
    return float(np.median(x))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rings", type=int, default=64)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--ops", default="1,4,16")
    ap.add_argument("--n-outer", type=int, default=2)
    ap.add_argument("--pool", type=int, default=1 << 21)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--host-repeats", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_align.json"))
    a = ap.parse_args()
    api.load_library()
    scans, guesses = make_drives(a.rings, 1, a.frames)
    ctx = api.Context(api.default_params(a.rings, batch=1, max_points=max(len(s) for s in scans[0])))
    one = api.CubeMaps(ctx, 1, *CAP[a.rings], pool_points=a.pool)
    for k in range(a.frames):
        ctx.upload_scan(0, scans[0][k]); ctx.extract(0, 1)
        one.process_slots(guesses[:1, k], [0])
    pts, off = one.export(api.MAP_ALL)
    lay = one.layout(0)
    one.close()
    res = {"tool": "tools/bench_map_align.py", "rings": a.rings, "frames": a.frames, "n_outer": a.n_outer, "pool_points": a.pool,
           "warmup": a.warmup, "repeats": a.repeats, "map_points": int(len(pts)), "map_corner_points": int(lay[1][0].sum()),
           "map_surf_points": int(lay[1][1].sum()), "map_cubes": int((lay[1].sum(0) > 0).sum()), "pose_tolerance": POSE_TOL, "by_ops": {}}
    for n_ops in [int(x) for x in a.ops.split(",")]:
        S = n_ops + 1
        cms = api.CubeMaps(ctx, S, *CAP[a.rings], pool_points=a.pool)
        cms.import_maps(np.concatenate([pts] * S), np.arange(S + 1, dtype=np.int64) * len(pts), [lay] * S)
        ops = []
        for i in range(n_ops):
            yaw = np.deg2rad(0.5 - 0.05 * i) / 2
            ops.append((i, n_ops, np.array([0.0, 0.0, np.sin(yaw), np.cos(yaw), 0.25 - 0.02 * i, -0.2 + 0.02 * i, 0.05])))
        # correctness first: both routes give the same poses
        T, ran, fit = cms.align(ops, n_outer=a.n_outer)
        ref = host_route(ctx, cms, ops, a.n_outer)
        diff = float(np.abs(T - ref).max())
        assert ran.all() and diff < POSE_TOL, f"the two routes differ by {diff}"
        wall, stage, syncs = [], [], []
        for rep in range(a.warmup + a.repeats):
            ctx.synchronize()
            s0 = cms.stats()[0]
            t0 = time.perf_counter()
            cms.align(ops, n_outer=a.n_outer)
            t = 1e3 * (time.perf_counter() - t0)
            if rep >= a.warmup:
                wall.append(t); stage.append(cms.align_timing()[0]); syncs.append(cms.stats()[0] - s0)
        cnt = cms.align_timing()[1]
        stage = np.array(stage)
        dev_ms = med(stage.sum(1))
        host = []
        for _ in range(a.host_repeats):
            ctx.synchronize()
            t0 = time.perf_counter()
            host_route(ctx, cms, ops, a.n_outer)
            host.append(1e3 * (time.perf_counter() - t0))
        r = {"maps": S, "stack_points": cnt[0], "map_points": cnt[1], "blocks_at_the_end": cnt[2], "max_pose_difference": diff,
             "rms_plane_m": [float(np.sqrt(f.sq_plane / max(f.n_plane, 1))) for f in fit][:n_ops],
             "align": {"wall_ms": med(wall), "wall_ms_min": min(wall), "wall_ms_max": max(wall), "build_ms": med(stage[:, 0]),
                       "search_fit_ms": med(stage[:, 1]), "evaluate_solve_ms": med(stage[:, 2]), "fit_record_ms": med(stage[:, 3]), "device_ms": dev_ms,
                       "stack_points_per_s_device": cnt[0] * a.n_outer / (dev_ms * 1e-3) if dev_ms > 0 else None, "host_syncs_per_call": med(syncs)},
             "host": {"wall_ms": med(host), "wall_ms_min": min(host), "wall_ms_max": max(host), "repeats": a.host_repeats},
             "host_over_align": med(host) / med(wall)}
        res["by_ops"][str(n_ops)] = r
        print(f"# ops {n_ops}: {r}", file=sys.stderr, flush=True)
        cms.close()
    ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
