"""Map merge (ll_cubemaps_merge) against the same merge done through the host, on the same maps in the same run.

    python tools/bench_map_merge.py [--rings 64] [--frames 200] [--ops 1,4,16] [--out profiles/map_merge.json]

One map is built by running `--frames` frames of one synthetic drive through ll_cubemaps_process_slots; its LL_MAP_ALL export and
layout are then imported into every map of an ll_cubemaps with n_ops + 1 maps, so that each op merges a map of that size (map
n_ops, the shared source) into another map of that size under its own pose.
  merge      ll_cubemaps_merge of all ops in one call: `--warmup` untimed calls, `--repeats` timed ones, the destinations put
             back by an (untimed) import before each.  Wall time per call (it ends in its last synchronisation), the library's
             device time per stage (ll_cubemaps_merge_timing: assign, sort + gather, filter, commit; events), source points
             per second of device time and of wall time, synchronisations per call.
  host       the only way without it: export the maps, pointAssociateToMap and the cube arithmetic in numpy (the library's f64
             operation order), ll_voxel_grid per touched cube (one cloud per call, host in and host out), the layout rebuilt by
             hand, import.  `--host-repeats` timed passes.
The host leg's bytes are compared with the merge's before anything is timed.  Prints one JSON line and writes it to --out.
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

W, H, D = 21, 21, 11
N = W * H * D


def associate(T, p):
    """pointAssociateToMap (laserMapping.cpp:125-134) in k_cm_assign's operation order"""
    ux, uy, uz, w = T[:4]
    v = p[:, :3].astype(np.float64)
    uvx = uy * v[:, 2] - uz * v[:, 1]; uvy = uz * v[:, 0] - ux * v[:, 2]; uvz = ux * v[:, 1] - uy * v[:, 0]
    uvx = uvx + uvx; uvy = uvy + uvy; uvz = uvz + uvz
    x = ((v[:, 0] + w * uvx) + (uy * uvz - uz * uvy)) + T[4]
    y = ((v[:, 1] + w * uvy) + (uz * uvx - ux * uvz)) + T[5]
    z = ((v[:, 2] + w * uvz) + (ux * uvy - uy * uvx)) + T[6]
    return np.stack([x.astype(np.float32), y.astype(np.float32), z.astype(np.float32), p[:, 3]], axis=1)


def cubes_of(p, cen):
    idx = []
    for k in range(3):
        v = p[:, k].astype(np.float64) + 25.0
        c = np.trunc(v / 50.0).astype(np.int64) + int(cen[k])
        c[v < 0] -= 1
        idx.append(c)
    i, j, k = idx
    return np.where((i >= 0) & (i < W) & (j >= 0) & (j < H) & (k >= 0) & (k < D), i + W * j + W * H * k, -1)


def split(pts, counts):
    """an LL_MAP_ALL cloud -> {(w, cube): cloud}"""
    out, at = {}, 0
    for c in np.nonzero(counts.sum(0))[0]:
        for w in (0, 1):
            n = int(counts[w, c])
            if n:
                out[(w, int(c))] = pts[at:at + n]; at += n
    return out


def host_merge(ctx, cms, ops, leaf):
    """export, transform and bin on the host, ll_voxel_grid per touched cube, layout by hand, import"""
    S = cms.n_seq
    pts, off = cms.export(api.MAP_ALL)
    lay = [cms.layout(q) for q in range(S)]
    maps = [split(pts[off[q]:off[q + 1]], lay[q][1]) for q in range(S)]
    calls = 0
    for dst, src, T in ops:
        for w in (0, 1):
            parts = [maps[src][(w, c)] for c in range(N) if (w, c) in maps[src]]
            if not parts:
                continue
            tp = associate(T, np.concatenate(parts))
            c = cubes_of(tp, lay[dst][0])
            order = np.argsort(c, kind="stable")
            cs, first, n = np.unique(c[order], return_index=True, return_counts=True)
            for cube, f, k in zip(cs, first, n):
                if cube < 0:
                    continue
                new = tp[order[f:f + k]]
                old = maps[dst].get((w, int(cube)))
                maps[dst][(w, int(cube))] = ctx.voxel_grid(new if old is None else np.concatenate([old, new]), leaf[w])
                calls += 1
    layouts, clouds, o2 = [], [], np.zeros(S + 1, np.int64)
    dsts = {d for d, _, _ in ops}
    for q in range(S):
        if q not in dsts:
            layouts.append(None); o2[q + 1] = o2[q]
            continue
        counts = np.zeros((2, N), np.int32)
        for (w, c), v in maps[q].items():
            counts[w, c] = len(v)
        part = [maps[q][(w, c)] for c in range(N) for w in (0, 1) if (w, c) in maps[q]]
        clouds += part
        o2[q + 1] = o2[q] + sum(len(v) for v in part)
        layouts.append((lay[q][0], counts, lay[q][2]))
    cms.import_maps(np.concatenate(clouds), o2, layouts)
    return calls


def med(x):
    return float(np.median(x))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rings", type=int, default=64)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--ops", default="1,4,16")
    ap.add_argument("--pool", type=int, default=1 << 21)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--host-repeats", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_merge.json"))
    a = ap.parse_args()
    api.load_library()
    leaf = (0.4, 0.8)
    scans, guesses = make_drives(a.rings, 1, a.frames)
    ctx = api.Context(api.default_params(a.rings, batch=1, max_points=max(len(s) for s in scans[0])))
    one = api.CubeMaps(ctx, 1, *CAP[a.rings], pool_points=a.pool)
    for k in range(a.frames):
        ctx.upload_scan(0, scans[0][k]); ctx.extract(0, 1)
        one.process_slots(guesses[:1, k], [0])
    pts, off = one.export(api.MAP_ALL)
    lay = one.layout(0)
    one.close()
    res = {"tool": "tools/bench_map_merge.py", "rings": a.rings, "frames": a.frames, "pool_points": a.pool, "warmup": a.warmup,
           "repeats": a.repeats, "map_points": int(len(pts)), "map_corner_points": int(lay[1][0].sum()), "map_surf_points": int(lay[1][1].sum()),
           "map_cubes": int((lay[1].sum(0) > 0).sum()), "by_ops": {}}
    for n_ops in [int(x) for x in a.ops.split(",")]:
        S = n_ops + 1
        cms = api.CubeMaps(ctx, S, *CAP[a.rings], pool_points=a.pool)
        o_all = np.arange(S + 1, dtype=np.int64) * len(pts)
        every = np.concatenate([pts] * S)
        fill = lambda: cms.import_maps(every, o_all, [lay] * S)
        ops = []
        for i in range(n_ops):                                     # a few metres and degrees apart: overlapping routes
            yaw = np.deg2rad(2.0 + 1.5 * i) / 2
            ops.append((i, n_ops, np.array([0.0, 0.0, np.sin(yaw), np.cos(yaw), 1.5 + 0.7 * i, -2.0 + 0.4 * i, 0.1])))
        # correctness first: both ways give the same bytes
        fill(); cms.merge(ops)
        ref = cms.export(api.MAP_ALL)[0].tobytes()
        fill(); calls = host_merge(ctx, cms, ops, leaf)
        assert cms.export(api.MAP_ALL)[0].tobytes() == ref, "the merge and the host leg differ"
        wall, stage, syncs = [], [], []
        for rep in range(a.warmup + a.repeats):
            fill(); ctx.synchronize()
            s0 = cms.stats()[0]
            t0 = time.perf_counter()
            added, dropped = cms.merge(ops)
            t = 1e3 * (time.perf_counter() - t0)
            if rep >= a.warmup:
                wall.append(t); stage.append(cms.merge_timing()[0]); syncs.append(cms.stats()[0] - s0)
        cnt = cms.merge_timing()[1]
        stage = np.array(stage)
        dev_ms = med(stage.sum(1))
        host = []
        for _ in range(a.host_repeats):
            fill(); ctx.synchronize()
            t0 = time.perf_counter()
            host_merge(ctx, cms, ops, leaf)
            host.append(1e3 * (time.perf_counter() - t0))
        r = {"maps": S, "points_in": cnt[0], "touched_cubes": cnt[1], "points_out": cnt[2], "added": int(added.sum()), "dropped": int(dropped.sum()),
             "merge": {"wall_ms": med(wall), "wall_ms_min": min(wall), "wall_ms_max": max(wall), "assign_ms": med(stage[:, 0]),
                       "sort_gather_ms": med(stage[:, 1]), "filter_ms": med(stage[:, 2]), "commit_ms": med(stage[:, 3]), "device_ms": dev_ms,
                       "points_per_s_device": cnt[0] / (dev_ms * 1e-3) if dev_ms > 0 else None, "points_per_s_wall": cnt[0] / (med(wall) * 1e-3),
                       "host_syncs_per_call": med(syncs)},
             "host": {"wall_ms": med(host), "wall_ms_min": min(host), "wall_ms_max": max(host), "voxel_grid_calls": calls, "repeats": a.host_repeats},
             "host_over_merge": med(host) / med(wall)}
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
