"""Map export (ll_cubemaps_export) against the per-cube loop of ll_cubemaps_download_cube, on the same maps in the same run.

    python tools/bench_map_export.py [--rings 64] [--seqs 1,8,32,128] [--frames 8] [--out profiles/r09_map_export.json]

The maps are built as tools/bench_mapping_sequences.py builds them (the same synthetic drives, guesses, capacities and number of
frames).  Then, for LL_MAP_ALL and LL_MAP_SURROUND of all S sequences:
  export     ll_cubemaps_export into page-locked host memory: `--warmup` untimed calls, `--repeats` timed ones; the wall time per
             call (host clock around the call, which ends in its one synchronisation) and the library's own split of the call
             (ll_cubemaps_export_timing): table build on the host clock, gather and copy between device events.  Medians, with
             the minimum and maximum of the wall time.  gather_GBps = 2 x 16 bytes x points (read + write) over the gather time.
  per_cube   the same clouds through one ll_cubemaps_download_cube per (sequence, cloud type, cube of the list) into a
             preallocated buffer -- one call per cube and type where the ROS wrapper made two: each non-empty cube costs a copy
             and a synchronisation.  One untimed pass, `--loop-repeats` timed ones (one at S = 128).
  tiles      the gather alone (device events) with LIGHTLOAM_EXPORT_TILE = 256 / 512 / 1024 / 2048 points, alternating, LL_MAP_ALL.
Both sides' bytes are compared before anything is timed.  Prints one JSON line and writes it to --out.
"""
import argparse
import ctypes as C
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
from bench_mapping_sequences import CAP, load, make_drives  # noqa: E402

NAMES = {api.MAP_ALL: "all", api.MAP_SURROUND: "surround"}
W, H, D = 21, 21, 11


def copy_rate():
    """the best flat device-to-device copy rate of profiles/r05_stream_rate.json, GB/s (read + write bytes)"""
    with open(os.path.join(ROOT, "profiles", "r05_stream_rate.json")) as f:
        rows = json.load(f)["stream_rate"]["results"]
    return max(r["GBps"] for r in rows if r["pattern"] == "flat" and r["mode"] == "copy")


def surround_list(guess_t, cen):
    c = []
    for k in range(3):
        v = int((guess_t[k] + 25.0) / 50.0) + cen[k]
        c.append(v - 1 if guess_t[k] + 25.0 < 0 else v)
    return [i + W * j + W * H * k for i in range(c[0] - 2, c[0] + 3) for j in range(c[1] - 2, c[1] + 3) for k in range(c[2] - 1, c[2] + 2)
            if 0 <= i < W and 0 <= j < H and 0 <= k < D]


class Pinned:
    def __init__(self, lib, points):
        self.lib = lib
        self.ptr = lib.ll_host_alloc(max(points, 1) * 16)
        if not self.ptr:
            raise MemoryError("ll_host_alloc")
        self.arr = np.ctypeslib.as_array(C.cast(self.ptr, C.POINTER(C.c_float)), shape=(max(points, 1), 4))

    def close(self):
        self.lib.ll_host_free(self.ptr)


def export_once(cms, w, buf, off):
    t0 = time.perf_counter()
    rc = cms.lib.ll_cubemaps_export(cms.h, w.ctypes.data, buf.ptr, len(buf.arr), off.ctypes.data)
    t = time.perf_counter() - t0
    if rc:
        raise api.LightLoamError(rc, cms.lib.ll_cubemaps_last_error(cms.h).decode())
    return 1e3 * t


def per_cube_loop(cms, lists, out):
    """lists[q]: the cube list of sequence q; the clouds land back to back in out.  Returns (ms, points, calls)"""
    lib, h = cms.lib, cms.h
    fn = lib.ll_cubemaps_download_cube
    fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    n = C.c_int(0); nref = C.byref(n)
    base, at, calls, cap = out.ptr, 0, 0, len(out.arr)
    t0 = time.perf_counter()
    for q, cubes in enumerate(lists):
        for c in cubes:
            for surf in (0, 1):
                rc = fn(h, q, surf, c, base + 16 * at, cap - at, nref)
                if rc:
                    raise api.LightLoamError(rc, lib.ll_cubemaps_last_error(h).decode())
                at += n.value
                calls += 1
    return 1e3 * (time.perf_counter() - t0), at, calls


def med(x):
    return float(np.median(x))


def run(rings, scans, guesses, S, pool, a):
    Dn, F = len(scans), len(scans[0])
    ctx = api.Context(api.default_params(rings, batch=S, max_points=max(len(s) for d in scans for s in d)))
    cms = api.CubeMaps(ctx, S, *CAP[rings], pool_points=pool)
    g = guesses[np.arange(S) % Dn]
    for k in range(F):
        load(ctx, scans, S, k)
        cms.process_slots(g[:, k], list(range(S)))
    ctx.synchronize()
    res = {}
    for which in (api.MAP_ALL, api.MAP_SURROUND):
        w = np.full(S, which, np.int32)
        sizes = cms.export_sizes(w)
        points = int(sizes[-1])
        buf, ref = Pinned(cms.lib, points), Pinned(cms.lib, points)
        off = np.zeros(S + 1, np.int64)
        lists = [list(range(W * H * D)) if which == api.MAP_ALL else surround_list(g[q, F - 1, 4:], cms.info(q)[0]) for q in range(S)]
        # correctness first: both ways give the same bytes
        export_once(cms, w, buf, off)
        _, n_loop, calls = per_cube_loop(cms, lists, ref)
        assert n_loop == points and (off == sizes).all()
        assert buf.arr[:points].tobytes() == ref.arr[:points].tobytes(), "export and the per-cube loop differ"
        for _ in range(a.warmup):
            export_once(cms, w, buf, off)
        s0 = cms.stats()[0]
        wall, split = [], []
        for _ in range(a.repeats):
            wall.append(export_once(cms, w, buf, off))
            ms, cnt = cms.export_timing()
            split.append(ms)
        syncs = (cms.stats()[0] - s0) / a.repeats
        split = np.array(split)
        gather_ms = med(split[:, 1])
        loop_reps = 1 if S >= 128 else a.loop_repeats
        loop_ms = [per_cube_loop(cms, lists, ref)[0] for _ in range(loop_reps)]
        nonempty = cnt[1]
        r = {"points": points, "bytes": 16 * points, "segments": cnt[1], "tiles": cnt[2],
             "export": {"wall_ms": med(wall), "wall_ms_min": min(wall), "wall_ms_max": max(wall), "table_build_ms": med(split[:, 0]),
                        "gather_ms": gather_ms, "copy_ms": med(split[:, 2]), "host_syncs_per_call": syncs, "repeats": a.repeats,
                        "gather_GBps": 2 * 16 * points / (gather_ms * 1e6) if gather_ms > 0 else None,
                        "copy_to_host_GBps": 16 * points / (med(split[:, 2]) * 1e6) if med(split[:, 2]) > 0 else None},
             "per_cube": {"wall_ms": med(loop_ms), "wall_ms_min": min(loop_ms), "wall_ms_max": max(loop_ms), "calls": calls,
                          "host_syncs_per_pass": nonempty, "repeats": loop_reps},
             "per_cube_over_export": med(loop_ms) / med(wall)}
        if which == api.MAP_ALL:
            tiles = {t: [] for t in (256, 512, 1024, 2048)}
            for rep in range(a.warmup + a.repeats):
                for t in tiles:
                    os.environ["LIGHTLOAM_EXPORT_TILE"] = str(t)
                    export_once(cms, w, buf, off)
                    if rep >= a.warmup:
                        tiles[t].append(cms.export_timing()[0][1])
            os.environ.pop("LIGHTLOAM_EXPORT_TILE", None)
            r["tiles_gather_ms"] = {str(t): {"median": med(v), "min": min(v), "max": max(v)} for t, v in tiles.items()}
        res[NAMES[which]] = r
        print(f"# S {S} {NAMES[which]}: {r}", file=sys.stderr, flush=True)
        buf.close(); ref.close()
    cms.close(); ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rings", type=int, default=64)
    ap.add_argument("--seqs", default="1,8,32,128")
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--drives", type=int, default=8)
    ap.add_argument("--pool", type=int, default=1 << 19)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--loop-repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_map_export.json"))
    a = ap.parse_args()
    lib = api.load_library()
    lib.ll_host_alloc.restype = C.c_void_p
    res = {"tool": "tools/bench_map_export.py", "rings": a.rings, "frames": a.frames, "drives": a.drives, "pool_points": a.pool,
           "warmup": a.warmup, "tile_points_default": 1024, "destination": "page-locked host memory",
           "flat_copy_GBps_r05_stream_rate": copy_rate(), "by_sequences": {}}
    scans, guesses = make_drives(a.rings, a.drives, a.frames)
    for S in [int(x) for x in a.seqs.split(",")]:
        res["by_sequences"][str(S)] = run(a.rings, scans, guesses, S, a.pool, a)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
