"""Lane checkpoints (ll_drives_save / ll_drives_restore) and map import against ll_cubemaps_export(LL_MAP_ALL) of the same lanes,
in the same run.

    python tools/bench_checkpoint.py [--rings 64] [--lanes 1,8,32] [--frames 8] [--out profiles/checkpoint.json]

S lanes run the synthetic drives of tools/bench_map_export.py for `--frames` frames through ll_drives.  Then, all into / out of
page-locked host memory, `--warmup` untimed and `--repeats` timed calls each, host clock around the call (every call ends in its
one synchronisation), medians with minimum and maximum:
  export     ll_cubemaps_export(LL_MAP_ALL) of all lanes: the yardstick -- the map part of a checkpoint moves the same bytes
  save       ll_drives_save of all lanes
  restore    ll_drives_restore of that blob into the same lanes (the state it writes is the state they hold)
  import     ll_cubemaps_import of the exported cloud into the lanes' maps
  per_cube   one lane's map through a ll_cubemaps_download_cube call per cube and type: the host route the gather replaces
The restored state is checked before anything is timed: a second save gives the first one's bytes.  Prints one JSON line and
writes it to --out."""
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
from bench_map_export import Pinned, per_cube_loop  # noqa: E402
from bench_mapping_sequences import CAP, make_drives  # noqa: E402


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter(); fn(); ms.append(1e3 * (time.perf_counter() - t0))
    return {"ms": float(np.median(ms)), "ms_min": min(ms), "ms_max": max(ms), "repeats": repeats}


def ck(rc, what):
    if rc:
        raise RuntimeError(f"{what}: {api.STATUS.get(rc, rc)}")


def run(rings, scans, S, pool, a):
    Dn, F = len(scans), len(scans[0])
    ctx = api.Context(api.default_params(rings, batch=2 * S, max_points=max(len(s) for d in scans for s in d)))
    dr = api.Drives(ctx, S, *CAP[rings], pool_points=pool)
    for k in range(F):
        slots = dr.slots()
        for q in range(S):
            ctx.upload_scan(int(slots[q]), scans[q % Dn][k])
        dr.step([api.START if k == 0 else api.RUN] * S)
    cms, lib = dr.cubemaps, dr.lib
    w = np.full(S, api.MAP_ALL, np.int32)
    off = cms.export_sizes(w)
    points = int(off[-1])
    lanes = np.ones(S, np.int32); into = np.arange(S, dtype=np.int32)
    size = dr.save_size(lanes)
    pts, blob, blob2 = Pinned(lib, points), Pinned(lib, size // 16 + 1), Pinned(lib, size // 16 + 1)
    got = C.c_longlong(0)
    layouts = [cms.layout(q) for q in range(S)]
    sel = np.ones(S, np.int32)
    cen = np.array([l[0] for l in layouts], np.int32); counts = np.array([l[1] for l in layouts], np.int32)
    valid = np.zeros((S, 125), np.int32); nv = np.array([len(l[2]) for l in layouts], np.int32)
    for q, l in enumerate(layouts):
        valid[q, :len(l[2])] = l[2]

    def export():
        ck(lib.ll_cubemaps_export(cms.h, w.ctypes.data, pts.ptr, points, off.ctypes.data), "export")

    def save(dst=blob):
        ck(lib.ll_drives_save(dr.h, lanes.ctypes.data, dst.ptr, size, C.addressof(got)), "save")

    def restore():
        ck(lib.ll_drives_restore(dr.h, into.ctypes.data, blob.ptr, size), "restore")

    def imp():
        ck(lib.ll_cubemaps_import(cms.h, sel.ctypes.data, pts.ptr, off.ctypes.data, cen.ctypes.data, counts.ctypes.data, valid.ctypes.data, nv.ctypes.data), "import")

    export(); save(); restore(); save(blob2)
    raw = lambda b: bytes((C.c_ubyte * size).from_address(b.ptr))  # noqa: E731
    assert raw(blob) == raw(blob2), "a save after the restore differs from the save before it"
    r = {"points": points, "map_bytes": 16 * points, "checkpoint_bytes": size,
         "export": timed(export, a.warmup, a.repeats), "save": timed(save, a.warmup, a.repeats),
         "restore": timed(restore, a.warmup, a.repeats), "import": timed(imp, a.warmup, a.repeats)}
    save(blob2)
    assert raw(blob) == raw(blob2), "the lanes changed under the timed calls"
    for name in ("save", "restore", "import"):
        r[name + "_over_export"] = r[name]["ms"] / r["export"]["ms"]
    one = int(off[1] - off[0])
    ref = Pinned(lib, one)
    loop = [per_cube_loop(cms, [list(range(4851))], ref)[0] for _ in range(1 + a.loop_repeats)][1:]
    r["per_cube_one_lane"] = {"points": one, "ms": float(np.median(loop)), "ms_min": min(loop), "ms_max": max(loop), "calls": 2 * 4851}
    for b in (pts, blob, blob2, ref):
        b.close()
    print(f"# S {S}: {r}", file=sys.stderr, flush=True)
    dr.close(); ctx.close()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rings", type=int, default=64)
    ap.add_argument("--lanes", default="1,8,32")
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--drives", type=int, default=8)
    ap.add_argument("--pool", type=int, default=1 << 19)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--loop-repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "checkpoint.json"))
    a = ap.parse_args()
    lib = api.load_library()
    lib.ll_host_alloc.restype = C.c_void_p
    res = {"tool": "tools/bench_checkpoint.py", "rings": a.rings, "frames": a.frames, "drives": a.drives, "pool_points": a.pool,
           "warmup": a.warmup, "memory": "page-locked host memory", "by_lanes": {}}
    scans, _ = make_drives(a.rings, a.drives, a.frames)
    for S in [int(x) for x in a.lanes.split(",")]:
        res["by_lanes"][str(S)] = run(a.rings, scans, S, a.pool, a)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
