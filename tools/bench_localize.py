"""Frames/s of read-only localising frames (ll_cubemaps_localize_slots) against mapping frames (ll_cubemaps_process_slots) at the
same S and scan shape, the host synchronisations per frame of both, and k_cms_fit's time.

    python tools/bench_localize.py [--rings 64] [--seqs 8,32] [--frames 8] [--out profiles/localize.json]

Sequence q replays synthetic drive q % drives (tools/bench_mapping_sequences.py's drives).  Pass 1 maps frames 0 .. frames-1 into the
S maps: frames 1 .. frames-1 are the timed mapping frames (frame 0 fills an empty map).  Pass 2 sends the same frames 1 ..
frames-1 through localize_slots, every sequence against its own now frozen map, with the fit record and without it; per frame
the S scans are uploaded and extracted (not timed), then the one call is timed, device-synchronised before and after.  Synchronisations
per frame come from ll_cubemaps_stats.  k_cms_fit's time is read from a second run of this tool under `rocprofv3 --kernel-trace
--stats` (a child process; "not measured" when the profiler is missing or fails).  Prints one JSON line and writes it to --out.
"""
import argparse
import json
import os
import shutil
import sqlite3
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import lightloam_amd  # noqa: E402,F401
from lightloam_amd import api  # noqa: E402
from bench_mapping_sequences import CAP, load, make_drives, timed  # noqa: E402


def run(rings, scans, guesses, S, pool):
    D, F = len(scans), len(scans[0])
    ctx = api.Context(api.default_params(rings, batch=S, max_points=max(len(s) for d in scans for s in d)))
    cms = api.CubeMaps(ctx, S, *CAP[rings], pool_points=pool)
    g = guesses[np.arange(S) % D]
    slots = list(range(S))
    tot_map, s0 = 0.0, 0
    for k in range(F):
        load(ctx, scans, S, k)
        if k == 1:
            s0 = cms.stats()[0]
        t, (_, ran) = timed(ctx, lambda: cms.process_slots(g[:, k], slots))
        if k:
            tot_map += t
            assert ran.all()
    syncs_map = (cms.stats()[0] - s0) / (F - 1)
    frames_mapped = cms.stats()[1]
    out = {"mapping": {"frames_per_s": S * (F - 1) / tot_map, "frame_ms": 1e3 * tot_map / (F - 1), "host_syncs_per_frame": syncs_map}}
    blocks = []
    for name, want_fit in (("localize_with_fit", True), ("localize_without_fit", False)):
        tot, s0 = 0.0, cms.stats()[0]
        for k in range(1, F):
            load(ctx, scans, S, k)
            t, (_, ran, fit) = timed(ctx, lambda: cms.localize_slots(g[:, k], slots, None, fit=want_fit))
            tot += t
            assert ran.all()
            if want_fit:
                blocks.append(np.mean([f.n_edge + f.n_plane for f in fit]))
        out[name] = {"frames_per_s": S * (F - 1) / tot, "frame_ms": 1e3 * tot / (F - 1), "host_syncs_per_frame": (cms.stats()[0] - s0) / (F - 1)}
    assert cms.stats()[1] == frames_mapped                     # nothing was mapped in pass 2
    out["residual_blocks_per_sequence"] = float(np.mean(blocks))
    out["localize_x_mapping"] = out["localize_with_fit"]["frames_per_s"] / out["mapping"]["frames_per_s"]
    cms.close(); ctx.close()
    return out


def fit_kernel_time(argv):
    """average / total duration of k_cms_fit over one more run of this tool under the kernel trace"""
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(prof):
        return "not measured: no rocprofv3"
    tmp = tempfile.mkdtemp(prefix="ll_localize_prof_")
    try:
        cmd = [prof, "--kernel-trace", "--stats", "-d", tmp, "-o", "loc", "--", sys.executable, os.path.abspath(__file__)] + argv + ["--child"]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
        if r.returncode != 0:
            return f"not measured: the traced run ended with {r.returncode}"
        dbs = [os.path.join(d, f) for d, _, fs in os.walk(tmp) for f in fs if f.endswith("_results.db")]
        if not dbs:
            return "not measured: no trace database"
        cur = sqlite3.connect(dbs[0]).cursor()
        durs = {}
        for name, dur in cur.execute("select name, duration from kernels"):         # nanoseconds per launch
            for key in ("k_cms_fit", "k_cms_knn", "k_cms_compact", "k_cms_lm"):
                if name.startswith(key):
                    durs.setdefault(key, []).append(float(dur) / 1e3)
        got = {k: {"calls": len(v), "avg_us": sum(v) / len(v), "max_us": max(v), "total_us": sum(v)} for k, v in durs.items()}
        return got or "not measured: the kernels are not in the trace"
    except Exception as e:                                      # the figures above stand without it
        return f"not measured: {type(e).__name__}: {e}"
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rings", type=int, nargs="+", default=[64])
    ap.add_argument("--seqs", default="8,32")
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--drives", type=int, default=8)
    ap.add_argument("--pool", type=int, default=1 << 19)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "localize.json"))
    ap.add_argument("--child", action="store_true", help="the run under the kernel trace: no nested trace, no output file")
    a = ap.parse_args()
    seqs = [int(x) for x in a.seqs.split(",")]
    res = {"tool": "tools/bench_localize.py", "frames": a.frames, "timed_frames": a.frames - 1, "drives": a.drives, "pool_points": a.pool, "curves": {}}
    for rings in a.rings:
        scans, guesses = make_drives(rings, a.drives, a.frames)
        res["curves"][str(rings)] = {}
        for S in seqs:
            info = run(rings, scans, guesses, S, a.pool)
            res["curves"][str(rings)][str(S)] = info
            print(f"# rings {rings} S {S}: {info}", file=sys.stderr, flush=True)
    if a.child:
        return
    # the traced run: the largest S of the first ring count only, so that it stays short
    res["kernel_trace"] = {"run": f"--rings {a.rings[0]} --seqs {seqs[-1]} --frames {a.frames}",
                           "kernels": fit_kernel_time(["--rings", str(a.rings[0]), "--seqs", str(seqs[-1]), "--frames", str(a.frames),
                                                       "--drives", str(a.drives), "--pool", str(a.pool)])}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
