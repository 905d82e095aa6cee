"""Map import and lane checkpoints: the library compared with itself across an interruption.  An LL_MAP_ALL export plus the layout,
imported into a new CubeMaps, must give the same map and the same future; a lane saved after step k and restored into another
lane of another Drives in another context (or another process) must continue bit for bit like the run that never stopped.
Poses are compared bytewise as float64, clouds bytewise as float32."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import assert_bit_equal
from test_gpu_drives import CAP as DRIVE_CAP, NAN7, _build, run_schedule, single_chain  # noqa: F401  (single_chain: the chain run_schedule's lanes are pinned to)
from test_gpu_mapping_sequences import CAP, _assert_same, _ctx, _guesses  # noqa: F401
from test_gpu_sequences import drives, max_points

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUR, ALL = 0, 1
SCHEDULE = [[(0, 0, 11)], [(1, 1, 10)], [(2, 2, 8)]]      # three ragged lanes: staggered starts, different lengths
T_END = 11


def same_f64(a, b, what):
    a = np.ascontiguousarray(a, np.float64); b = np.ascontiguousarray(b, np.float64)
    assert a.shape == b.shape and a.tobytes() == b.tobytes(), f"{what}: {a} vs {b}"


def assert_maps_equal(a, qa, b, qb, what):
    """centre, per-cube counts, valid list, every non-empty cube and both export modes of map qa of a and map qb of b"""
    la, lb = a.layout(qa), b.layout(qb)
    assert a.info(qa)[0] == b.info(qb)[0] == tuple(la[0]), what
    for x, y, name in zip(la, lb, ("cen", "counts", "valid")):
        assert x.shape == y.shape and (x == y).all(), f"{what}: {name}"
    for s, c in zip(*np.nonzero(la[1])):                      # the other 4851 x 2 - n cubes are empty in both (counts)
        n = int(la[1][s, c])
        assert_bit_equal(a.cube(qa, int(s), int(c), cap=n), b.cube(qb, int(s), int(c), cap=n), f"{what}: cube {s} {c}")
    for which in (SUR, ALL):
        wa = np.full(a.n_seq, -1, np.int32); wa[qa] = which
        wb = np.full(b.n_seq, -1, np.int32); wb[qb] = which
        pa, _ = a.export(wa); pb, _ = b.export(wb)
        assert pa.shape == pb.shape and pa.tobytes() == pb.tobytes(), f"{what}: export {which}"


# ------------------------------------------------------------------ 1. map round trip, 2. one synchronisation
@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("rings", [16, 64])
def test_map_round_trip(api, synth, rings, device):
    """ll_cubemaps_info's four cloud sizes describe the clouds gathered for the last frame, which no export holds: an imported map
    reports 0 for them until its next frame, as after ll_cubemaps_reset, so info is compared by its centre"""
    S, n0, n1 = 3, 4, 3
    cfgs, scans, _ = drives(synth, rings, S, n0 + n1)
    ctx = _ctx(api, rings, scans)
    c, s, pool = CAP[rings]
    many = api.CubeMaps(ctx, S, c, s, pool_points=pool)

    def frame(maps, k, ragged):
        slots = [k * S + q for q in range(S)]
        if ragged and k == 2:
            slots[1] = -1                                                          # sequence 1 sits a frame out
        if ragged and k == 0:
            slots[2] = -1                                                          # sequence 2 starts late
        return maps.process_slots(_guesses(synth, cfgs, k, [(0.0, 0.0, 0.0), (-431.0, 512.5, 30.0), (0.0, 0.0, 0.0)]), slots)

    for k in range(n0):
        frame(many, k, True)
    s0 = many.stats()
    layouts = [many.layout(q) for q in range(S)]
    assert many.stats() == s0                                                      # layout: host bookkeeping
    fresh = api.CubeMaps(ctx, S, c, s, pool_points=pool)
    f0 = fresh.stats()
    if device:
        import torch
        off = many.export_sizes(ALL)
        dev = torch.zeros((int(off[-1]), 4), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        w = np.full(S, ALL, np.int32)
        assert many.lib.ll_cubemaps_export(many.h, w.ctypes.data, dev.data_ptr(), len(dev), off.ctypes.data) == 0
        fresh.import_maps(None, off, layouts, device_ptr=dev.data_ptr())
    else:
        pts, off = many.export(ALL)
        fresh.import_maps(pts, off, layouts)
    assert fresh.stats() == (f0[0] + 1, f0[1])                                     # all sequences: one synchronisation
    assert many.layout(1)[0].tolist() != [10, 10, 5]                               # a shifted map is among them
    for q in range(S):
        assert_maps_equal(many, q, fresh, q, f"after import, sequence {q}")
        assert fresh.info(q)[1] == (0, 0, 0, 0)
    for k in range(n0, n0 + n1):
        pa, ra = frame(many, k, False)
        pb, rb = frame(fresh, k, False)
        same_f64(pa, pb, f"frame {k} poses"); assert (ra == rb).all() and ra.all()
    for q in range(S):
        assert many.info(q) == fresh.info(q)
        for w in range(4):
            assert_bit_equal(many.cloud(q, w), fresh.cloud(q, w), f"sequence {q} cloud {w}")
        assert_maps_equal(many, q, fresh, q, f"after {n1} more frames, sequence {q}")
    if not device:
        # one selected sequence: one synchronisation, the others untouched; into another sequence index
        pts, off = many.export(ALL)
        lay = [many.layout(q) for q in range(S)]
        before = fresh.stats()
        one_off = np.array([0, 0, off[1] - off[0], off[1] - off[0]], np.int64)      # sequence 0's cloud offered to sequence 1
        fresh.import_maps(pts[off[0]:off[1]], one_off, [None, lay[0], None])
        assert fresh.stats() == (before[0] + 1, before[1])
        assert_maps_equal(many, 0, fresh, 1, "sequence 0 imported as sequence 1")
        assert_maps_equal(many, 0, fresh, 0, "unselected sequence 0"); assert_maps_equal(many, 2, fresh, 2, "unselected sequence 2")
    fresh.close(); many.close(); ctx.close()


def test_single_map_round_trip(api, synth):
    cfgs, scans, _ = drives(synth, 16, 1, 4)
    ctx = _ctx(api, 16, scans)
    c, s, pool = CAP[16]
    a = api.CubeMap(ctx, c, s, pool_points=pool); b = api.CubeMap(ctx, c, s, pool_points=pool)
    for k in range(3):
        a.process_slot(_guesses(synth, cfgs, k, [(0.0, 0.0, 0.0)])[0], k)
    b.import_map(a.export(ALL), a.layout())
    for x, y in zip(a.layout(), b.layout()):
        assert (x == y).all()
    for which in (SUR, ALL):
        assert a.export(which).tobytes() == b.export(which).tobytes()
    g = _guesses(synth, cfgs, 3, [(0.0, 0.0, 0.0)])[0]
    pa, ra = a.process_slot(g, 3); pb, rb = b.process_slot(g, 3)
    same_f64(pa, pb, "pose after import"); assert ra == rb is True
    assert a.export(ALL).tobytes() == b.export(ALL).tobytes()
    lay = a.layout()
    bad = lay[1].copy(); bad[0, np.nonzero(lay[1][0])[0][0]] += 1
    with pytest.raises(api.LightLoamError) as e:
        b.import_map(a.export(ALL), (lay[0], bad, lay[2]))
    assert e.value.code == -2
    assert a.export(ALL).tobytes() == b.export(ALL).tobytes()
    # the centre is the array index of the world's origin cube: far outside 0 .. 20 after a long drive, refused only beyond +-2^24
    for cen, ok in (((40, -30, 5), True), ((-(1 << 24), 1 << 24, 0), True), (((1 << 24) + 1, 0, 0), False), ((0, -(1 << 24) - 1, 0), False)):
        if ok:
            b.import_map(a.export(ALL), (np.array(cen, np.int32), lay[1], lay[2]))
            assert b.layout()[0].tolist() == list(cen) and b.export(ALL).tobytes() == a.export(ALL).tobytes()
        else:
            with pytest.raises(api.LightLoamError) as e:
                b.import_map(a.export(ALL), (np.array(cen, np.int32), lay[1], lay[2]))
            assert e.value.code == -2 and b.layout()[0].tolist() == [-(1 << 24), 1 << 24, 0]
    a.close(); b.close(); ctx.close()


# ------------------------------------------------------------------ 3. resume equals uninterrupted, 4. save is read-only
def truncated(schedule, k):
    """the schedule's steps 0 .. k"""
    return [[(s0, d, min(f, k + 1 - s0)) for s0, d, f in runs if s0 <= k] for runs in schedule]


def full_run(api, synth, rings, schedule, hook=None):
    """run_schedule with registered clouds kept: (rows per lane, registered clouds per (step, lane), final export + layouts)"""
    reg = {}; step = [0]

    def check(ctx, dr, slots, frame, mapped):
        for q in frame:
            reg[(step[0], q)] = dr.registered(q)
        if hook:
            hook(step[0], ctx, dr)
        step[0] += 1
    got, dr, ctx, scans, pose0 = run_schedule(api, synth, rings, schedule, len(schedule), check_step=check, keep_registered=True)
    pts, off = dr.export_maps(ALL)
    lay = [dr.cubemaps.layout(q) for q in range(len(schedule))]
    return got, reg, (pts, off, lay), dr, ctx, scans, pose0


def continue_run(api, ctx, dr, schedule, into, scans, t0, t1, registered=True):
    """steps t0 .. t1 - 1 of the schedule on `dr`, lane q of the schedule living in lane into[q]: rows and registered clouds per schedule lane"""
    rows, reg = {}, {}
    for t in range(t0, t1):
        cmd = np.zeros(dr.n_lanes, np.int32); live = {}
        for q, runs in enumerate(schedule):
            for s0, d, f in runs:
                if s0 <= t < s0 + f:
                    assert t > s0, "the continued steps hold no drive start"
                    cmd[into[q]] = api.RUN; live[q] = (d, t - s0)
        slots = dr.slots()
        for q, (d, k) in live.items():
            ctx.upload_scan(int(slots[into[q]]), scans[d][k])
        odom, mapped, ran = dr.step(cmd, None)
        for q in live:
            rows.setdefault(q, []).append((odom[into[q]], mapped[into[q]], ran[into[q]]))
            if registered:
                reg[(t, q)] = dr.registered(into[q])
    return rows, reg


@pytest.mark.parametrize("k", [3, 8])
@pytest.mark.parametrize("rings", [16, 64])
def test_resume_equals_uninterrupted(api, synth, rings, k):
    """k = 3: the lanes are restored at frames 3, 2, 1 and cross frame 6 (the vote switch) afterwards; k = 8: at frames 8, 7, 6, the
    switch behind them"""
    got, reg, (pts, off, lay), dr, ctx, scans, pose0 = full_run(api, synth, rings, SCHEDULE)
    dr.close(); ctx.close()
    _, _, _, dr, ctx, _, _ = full_run(api, synth, rings, truncated(SCHEDULE, k))
    s0 = (dr.stats(), dr.cubemaps.stats())
    size = dr.save_size([1, 1, 1])
    assert (dr.stats(), dr.cubemaps.stats()) == s0                                 # host bookkeeping
    blob = dr.save([1, 1, 1])
    assert len(blob) == size and dr.stats() == (s0[0][0] + 1, s0[0][1]) and dr.cubemaps.stats() == (s0[1][0] + 1, s0[1][1])
    info = api.describe_checkpoint(blob)
    assert [r["frame_index"] for r in info["records"]] == [k, k - 1, k - 2] and info["n_scans"] == rings
    dr.close(); ctx.close()                                                         # the Drives AND the context are gone

    S2, into = 5, [3, 0, 4]                                                         # another S, the lanes permuted
    ctx = api.Context(api.default_params(rings, batch=2 * S2 + 1, max_points=max_points(scans)))
    c, s_, pool = DRIVE_CAP[rings]
    dr = api.Drives(ctx, S2, c, s_, pool_points=pool, base=1, keep_registered=True)
    s0 = (dr.stats(), dr.cubemaps.stats())
    dr.restore(blob, into)
    assert dr.stats() == (s0[0][0] + 1, s0[0][1]) and dr.cubemaps.stats() == (s0[1][0] + 1, s0[1][1])
    rows, reg2 = continue_run(api, ctx, dr, SCHEDULE, into, scans, k + 1, T_END)
    for q, runs in enumerate(SCHEDULE):
        s0_, _, f = runs[0]
        want = got[(q, 0)][k + 1 - s0_:]
        assert len(rows.get(q, [])) == len(want) > 0
        for i, (a, b) in enumerate(zip(rows[q], want)):
            same_f64(a[0], b[0], f"lane {q} frame {k + 1 - s0_ + i} odom"); same_f64(a[1], b[1], f"lane {q} frame {k + 1 - s0_ + i} mapped")
            assert bool(a[2]) == bool(b[2])
    assert sorted(reg2) == sorted(key for key in reg if key[0] > k)
    for key, cloud in reg2.items():
        assert_bit_equal(cloud, reg[key], f"registered cloud, step {key[0]} lane {key[1]}")
    w = np.full(S2, -1, np.int32)
    for q in range(3):
        w[:] = -1; w[into[q]] = ALL
        p2, _ = dr.cubemaps.export(w)
        want = pts[off[q]:off[q + 1]]
        assert p2.shape == want.shape and p2.tobytes() == want.tobytes(), f"lane {q}: final map"
        for x, y in zip(dr.cubemaps.layout(into[q]), lay[q]):
            assert (x == y).all()
    dr.close(); ctx.close()


def test_save_is_read_only_and_partial_selections(api, synth):
    """a run with saves in the middle (all lanes; one lane: one synchronisation each) equals the run without, bit for bit; a lane
    restored and not stepped since can be saved again, to the same bytes apart from the lane number"""
    blobs = {}

    def hook(t, ctx, dr):
        if t == 5:
            s0 = dr.stats()[0]
            blobs["all"] = dr.save([1, 1, 1]); blobs["one"] = dr.save([0, 1, 0])
            assert dr.stats()[0] == s0 + 2
    a = full_run(api, synth, 16, SCHEDULE)
    a[3].close(); a[4].close()
    b = full_run(api, synth, 16, SCHEDULE, hook)
    for key in a[0]:
        for (o1, m1, r1), (o2, m2, r2) in zip(a[0][key], b[0][key]):
            same_f64(o1, o2, "odom"); same_f64(m1, m2, "mapped"); assert r1 == r2
    assert sorted(a[1]) == sorted(b[1])
    for key in a[1]:
        assert_bit_equal(a[1][key], b[1][key], f"registered {key}")
    assert a[2][0].tobytes() == b[2][0].tobytes() and (a[2][1] == b[2][1]).all()
    dr, ctx = b[3], b[4]
    one = api.describe_checkpoint(blobs["one"]); every = api.describe_checkpoint(blobs["all"])
    assert one["n_records"] == 1 and {k: v for k, v in one["records"][0].items() if k != "offset"} == {k: v for k, v in every["records"][1].items() if k != "offset"}
    # lane 1's record into the (now idle) lane 0 of the same object; saved again before any step: the same payload
    dr.restore(blobs["one"], [0])
    again = dr.save([1, 0, 0])
    r0, r1 = api.describe_checkpoint(again)["records"][0], one["records"][0]
    assert again[r0["offset"]:r0["offset"] + r0["bytes"]] == blobs["one"][r1["offset"]:r1["offset"] + r1["bytes"]]
    dr.close(); ctx.close()


# ------------------------------------------------------------------ 5. fresh processes
CHILD = r'''
import sys
sys.path[:0] = [{root!r}, {tests!r}]
import numpy as np
import lightloam_amd  # noqa: F401
from lightloam_amd import api, synth
from test_gpu_checkpoint import SCHEDULE, T_END, continue_run, truncated
from test_gpu_drives import CAP, run_schedule
from test_gpu_sequences import drives, max_points
mode, k, path = sys.argv[1], int(sys.argv[2]), sys.argv[3]
rings = 16
if mode == "save":
    got, dr, ctx, scans, pose0 = run_schedule(api, synth, rings, truncated(SCHEDULE, k), 3)
    open(path, "wb").write(dr.save([1, 1, 1]))
else:
    _, scans, _ = drives(synth, rings, 3, T_END)
    into = [0, 1, 2] if mode == "full" else [2, 0, 1]
    if mode == "full":
        got, dr, ctx, _, _ = run_schedule(api, synth, rings, SCHEDULE, 3)
        rows = {{q: got[(q, 0)][k + 1 - SCHEDULE[q][0][0]:] for q in range(3)}}
    else:
        ctx = api.Context(api.default_params(rings, batch=6, max_points=max_points(scans)))
        c, s_, pool = CAP[rings]
        dr = api.Drives(ctx, 3, c, s_, pool_points=pool)
        dr.restore(open(path, "rb").read(), into)
        rows, _ = continue_run(api, ctx, dr, SCHEDULE, into, scans, k + 1, T_END, registered=False)
    w = np.full(3, -1, np.int32)
    out = {{}}
    for q in range(3):
        out[f"odom{{q}}"] = np.array([r[0] for r in rows[q]]); out[f"mapped{{q}}"] = np.array([r[1] for r in rows[q]])
        w[:] = -1; w[into[q]] = 1
        out[f"map{{q}}"] = dr.cubemaps.export(w)[0]
    np.savez(path + "." + mode + ".npz", **out)
dr.close()
'''


def test_fresh_process(tmp_path):
    """save in one child process, restore in another, compare with a third that never stopped; every child is a freshly started
    interpreter under its own time limit, and the first non-zero status ends the test.  The parent never opens the GPU."""
    script = tmp_path / "child.py"
    script.write_text(CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests")))
    blob = str(tmp_path / "lanes.ckpt")
    py = [sys.executable] + (["-s"] if sys.flags.no_user_site else [])
    for mode in ("save", "resume", "full"):
        out = subprocess.run(["timeout", "-k", "10", "300"] + py + [str(script), mode, "4", blob], capture_output=True, text=True)
        assert out.returncode == 0, f"{mode}: status {out.returncode}\n{out.stdout[-2000:]}\n{out.stderr[-4000:]}"
    a, b = np.load(blob + ".full.npz"), np.load(blob + ".resume.npz")
    assert sorted(a.files) == sorted(b.files) and len(a.files) == 9
    for name in a.files:
        assert a[name].shape == b[name].shape and a[name].size > 0 and a[name].tobytes() == b[name].tobytes(), name


@pytest.mark.parametrize("at", [3, 4])
def test_kitti_drives_tool_checkpoint_and_resume(tmp_path, at):
    """three synthetic .bin drives (6, 4 and 3 scans) queued over 2 lanes: the pose files a run wrote up to step `at`, continued by
    --resume in a new process, equal the uninterrupted tool's files byte for byte.  at = 3: both lanes are inside a drive; at = 4:
    lane 1's drive ends on the saved step and the resumed run starts the queued drive there.  Every tool run is a fresh process
    under its own time limit, and the first non-zero status ends the test."""
    import scangen
    exe = _build(tmp_path, "ll_kitti_drives")
    scans = [scangen.hdl64_scan(k, order="kitti") for k in range(6)]
    dirs = []
    for i, n in enumerate((6, 4, 3)):
        d = tmp_path / f"drive{i}"; d.mkdir()
        for k in range(n):
            scans[k + i].astype("<f4").tofile(d / f"{k:06d}.bin")
        dirs.append(str(d))
    tail = ["64", "1.0", "4608", "2"] + dirs
    ck = str(tmp_path / "lanes.llkd")

    def tool(res, *opts):
        os.makedirs(res, exist_ok=True)
        out = subprocess.run(["timeout", "-k", "10", "300", exe] + list(opts) + [str(res)] + tail, capture_output=True, text=True)
        assert out.returncode == 0, f"{opts}: status {out.returncode}\n{out.stdout[-2000:]}\n{out.stderr[-4000:]}"

    whole, first, rest = tmp_path / "whole", tmp_path / "first", tmp_path / "rest"
    tool(whole)
    tool(first, "--checkpoint", ck, "--checkpoint-at", str(at))
    os.makedirs(rest)
    for i in range(3):                                                              # a saving run carries on: the same files
        assert (first / f"{i}.txt").read_bytes() == (whole / f"{i}.txt").read_bytes(), i
    for i in (0, 1):                                                                # what the first run had written after step `at`
        lines = (first / f"{i}.txt").read_text().splitlines(keepends=True)
        assert len(lines) == (6, 4)[i] and len(lines) >= at
        (rest / f"{i}.txt").write_text("".join(lines[:at]))
    tool(rest, "--resume", ck)
    for i in range(3):
        assert (rest / f"{i}.txt").read_bytes() == (whole / f"{i}.txt").read_bytes(), f"drive {i} resumed after step {at}"


# ------------------------------------------------------------------ 6. errors change nothing
def test_errors_change_nothing(api, synth):
    """every refusal is made on the host before any launch: after all of them the run goes on, every lane included, exactly like a
    run that never made the failing calls"""
    schedule = [[(0, 0, 9)], [(0, 1, 9)], [(6, 2, 3)]]
    seen = []

    def hook(t, ctx, dr):
        if t != 5:
            return
        lib, cms = dr.lib, dr.cubemaps
        stats = (dr.stats(), cms.stats())

        def refused(code, fn, *a):
            with pytest.raises(api.LightLoamError) as e:
                fn(*a)
            assert e.value.code == code, (code, e.value)
            assert (dr.stats(), cms.stats()) == stats, "a refused call synchronised"
            seen.append(code)
        refused(-7, dr.save, [0, 0, 1])                                            # lane 2 has not run: STATE
        refused(-7, dr.save_size, [1, 1, 1])
        size = dr.save_size([1, 1, 0])
        canary = np.full(1024, 0xA5, np.uint8); before = canary.copy(); n = C.c_longlong(0)
        sel = np.array([1, 1, 0], np.int32)
        assert lib.ll_drives_save(dr.h, sel.ctypes.data, canary.ctypes.data, canary.size, C.addressof(n)) == -4
        assert n.value == size and (canary == before).all() and (dr.stats(), cms.stats()) == stats
        blob = dr.save([1, 1, 0])
        stats = (dr.stats(), cms.stats())
        raw = bytearray(blob)
        for at, what in ((0, "magic"), (4, "version")):
            bad = bytearray(raw); bad[at] ^= 0xFF
            refused(-2, dr.restore, bytes(bad), [0, 1])
            assert what in lib.ll_drives_last_error(dr.h).decode()
        refused(-2, dr.restore, bytes(raw[:len(raw) - 4096]), [0, 1])              # truncated
        refused(-2, dr.restore, bytes(raw[:40]), [0, 1])
        for into in ([0, 0], [2, 2], [0, 3], [-2, 1]):                             # two records into one lane; no such lane
            rc = lib.ll_drives_restore(dr.h, np.array(into, np.int32).ctypes.data, np.frombuffer(blob, np.uint8).ctypes.data, len(blob))
            assert rc == -2 and (dr.stats(), cms.stats()) == stats, into
        info = api.describe_checkpoint(blob)
        assert max(info["records"][0]["n_corner"], info["records"][0]["n_surf"]) > 4096, info["records"][0]
        small = api.Context(api.default_params(16, batch=2, max_points=ctx.params.max_points))
        d2 = api.Drives(small, 1, 2048, 4096, pool_points=4096)                    # a pool smaller than the saved map
        with pytest.raises(api.LightLoamError) as e:
            d2.restore(blob, [0, -1])
        assert e.value.code == -4 and d2.stats()[0] == 0
        d2.close(); small.close()
        wide = api.Context(api.default_params(64, batch=2, max_points=ctx.params.max_points))
        c, s_, pool = DRIVE_CAP[64]
        d3 = api.Drives(wide, 1, c, s_, pool_points=pool)                          # a 16-ring blob into a 64-ring context
        with pytest.raises(api.LightLoamError) as e:
            d3.restore(blob, [0, -1])
        assert e.value.code == -2 and "n_scans" in str(e.value)
        d3.close(); wide.close()
        pts, off = cms.export(ALL)
        lay = [cms.layout(q) for q in range(3)]
        stats = (dr.stats(), cms.stats())
        counts = lay[0][1].copy(); counts[1, np.nonzero(counts[1])[0][0]] -= 1     # counts that disagree with offset
        refused(-2, cms.import_maps, pts, off, [(lay[0][0], counts, lay[0][2]), None, None])
        counts = lay[0][1].copy(); counts[0, 7] = -1
        refused(-2, cms.import_maps, pts, off, [(lay[0][0], counts, lay[0][2]), None, None])
        refused(-2, cms.import_maps, pts, off, [(lay[0][0], lay[0][1], np.array([5, 5], np.int32)), None, None])
        refused(-2, cms.import_maps, pts, off, [(np.array([1 << 30, 0, 0], np.int32), lay[0][1], lay[0][2]), None, None])
        p2, o2 = cms.export(ALL)
        assert p2.tobytes() == pts.tobytes() and (o2 == off).all()
    good = full_run(api, synth, 16, schedule)
    good[3].close(); good[4].close()
    bad = full_run(api, synth, 16, schedule, hook)
    assert len(seen) >= 10
    for key in good[0]:
        for (o1, m1, r1), (o2, m2, r2) in zip(good[0][key], bad[0][key]):
            same_f64(o1, o2, "odom"); same_f64(m1, m2, "mapped"); assert r1 == r2
    for key in good[1]:
        assert_bit_equal(good[1][key], bad[1][key], f"registered {key}")
    assert good[2][0].tobytes() == bad[2][0].tobytes() and (good[2][1] == bad[2][1]).all()
    bad[3].close(); bad[4].close()
