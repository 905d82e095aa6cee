"""Map export: laserCloudSurround (laserMapping.cpp:2173-2188) and laserCloudMap (:2190-2203) of many cube maps in one gather.
Every comparison is bytewise: sequence q's range of an export must be the concatenation of cube(q, 0, c), cube(q, 1, c) over the
expected cube list.  The surround list is rebuilt here from the guess the test passed and info(q)'s centre, the way the ROS node
did before it used the export -- never from anything the export returns."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_gpu_drives import CAP as DRIVE_CAP, NAN7, _build
from test_gpu_mapping_sequences import CAP, _ctx, _guesses
from test_gpu_sequences import drives, max_points

pytestmark = pytest.mark.gpu

SUR, ALL, NONE = 0, 1, -1
W, H, D = 21, 21, 11
EVERY = list(range(W * H * D))


def surround_list(guess_t, cen):
    """laserCloudSurroundInd of a frame whose pose guess was guess_t (:1584-1593 after the shifts, :1784-1801)"""
    c = []
    for k in range(3):
        v = int((guess_t[k] + 25.0) / 50.0) + cen[k]
        if guess_t[k] + 25.0 < 0:
            v -= 1
        c.append(v)
    return [i + W * j + W * H * k for i in range(c[0] - 2, c[0] + 3) for j in range(c[1] - 2, c[1] + 3) for k in range(c[2] - 1, c[2] + 2)
            if 0 <= i < W and 0 <= j < H and 0 <= k < D]


def concat(cube, cubes):
    """cube(surf, index) -> the expected export over `cubes`: per cube corner then surf"""
    parts = [cube(s, c) for c in cubes for s in (0, 1)]
    parts = [p for p in parts if len(p)]
    return np.concatenate(parts) if parts else np.zeros((0, 4), np.float32)


def same_bytes(got, want, what):
    got = np.ascontiguousarray(got, np.float32); want = np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, f"{what}: {got.shape} vs {want.shape}"
    assert got.tobytes() == want.tobytes(), what


def check_export(many, which, lists, what):
    """one export call; lists[q]: the expected cube list of sequence q (None: left out / empty)"""
    pts, off = many.export(which)
    assert off[0] == 0 and len(off) == many.n_seq + 1 and off[-1] == len(pts), what
    assert (many.export_sizes(which) == off).all(), what
    for q in range(many.n_seq):
        want = concat(lambda s, c: many.cube(q, s, c), lists[q] or [])
        same_bytes(pts[off[q]:off[q + 1]], want, f"{what}: sequence {q}")
    return pts, off


def run_frames(api, synth, rings, S, n, offsets=None, check=None):
    offsets = offsets or [(0.0, 0.0, 0.0)] * S
    cfgs, scans, _ = drives(synth, rings, S, n)
    ctx = _ctx(api, rings, scans)
    c, s, pool = CAP[rings]
    many = api.CubeMaps(ctx, S, c, s, pool_points=pool)
    guesses = []
    for k in range(n):
        guess = _guesses(synth, cfgs, k, offsets)
        many.process_slots(guess, [k * S + q for q in range(S)])
        guesses.append(guess)
        if check:
            check(k, many, guess)
    return ctx, many, guesses


@pytest.mark.parametrize("rings,S,n", [(16, 3, 7), (64, 2, 7)])
def test_equals_the_per_cube_reads(api, synth, rings, S, n):
    def check(k, many, guess):
        if k in (0, 5):
            check_export(many, SUR, [surround_list(guess[q, 4:], many.info(q)[0]) for q in range(S)], f"frame {k} surround")
    ctx, many, guesses = run_frames(api, synth, rings, S, n, check=check)
    pts, off = check_export(many, ALL, [EVERY] * S, "whole map")
    assert off[-1] > 0 and all(off[q + 1] > off[q] for q in range(S))
    many.close(); ctx.close()


def test_after_shifts(api, synth):
    """the drive of test_shift_loops_and_negative_coordinates: window shifts on all three axes, negative coordinates"""
    offsets = [(-431.0, 512.5, 30.0), (0.0, 0.0, 0.0), (260.0, -140.0, -60.0), (0.0, 0.0, 0.0)]
    ctx, many, guesses = run_frames(api, synth, 16, 4, 5, offsets)
    assert many.info(0)[0] != (10, 10, 5) and many.info(1)[0] == (10, 10, 5)
    check_export(many, SUR, [surround_list(guesses[-1][q, 4:], many.info(q)[0]) for q in range(4)], "surround after shifts")
    check_export(many, ALL, [EVERY] * 4, "whole map after shifts")
    many.close(); ctx.close()


def test_mixed_selection_and_empty_sequences(api, synth):
    S, n = 3, 3
    ctx, many, guesses = run_frames(api, synth, 16, S, n)
    sur2 = surround_list(guesses[-1][2, 4:], many.info(2)[0])
    pts, off = check_export(many, [ALL, NONE, SUR], [EVERY, None, sur2], "mixed")
    assert off[1] == off[2] and off[1] > 0 and off[3] > off[2]
    many.reset(1)
    for which in (SUR, ALL):
        pts, off = many.export([NONE, which, NONE])
        assert len(pts) == 0 and (off == 0).all()
    fresh = api.CubeMaps(ctx, 2, *CAP[16][:2], pool_points=CAP[16][2])          # never ran
    for which in (SUR, ALL):
        pts, off = fresh.export(which)
        assert len(pts) == 0 and (off == 0).all()
    fresh.close(); many.close(); ctx.close()


def test_ragged_frames(api, synth):
    """the schedule of test_ragged_frames_and_a_late_start: a sequence that skipped a call exports the surround set of its own
    last frame"""
    S, n = 4, 6
    cfgs, scans, _ = drives(synth, 16, S, n)
    ctx = _ctx(api, 16, scans)
    c, s, pool = CAP[16]
    many = api.CubeMaps(ctx, S, c, s, pool_points=pool)
    last = [None] * S
    for k in range(n):
        guess = _guesses(synth, cfgs, k, [(0.0, 0.0, 0.0)] * S)
        slots = [k * S + q for q in range(S)]
        if k in (2, 4):
            slots[1] = -1
        if k < 3:
            slots[3] = -1
        many.process_slots(guess, slots)
        for q in range(S):
            if slots[q] >= 0:
                last[q] = guess[q, 4:].copy()
        lists = [surround_list(last[q], many.info(q)[0]) if last[q] is not None else None for q in range(S)]
        check_export(many, SUR, lists, f"frame {k}")
        if k < 3:
            off = many.export_sizes(ALL)
            assert off[4] == off[3]                                             # sequence 3 has not started
    many.close(); ctx.close()


def test_read_only(api, synth):
    S, n = 2, 6
    cfgs, scans, _ = drives(synth, 16, S, n)
    ctx = _ctx(api, 16, scans)
    c, s, pool = CAP[16]
    a = api.CubeMaps(ctx, S, c, s, pool_points=pool)
    b = api.CubeMaps(ctx, S, c, s, pool_points=pool)
    for k in range(n):
        guess = _guesses(synth, cfgs, k, [(0.0, 0.0, 0.0)] * S)
        slots = [k * S + q for q in range(S)]
        pa, ra = a.process_slots(guess, slots)
        pb, rb = b.process_slots(guess, slots)
        a.export(SUR); a.export(ALL)
        assert pa.tobytes() == pb.tobytes() and (ra == rb).all(), k
        for q in range(S):
            assert a.info(q) == b.info(q), (k, q)
    for q in range(S):
        for surf in (0, 1):
            for cube in EVERY:
                same_bytes(a.cube(q, surf, cube, cap=1 << 16), b.cube(q, surf, cube, cap=1 << 16), f"sequence {q} cube {surf} {cube}")
    a.close(); b.close(); ctx.close()


@pytest.mark.parametrize("S", [1, 8])
def test_one_synchronisation_per_export(api, synth, S):
    ctx, many, guesses = run_frames(api, synth, 16, S, 3)
    for which in (SUR, ALL, [ALL if q % 2 else SUR for q in range(S)]):
        s0, f0 = many.stats()
        sizes = many.export_sizes(which)
        assert many.stats() == (s0, f0)
        w = np.full(S, which, np.int32) if np.ndim(which) == 0 else np.array(which, np.int32)
        out = np.zeros((int(sizes[-1]), 4), np.float32); off = np.zeros(S + 1, np.int64)
        rc = many.lib.ll_cubemaps_export(many.h, w.ctypes.data, out.ctypes.data, len(out), off.ctypes.data)
        assert rc == 0 and (off == sizes).all()
        assert many.stats() == (s0 + 1, f0), (S, which)
    many.close(); ctx.close()


def crafted_scene():
    """corner: a filled plane inside the centre cube (0.45 m pitch, one point per 0.4 m leaf) and one lone point in the next
    cube; surf: a 25 m lattice over the whole 21 x 21 cube floor (four points per cube)"""
    g = np.arange(-24.0, 24.0, 0.45, dtype=np.float32)
    x, y = np.meshgrid(g, g, indexing="ij")
    corner = np.stack([x.ravel(), y.ravel(), np.full(x.size, 0.2, np.float32), np.zeros(x.size, np.float32)], 1)
    corner = np.concatenate([corner, np.array([[40.0, 0.1, 0.2, 0.0]], np.float32)])
    g = np.arange(-510.0, 511.0, 25.0, dtype=np.float32) + np.float32(0.5)
    x, y = np.meshgrid(g, g, indexing="ij")
    surf = np.stack([x.ravel(), y.ravel(), np.full(x.size, 0.3, np.float32), np.ones(x.size, np.float32)], 1)
    return np.ascontiguousarray(corner, np.float32), np.ascontiguousarray(surf, np.float32)


def test_tiles_on_a_crafted_map(api, synth):
    """segments far above one tile, of exactly one point, and hundreds of small ones, in one gather"""
    corner, surf = crafted_scene()
    ctx = api.Context(api.default_params(16, batch=1, max_points=4096))
    many = api.CubeMaps(ctx, 2, len(corner), len(surf), pool_points=1 << 16)
    pose = np.array([[0, 0, 0, 1.0, 0, 0, 0], [0, 0, 0, 1.0, 0, 0, 0]])
    many.process(pose, [corner, None], [surf, None])
    counts = np.array([[len(many.cube(0, s, c, cap=1 << 15)) for c in EVERY] for s in (0, 1)])
    assert counts.max() > 4096, counts.max()
    assert (counts == 1).any()
    assert ((counts[0] > 0) | (counts[1] > 0)).sum() >= 300
    check_export(many, [ALL, ALL], [EVERY, EVERY], "crafted map")
    check_export(many, [SUR, NONE], [surround_list([0.0, 0.0, 0.0], many.info(0)[0]), None], "crafted surround")
    many.close(); ctx.close()


def test_errors(api, synth):
    S = 2
    ctx, many, guesses = run_frames(api, synth, 16, S, 2)
    lib = many.lib
    w = np.full(S, ALL, np.int32)
    sizes = many.export_sizes(ALL)
    n = int(sizes[-1])
    canary = np.full((n, 4), -7.25, np.float32)
    out = canary.copy(); off = np.full(S + 1, -1, np.int64)
    s0 = many.stats()
    rc = lib.ll_cubemaps_export(many.h, w.ctypes.data, out.ctypes.data, n - 1, off.ctypes.data)
    assert rc == -4 and (off == sizes).all() and out.tobytes() == canary.tobytes() and many.stats() == s0
    rc = lib.ll_cubemaps_export(many.h, w.ctypes.data, out.ctypes.data, n, off.ctypes.data)
    assert rc == 0 and many.stats()[0] == s0[0] + 1
    same_bytes(out, many.export(ALL)[0], "after the refused call")
    assert not (out == -7.25).all(axis=1).any()
    s0 = many.stats()
    bad = np.array([ALL, 2], np.int32)
    assert lib.ll_cubemaps_export(many.h, bad.ctypes.data, out.ctypes.data, n, off.ctypes.data) == -2
    assert lib.ll_cubemaps_export_sizes(many.h, bad.ctypes.data, off.ctypes.data) == -2
    assert lib.ll_cubemaps_export(many.h, w.ctypes.data, None, n, off.ctypes.data) == -2
    assert lib.ll_cubemaps_export(many.h, w.ctypes.data, out.ctypes.data, -1, off.ctypes.data) == -2
    assert lib.ll_cubemaps_export(many.h, None, out.ctypes.data, n, off.ctypes.data) == -2
    assert many.stats() == s0
    many.close(); ctx.close()


def test_device_destination(api, synth):
    import torch
    S = 3
    ctx, many, guesses = run_frames(api, synth, 16, S, 3)
    host, off = many.export([ALL, SUR, ALL])
    dev = torch.zeros((len(host), 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    w = np.array([ALL, SUR, ALL], np.int32); off2 = np.zeros(S + 1, np.int64)
    rc = many.lib.ll_cubemaps_export(many.h, w.ctypes.data, C.c_void_p(dev.data_ptr()), len(host), off2.ctypes.data)
    assert rc == 0 and (off2 == off).all()
    same_bytes(dev.cpu().numpy(), host, "device destination")
    many.close(); ctx.close()


def _single(api, synth, rings, n, shard=None):
    """sequence 0 of run_frames on one ll_cubemap (frame k in slot k)"""
    cfgs, scans, _ = drives(synth, rings, 1, n)
    ctx = _ctx(api, rings, scans)
    c, s, pool = CAP[rings]
    one = api.CubeMap(ctx, c, s, pool_points=pool)
    if shard:
        one.set_shard(*shard)
    for k in range(n):
        guess = _guesses(synth, cfgs, k, [(0.0, 0.0, 0.0)])[0]
        if shard:                                                              # a shard has no optimize: prepare + update with the guess
            f = ctx.features(k)
            one.prepare(guess[4:], f["less_sharp"], f["less_flat"]); one.update(guess)
        else:
            one.process_slot(guess, k)
    return ctx, one, guess


@pytest.mark.parametrize("shard", [None, (1, 3)])
def test_single_map(api, synth, shard):
    ctx, one, guess = _single(api, synth, 16, 7, shard)
    sur = surround_list(guess[4:], one.info()[0])
    want_sur, want_all = concat(one.cube, sur), concat(one.cube, EVERY)
    assert len(want_all) >= len(want_sur) and len(want_all) > 0 and (shard or len(want_sur) > 0)
    same_bytes(one.export(SUR), want_sur, "single map surround")
    same_bytes(one.export(ALL), want_all, "single map whole")
    n = C.c_longlong(-1); out = np.zeros((4, 4), np.float32)
    assert one.lib.ll_cubemap_export(one.h, 2, out.ctypes.data, 4, C.byref(n)) == -2
    assert one.lib.ll_cubemap_export(one.h, ALL, out.ctypes.data, 4, C.byref(n)) == -4 and n.value == len(want_all)
    one.close(); ctx.close()


def _two_lane_run(api, synth, export_at=None):
    """the two-lane 64-ring schedule of test_lanes_equal_the_single_drive_chain"""
    schedule = [[(0, 0, 5), (5, 1, 4)], [(1, 2, 6)]]
    n_lanes, rings = 2, 64
    cfgs, scans, pose0 = drives(synth, rings, 3, 6)
    ctx = api.Context(api.default_params(rings, batch=2 * n_lanes, max_points=max_points(scans)))
    c, s_, pool = DRIVE_CAP[rings]
    dr = api.Drives(ctx, n_lanes, c, s_, pool_points=pool)
    T = max(s0 + f for runs in schedule for s0, _, f in runs)
    mapped_all, exports = [], {}
    for t in range(T):
        cmd = np.zeros(n_lanes, np.int32); frame = {}
        for q, runs in enumerate(schedule):
            for s0, d, f in runs:
                if s0 <= t < s0 + f:
                    cmd[q] = api.START if t == s0 else api.RUN
                    frame[q] = (d, t - s0)
        slots = dr.slots()
        for q, (d, k) in frame.items():
            ctx.upload_scan(int(slots[q]), scans[d][k])
        p0 = np.array([pose0[frame[q][0]] if q in frame else NAN7 for q in range(n_lanes)])
        odom, mapped, ran = dr.step(cmd, p0)
        mapped_all.append(mapped)
        if export_at is not None and t in export_at:
            exports[t] = dr.export_maps(ALL)
            dr.export_maps(SUR)
    return ctx, dr, mapped_all, exports, T


def test_drives_export(api, synth):
    ctx_a, a, mapped_a, exports, T = _two_lane_run(api, synth, export_at=(2, 4, 8))
    ctx_b, b, mapped_b, _, _ = _two_lane_run(api, synth)
    for t in range(T):                                                         # every step after an export: the twin's poses
        assert mapped_a[t].tobytes() == mapped_b[t].tobytes(), t
    assert a.stats() == b.stats()                                              # ll_drives_stats counts the steps' synchronisations only
    cms = a.cubemaps
    pts, off = a.export_maps(ALL)
    for q in range(2):
        same_bytes(pts[off[q]:off[q + 1]], concat(lambda s, c: cms.cube(q, s, c), EVERY), f"lane {q}")
    same_bytes(pts, exports[T - 1][0], "the export right after the last step")
    assert off[2] > off[1] > 0
    a.close(); ctx_a.close(); b.close(); ctx_b.close()


def test_kitti_drives_tool_writes_the_maps(tmp_path, api):
    """ll_kitti_drives --maps: <drive>_map.bin is Drives.export_maps(MAP_ALL) of that drive; without --maps the directory holds
    what it held before"""
    import scangen
    exe = _build(tmp_path, "ll_kitti_drives")
    scans = [scangen.hdl64_scan(k, order="kitti") for k in range(5)]
    dirs = []
    for i, n in enumerate((5, 3)):
        d = tmp_path / f"drive{i}"; d.mkdir()
        for k in range(n):
            scans[k].astype("<f4").tofile(d / f"{k:06d}.bin")
        dirs.append(str(d))
    plain = tmp_path / "plain"; plain.mkdir()
    maps = tmp_path / "maps"; maps.mkdir()
    for res, flag in ((plain, []), (maps, ["--maps"])):
        out = subprocess.run([exe] + flag + [str(res), "64", "1.0", "4608", "2"] + dirs, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stdout + out.stderr
    assert sorted(os.listdir(plain)) == ["0.txt", "1.txt"]
    assert sorted(os.listdir(maps)) == ["0.txt", "0_map.bin", "1.txt", "1_map.bin"]
    for name in ("0.txt", "1.txt"):
        assert (plain / name).read_bytes() == (maps / name).read_bytes(), name
    # the same two drives through the Python Drives with the tool's parameters
    lengths = (5, 3)
    ctx = api.Context(api.default_params(64, batch=4, max_ring_points=4608, input_stride_floats=3))
    dr = api.Drives(ctx, 2, 64 * 120 + 64, 400000, pool_points=1 << 22)
    pose0 = np.array([[0, 0, 0, 1.0, 1.0, 0, 0]] * 2)
    got = {}
    for t in range(max(lengths)):
        cmd = np.array([(api.START if t == 0 else api.RUN) if t < lengths[q] else api.IDLE for q in range(2)], np.int32)
        slots = dr.slots()
        for q in range(2):
            if cmd[q] != api.IDLE:
                ctx.upload_scan(int(slots[q]), scans[t])
        dr.step(cmd, pose0)
        which = [ALL if t == lengths[q] - 1 else NONE for q in range(2)]
        if ALL in which:
            pts, off = dr.export_maps(which)
            for q in range(2):
                if which[q] == ALL:
                    got[q] = pts[off[q]:off[q + 1]].copy()
    for q in range(2):
        data = np.fromfile(maps / f"{q}_map.bin", "<f4").reshape(-1, 4)
        assert len(data) > 0
        same_bytes(data, got[q], f"drive {q} map file")
    dr.close(); ctx.close()
