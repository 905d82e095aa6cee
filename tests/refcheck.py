"""Shared by tests/test_ref_scan_registration.py (oracle, CPU) and tests/test_gpu_ref_extract.py (kernels, GPU): the inputs,
the edge scans and the comparison against the output of the reference's OWN scan registration (oracle/ref.py: the
reference's source file compiled unchanged against declared container doubles).  Test infrastructure only.

THE TIE RULE.  comp() (scanRegistration.cpp:42) orders by curvature alone and std::sort is not stable; the oracle and the
kernels define equal curvatures as ascending index, the reference leaves them to libstdc++.  A ring is therefore left out
of the label / pick / voxel-input comparison -- never out of the cloud, bounds and curvature comparison -- iff one of its
six segments holds two equal curvature values in the REFERENCE's cloudCurvature (not in the output under test).
"""
import os

import numpy as np

import scangen
from conftest import assert_bit_equal

SHAPES = {                       # tests/test_gpu_parity.py's, without S128_linear_model: the reference aborts on 128 rings (:170-174)
    "S64": dict(rings=64),
    "S16": dict(rings=16),
    "S32": dict(rings=32),
    "S64_azmajor_jitter_nan": dict(rings=64, order=1, az_jitter_deg=0.4, drop_prob=0.03, emit_nan=1),
    "S64_ringmajor_jitter": dict(rings=64, az_jitter_deg=0.4),
    "HDL64E_table_kitti_order": dict(rings=64, gen="hdl64", order="kitti"),
    "HDL64E_table_firing_order": dict(rings=64, gen="hdl64", order="firing"),
}
MAX_LEFT_OUT = 0.05              # share of the non-skipped rings of a shape that ties may take out of the pick comparison


def require_ref(ref):
    """The live-binary tests fail when the reference tree is there and the recipe produced no binary; they skip only where
    neither the reference nor oracle/_ref/ exists."""
    import pytest
    ref.build()
    have = [ref.available(v) for v in ref.VARIANTS]
    if all(have):
        return
    if ref.reference_present() or os.path.isdir(ref.OUT):
        raise AssertionError(f"oracle/_ref/ lacks a reference binary ({dict(zip(ref.VARIANTS, have))}): oracle.ref.build() did not produce it")
    pytest.skip("neither the reference tree nor oracle/_ref/ exists on this machine")


def shape_scans(shape, synth, n):
    """-> (rings, [n consecutive scans])"""
    kw = dict(SHAPES[shape]); rings = kw.pop("rings")
    if kw.pop("gen", None) == "hdl64":
        return rings, [scangen.hdl64_scan(k, **kw) for k in range(n)]
    cfg = synth.default_cfg(rings, **kw)
    return rings, [synth.scan(cfg, k) for k in range(n)]


def segments(s, e):
    """the six (sp, ep) of a ring, :253-254; Python's // equals C's / here: every operand is >= 0"""
    return [(s + (e - s) * j // 6, s + (e - s) * (j + 1) // 6 - 1) for j in range(6)]


def picked_rings(ss, se):
    return [i for i in range(len(ss)) if se[i] - ss[i] >= 6]            # :248


def tied_rings(r):
    """rings of the reference result r that the tie rule leaves out"""
    out = set()
    for i in picked_rings(r["scan_start"], r["scan_end"]):
        for sp, ep in segments(int(r["scan_start"][i]), int(r["scan_end"][i])):
            c = r["curv"][sp:ep + 1]
            if len(np.unique(c)) != len(c):
                out.add(i); break
    return out


def voxel_inputs_from_labels(cloud, label, ss, se):
    """what :361-367 hands to the ring's VoxelGrid: points k of the ring's six segments with label <= 0 -> {ring: points}"""
    out = {}
    for i in picked_rings(ss, se):
        idx = np.concatenate([np.arange(sp, ep + 1) for sp, ep in segments(int(ss[i]), int(se[i]))])
        out[i] = cloud[idx[label[idx] <= 0]]
    return out


def _by_ring(points, ring_of, rings):
    ring = ring_of(points)
    return {i: points[ring == i] for i in range(rings)}


def compare_with_reference(got, r, rings, ring_of, what):
    """got: cloud, scan_start, scan_end, curv, label, sharp, less_sharp, flat of the code under test (orc.extract's keys);
    r: the reference binary's result for the same scan.  Everything bitwise / exact.  Returns (rings left out, rings picked)."""
    assert_bit_equal(got["cloud"], r["cloud"], f"{what} laserCloud")
    n = len(r["cloud"])
    assert (np.asarray(got["scan_start"]) == r["scan_start"]).all() and (np.asarray(got["scan_end"]) == r["scan_end"]).all(), f"{what} scanStartInd / scanEndInd"
    assert_bit_equal(got["curv"][5:n - 5], r["curv"][5:n - 5], f"{what} cloudCurvature")
    picked = picked_rings(r["scan_start"], r["scan_end"])
    tied = tied_rings(r)
    keep = np.zeros(n, bool); keep[5:max(n - 5, 5)] = True
    for i in tied:                                                     # a ring's points: scan_start - 5 .. scan_end + 5
        keep[r["scan_start"][i] - 5:r["scan_end"][i] + 6] = False
    lab = np.asarray(got["label"]).astype(np.int32)
    bad = np.flatnonzero((lab != r["label"]) & keep)
    assert len(bad) == 0, f"{what} cloudLabel: {len(bad)} differ, first at {bad[:5].tolist()}: {lab[bad[:5]].tolist()} vs {r['label'][bad[:5]].tolist()}"
    for name in ("sharp", "less_sharp", "flat"):
        a, b = _by_ring(np.asarray(got[name], np.float32).reshape(-1, 4), ring_of, rings), _by_ring(r[name], ring_of, rings)
        for i in range(rings):
            if i not in tied:
                assert_bit_equal(a[i], b[i], f"{what} {name} of ring {i}")
        if not tied:
            assert_bit_equal(got[name], r[name], f"{what} {name}")
    vin = voxel_inputs_from_labels(got["cloud"], lab, r["scan_start"], r["scan_end"])
    assert len(r["voxel_inputs"]) == len(picked), f"{what}: {len(r['voxel_inputs'])} VoxelGrid calls for {len(picked)} rings"
    for call, i in enumerate(picked):
        if i not in tied:
            assert_bit_equal(vin[i], r["voxel_inputs"][call], f"{what} VoxelGrid input of ring {i}")
    return len(tied), len(picked)


# ----------------------------------------------------------------------------- edge scans
def _f32_d2(p):
    p = np.asarray(p, np.float32)
    return (p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2]      # the f32 expression of :72, left to right


def minimum_range_scan(rng, rings, minimum_range, n=24000):
    """points whose f32 squared range is exactly thres * thres, a few float steps either side (just inside = dropped, :72),
    over the elevations of the sensor, in one clockwise sweep"""
    T = np.float32(minimum_range) * np.float32(minimum_range)
    lo, hi = {16: (-14.0, 14.0), 32: (-29.0, 9.0), 64: (-24.0, 1.5)}[rings]
    el = np.deg2rad(rng.uniform(lo, hi, n)); az = -2 * np.pi * np.arange(n) / n
    d = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], axis=1)
    d[::50] = [0.6, -0.8, 0.0]                                             # 3-4-5: hits thres * thres exactly where thres is a small integer
    p = (d * float(np.float32(minimum_range))).astype(np.float32)
    big = np.abs(p).argmax(axis=1)                                         # nudge the largest component by -6 .. 6 float steps
    step = rng.integers(-6, 7, n).astype(np.int32)
    v = p[np.arange(n), big].copy()
    v = (v.view(np.int32) + np.where(v > 0, step, -step)).view(np.float32)
    p[np.arange(n), big] = v
    p[0] = d[0] * 3 * minimum_range; p[-1] = d[-1] * 3 * minimum_range     # first and last point survive: startOri / endOri well defined
    d2 = _f32_d2(p)
    assert (d2 == T).any() and (d2 == np.nextafter(T, np.float32(0))).any() and (d2 > T).any(), "minimum_range coverage"
    return np.concatenate([p, np.zeros((n, 1), np.float32)], axis=1)


def z_axis_scan(rng, rings):
    """a rough ring-major scan with returns exactly on the z axis (x = y = 0: z / sqrt(0) = +-inf, atan -> +-90 deg, ring
    rejected) scattered through it, as its very first and its very last point too (startOri = endOri's atan2(0, 0))"""
    p = rough_rings_scan(rng, rings, [200] * 6)
    n = len(p)
    at = np.concatenate([[0, n - 1], rng.integers(1, n - 1, 40)])
    p[at, 0] = 0.0; p[at, 1] = 0.0
    p[at, 2] = np.where(rng.random(len(at)) < 0.5, -1.0, 1.0) * rng.uniform(8.0, 40.0, len(at))
    p[at[:6], 1] = [0.0, -0.0, -0.0, 0.0, -0.0, 0.0]; p[at[:6], 0] = [0.0, 0.0, -0.0, -0.0, 0.0, -0.0]      # signed zeros: atan2's special cases
    return p


def _ring_elevation(rings, ring):
    if rings == 16:
        return -15.0 + 2.0 * ring
    if rings == 32:
        return -92.0 / 3.0 + 4.0 / 3.0 * (ring + 0.5)
    return -24.9 + 26.9 * ring / 63.0


def rough_rings_scan(rng, rings, lengths, bumps=None):
    """ring-major scan: ring i (of the first len(lengths) rings, spread over the sensor) is lengths[i] points of a wall at
    x ~ 10 m swept clockwise, with lateral noise of random scale (random f32 noise: distinct curvatures by construction)
    and random point spacing, so that suppression does and does not cross segment borders"""
    out = []
    ids = np.linspace(1, rings - 2, len(lengths)).astype(int) if len(lengths) < rings else np.arange(rings)
    assert len(np.unique(ids)) == len(lengths)
    for ring, n in zip(ids, lengths):
        el = np.deg2rad(_ring_elevation(rings, ring))
        y = -(np.arange(n) - n / 2) * rng.choice([0.02, 0.05, 0.3]) - 0.01 + rng.normal(0, 0.002, n)
        x = 10 + rng.normal(0, rng.choice([0.003, 0.02, 0.2]), n)
        if bumps is not None:
            x[bumps[bumps < n]] += 1.0
        out.append(np.stack([x, y, np.hypot(x, y) * np.tan(el), np.zeros(n)], axis=1))
    return np.concatenate(out).astype(np.float32)


def edge_groups(orc, rings):
    """-> (minimum_range, [(name, scan, tests_the_pick)]): the edge scans of one ring count, delivered in this order to ONE
    reference process.  Every scan is non-empty after filtering and below 400 000 points."""
    from test_gpu_a1_edges import _threshold_points
    P = orc.params(rings)
    mr = P.minimum_range
    rng = np.random.default_rng(7000 + rings)
    lo, hi = {16: (-15.0, 15.0), 32: (-92.0 / 3.0, 92.0 / 3.0 - 20.0), 64: (-24.9, 2.0)}[rings]
    out = [("ring_thresholds", _threshold_points(orc, P, rng)[0], False),          # on and +-1..3 float steps around every threshold, beyond both ends
           ("spread_sweep", scangen.spread_scan(rng, 60000, lo - 3.0, hi + 3.0, sweep=True), False),      # NaN / inf, inside minimum_range, rejected rings
           ("spread_random_order", scangen.spread_scan(rng, 60000, lo - 3.0, hi + 3.0, sweep=False), False),
           ("minimum_range", minimum_range_scan(rng, rings, mr), False),
           ("z_axis", z_axis_scan(rng, rings), False)]
    if rings == 16:
        for s0, last_gap in [(0.3, 0.01), (np.pi / 2, 0.2), (3.1, 0.05), (-3.1, 1.0), (-1.2, 3.3), (0.0, 2 * np.pi - 0.3)]:    # test_gpu_a1_edges.py's list
            out.append((f"wrap_s0={s0:.2f}_gap={last_gap:.2f}", scangen.wrap_scan(np.random.default_rng(int(abs(s0) * 1000) + 7), s0, last_gap), False))
    short = [3, 10, 11, 16, 17, 18, 19, 20, 22, 23, 24, 28, 29, 30, 34, 35, 36, 41, 47, 53, 64, 77, 100, 129, 130]
    k = min(rings - 2, len(short))
    for seed in range(3):                                # rings below 6 + 11 points are skipped (:248); 17 .. 130: segments of 1 .. 20 points
        r = np.random.default_rng(7100 + 10 * rings + seed)
        must = [10, 16, 17, 18, 130]                     # in every scan: skipped rings, the first ring that is not, one-point segments, a long one
        lengths = r.permutation(must + list(r.permutation([v for v in short if v not in must])[:k - len(must)]))
        out.append((f"short_rings_{seed}", rough_rings_scan(r, rings, [int(v) for v in lengths]), True))
    r = np.random.default_rng(7200 + rings)
    out.append(("over_20_corners", rough_rings_scan(r, rings, [600, 400, 900], bumps=np.arange(6, 900, 2)), True))   # every 2nd point a 1 m corner
    for name, s, _ in out:
        assert 0 < len(s) <= 400000, name
    return mr, out
