"""The oracle's extract stage (a1-a3 and the less-flat selection) against the reference's OWN scanRegistration.cpp, compiled
unchanged against declared container doubles (oracle/ref.py, oracle/ref_standins/) -- not against a restatement.

Everything is bitwise / exact: laserCloud, scanStartInd / scanEndInd, cloudCurvature and cloudLabel on [5, n-5), the sharp /
less-sharp / flat topics point for point in order, and the per-ring VoxelGrid inputs.  What the doubles replace pins nothing:
PCL's VoxelGrid (a4's centroids and order; "/laser_cloud_less_flat" of this binary is never compared), removeNaNFromPointCloud,
the message conversions.  Ties: see tests/refcheck.py.  The scans of a shape go to ONE reference process in order (its arrays
are globals that live on between scans; the oracle has no such state), as 16-byte and as 12-byte input points.
"""
import os

import numpy as np
import pytest

import refcheck
from conftest import assert_bit_equal

N_SCANS = 24                    # consecutive scans per shape
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def ref():
    from oracle import ref as r
    refcheck.require_ref(r)
    return r


_cache = {}


def _shape(shape, synth):
    if shape not in _cache:
        _cache[shape] = refcheck.shape_scans(shape, synth, N_SCANS)
    return _cache[shape]


@pytest.mark.parametrize("point_bytes", [16, 12])
@pytest.mark.parametrize("shape", list(refcheck.SHAPES))
def test_oracle_equals_reference_binary(shape, point_bytes, orc, ref, synth):
    rings, scans = _shape(shape, synth)
    P = orc.params(rings)                                            # the launch files' minimum_range
    given = scans if point_bytes == 16 else [np.ascontiguousarray(s[:, :3]) for s in scans]
    want = ref.extract(given, rings, P.minimum_range, variant="f32")
    left = total = 0
    for k, (s, r) in enumerate(zip(given, want)):
        got = orc.extract(s, P)
        assert got["rc"] == 0
        t, p = refcheck.compare_with_reference(got, r, rings, ref.ring_of, f"{shape} scan {k} ({point_bytes}-byte points)")
        left += t; total += p
    assert total >= N_SCANS * rings // 2
    print(f"\n{shape} ({point_bytes}-byte points): {left} of {total} rings left out of the pick comparison for curvature ties = {100.0 * left / total:.2f} %")
    assert left <= refcheck.MAX_LEFT_OUT * total, f"{shape}: ties leave out {left} of {total} rings, more than 5 %"


@pytest.mark.parametrize("rings", [16, 32, 64])
def test_oracle_equals_reference_binary_on_edge_scans(rings, orc, ref):
    """ring thresholds (on and one float either side, beyond both ends), azimuth wrap / half sweep, NaN / inf, minimum_range
    exactly and just inside, the z axis, rings below and around 6 + 11 points, more than 20 corners in a segment, ring-rejected
    points (count < cloudSize): all of one ring count to one reference process, one after the other"""
    mr, cases = refcheck.edge_groups(orc, rings)
    P = orc.params(rings)
    want = ref.extract([s for _, s, _ in cases], rings, mr, variant="f32")
    for (name, s, tests_pick), r in zip(cases, want):
        got = orc.extract(s, P)
        assert got["rc"] == 0
        left, total = refcheck.compare_with_reference(got, r, rings, ref.ring_of, f"{rings}-ring edge scan {name}")
        print(f"\n{rings}-ring edge scan {name}: n_in {len(s)}, laserCloud {len(r['cloud'])}, {left} of {total} rings left out for ties")
        if tests_pick:
            assert left == 0 and total > 0, f"{name}: built to be free of curvature ties"
        finite = np.isfinite(s[:, :3]).all(axis=1)
        if name in ("ring_thresholds", "spread_sweep", "spread_random_order", "z_axis"):
            kept = finite & (refcheck._f32_d2(np.where(finite[:, None], s[:, :3], 0)) >= np.float32(mr) * np.float32(mr))
            assert len(r["cloud"]) < kept.sum(), f"{name}: no ring-rejected point"                 # count < cloudSize (:145-168)
        if name.startswith("spread"):
            assert (~finite).any()                      # ranges start at 1.5 m: inside the 64-ring launch file's 5 m; "minimum_range" covers 0.3 m
            assert mr < 1.5 or (refcheck._f32_d2(s[finite]) < mr * mr).any()
        if name.startswith("short_rings"):
            span = r["scan_end"] - r["scan_start"]
            n_ring = span + 11
            assert ((n_ring > 0) & (span < 6)).any() and (span == 6).any() and (span >= 100).any(), "skipped, 17-point and long rings"
        if name == "over_20_corners":
            lab = r["label"]; ss, se = r["scan_start"], r["scan_end"]
            full = [(sp, ep) for i in refcheck.picked_rings(ss, se) for sp, ep in refcheck.segments(int(ss[i]), int(se[i]))
                    if (lab[sp:ep + 1] == 2).sum() == 2 and (lab[sp:ep + 1] == 1).sum() == 18]
            assert len(full) >= 6, "no segment reached the 21st corner (:281-284)"


@pytest.mark.parametrize("shape", list(refcheck.SHAPES))
def test_float_and_double_overloads_at_line_139(shape, orc, ref, synth):
    """The unqualified atan / sqrt of scanRegistration.cpp:139 bind to the float overloads under libstdc++'s <math.h> (variant
    f32, assumption A1) and to the double functions under <cmath> alone (f64, the file as written).  This MEASURES the reference
    against itself -- points whose ring differs, published feature points that differ -- and prints it (DESIGN section 6 records
    the figures); no pass mark.  It ASSERTS what does not pass through :139: startOri / endOri and relTime (the intensity
    fraction of every point both variants put in the same ring, where both kept the same points: halfPassed is updated by kept
    points only), filtering (both clouds hold the same points unless a ring id moved one across an end of the ring range), and
    curvature given the same cloud."""
    rings, scans = _shape(shape, synth)
    mr = orc.params(rings).minimum_range
    A = ref.extract(scans, rings, mr, variant="f32")
    B = ref.extract(scans, rings, mr, variant="f64")
    ring_moved = only_one = n_points = 0
    feat = dict(sharp=[0, 0], less_sharp=[0, 0], flat=[0, 0])
    key = lambda c: np.ascontiguousarray(c[:, :3]).view([("k", "V12")]).ravel()
    for k, (a, b) in enumerate(zip(A, B)):
        ka, kb = key(a["cloud"]), key(b["cloud"])
        ua, ia = np.unique(ka, return_index=True); ub, ib = np.unique(kb, return_index=True)
        assert len(ua) == len(ka) and len(ub) == len(kb), "the shapes' points are distinct"
        common, ca, cb = np.intersect1d(ua, ub, return_indices=True)
        pa, pb = a["cloud"][ia[ca]], b["cloud"][ib[cb]]
        moved = ref.ring_of(pa) != ref.ring_of(pb)
        ring_moved += int(moved.sum()); only_one += len(ka) + len(kb) - 2 * len(common); n_points += len(ka)
        if len(common) == len(ka) == len(kb):
            frac = lambda p: p[:, 3].astype(np.float64) - ref.ring_of(p)
            # same relTime; the f32 sum scanID + 0.1 * relTime rounds by the ring's magnitude, so compare where the ring agrees
            assert_bit_equal(pa[~moved, 3], pb[~moved, 3], f"{shape} scan {k}: intensity of points in the same ring")
            assert np.abs(frac(pa) - frac(pb)).max() < 1e-5
        else:
            # every point only one variant kept sits in an end ring of that variant (rejected beyond it by the other)
            for c, u, i in ((a, ua, ia), (b, ub, ib)):
                lone = c["cloud"][i[~np.isin(u, common)]]
                assert np.isin(ref.ring_of(lone), [0, rings - 1]).all()
        n = len(b["cloud"])
        if a["cloud"][:, :3].tobytes() == b["cloud"][:, :3].tobytes():
            assert_bit_equal(a["curv"][5:n - 5], b["curv"][5:n - 5], f"{shape} scan {k}: curvature of the same cloud")
        assert_bit_equal(orc.curvature(b["cloud"])[5:n - 5], b["curv"][5:n - 5], f"{shape} scan {k}: f64 variant's curvature of its own cloud")
        key16 = lambda c: np.ascontiguousarray(c).view([("k", "V16")]).ravel()
        for name in feat:                                                # a published point = xyz and intensity
            sa = set(key16(a[name]).tolist()); sb = set(key16(b[name]).tolist())
            feat[name][0] += len(sa ^ sb); feat[name][1] += len(sa)
    print(f"\n{shape}: {N_SCANS} scans, {n_points} points: ring id differs (f64 vs f32) for {ring_moved}, kept by one variant only {only_one}; "
          + ", ".join(f"{n} points differing {d} of {t}" for n, (d, t) in feat.items()))


def _golden_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(HERE, "golden", "make_golden.py"))
    m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
    return m


RECORDED = ["scanreg_s16", "scanreg_s32", "scanreg_s64_azmajor_jitter_nan"]


@pytest.mark.parametrize("name", RECORDED)
def test_oracle_reproduces_recorded_reference_output(name, orc):
    """tests/golden/reference/*.npz hold what the f32 reference binary published (see tests/golden/make_golden.py); this needs
    neither the reference tree nor oracle/_ref/ and never skips.  Same assertions and tie rule as the live comparison."""
    from oracle import ref as refmod                              # ring_of / scan_bounds only: no binary is run
    mg = _golden_module()
    assert list(mg.REF_CASES) == RECORDED
    G = np.load(os.path.join(HERE, "golden", "reference", name + ".npz"))
    rings, scan = mg.reference_input(name)
    assert rings == int(G["rings"]) and len(scan) == int(G["n_in"])
    r = dict(cloud=G["cloud"], curv=G["curv"], label=G["label"].astype(np.int32), sharp=G["sharp"], less_sharp=G["less_sharp"], flat=G["flat"])
    r["scan_start"], r["scan_end"] = refmod.scan_bounds(r["cloud"], rings)
    assert (G["voxel_ring"] == refcheck.picked_rings(r["scan_start"], r["scan_end"])).all()
    cut = np.cumsum(G["voxel_count"])[:-1]
    r["voxel_inputs"] = [r["cloud"][idx] for idx in np.split(G["voxel_index"], cut)]
    got = orc.extract(scan, orc.params(rings))
    left, total = refcheck.compare_with_reference(got, r, rings, refmod.ring_of, f"recorded {name}")
    print(f"\nrecorded {name}: {left} of {total} rings left out of the pick comparison for curvature ties")
    assert left <= refcheck.MAX_LEFT_OUT * total
