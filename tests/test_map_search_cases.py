"""The crafted inputs of mapsearchcases.py checked on the CPU: the independent numpy reference (brute-force f32 search, LAPACK eigh,
SVD least squares) equals the oracle (grid-free scan, cyclic Jacobi, pivoted Householder QR) on every case -- sources exactly,
values within 1e-9 * max(1, |value|) --, every family reaches what it is named for, no fit decision lies within 1e-9 of its
threshold, and a deliberately wrong reference fails at least one case of the matching family."""
import numpy as np
import pytest

import mapsearchcases as ms

REL = 1e-9                                              # test_gpu_mapping.REL


def oracle_blocks(orc, name):
    """orc.map_associate of a map case; a case with gids is given to the oracle with its map re-ordered so that position == gid"""
    c = ms.map_cases()[name]
    cm, sm = c["cm"], c["sm"]
    if c["gid_c"] is not None:
        cm = np.zeros_like(cm); cm[c["gid_c"]] = c["cm"]
        sm = np.zeros_like(sm); sm[c["gid_s"]] = c["sm"]
    orc.set_nn_mode(0)                                                                   # the oracle's linear scan
    return orc.map_associate(c["pose"][:4], c["pose"][4:], c["cs"], cm, c["ss"], sm)


def oracle_merged_blocks(orc, name):
    """the oracle's own eigen / QR routines on the merged five (np_merge5 is checked against a plain loop below)"""
    c = ms.merged_cases()[name]
    out = [[], [], [], [], [], []]
    pts, d, _, nb = ms.np_merge5(c["cn"], c["ci"])
    for i in np.flatnonzero((nb == 5) & (d[:, 4] < 1.0)):
        P = pts[i].astype(np.float64)
        ctr = np.zeros(3)
        for j in range(5):
            ctr = ctr + P[j]
        ctr = ctr / 5.0
        cov = np.zeros((3, 3))
        for j in range(5):
            cov = cov + np.outer(P[j] - ctr, P[j] - ctr)
        w, V = orc.sym_eig3(cov)
        if w[2] > 3 * w[1]:
            out[0].append(i); out[1].append(0.1 * V[:, 2] + ctr); out[2].append(-0.1 * V[:, 2] + ctr)
    pts, d, _, nb = ms.np_merge5(c["sn"], c["si"])
    for i in np.flatnonzero((nb == 5) & (d[:, 4] < 1.0)):
        P = pts[i].astype(np.float64)
        x = orc.qr_solve_5x3(P, -np.ones(5))
        ln = np.sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2])
        n = x / ln
        if (np.abs(P @ n + 1 / ln) <= 0.2).all():
            out[3].append(i); out[4].append(n); out[5].append(1 / ln)
    return (np.array(out[0], np.int32), np.array(out[1]).reshape(-1, 3), np.array(out[2]).reshape(-1, 3),
            np.array(out[3], np.int32), np.array(out[4]).reshape(-1, 3), np.array(out[5]))


@pytest.mark.parametrize("name", ms.MAP_NAMES)
def test_reference_equals_the_oracle_on_map_cases(orc, name):
    bad, worst = ms.block_differences(ms.reference(name)[:6], oracle_blocks(orc, name), REL)
    print(name, "largest |numpy - oracle| in a/b, n, d:", worst)
    assert not bad, (name, bad, worst)


@pytest.mark.parametrize("name", ms.MERGED_NAMES)
def test_reference_equals_the_oracle_on_merged_cases(orc, name):
    bad, worst = ms.block_differences(ms.reference(name)[:6], oracle_merged_blocks(orc, name), REL)
    print(name, "largest |numpy - oracle| in a/b, n, d:", worst)
    assert not bad, (name, bad, worst)


def test_to_world_equals_the_oracle(orc):
    rng = np.random.default_rng(3)
    pts = ms.f4(rng.uniform(-60, 60, (500, 3)))
    for pose in (ms.IDENT, ms.small_pose()):
        got = ms.np_to_world(pose, pts)
        assert got.tobytes() == np.ascontiguousarray(orc.point_associate_to_map(pose[:4], pose[4:], pts)[:, :3]).tobytes()
    assert ms.np_to_world(ms.IDENT, pts).tobytes() == np.ascontiguousarray(pts[:, :3]).tobytes()       # identity: the world point IS the stack point


def test_merge5_equals_a_plain_loop():
    for name in ms.MERGE_NAMES:
        c = ms.merged_cases()[name]
        pts, d, ids, nb = ms.np_merge5(c["cn"], c["ci"])
        for i in range(c["ci"].shape[1]):
            cand = sorted((float(c["cn"][p, i, j, 3]), int(c["ci"][p, i, j]), p, j) for p in range(3) for j in range(5) if c["ci"][p, i, j] != ms.INT_MAX)[:5]
            assert nb[i] == len(cand)
            for k, (dk, idk, p, j) in enumerate(cand):
                assert ids[i, k] == idk and d[i, k] == np.float32(dk) and pts[i, k].tobytes() == c["cn"][p, i, j, :3].tobytes()


# ------------------------------------------------------------------------------------------------ the bands
@pytest.mark.parametrize("name", ms.MAP_NAMES + ms.MERGED_NAMES)
def test_no_fit_decision_lies_in_the_band(name):
    x = ms.reference(name)[6]
    print(name, "smallest margins: line", x["margin_edge"], "plane", x["margin_plane"])
    assert x["margin_edge"] >= ms.MARGIN_MIN and x["margin_plane"] >= ms.MARGIN_MIN
    assert x["min_rank"] == (2 if name == "fit-plane-z0" else 3)                           # the only rank-deficient plane systems: all z == 0
    if name == "ties-gid":                                                                 # Map.associate reads no gids: its five-sets are other ones
        y = ms.reference_by_position(name)[6]
        assert y["margin_edge"] >= ms.MARGIN_MIN and y["margin_plane"] >= ms.MARGIN_MIN and y["min_rank"] == 3


# ------------------------------------------------------------------------------------------------ the families reach what they name
def test_tie_family_depends_on_the_index_rule():
    for name in ms.TIE_NAMES:
        c = ms.map_cases()[name]
        n = 0
        for stack, cloud, gid in ((c["cs"], c["cm"], c["gid_c"]), (c["ss"], c["sm"], c["gid_s"])):
            s = ms.np_to_world(c["pose"], stack)
            low = ms.np_search5(s, cloud, gid)[0]; high = ms.np_search5(s, cloud, gid, wrong=("tie_high",))[0]
            n += int((np.sort(low, axis=1) != np.sort(high, axis=1)).any(axis=1).sum())
        print(name, "queries whose five-set depends on the index rule:", n, "of", len(c["cs"]) + len(c["ss"]))
        assert n >= 200
    c = ms.map_cases()["ties-gid"]
    s = ms.np_to_world(c["pose"], c["cs"])
    assert (np.sort(ms.np_search5(s, c["cm"], c["gid_c"])[0], axis=1) != np.sort(ms.np_search5(s, c["cm"])[0], axis=1)).any()   # gid order is not position order


def test_grid_family_shapes():
    mc = ms.map_cases()
    assert (ms.grid_dims(mc["grid-one-cell"]["cm"])[0] == 1).all()
    for ax, name in enumerate("xyz"):
        d = ms.grid_dims(mc[f"grid-flat-{name}"]["cm"])[0]
        assert d[ax] == 1 and (np.delete(d, ax) > 1).all()
    assert ms.grid_dims(mc["grid-thin-long"]["cm"])[0].tolist() == [40, 1, 1]
    for n in (300, 301):
        cm = mc[f"grid-dense-{n}"]["cm"]
        cells = ms.cell_of(cm, cm); dims = ms.grid_dims(cm)[0]
        flat = (cells[:, 2] * dims[1] + cells[:, 1]) * dims[0] + cells[:, 0]
        counts = np.bincount(flat, minlength=int(dims.prod()))
        assert counts.max() == n and (counts == 0).sum() > 100                           # one long row (even / odd) beside empty cells
    dims = ms.grid_dims(mc["grid-two-clusters"]["cm"])[0]
    assert int(dims.prod()) > ms.MAX_CELLS                                                 # 1.01 m cells do not fit: the cell *= 1.5 path runs
    assert int(ms.grid_dims(mc["grid-two-clusters"]["cm"], np.float32(1.01) * np.float32(1.5))[0].prod()) <= ms.MAX_CELLS


def test_map_size_family():
    for n in (0, 1, 4, 5, 6):
        c = ms.map_cases()[f"mapsize-{n}"]
        ref = ms.reference(f"mapsize-{n}")
        assert len(c["cm"]) == n and len(c["sm"]) == n
        assert (len(ref[0]) > 0) == (n >= 5) and (len(ref[3]) > 0) == (n >= 5)


def test_box_family():
    mc = ms.map_cases()
    m = mc["box-outside"]["cm"][:, :3]
    mn, mx = m.min(axis=0), m.max(axis=0)
    q = np.concatenate([mc["box-outside"]["cs"], mc["box-outside"]["ss"]])[:, :3]
    out = np.where(q < mn, mn - q, 0) + np.where(q > mx, q - mx, 0)
    for ax in range(3):
        for side in (q[:, ax] < mn[ax], q[:, ax] > mx[ax]):
            by = out[side, ax]
            assert (np.abs(by - 0.5) < 1e-5).any() and (np.abs(by - 3.0) < 1e-5).any()
    assert len(ms.reference("box-outside")[0]) > 0 and len(ms.reference("box-outside")[3]) > 0      # some of the 0.5 m ones still find five within 1 m
    corners = mc["box-corners"]["cs"][:, :3]
    assert corners.min(axis=0).tobytes() == mn.tobytes() and corners.max(axis=0).tobytes() == mx.tobytes() and len(np.unique(corners, axis=0)) == 8
    c = mc["box-cell-boundary"]
    q = np.concatenate([c["cs"], c["ss"]])[:, :3]
    t = (q - mn) / ms.CELL                                                               # the device's f32 cell coordinate
    assert t.dtype == np.float32
    k = np.rint(t)
    on = (np.abs(t - k) < 4e-6) & (k >= 1)                                               # a few ulp of a cell coordinate below 8
    assert on.any(axis=1).all()
    below = (np.floor(t) == k - 1) & on; above = (np.floor(t) == k) & on
    assert below.any(axis=0).all() and above.any(axis=0).all()                           # both sides of a boundary, along every axis


def test_gate_family():
    for name in ms.GATE_NAMES:
        c = ms.map_cases()[name]
        ref = ms.reference(name)
        x = ref[6]
        assert np.array_equal(x["ok_corner"], c["expect"]), name                         # blocks exactly where the f32 distance is < 1
        d5 = x["d_corner"][:, 4]
        assert ((d5 < 1.0) == c["expect"]).all() and c["expect"].any() and (~c["expect"]).any()
        if c["kind"] == "rounding":
            exact = ms.np_search5(ms.np_to_world(c["pose"], c["cs"]), c["cm"], wrong=("dist_f64",))[1][:, 4]
            assert d5[0] == 1.0 and exact[0] < 1.0 and d5[1] < 1.0 and exact[1] >= 1.0
            continue
        assert np.array_equal(x["ok_surf"], c["expect"]), name
        want = np.tile(np.array(ms.GATE_R, np.float64) ** 2, 2).astype(np.float32)         # fl(r * r): 1 - 2^-23, 1, 1 + 2^-22
        assert d5.tobytes() == want.tobytes() and x["d_surf"][:, 4].tobytes() == want.tobytes()
        for stack, cloud, pos in ((c["cs"], c["cm"], x["pos_corner"]), (c["ss"], c["sm"], x["pos_surf"])):
            cq = ms.cell_of(cloud, stack); c5 = ms.cell_of(cloud, cloud[pos[:, 4]])
            step = (c5 - cq)[:, c["axis"]]
            assert (np.delete(c5 - cq, c["axis"], axis=1) == 0).all()
            assert (step == 0).all() if c["kind"] == "same" else sorted(set(step.tolist())) == [-1, 1]


def test_stack_family():
    seen_c, seen_s = set(), set()
    for name in ms.STACK_NAMES:
        c = ms.map_cases()[name]
        x = ms.reference(name)[6]
        seen_c.add(len(c["cs"])); seen_s.add(len(c["ss"]))
        for ok in (x["ok_corner"], x["ok_surf"]):
            for at in range(0, len(ok), ms.CMPB):
                chunk = ok[at:at + ms.CMPB]
                if len(chunk) >= 32:
                    assert chunk.any() and (~chunk).any(), (name, at)                   # valid and invalid points in every compaction workgroup
    assert seen_c == set(ms.STACK_SIZES) and seen_s == set(ms.STACK_SIZES)
    assert len(ms.map_cases()["stack-0-1025"]["cs"]) == 0 and len(ms.map_cases()["stack-1025-0"]["ss"]) == 0


def test_ladders_straddle_their_thresholds():
    for name, key, ok in [(n, "margins_corner", "ok_corner") for n in ("fit-ratio-0", "fit-ratio-50", "fit-ratio-1000", "fit-ratio-map-50", "fit-ratio-map-1000")] + \
                         [(n, "margins_surf", "ok_surf") for n in ("fit-residual", "fit-residual-map")]:
        x = ms.reference(name)[6]
        close = x[key] <= 1e-3
        print(name, "within 1e-3 of the threshold:", int(close.sum()), "yes among them:", int(x[ok][close].sum()), "smallest margin:", float(x[key].min()))
        assert x[ok][close].any() and (~x[ok][close]).any(), name


def test_degenerate_fits():
    x = ms.reference("fit-eigen-degenerate")[6]
    kind = np.arange(len(x["ok_corner"])) % 4
    assert x["ok_corner"][kind == 0].all() and not x["ok_corner"][kind != 0].any()         # exact lines only
    assert np.isinf(x["margins_corner"][kind == 3]).all()                                  # zero covariance: exact, no margin
    x = ms.reference("fit-plane-z0")
    assert len(x[3]) > 10 and (x[4][:, 2] == 0).all()                                      # blocks, and the normal's z is an exact zero
    off = np.abs(ms.reference("fit-plane")[5])
    for d in ms.PLANE_OFFSETS:
        assert (np.abs(off - d) < max(0.06, 0.05 * d)).sum() >= 100, d                  # negative_OA_dot_norm at every offset (0.05 m of noise tilts the fit)


# ------------------------------------------------------------------------------------------------ a wrong reference is seen
def _differs(a, b):
    return bool(ms.block_differences(a[:6], b[:6], REL)[0])


def _wrong_map(name, wrong):
    c = ms.map_cases()[name]
    return ms.np_map_associate(c["pose"], c["cs"], c["cm"], c["ss"], c["sm"], c["gid_c"], c["gid_s"], wrong=wrong)


def _wrong_merged(name, wrong):
    c = ms.merged_cases()[name]
    return ms.np_merge_associate(c["cn"], c["ci"], c["sn"], c["si"], wrong=wrong)


@pytest.mark.parametrize("wrong,names", [("tie_high", ms.TIE_NAMES), ("gate_le", ms.GATE_NAMES + ("merge-gate",)), ("dist_f64", ms.GATE_NAMES + ms.TIE_NAMES),
                                         ("ratio_ge", ("fit-eigen-degenerate", "fit-eigen-degenerate-map")),
                                         ("residual_no_abs", ("fit-residual", "fit-residual-map"))])
def test_a_wrong_reference_fails_its_family(wrong, names):
    seen = [n for n in names if _differs((_wrong_map if n in ms.MAP_NAMES else _wrong_merged)(n, (wrong,)), ms.reference(n))]
    print(wrong, "is seen by", seen)
    assert seen, wrong
    if wrong in ("gate_le", "tie_high"):
        assert len(seen) == len(names)                                                   # every member sees these two


def test_strict_residual_comparison_cannot_be_seen():
    """`all |r| < 0.2` in place of `<= 0.2` differs from the right rule only where a residual EQUALS the double 0.2.  No independent
    reference can be trusted to the last bit there (the margin would be 0, inside the band that must stay empty), so no case can
    tell the two apart -- stated here so that nobody takes the ladder for a guard against it.  What the ladder does see is a
    residual rule that is wrong by more than rounding (residual_no_abs above)."""
    for name in ("fit-residual", "fit-residual-map", "fit-plane", "fit-plane-z0"):
        assert not _differs((_wrong_map if name in ms.MAP_NAMES else _wrong_merged)(name, ("residual_lt",)), ms.reference(name))
