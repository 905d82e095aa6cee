"""The crafted inputs of assoccases.py checked on the CPU: the independent numpy reference (brute-force f32 search, the two walks as a
lexicographic minimum and as plain loops) equals the oracle exactly on every case the oracle can run (NEARBY_SCAN 2.5, limit 25), in
both of its search modes; every family reaches the route of ll_associate_block it is named for, shown from the reference's own
intermediate values and printed as counts; and a deliberately wrong reference fails at least one case of the family aimed at it."""
import numpy as np
import pytest

import assoccases as ac

ORACLE_NAMES = tuple(n for n in ac.NAMES if ac.cases()[n]["nearby"] == 2.5 and ac.cases()[n]["dmax"] == 25.0)


# ------------------------------------------------------------------------------------------------ the reference itself
@pytest.mark.parametrize("name", ORACLE_NAMES)
def test_reference_equals_the_oracle(orc, name):
    c = ac.cases()[name]
    ref = ac.reference(name)
    q, t = c["pose"][:4], c["pose"][4:]
    try:
        for mode in (0, 1):
            orc.set_nn_mode(mode)
            assert ac.same_result(orc.associate_corner(q, t, c["sharp"], c["corner"]), ref[0]), (name, "corner", mode)
            assert ac.same_result(orc.associate_plane(q, t, c["flat"], c["surf"]), ref[1]), (name, "plane", mode)
    finally:
        orc.set_nn_mode(0)


def test_to_start_equals_the_oracle(orc):
    pts = np.concatenate([ac.cases()["inside"]["sharp"], ac.cases()["borders"]["flat"]])
    for pose in ac.POSES:
        got = ac.np_to_start(pose, pts)
        assert got.tobytes() == np.ascontiguousarray(orc.transform_to_start(pose[:4], pose[4:], pts)[:, :3]).tobytes()
    assert ac.np_to_start(ac.IDENT, pts).tobytes() == np.ascontiguousarray(pts[:, :3]).tobytes()


@pytest.mark.parametrize("name", ac.NAMES)
def test_the_lexicographic_walks_equal_the_plain_loops(name):
    """every case of every family, the whole case"""
    c = ac.cases()[name]
    ref = ac.reference(name)
    assert ac.same_result(ac.np_associate(c["pose"], c["sharp"], c["corner"], False, c["nearby"], c["dmax"], loop=True), ref[0])
    assert ac.same_result(ac.np_associate(c["pose"], c["flat"], c["surf"], True, c["nearby"], c["dmax"], loop=True), ref[1])


@pytest.mark.parametrize("wrong", ac.WRONG)
def test_the_wrong_walks_agree_too(wrong):
    """the wrong variants mean the same mistake in both forms (so a variant that is seen is seen for what it says)"""
    for name in ("ties", "vnm", "invalid-ahead", "far", "nearby-3.5"):
        a = ac.wrong_reference(name, (wrong,)); b = ac.wrong_reference(name, (wrong,), loop=True)
        assert ac.same_result(a[0], b[0]) and ac.same_result(a[1], b[1]), (wrong, name)


def test_cases_are_finite_sized_and_named():
    assert set(ac.NAMES) == set(ac.cases()) and set(c["family"] for c in ac.cases().values()) == set(ac.FAMILIES)
    for name, c in ac.cases().items():
        for k in ("sharp", "corner", "flat", "surf"):
            assert c[k].dtype == np.float32 and c[k].shape[1] == 4 and np.isfinite(c[k]).all(), (name, k)
        assert np.isfinite(c["pose"]).all()
        assert len(c["sharp"]) <= ac.CAP_SHARP and len(c["flat"]) <= ac.CAP_FLAT and len(c["corner"]) <= ac.CAP_LSHARP and len(c["surf"]) <= ac.MAX_POINTS
        ne, npl = len(ac.reference(name)[0][0]), len(ac.reference(name)[1][0])
        print(name, "queries", len(c["sharp"]), len(c["flat"]), "targets", len(c["corner"]), len(c["surf"]), "correspondences", ne, npl)
        if name in ac.ZERO_OK:                          # the window holds ring rc alone: no other ring can give a corner's partner or a plane's c
            assert ne == 0 and npl == 0
        else:
            assert ne > 0 and npl > 0, name


# ------------------------------------------------------------------------------------------------ the families reach what they name
def _routes(name):
    c = ac.cases()[name]
    return ac.routes(c, False), ac.routes(c, True)


def _margin_ok(r):
    return bool((r["margin"][r["nn"] >= 0] >= 0.05).all())


def test_inside_family_uses_the_table():
    for r, what in zip(_routes("inside"), ("corner", "plane")):
        has = r["nn"] >= 0
        off = (r["ring"][np.maximum(r["b" if what == "corner" else "c"], 0)] - r["rc"])[r["ok"]]
        print("inside", what, "queries", len(has), "window inside the table", int(r["inside"].sum()), "pred == rc", int((r["pred"] == r["rc"])[has].sum()),
              "in-ring ties", int(r["tie"].sum()), "without correspondence", int((~r["ok"]).sum()), "partner ring offsets", sorted(set(off.tolist())))
        assert r["flags"] == 3 and has.all() and _margin_ok(r)
        assert (r["pred"] == r["rc"]).all() and r["inside"].all() and not r["tie"].any()         # every query: table used
        assert (~r["ok"]).sum() >= 40 and set(off.tolist()) == {-2, -1, 1, 2}
        present = set(r["ring"].tolist())
        assert len(set(range(min(present), max(present))) - present) >= 3                      # rings absent from the target


def test_edges_family_straddles_the_table():
    for r, what in zip(_routes("edges-delta"), ("corner", "plane")):
        d = r["rc"] - r["pred"]
        assert r["flags"] == 3 and (r["nn"] >= 0).all() and _margin_ok(r)
        for delta, inside in ((-6, False), (-5, True), (4, True), (5, False)):
            print("edges-delta", what, "rc - pred =", delta, "queries", int((d == delta).sum()), "inside", int(r["inside"][d == delta].sum()))
            assert (d == delta).sum() >= 30 and (r["inside"][d == delta] == inside).all()
        assert set(d.tolist()) == {-6, -5, 4, 5}
        assert (r["ok"] & r["inside"]).sum() >= 10 and (r["ok"] & ~r["inside"]).sum() >= 10
    for r, what in zip(_routes("edges-low"), ("corner", "plane")):
        assert r["flags"] == 3 and _margin_ok(r) and (r["pred"] <= 5).all() and set(r["rc"].tolist()) == {0, 1, 2}
        neg = r["pred"] - ac.ATAB_BACK < 0                                                      # the table's first ring is negative: the unsigned compare wraps
        print("edges-low", what, "queries", len(neg), "negative first ring", int(neg.sum()), "inside", int(r["inside"].sum()), "outside", int((~r["inside"]).sum()),
              "window below ring 0", int((ac.ring_lo(r["rc"], 2.5) < 0).sum()))
        assert neg.all() and r["inside"].all() and r["ok"].sum() >= 20 and (ac.ring_lo(r["rc"], 2.5) < 0).sum() >= 20
    for r, what in zip(_routes("edges-high"), ("corner", "plane")):
        assert r["flags"] == 3 and _margin_ok(r) and (r["pred"] >= 60).all()
        print("edges-high", what, "queries", len(r["pred"]), "inside", int(r["inside"].sum()), "outside", int((~r["inside"]).sum()), "rc beyond ring 63", int((r["rc"] > 63).sum()))
        assert r["inside"].sum() >= 20 and (~r["inside"]).sum() >= 20 and (r["rc"] > 63).sum() >= 10 and r["ring"].max() < ac.TAB


def test_bypass_family_never_uses_the_table():
    for r, what in zip(_routes("bypass"), ("corner", "plane")):
        print("bypass", what, "queries", len(r["pred"]), "window outside the table", int((~r["inside"]).sum()), "ring ids", int(r["ring"].min()), "..", int(r["ring"].max()))
        assert r["flags"] == 3 and r["ring"].min() >= 100 and r["ring"].max() <= 110 and (r["pred"] <= 63).all()
        assert (r["nn"] >= 0).all() and not r["inside"].any() and r["ok"].sum() >= 50


def test_tie_family_holds_the_ties():
    c = ac.cases()["ties"]
    total = 0
    for plane, r, what in ((False, ac.routes(c, False), "corner"), (True, ac.routes(c, True), "plane")):
        assert r["flags"] == 3 and _margin_ok(r) and (r["pred"] == r["rc"]).all()
        route_tie = r["tie"]
        n3 = 0
        for i in np.flatnonzero(r["nn"] >= 0):
            d = ac.walk_dist(r["sel"][i], c["surf" if plane else "corner"])
            n3 += int(((d == np.float32(ac.D * ac.D)) & (r["ring"] != r["rc"][i])).sum() >= 3)
        t = c["surf"] if plane else c["corner"]
        own = (ac.cell_of(t[:, 0])[None, :] == ac.cell_of(r["sel"][:, 0])[:, None]) & (ac.cell_of(t[:, 1])[None, :] == ac.cell_of(r["sel"][:, 1])[:, None])
        near = ac.nn_dist(r["sel"], t) < 1.0
        print("ties", what, "queries", len(route_tie), "in-ring tie at the window minimum, window inside the table", int((route_tie & r["inside"]).sum()),
              "table still usable", int((~r["tie"] & r["inside"]).sum()), "three or more equal candidates", n3)
        assert (near <= own).all()                                                              # every point within 1 m lies in the query's own cell: the first entry scanned
        assert (route_tie & r["inside"]).sum() >= 40 and (~r["tie"] & r["inside"]).sum() >= 10 and n3 >= 20
        total += int((route_tie & r["inside"]).sum())
    # what the rules decide here, from the reference: the down-walk keeps the higher index, the up-walk the lower, up beats down
    rc_, rp = ac.routes(c, False), ac.routes(c, True)
    kind = np.arange(256) % ac.TIE_KINDS
    tc, tp = c["corner"], c["surf"]
    for k in (3, 4, 5):
        b = rc_["b"][kind == k]
        assert (b < rc_["nn"][kind == k]).all() and ((tc[b, :3] == tc[b - 1, :3]).sum(axis=1) == 2).all()      # the pair's higher index: its mirror twin sits just below
    for k in (0, 1, 2):
        b = rc_["b"][kind == k]
        assert (b > rc_["nn"][kind == k]).all() and ((tc[b, :3] == tc[b + 1, :3]).sum(axis=1) == 2).all()      # the lower index
    for k in (9, 10):
        assert (rc_["b"][kind == k] > rc_["nn"][kind == k]).all()                                                   # up before down
    b = rp["b"][kind == 11]
    assert (b == rp["nn"][kind == 11] + 1).all() and (tp[b][:, :3] == tp[b - 1][:, :3]).all()                       # the twin is plane point b ...
    bc = rc_["b"][kind == 11]
    assert (rc_["ring"][bc] == rc_["rc"][kind == 11] + 1).all()                                                     # ... and never a corner's partner
    print("ties: queries whose table holds a tie", total)


def test_displaced_family():
    c = ac.cases()["displaced"]
    for plane, what in ((False, "corner"), (True, "plane")):
        r = ac.routes(c, plane)
        t = c["surf" if plane else "corner"]
        n = len(r["pred"])
        assert r["flags"] == 3 and _margin_ok(r) and r["inside"].all() and not r["tie"].any() and r["ok"].all()
        assert (r["own"] >= 9).all() and (r["own"] <= 40).all()
        cx, cy = ac.cell_of(t[:, 0]), ac.cell_of(t[:, 1])
        first = last = lane = second = left_before = 0
        for i in range(n):
            qx, qy = ac.cell_of(r["sel"][i, 0]), ac.cell_of(r["sel"][i, 1])
            own = np.flatnonzero((cx == qx) & (cy == qy))
            row = np.flatnonzero((cy == qy) & (np.abs(cx - qx) <= 1))                           # entry 0 of the three-row layout: cells in x order, index order inside a cell
            row = row[np.argsort(cx[row], kind="stable")]
            nn = int(r["nn"][i])
            assert nn in own                                                                    # the nearest lies in the own cell
            first += nn == own[0]; last += nn == own[-1]
            pos = int(np.flatnonzero(row == nn)[0])
            lane += pos % 8 != 0
            left_before += (cx[row[:pos]] < qx).any()
            d = ac.nn_dist(r["sel"][i:i + 1], t)[0]
            partner = int(r["c" if plane else "b"][i])
            second += partner == int(np.argsort(d, kind="stable")[1])
        print("displaced", what, "queries", n, "own cell", int(r["own"].min()), "..", int(r["own"].max()), "points; nearest first of its cell", first, "last", last,
              "held by another lane than 0", lane, "running minimum set from the cell to the left first", left_before, "partner = second-nearest overall", second)
        assert first >= 30 and last >= 30 and lane >= 40 and left_before >= 40 and second == n


def test_vnm_family_has_valid_tables_that_are_not_monotone():
    c = ac.cases()["vnm"]
    for plane, what in ((False, "corner"), (True, "plane")):
        r = ac.routes(c, plane)
        ring = r["ring"]
        back = int((np.diff(ring) < 0).sum())
        ahead = int((ring - np.minimum.accumulate(ring[::-1])[::-1]).max()); behind = int((np.maximum.accumulate(ring) - ring).max())
        has = r["nn"] >= 0
        up = r["b"] > r["nn"]
        wrong_side = has & (r["b"] >= 0) & (ring[np.maximum(r["b"], 0)] != r["rc"])
        print("vnm", what, "flags", r["flags"], "descents in the ring sequence", back, "furthest ahead / behind", ahead, behind,
              "b on the other side's ring (plane)" if plane else "partners", int(wrong_side.sum()) if plane else int(r["ok"].sum()))
        assert r["flags"] == 1 and back >= 40 and 1 <= ahead <= 2 and 1 <= behind <= 2 and ((ring >= 0) & (ring < ac.TAB)).all()
        if plane:
            assert (wrong_side & up).sum() >= 10 and (wrong_side & ~up).sum() >= 10
        else:
            assert (~r["ok"]).sum() >= 10                                                       # the corner partners the walks never meet
    assert ac.table_flags(ac.cases()["ties"]["corner"], 2.5) == 3


def test_invalid_family_takes_the_sequential_walk():
    for name in ac.family("invalid"):
        c = ac.cases()[name]
        for plane, what in ((False, "corner"), (True, "plane")):
            r = ac.routes(c, plane)
            ring = r["ring"]
            ups, downs = [], []
            for i in np.flatnonzero(r["nn"] >= 0):
                cc = int(r["nn"][i])
                _, _, su, sd = ac._window(ring, cc, 2.5, ())
                if su < len(ring):
                    ups.append((su - cc - 1) % 64)
                if sd >= 0:
                    downs.append((cc - 1 - sd) % 64)
            print(name, what, "flags", r["flags"], "ring ids up to", int(ring.max()), "up-walk breaks on lanes", len(set(ups)), "of 64, first", ups.count(0), "last", ups.count(63),
                  "down-walk first", downs.count(0), "last", downs.count(63), "in-ring ties", int(r["tie"].sum()))
            assert r["flags"] == 0 and r["tie"].sum() >= 40
            assert (ring.max() >= ac.TAB) == (name == "invalid-ring200")
            for lanes in (ups, downs):
                assert lanes.count(0) >= 1 and lanes.count(63) >= 1 and len(set(lanes) - {0, 63}) >= 30
    a = ac.cases()["invalid-ahead"]["corner"]
    ring = ac.rings_of(a)
    assert (np.maximum.accumulate(ring) - ring).max() >= 5                                     # ahead by more than nearby


def test_nearby_family():
    for nb in ac.NEARBY_VALUES:
        for r, what in zip(_routes(f"nearby-{nb}"), ("corner", "plane")):
            key = "b" if what == "corner" else "c"
            off = np.abs(r["ring"][np.maximum(r[key], 0)] - r["rc"])[r["ok"]]
            print(f"nearby-{nb}", what, "queries", len(r["pred"]), "inside", int(r["inside"].sum()), "partner ring offsets", sorted(set(off.tolist())), "correspondences", int(r["ok"].sum()))
            assert r["flags"] == 3 and _margin_ok(r) and (r["pred"] == r["rc"]).all()
            assert r["inside"].all() == (nb < 4.0) and r["inside"].any() == (nb < 4.0)          # 4.0: hi - lo = 8, the table may not be used
            assert set(off.tolist()) == set(range(1, int(nb) + 1))                              # the ring exactly on the bound is accepted, the next one breaks
    same = [ac.same_result(ac.reference("nearby-2.5")[0], ac.reference(f"nearby-{nb}")[0]) for nb in ac.NEARBY_VALUES]
    assert same == [False, False, True, False, False]


def test_far_family():
    c = ac.cases()["far"]
    for plane, what in ((False, "corner"), (True, "plane")):
        r = ac.routes(c, plane)
        t = c["surf" if plane else "corner"]
        p = r["c" if plane else "b"]
        ok = r["ok"]
        dx = (ac.cell_of(t[np.maximum(p, 0), 0]) - ac.cell_of(r["sel"][:, 0]))[ok]; dy = (ac.cell_of(t[np.maximum(p, 0), 1]) - ac.cell_of(r["sel"][:, 1]))[ok]
        d = np.array([ac.walk_dist(r["sel"][i], t)[p[i]] for i in np.flatnonzero(ok)])
        cls = dict(left=int(((np.abs(dy) <= 2) & (dx < -2)).sum()), right=int(((np.abs(dy) <= 2) & (dx > 2)).sum()), above=int((dy > 2).sum()), below=int((dy < -2).sum()))
        kind = np.arange(len(ok)) % 8
        print("far", what, "partners per class of annulus entry", cls, "partner distances", float(np.sqrt(d.min())), "..", float(np.sqrt(d.max())),
              "without neighbour", int((r["nn"] < 0).sum()), "without partner", int(((r["nn"] >= 0) & ~ok).sum()))
        assert min(cls.values()) >= 8 and d.min() >= 16.0 and d.max() < 25.0
        assert (r["nn"][kind == 7] < 0).all() and (r["nn"][kind != 7] >= 0).all() and not ok[kind == 5].any() and ok[(kind != 5) & (kind != 7)].all()
        assert (d[kind[ok] == 4] == np.float32(24.50390625)).all()                              # the one just inside, not the one at exactly 25
        assert r["flags"] == 3
    c = ac.cases()["far-round2"]
    rmax = int(np.ceil(np.sqrt(c["dmax"]))) + 1
    assert 2 * rmax + 6 == 20 and 2 * (int(np.ceil(np.sqrt(25.0))) + 1) + 6 == 18               # two rounds of 18 at dmax 36, one at 25
    for plane, what in ((False, "corner"), (True, "plane")):
        r = ac.routes(c, plane)
        t = c["surf" if plane else "corner"]
        cy = ac.cell_of(t[:, 1])[None, :] - ac.cell_of(r["sel"][:, 1])[:, None]; cx = ac.cell_of(t[:, 0])[None, :] - ac.cell_of(r["sel"][:, 0])[:, None]
        second = ((np.abs(cy) == rmax) & (np.abs(cx) <= rmax)).sum(axis=1)
        pd = np.array([ac.walk_dist(r["sel"][i], t)[r["c" if plane else "b"][i]] for i in range(len(second))])
        print("far-round2", what, "queries with target points in second-round entries", int((second >= 2).sum()), "partner distances", float(np.sqrt(pd.min())), "..", float(np.sqrt(pd.max())))
        assert (second >= 2).sum() >= 10 and r["ok"].all() and pd.min() > 25.0 and pd.max() < 36.0     # partners the default limit would refuse
        assert (ac.nn_dist(r["sel"], t)[(np.abs(cy) == rmax)] >= c["dmax"]).all()               # nothing in those rows is acceptable


def test_dense_family_mixes_the_two_layouts():
    c = ac.cases()["dense"]
    r = ac.routes(c, True)
    t = c["surf"]
    counts = sorted(set(r["own"].tolist()))
    nn_dx = ac.cell_of(t[r["nn"], 0]) - ac.cell_of(r["sel"][:, 0]); nn_dy = ac.cell_of(t[r["nn"], 1]) - ac.cell_of(r["sel"][:, 1])
    dense = r["own"] >= ac.ROWS_BELOW
    e3, e4 = int((dense & (nn_dx == -1) & (nn_dy == 0)).sum()), int((dense & (nn_dx == 1) & (nn_dy == 0)).sum())
    mixed = {qpb: sum(len(s) == 2 for s in ac.deal_octets(r["own"], qpb)) for qpb in (32, 256)}
    print("dense: own-cell counts", counts, "queries per count", [int((r["own"] == k).sum()) for k in counts], "nearest in entry 3", e3, "in entry 4", e4,
          "octets holding both layouts", mixed, "correspondences", int(r["ok"].sum()))
    assert counts == list(ac.DENSE_COUNTS) and r["flags"] == 3 and r["ok"].all()
    assert e3 >= 7 and e4 >= 7 and mixed[32] >= 1 and mixed[256] >= 1
    sparse_side = int((~dense & (nn_dx != 0)).sum())
    assert sparse_side >= 7                                                                     # and the three-row layout finds its nearest beside the own cell too


def test_border_family():
    c = ac.cases()["borders"]
    for plane in (False, True):
        r = ac.routes(c, plane)
        q = c["flat" if plane else "sharp"]; t = c["surf" if plane else "corner"]
        cx, cy = ac.cell_of(q[:, 0]), ac.cell_of(q[:, 1])
        assert {0, 127} <= set(cx.tolist()) and {0, 127} <= set(cy.tolist()) and {0, 127} <= set(ac.cell_of(t[:, 0]).tolist()) and {0, 127} <= set(ac.cell_of(t[:, 1]).tolist())
        beyond = (np.abs(q[:, :2]) > 64).any(axis=1)
        on_int = (q[:, 0] == np.round(q[:, 0])) & (q[:, 1] == np.round(q[:, 1]))
        i70 = int(np.flatnonzero(q[:, 0] == 70.0)[0])
        print("borders", "plane" if plane else "corner", "queries beyond the grid", int(beyond.sum()), "on integer coordinates", int(on_int.sum()), "correspondences", int(r["ok"].sum()))
        assert beyond.sum() >= 5 and on_int.sum() >= 7 and r["ok"].all() and t[r["nn"][i70], 0] == 72.0 and r["flags"] == 3
    c = ac.cases()["one-cell"]
    for k in ("corner", "surf"):
        assert len(set(zip(ac.cell_of(c[k][:, 0]).tolist(), ac.cell_of(c[k][:, 1]).tolist()))) == 1
    r = ac.routes(c, True)
    assert (r["own"] == 0).sum() >= 10 and (r["own"] == 40).sum() >= 10


def test_size_family():
    assert [len(ac.cases()[f"size-{n}"]["sharp"]) for n in ac.SIZES] == list(ac.SIZES) and [len(ac.cases()[f"size-{n}"]["flat"]) for n in ac.SIZES] == list(ac.SIZES)
    for n in ac.SIZES:
        for r in _routes(f"size-{n}"):
            assert r["flags"] == 3 and r["inside"].all()


# ------------------------------------------------------------------------------------------------ a wrong reference is seen
AIMED = {"nn_tie_high": ("ties",), "down_tie_low": ("ties", "invalid"), "down_before_up": ("ties", "vnm", "invalid"), "limit_le": ("far",),
         "nearby_floor": ("nearby", "inside", "edges"), "plane_same_eq": ("vnm",), "dist_f64": ("ties",), "break_inclusive": ("invalid",)}


@pytest.mark.parametrize("wrong", ac.WRONG)
def test_a_wrong_reference_fails_its_family(wrong):
    assert set(AIMED) == set(ac.WRONG)
    for fam in AIMED[wrong]:
        seen = []
        for name in ac.family(fam):
            w = ac.wrong_reference(name, (wrong,))
            ref = ac.reference(name)
            if not (ac.same_result(w[0], ref[0]) and ac.same_result(w[1], ref[1])):
                seen.append(name)
        print(wrong, "is seen by", seen, "of family", fam)
        assert seen, (wrong, fam)
        if wrong == "break_inclusive":
            assert len(seen) == len(ac.family(fam))                                          # by the ring-200 case and by the running-ahead case


def test_flooring_nearby_itself_cannot_be_seen():
    """rc +- floor(nearby) in place of rc +- nearby changes nothing: ring ids are integers, so rj > rc + 2.5 and rj > rc + 2 are the same
    test.  No case can tell the two apart -- stated here so that nobody takes the nearby family for a guard against it.  What the
    family does see is a window bound rounded the wrong way (nearby_floor above)."""
    for nb in ac.NEARBY_VALUES:
        c = ac.cases()[f"nearby-{nb}"]
        for plane, q, t in ((False, c["sharp"], c["corner"]), (True, c["flat"], c["surf"])):
            assert ac.same_result(ac.np_associate(c["pose"], q, t, plane, float(np.floor(nb)), c["dmax"]), ac.reference(c["name"])[int(plane)])
