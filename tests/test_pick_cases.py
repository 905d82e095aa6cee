"""The crafted rings of pickcases.py on the CPU: the numpy reference against the oracle, the census conditions of every family as hard
assertions, and every deliberately wrong variant of the reference seen by the family meant to catch it.  No GPU, a few seconds.

What the census conditions say is which route of k_ring_pick (ll_pick.hip) a family forces; test_gpu_pick_cases.py runs the same cases
on the device.  A failing id names the family, and the family names the route:
  routes      the pick loop's instantiations (ranked walk, one / two / three compacted rows, the segment's own rows) and their tie paths
  caps        the break at the 21st corner, the fourth flat pick that does not mark, segments with nothing to pick
  extents     the ten gap flags around a pick, across rows of the ballot words, below the first centre, beyond the last row
  lengths     row counts, unequal segments, short and empty rings, the tile seam at segment position 192
  imports     marks that cross into later segments, the bitmap's word borders
  tiers       the 8-, 12- and 22-row kernels and their work lists, every tile seam
  thresholds  the f32 images of the two double thresholds, at values equal to them and one ulp either side
"""
import numpy as np
import pytest

import pickcases as pc


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ reference == oracle
@pytest.mark.parametrize("name", pc.NAMES)
def test_input_order_is_kept_and_reference_equals_oracle(orc, name):
    """the oracle's organised cloud is the input (the precondition that lets np_pick work on the input); at the default thresholds
    its curvature, labels and clouds equal np_pick's bit for bit (orc.params has no threshold fields: the other cases stop after the
    first check)"""
    c = pc.cases()[name]
    o = orc.extract(c["scan"], orc.params(pc.RINGS, minimum_range=pc.MIN_RANGE))
    n = len(c["scan"])
    assert o["rc"] == 0 and len(o["cloud"]) == n
    assert np.array_equal(_bits(o["cloud"][:, :3]), _bits(c["scan"][:, :3])), "the organise stage must keep the input's order"
    for k in range(pc.RINGS):
        assert o["scan_start"][k] == c["off"][k] + 5 and o["scan_end"][k] == c["off"][k + 1] - 6
    if not pc.is_default(c):
        return
    ref = pc.reference(name)
    assert np.array_equal(_bits(o["curv"][5:n - 5]), _bits(ref["curv"][5:n - 5]))
    assert np.array_equal(o["label"], ref["label"])
    for kind in ("sharp", "less_sharp", "flat"):
        assert np.array_equal(_bits(o[kind][:, :3]), _bits(c["scan"][ref[kind], :3])), kind


def test_curvature_and_gap_flags_against_plain_loops():
    """the vectorised eleven taps and the gap test against the statements of :228-231 and :290-293 written out, at a few hundred points"""
    c = pc.cases()["imports-short"]
    p = c["scan"][:, :3]
    n = len(p)
    curv, g = pc.np_curvature(p), pc.np_gap_sq(p)
    f = np.float32
    for i in range(5, n - 5):
        d = [f(0), f(0), f(0)]
        for a in range(3):
            s = p[i - 5, a]
            for k in (-4, -3, -2, -1):
                s = f(s + p[i + k, a])
            s = f(s - f(f(10) * p[i, a]))
            for k in (1, 2, 3, 4, 5):
                s = f(s + p[i + k, a])
            d[a] = s
        assert _bits(curv[i]) == _bits(f(f(f(d[0] * d[0]) + f(d[1] * d[1])) + f(d[2] * d[2])))
    for i in range(1, n):
        dx, dy, dz = (f(p[i, a] - p[i - 1, a]) for a in range(3))
        assert _bits(g[i]) == _bits(f(f(f(dx * dx) + f(dy * dy)) + f(dz * dz)))
    assert pc.threshold(np.float32(0.1), 0.1) == 0.1 and pc.threshold(np.float32(0.05), 0.05) == 0.05
    assert pc.threshold(0.125, 0.1) == 0.125 and pc.threshold(0.3, 0.1) == float(np.float32(0.3)) != 0.3


# ------------------------------------------------------------------------------------------------ the census, family by family
MULTI = ("row2", "row3", "own")


def test_routes_census():
    segs = pc.family_census("routes")
    by = {cls: [s for s in segs if s["cls"] == cls] for cls in ("none", "walk", "row1") + MULTI}
    assert all(s["tier"] == 0 for s in segs)
    for cls, ss in by.items():
        assert ss, cls
        print("routes", cls, len(ss), "segments")
    assert all(s["n_corner"] == 0 for s in by["none"]) and all(not s["any_tie"] and not any(s["pick_ties"]) for s in by["walk"])
    assert any(s["broke"] for s in by["walk"]) and any(not s["broke"] for s in by["walk"])
    for cls in ("row1",) + MULTI:                                        # each arg-max instantiation with untied and with tied picks
        assert any(s["n_corner"] >= 2 and not any(s["pick_ties"]) for s in by[cls]), (cls, "untied picks")
        assert any(any(s["pick_ties"]) for s in by[cls]), (cls, "tied picks")
    for cls in MULTI:                                                    # the lane-local row scan and the second wave reduction
        assert any("rows" in s["pick_ties"] for s in by[cls]), (cls, "a tie in one lane of different rows")
        assert any("lanes" in s["pick_ties"] for s in by[cls]), (cls, "a tie in different lanes")
    assert any(s["any_tie"] and not any(s["pick_ties"]) and s["broke"] for s in by["row1"]), "candidates tie, picks do not: the tie lies behind the break"
    assert any("lanes" in s["flat_ties"] for s in segs) and any("rows" in s["flat_ties"] for s in segs), "flat ties in the segment's own rows"


def test_caps_census():
    segs = pc.family_census("caps")
    eligible = {s["n_corner"] + int(s["broke"]) for s in segs if s["nc"] <= 23}
    assert eligible == set(pc.CAPS_CORNERS) - {23} | {21}, eligible      # 21 and 23 candidates: twenty picks and the break
    assert {s["nc"] for s in segs} >= set(pc.CAPS_CORNERS)
    assert any(s["nc"] == 20 and s["n_corner"] == 20 and not s["broke"] for s in segs)
    assert any(s["nc"] == 21 and s["n_corner"] == 20 and s["broke"] for s in segs)
    assert any(s["nc"] > 192 and s["broke"] for s in segs)
    assert {s["nf"] for s in segs} >= set(pc.CAPS_FLATS) and any(s["nf"] > 100 for s in segs)
    assert {s["n_flat"] for s in segs} >= {0, 1, 3, 4}
    assert any(s["nf"] == 4 and s["n_flat"] == 4 for s in segs) and any(s["nf"] == 5 and s["n_flat"] == 4 for s in segs)
    # a fourth flat pick whose would-be marks hold the next segment's first flat pick
    hit = 0
    for a, b in zip(segs, segs[1:]):
        if a["flat4"] and a["ring"] == b["ring"] and b["picks"]:
            ind, bn, fn = a["flat4"]
            hit += any(p["kind"] == "flat" and ind < p["ind"] <= ind + fn and p["ind"] > a["ep"] for p in b["picks"])
    assert hit >= 1


def _extent_conditions(picks, what, below_qs=(0, 1, 2, 3)):
    assert {(p["bn"], p["fn"]) for p in picks} == {(b, f) for b in range(6) for f in range(6)}, what
    assert {p["lane"] for p in picks if p["back"] == "prev_row"} >= {0, 1, 2, 3}, what
    assert {p["lane"] for p in picks if p["fwd"] == "next_row"} >= {59, 60, 61, 62, 63}, what
    assert {p["q"] for p in picks if p["back"] == "below"} >= set(below_qs), what
    assert {p["from_end"] for p in picks if p["fwd"] == "beyond"} >= {0, 1, 2}, what
    assert any(p["q"] <= 4 for p in picks) and any(p["from_end"] <= 4 for p in picks)


def test_extents_census():
    """all 36 (bn, fn) and the four places of the stopping flag, for the corner picks of each route that carries extents its own way (the
    ranked walk, the compacted rows, the segment's own rows) and for the flat picks"""
    for name, classes in (("extents-corner-walk", ("walk",)), ("extents-corner-rows", ("row2", "row3")), ("extents-corner-own", ("own",))):
        picks = [p for s in pc.case_census(name) if s["cls"] in classes for p in s["picks"] if p["kind"] == "corner"]
        _extent_conditions(picks, name)
    flats = [p for s in pc.case_census("extents-flat") for p in s["picks"] if p["kind"] == "flat"]
    _extent_conditions(flats, "extents-flat")
    assert all(s["nc"] == 0 for s in pc.case_census("extents-flat")), "at the raised threshold nothing is a corner"
    c = pc.cases()
    assert c["extents-flat"]["curv"] > 0.1 and c["extents-flat"]["gap"] < 0.05 and c["extents-corner-own"]["gap"] > 0.05


def test_lengths_census():
    segs = pc.family_census("lengths")
    lens = {s["len"] for s in segs}
    assert lens >= set(pc.LENGTH_SEGS), sorted(set(pc.LENGTH_SEGS) - lens)
    assert {s["nr"] for s in segs} >= set(pc.LENGTH_RINGS) | {17, 18, 22, 23, 2304}
    assert {s["nrows"] for s in segs} == {1, 2, 3, 4, 5, 6}
    for n in pc.NAMES:                                                   # the short and empty rings are there, and have no segments
        if pc.cases()[n]["family"] == "lengths":
            sizes = np.diff(pc.cases()[n]["off"])
            assert all(((sizes == k).sum() == 0) or k >= 17 or not any(s["nr"] == k for s in pc.case_census(n)) for k in (0, 1, 16))
    all_sizes = np.concatenate([np.diff(pc.cases()[n]["off"]) for n in pc.NAMES if pc.cases()[n]["family"] == "lengths"])
    assert set(pc.LENGTH_SHORT) | {2304} <= set(all_sizes.tolist())
    rings = {}
    for s in segs:
        rings.setdefault((s["case"], s["ring"]), set()).add(s["len"])
    assert any(len(v) == 2 for v in rings.values()), "segments of unequal length side by side"
    seam = [p for s in segs for p in s["picks"] if p["seam"]]
    assert any(p["kind"] == "corner" and p["q"] < 192 for p in seam) and any(p["kind"] == "corner" and p["q"] >= 192 for p in seam)
    assert any(p["kind"] == "flat" and p["q"] >= 192 for p in seam) and any(p["kind"] == "flat" for p in seam)


def test_imports_census():
    segs = pc.family_census("imports")
    short = [s for s in segs if s["case"] == "imports-short"]
    assert {s["len"] for s in short} >= set(range(1, 13))
    span = 0
    for a, b in zip(short, short[1:]):
        if a["ring"] == b["ring"]:
            span += sum(p["reach"] > b["len"] for p in a["picks"])
    assert span >= 5, "marks that run through a whole segment into the one behind it"
    marks = [s for s in segs if s["case"] == "imports-marks"]
    blocked = {(code, kind) for s in marks for (_, code, kind) in s["blocked"]}
    assert blocked == {(1, "corner"), (1, "flat"), (2, "corner"), (2, "flat")}, blocked
    assert {p["reach"] for s in marks for p in s["picks"] if p["kind"] == "flat"} >= {1, 2, 3, 4, 5}
    assert any(s["nc"] == 0 and any(k == "corner" for (_, _, k) in s["blocked"]) for s in marks), "a corner only an earlier segment's mark keeps out"
    for kind in ("corner", "flat"):
        assert any(p["word_cross"] and p["kind"] == kind for s in segs for p in s["picks"]), (kind, "marks across a word of the bitmap")
        assert any(not p["word_cross"] and p["kind"] == kind and p["reach"] for s in segs for p in s["picks"]), kind


def test_tiers_census():
    segs = pc.family_census("tiers")
    assert {s["tier"] for s in segs} == {0, 1, 2, 3}
    assert {s["nr"] for s in segs} >= {2305, 3072, 3073, 4608, 4609, 8192}
    for case, cap in (("tiers-4608", 4608), ("tiers-8192", 8192)):
        sizes = np.diff(pc.cases()[case]["off"])
        assert sizes.max() == cap == pc.cases()[case]["max_ring"] and (sizes == 0).any() and ((sizes > 0) & (sizes < 17)).any()
    for tier in (1, 2, 3):
        ss = [s for s in segs if s["tier"] == tier]
        assert any(s["cls"] == "own" and "rows" in s["pick_ties"] for s in ss), (tier, "tied picks in one lane of different rows")
        assert any(s["cls"] == "own" and "lanes" in s["pick_ties"] for s in ss), tier
        assert any(s["cls"] == "own" and not any(s["pick_ties"]) for s in ss), (tier, "untied")
        seams = {p["q"] // 192 + (p["q"] % 192 > 96) for s in ss for p in s["picks"] if p["seam"] and p["kind"] == "corner"}
        want = set(range(1, (max(s["len"] for s in ss) - 13) // 192 + 1))
        assert seams >= want, (tier, sorted(want - seams))
        fseams = {p["q"] // 192 + (p["q"] % 192 > 96) for s in ss for p in s["picks"] if p["seam"] and p["kind"] == "flat"}
        assert fseams >= want, (tier, "flat", sorted(want - fseams))
        assert max(s["nrows"] for s in ss) > pc.TIER_ROWS[tier - 1]


def test_thresholds_census():
    """the special points have exactly the curvature / squared gap they were made for, and the reference's labels say what a comparison
    of an f32 with the double threshold says"""
    for name in ("thresholds-default", "thresholds-eighth"):
        c, ref = pc.cases()[name], pc.reference(name)
        v, sp = c["spec_values"], c["spec"]
        g = pc.np_gap_sq(c["scan"])
        lab = {t: int(ref["label"][i]) for t, i in sp.items()}
        for t, i in sp.items():
            if t.startswith("gap"):
                assert _bits(g[i + 1]) == _bits(v[t]), t
            else:
                assert _bits(ref["curv"][i]) == _bits(v[t.split("_")[1]]), t
                assert ref["flag"][i] and ref["flag"][i + 1], (t, "alone between two gaps")
        thr_c, thr_g = pc.threshold(c["curv"], 0.1), pc.threshold(c["gap"], 0.05)
        assert float(v["below"]) < thr_c < float(v["above"]) and float(v["gap_below"]) < thr_g < float(v["gap_above"])
        at_is_corner = float(v["at"]) > thr_c
        assert at_is_corner == (name == "thresholds-default") and (float(v["gap_at"]) > thr_g) == (name == "thresholds-default")
        assert lab["plain_below"] == 0 and lab["plain_above"] > 0 and (lab["plain_at"] > 0) == at_is_corner
        assert lab["zig_below"] == -1 and lab["zig_at"] == 0
        both = lambda t: ref["label"][sp[t]] > 0 and ref["label"][sp[t] + 1] > 0
        assert both("gap_above") and not both("gap_below") and both("gap_at") == (name == "thresholds-default")
    assert float(np.float32(0.1)) > 0.1 and float(np.float32(0.05)) > 0.05             # why the default "at" cases are a corner and a gap


# ------------------------------------------------------------------------------------------------ the wrong variants
CAUGHT_BY = {"corner_tie_low": "routes", "flat_tie_high": "routes", "no_import": "imports", "flat4_marks": "caps", "cap_20": "caps",
             "gap_ge": "thresholds", "thr_f32": "thresholds", "walk_4": "extents", "back_stop_marks": "extents", "flat_le": "thresholds"}


def _differs(a, b):
    return not (np.array_equal(a["label"], b["label"]) and all(np.array_equal(a[k], b[k]) for k in ("sharp", "less_sharp", "flat")))


@pytest.mark.parametrize("wrong", pc.WRONG)
def test_wrong_variant_is_seen(wrong):
    family = CAUGHT_BY[wrong]
    seen = []
    for name in pc.NAMES:
        c = pc.cases()[name]
        if c["family"] == family and _differs(pc.np_pick(c["scan"], c["off"], c["curv"], c["gap"], wrong=[wrong]), pc.reference(name)):
            seen.append(name)
    print(wrong, "changes", seen)
    assert seen, (wrong, "is not seen by any case of", family)


def test_every_wrong_variant_has_a_family():
    assert set(CAUGHT_BY) == set(pc.WRONG) and set(CAUGHT_BY.values()) <= set(pc.FAMILIES)
