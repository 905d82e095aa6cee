"""Crafted rings for the per-segment feature pick (k_ring_pick, ll_pick.hip), an independent reference of it, and a census of what
a case makes the kernel do.

A plain helper module (not a conftest): test_pick_cases.py checks the reference, the census and the generators on the CPU,
test_gpu_pick_cases.py runs the same cases through Context.upload_scan / extract / scan_info / cloud / labels / features.  Everything
compared is a bit pattern or an index: there is no tolerance anywhere.

The reference restates scanRegistration.cpp:225-235 and :246-359, not oracle/ll_oracle.c:
  np_curvature   the eleven taps summed strictly left to right in f32, vectorised over the cloud
  np_gap_flags   ((dx*dx + dy*dy) + dz*dz) in f32 of consecutive points, compared as double against the threshold
  np_pick        scanStartInd / scanEndInd, the "< 6" skip, per segment a sort by ascending (curvature, index), the descending corner
                 walk (labels 2 and 1, the break at the 21st eligible candidate), the two marking walks, the ascending flat walk whose
                 fourth pick is labelled but marks nothing.  std::sort leaves the order of equal curvatures open; the project defines
                 ascending index there (ll_pick.hip, oracle/ll_oracle.c), and so does this reference.
Thresholds are compared as the reference compares them, an f32 value against a double: the default parameters 0.1f / 0.05f stand for
the double literals 0.1 / 0.05 (ll_api.hip maps them back), any other float parameter is widened.  All cases are ring-major VLP-16
input (16 rings, elevation -15 + 2 k degrees, z = r tan(e)) which the organise stage keeps in its order, so the reference works on the
input itself and needs nothing from the code under test; test_pick_cases.py checks that precondition against the oracle.

`wrong` (a set of names) turns the reference into a deliberately wrong one -- only to show that the cases can see such an error:
  "corner_tie_low"   corner ties go to the lowest index           "flat_tie_high"    flat ties go to the highest index
  "no_import"        marks made by segment j are forgotten in j+1  "flat4_marks"      the fourth flat pick marks its neighbours
  "cap_20"           the corner walk breaks at the 20th candidate  "gap_ge"           the gap test is >=
  "thr_f32"          thresholds compared in f32 after rounding to nearest            "walk_4"   the marking walks stop after four steps
  "back_stop_marks"  the point at which a walk breaks is still marked                "flat_le"  a flat candidate is <= the threshold

The census (census()) restates the kernel's routing from the header comment of ll_pick.hip and from ll_common.h, from the reference's
values only: six segments per ring, rows of 64 segment points, corner candidates compacted (ascending index) into one, two or three
rows of 64 when there are at most 192 of them, else the segment's own rows; the ranked walk for at most 64 candidates without a tie;
the extents (bn, fn) as ten gap flags around a pick; the marks in a bitmap of 32-bit words over the ring's local indices; tiles of three
rows (a seam every 192 segment points); kernels of 6 rows (rings up to 2304 points), 8 (3072), 12 (4608) and 22 (8192).

Left out on purpose: non-finite points (a1 removes them; test_gpu_a1_edges.py owns that), the less-flat voxel filter
(test_gpu_features_chain.py owns it; here the less-flat cloud is only compared with the oracle at the default thresholds), and a tier
work list longer than the resident grid (6144 rings: too big for a unit test).
"""
import functools

import numpy as np

F32 = np.float32
RINGS = 16
SEGS = 6
MIN_RANGE = 0.01                                        # every case: nothing is removed by the range filter
CORNER_CAP, SHARP_CAP, FLAT_CAP = 20, 2, 4              # :270, :276, :328
CROWS = 3                                               # LL_PK_CROWS: rows of compacted corner candidates
TILE_ROWS = 3                                           # LL_PK_TILE_ROWS: a DMA tile seam every 192 segment points
TIER_RINGS = (2304, 3072, 4608, 8192)                   # longest ring of the 6-, 8-, 12- and 22-row kernels
TIER_ROWS = (6, 8, 12, 22)
WRONG = ("corner_tie_low", "flat_tie_high", "no_import", "flat4_marks", "cap_20", "gap_ge", "thr_f32", "walk_4", "back_stop_marks", "flat_le")


# ------------------------------------------------------------------------------------------------ the reference
def threshold(param, default, wrong=()):
    """the double a float parameter stands for: the default float is the reference's double literal, any other is widened"""
    p = F32(param)
    t = float(default) if p == F32(default) else float(p)
    return float(p) if "thr_f32" in wrong else t


def np_curvature(xyz):
    """:225-235: cloudCurvature over [5, n - 5) (zero elsewhere), f32, the sums strictly left to right"""
    p = np.ascontiguousarray(xyz, F32)[:, :3]
    n = len(p)
    c = np.zeros(n, F32)
    if n < 11:
        return c
    m = n - 10
    d = p[0:m].copy()
    for k in range(1, 11):
        d = (d - F32(10) * p[5:5 + m]) if k == 5 else (d + p[k:k + m])
        assert d.dtype == F32
    c[5:n - 5] = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    return c


def np_gap_sq(xyz):
    """:290-293: g[i] = squared distance of point i to point i - 1 in f32 (g[0] = 0)"""
    p = np.ascontiguousarray(xyz, F32)[:, :3]
    g = np.zeros(len(p), F32)
    if len(p) > 1:
        d = p[1:] - p[:-1]
        g[1:] = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    return g


def np_gap_flags(xyz, gap_thr=0.05, wrong=()):
    """flag[i]: the walks stop between point i - 1 and point i"""
    g = np_gap_sq(xyz)
    if "thr_f32" in wrong:
        return g >= F32(gap_thr) if "gap_ge" in wrong else g > F32(gap_thr)
    g = g.astype(np.float64)
    return g >= gap_thr if "gap_ge" in wrong else g > gap_thr


def np_pick(xyz, ring_offsets, curv_param=0.1, gap_param=0.05, wrong=()):
    """:246-359 over a ring-major cloud.  ring_offsets: RINGS + 1 offsets.  Returns dict(curv, label, sharp, less_sharp, flat: index
    lists in push order, segs: one record per segment for the census)."""
    wrong = frozenset(wrong)
    assert wrong <= set(WRONG)
    xyz = np.ascontiguousarray(xyz, F32)[:, :3]
    n = len(xyz)
    curv_thr, gap_thr = threshold(curv_param, 0.1, wrong), threshold(gap_param, 0.05, wrong)
    curv = np_curvature(xyz)
    cmp_t = F32 if "thr_f32" in wrong else np.float64
    cc = curv.astype(cmp_t); ct = cmp_t(curv_thr)
    is_corner = (cc > ct).tolist()
    is_flat = ((cc <= ct) if "flat_le" in wrong else (cc < ct)).tolist()
    flag = np_gap_flags(xyz, gap_thr, wrong).tolist()
    steps = 4 if "walk_4" in wrong else 5
    cap = CORNER_CAP - 1 if "cap_20" in wrong else CORNER_CAP
    picked = [0] * (n + 8)
    label = np.zeros(n, np.int32)
    sharp, less_sharp, flat, segs = [], [], [], []

    def mark(ind, code=1):
        """:286-311: the pick and what its two walks reach -> (bn, fn).  cloudNeighborPicked is 1 in the reference; here a flat pick
        writes 2, so that the census can tell whose mark blocks a candidate -- the pick only asks for non-zero"""
        picked[ind] = code
        fn = bn = 0
        for l in range(1, steps + 1):
            if flag[ind + l]:
                if "back_stop_marks" in wrong:
                    picked[ind + l] = code
                break
            picked[ind + l] = code; fn += 1
        for l in range(-1, -steps - 1, -1):
            if flag[ind + l + 1]:
                if "back_stop_marks" in wrong:
                    picked[ind + l] = code
                break
            picked[ind + l] = code; bn += 1
        return bn, fn

    for r in range(len(ring_offsets) - 1):
        S, E = int(ring_offsets[r]) + 5, int(ring_offsets[r + 1]) - 6         # :218-220
        if E - S < 6:                                                          # :248
            continue
        for j in range(SEGS):
            sp, ep = S + (E - S) * j // 6, S + (E - S) * (j + 1) // 6 - 1      # :253-254
            if "no_import" in wrong:
                for i in range(sp, min(ep + 1, sp + 5)):
                    picked[i] = 0
            idx = np.arange(sp, ep + 1)
            order = idx[np.lexsort((idx, curv[sp:ep + 1]))]                    # ascending (curvature, index)
            corner_order = order[::-1]
            if "corner_tie_low" in wrong:
                corner_order = idx[np.lexsort((idx, -curv[sp:ep + 1].astype(np.float64)))]
            flat_order = order
            if "flat_tie_high" in wrong:
                flat_order = idx[np.lexsort((-idx, curv[sp:ep + 1]))]
            rec = dict(ring=r, seg=j, S=S, sp=sp, ep=ep, off=int(ring_offsets[r]), nr=int(ring_offsets[r + 1] - ring_offsets[r]),
                       cand=[i for i in range(sp, ep + 1) if is_corner[i] and not picked[i]], corners=[], broke=False, flats=[],
                       blocked=[(i, picked[i], "corner" if is_corner[i] else "flat") for i in range(sp, min(ep, sp + 4) + 1)
                                if picked[i] and (is_corner[i] or is_flat[i])])
            largest = 0
            for ind in corner_order.tolist():                                  # :261-313
                if picked[ind] == 0 and is_corner[ind]:
                    largest += 1
                    if largest <= SHARP_CAP:
                        label[ind] = 2; sharp.append(ind); less_sharp.append(ind)
                    elif largest <= cap:
                        label[ind] = 1; less_sharp.append(ind)
                    else:
                        rec["broke"] = True
                        break
                    rec["corners"].append((ind,) + mark(ind))
            rec["fcand"] = [i for i in range(sp, ep + 1) if is_flat[i] and not picked[i]]
            smallest = 0
            for ind in flat_order.tolist():                                    # :316-359
                if picked[ind] == 0 and is_flat[ind]:
                    label[ind] = -1; flat.append(ind)
                    smallest += 1
                    if smallest >= FLAT_CAP:
                        if "flat4_marks" in wrong:
                            mark(ind, 2)
                        rec["flats"].append((ind, -1, -1))
                        break
                    rec["flats"].append((ind,) + mark(ind, 2))
            segs.append(rec)
    return dict(curv=curv, label=label, sharp=np.array(sharp, np.int64), less_sharp=np.array(less_sharp, np.int64),
                flat=np.array(flat, np.int64), segs=segs, flag=np.array(flag, bool))


# ------------------------------------------------------------------------------------------------ the census
def np_extents(flag, ind, steps=5):
    """(bn, fn) of a pick at ind: how far the backward / forward walk gets (:288-311), without marking anything"""
    fn = 0
    while fn < steps and not flag[ind + fn + 1]:
        fn += 1
    bn = 0
    while bn < steps and not flag[ind - bn]:
        bn += 1
    return bn, fn


def tier_of(nr):
    """index into TIER_ROWS of the kernel that takes a ring of nr points"""
    return next(t for t, cap in enumerate(TIER_RINGS) if nr <= cap)


def _tie_kind(pos):
    lanes = {p & 63 for p in pos}
    return "rows" if len(lanes) == 1 else "lanes"


def census(ref):
    """What the reference's result makes k_ring_pick do, per segment and per pick.  Returns a list of segment records:
      len, nrows, tier, nc, cls ("none" | "walk" | "row1" | "row2" | "row3" | "own"), any_tie (two corner candidates with one curvature),
      pick_ties: per corner pick with an equal still-eligible candidate "rows" (all of them in one lane of the scanned rows) or "lanes",
      n_corner, broke, nf (flat candidates at the start of the flat pass), n_flat, flat_ties (as pick_ties, over the segment's own rows),
      picks: per marking pick dict(kind "corner" | "flat", ind, q, lane, row, bn, fn, back ("" | "prev_row" | "below"),
             fwd ("" | "next_row" | "beyond"), word_cross, reach (points of the next segment it marks), seam (within five points of a tile seam)),
      flat4: the fourth flat pick as (ind, bn, fn) or None,
      blocked: the corner / flat candidates among the segment's first five points that an EARLIER segment's mark keeps out, as
               (index, 1 = a corner pick's mark | 2 = a flat pick's, "corner" | "flat")."""
    curv, flag = ref["curv"], ref["flag"]
    out = []
    for s in ref["segs"]:
        sp, ep, off = s["sp"], s["ep"], s["off"]
        ln = ep - sp + 1
        nrows = (ln + 63) >> 6
        cand = s["cand"]
        nc = len(cand)
        bits = curv[cand].view(np.uint32) if nc else np.zeros(0, np.uint32)
        any_tie = len(np.unique(bits)) < nc
        cls = ("none" if nc == 0 else "walk" if nc <= 64 and not any_tie else "row1" if nc <= 64 else "row2" if nc <= 128 else
               "row3" if nc <= 64 * CROWS else "own")
        pos_of = {i: (k if nc <= 64 * CROWS else i - sp) for k, i in enumerate(cand)}
        picks, pick_ties = [], []

        def describe(kind, ind, bn, fn):
            q = ind - sp
            row = q >> 6
            qb, qf = q - bn, q + fn + 1
            back = "" if bn == 5 else "below" if qb < 0 else "prev_row" if (qb >> 6) < row else ""
            fwd = "" if fn == 5 else "beyond" if qf >= nrows * 64 else "next_row" if (qf >> 6) > row else ""
            li = ind - off
            f0 = max(li - bn, (sp if kind == "corner" else ep + 1) - off)
            shi = li + fn
            return dict(kind=kind, ind=ind, q=q, lane=q & 63, row=row, bn=bn, fn=fn, back=back, fwd=fwd,
                        word_cross=shi >= f0 and (f0 >> 5) != (shi >> 5), reach=max(0, ind + fn - ep), from_end=ep - ind,
                        seam=any(abs(q - m * 64 * TILE_ROWS) <= 5 for m in range(1, 8)))

        elig = set(cand)
        for ind, bn, fn in s["corners"]:
            tied = [i for i in elig if curv[i] == curv[ind]]
            pick_ties.append(_tie_kind([pos_of[i] for i in tied]) if len(tied) > 1 else "")
            elig -= set(range(ind - bn, ind + fn + 1))
            picks.append(describe("corner", ind, bn, fn))
        felig = set(s["fcand"])
        flat_ties, flat4 = [], None
        for ind, bn, fn in s["flats"]:
            tied = [i for i in felig if curv[i] == curv[ind]]
            flat_ties.append(_tie_kind([i - sp for i in tied]) if len(tied) > 1 else "")
            if bn < 0:
                flat4 = (ind,) + np_extents(flag, ind)
                break
            felig -= set(range(ind - bn, ind + fn + 1))
            picks.append(describe("flat", ind, bn, fn))
        out.append(dict(ring=s["ring"], seg=s["seg"], len=ln, nrows=nrows, tier=tier_of(s["nr"]), nr=s["nr"], nc=nc, cls=cls, any_tie=any_tie,
                        pick_ties=pick_ties, n_corner=len(s["corners"]), broke=s["broke"], nf=len(s["fcand"]), n_flat=len(s["flats"]),
                        flat_ties=flat_ties, picks=picks, flat4=flat4, sp=sp, ep=ep, blocked=s["blocked"]))
    return out


# ------------------------------------------------------------------------------------------------ geometry
def vlp_ring(k, radius, phase=None):
    """ring k of a VLP-16: len(radius) points of a full clockwise sweep at elevation -15 + 2 k degrees, f64 (n, 3)"""
    r = np.asarray(radius, np.float64)
    n = len(r)
    if n == 0:
        return np.zeros((0, 3))
    az = -(np.arange(n) + (0.25 * (k % 4) if phase is None else phase)) * (2 * np.pi / n)
    return np.stack([r * np.cos(az), r * np.sin(az), r * np.tan(np.deg2rad(-15 + 2 * k))], axis=1)


UNIT = 1.0 / 64                                         # the exact rings' grid: every coordinate a small multiple of it


def octagon_walls(m1, m2):
    """[(first index, one past the last, "axis" | "diag")] of the nine wall pieces of octagon_ring"""
    out, i = [], 0
    for cnt, kind in ((m1 // 2, "axis"), (m2, "diag"), (m1, "axis"), (m2, "diag"), (m1, "axis"), (m2, "diag"), (m1, "axis"), (m2, "diag"), (m1 // 2, "axis")):
        out.append((i, i + cnt, kind)); i += cnt
    return out


def octagon_ring(k, m1, m2, offs, tang=None, z=None):
    """ring k as an octagon of 4 (m1 + m2) points whose coordinates are small multiples of 2^-6: axis-parallel walls of m1 steps of 1/32,
    diagonal walls of m2 steps of (1/32, 1/32), clockwise from the middle of the wall x = +A; point i is pushed offs[i] / 64 along its
    wall's outward normal ((1, 0) ... or (1, 1) ...) and tang[i] / 64 along the wall, z is one multiple of 2^-6 unless given per point.  The eleven-tap sums and their squares are exact in
    f32, so equal offset patterns on one kind of wall give EQUAL curvatures: exact ties where they are wanted."""
    assert m1 % 2 == 0
    walls = [((0, -1), (1, 0), m1 // 2), ((-1, -1), (1, -1), m2), ((-1, 0), (0, -1), m1), ((-1, 1), (-1, -1), m2), ((0, 1), (-1, 0), m1),
             ((1, 1), (-1, 1), m2), ((1, 0), (0, 1), m1), ((1, -1), (1, 1), m2), ((0, -1), (1, 0), m1 // 2)]
    x, y = m1 + 2 * m2, 0                                 # units of 1/64; a step is two units
    pts = []
    for (dx, dy), (nx, ny), cnt in walls:
        for _ in range(cnt):
            o = int(offs[len(pts)])
            t = 0 if tang is None else int(tang[len(pts)])
            pts.append((x + o * nx + t * dx, y + o * ny + t * dy))
            x += 2 * dx; y += 2 * dy
    assert (x, y) == (m1 + 2 * m2, 0) and len(pts) == len(offs) == 4 * (m1 + m2)
    xy = np.array(pts, np.float64) * UNIT
    if z is None:
        z = np.full(len(xy), round(1.04 * (m1 + 2 * m2) * UNIT * np.tan(np.deg2rad(-15 + 2 * k)) / UNIT) * UNIT)
    return np.concatenate([xy, np.asarray(z, np.float64).reshape(-1, 1)], axis=1)


def assemble(rings):
    """ring-major scan (N x 4 f32, intensity 0) and the RINGS + 1 ring offsets from per-ring (n, 3) arrays (None / empty: no points)"""
    rings = [np.zeros((0, 3)) if r is None else np.asarray(r, np.float64).reshape(-1, 3) for r in rings]
    rings += [np.zeros((0, 3))] * (RINGS - len(rings))
    assert len(rings) == RINGS
    pts = np.concatenate(rings).astype(F32)
    off = np.concatenate([[0], np.cumsum([len(r) for r in rings])]).astype(np.int64)
    return np.concatenate([pts, np.zeros((len(pts), 1), F32)], axis=1), off


def base_radius(n, want=6.0):
    """a radius at which a smooth ring of n points has curvature of about 0.06 at most: flat candidates everywhere"""
    delta = 2 * np.pi / max(n, 1)
    return max(0.05, min(want, 0.25 / (55 * delta * delta)))         # never inside the range filter


def seg_bounds(n):
    """[(sp, ep)] of a ring of n points in LOCAL indices (:253-254 with scanStartInd = 5), [] below the '< 6' skip"""
    S, E = 5, n - 6
    return [] if E - S < 6 else [(S + (E - S) * j // 6, S + (E - S) * (j + 1) // 6 - 1) for j in range(SEGS)]


# ------------------------------------------------------------------------------------------------ crafted structures
def _case(name, family, rings, curv=0.1, gap=0.05, max_ring=2304):
    scan, off = assemble(rings)
    return dict(name=name, family=family, scan=scan, off=off, curv=float(curv), gap=float(gap), max_ring=int(max_ring))


def plateau(r, li, bn, fn, B, e):
    """a corner pick at local index li that marks exactly li - bn .. li + fn: those points stand B outwards (a gap above the threshold at
    either end when bn, fn < 5; at 5 the plateau runs on past the walk's reach), li another e: the largest curvature of the plateau"""
    lo = li - bn - (1 if bn == 5 else 0)
    hi = li + fn + (1 if fn == 5 else 0)
    r[lo:hi + 1] += B
    r[li] += e


def stair(r, li, bn, fn, B, kappa, sign):
    """a flat pick at li that marks exactly li - bn .. li + fn: the ring steps by sign * B before li - bn and again after li + fn (two gaps);
    between the steps the radial part of li's eleven-tap sum is made to cancel (the smallest curvature around): li itself is moved when
    that is a small move, otherwise the plateau gets a slope -- a point whose ten neighbours lie five on a lower level and five on its own
    can only be their mean on a slope.  kappa: what the ring's own bend adds to the sum.  Changes the level of everything behind it."""
    lo = li - bn - (1 if bn == 5 else 0)
    hi = li + fn + (1 if fn == 5 else 0)
    A, F = min(5, li - lo), min(5, hi - li)
    a, f = 5 - A, 5 - F                                                       # taps on the level before / behind the plateau
    s = e = 0.0
    if abs(f - a) >= 4:
        s = (a - f) * B / (F * (F + 1) / 2 - A * (A + 1) / 2 - a * A + f * F)
    else:
        e = (f - a) * B / 10.0
    r[lo:hi + 1] += sign * (B + (np.arange(lo, hi + 1) - lo) * s)
    r[hi + 1:] += sign * (2 * B + (hi - lo) * s)
    r[li] += sign * e - kappa / 10.0


EXT_N = 11 + 6 * 254                                    # extents rings: six segments of 254 points, four rows, the last two short


def extent_requests(kind, ln=254):
    """(q, bn, fn) wanted in some segment of length ln: all 36 pairs; the stopping flag in the previous row (lanes 0..3) / the next row
    (lanes 59..63) / below the segment's first centre (q 0..3) / beyond the last row's centres (the last three points).  A corner pick
    whose marks begin below its segment goes into a ring's segment 0, where the points below belong to no segment: in a later
    segment they are corners of the segment before (they lie next to a gap), are picked there and mark the wanted pick away.  The
    flat picks cover that class in the later segments."""
    req = [(100 + 3 * bn + fn, bn, fn) for bn in range(6) for fn in range(6)]
    req += [(64 + l, b, (l + b) % 6) for l in range(4) for b in range(l + 1, 5)]                       # previous row
    req += [(q, (q + f) % 6, f) for q in range(59, 64) for f in range(63 - q, 5)]                      # next row
    req += [(q, b, (q + b) % 6) for q in range(4) for b in range(q + 1, 5)]                            # below the first centre
    req += [(ln - 1 - t, (t + f) % 6, f) for t in range(3) for f in range(2 + t, 5)]                   # beyond the last row
    return req


def place_requests(req, n, per_seg, apart=40, first_seg_below=False):
    """deal the requests over rings and segments: at most per_seg in a segment, local indices at least `apart` apart within a ring"""
    segs = seg_bounds(n)
    placed = [[] for _ in range(RINGS)]                   # per ring: (li, bn, fn)
    count = {}
    for q, bn, fn in req:
        done = False
        for k in range(RINGS):
            for j, (sp, ep) in enumerate(segs):
                li = sp + q
                if first_seg_below and q < bn and j > 0:
                    continue
                if count.get((k, j), 0) < per_seg and li <= ep and all(abs(li - o[0]) >= apart for o in placed[k]):
                    placed[k].append((li, bn, fn)); count[(k, j)] = count.get((k, j), 0) + 1; done = True
                    break
            if done:
                break
        assert done, ("no room for", q, bn, fn)
    return placed


def extents_corner_case(name, sigma, B, e, gap):
    """plateaus on a smooth ring (sigma next to nothing, only to keep mirror-image points from tying: few candidates, the ranked walk) or on a rough one (most points are corner candidates: the
    compacted rows or the segment's own), B and e large against the roughness, the gap threshold raised to match"""
    rng = np.random.default_rng(sum(map(ord, name)))
    placed = place_requests(extent_requests("corner"), EXT_N, 3, first_seg_below=True)
    rings = []
    for k in range(RINGS):
        r = np.full(EXT_N, 6.0) + sigma * rng.standard_normal(EXT_N)
        for li, bn, fn in placed[k]:
            plateau(r, li, bn, fn, B, e)
        rings.append(vlp_ring(k, r))
    return _case(name, "extents", rings, gap=gap)


def extents_flat_case(name, curv=100.0, gap=0.02):
    """stairs on a zigzag ring (every point +-0.02: curvature about 0.06 everywhere) at a curvature threshold above every curvature: no
    corner candidate at all, every point a flat candidate, and the stairs' centres the smallest of their segments.  The gap threshold is
    lowered to 0.02 so that a step of 0.3 less the centre's own move (0.09 at most) still is a gap and the move itself is none."""
    placed = place_requests(extent_requests("flat"), EXT_N, 3)
    delta = 2 * np.pi / EXT_N
    rings = []
    for k in range(RINGS):
        r = np.full(EXT_N, 6.0)
        zig = 0.02 * (1.0 - 2.0 * (np.arange(EXT_N) % 2))
        for t, (li, bn, fn) in enumerate(sorted(placed[k])):
            stair(r, li, bn, fn, 0.3, 55.0 * 6.0 * delta * delta, 1 if t % 2 == 0 else -1)
            zig[li - 5:li + 6] = 0.0
        rings.append(vlp_ring(k, r + zig))
    return _case(name, "extents", rings, curv=curv, gap=gap)


def dent(r, li, kappa):
    """li becomes the mean of its ten neighbours (less the ring's own bend): a curvature of almost nothing, the smallest around"""
    r[li] = (r[li - 5:li].sum() + r[li + 1:li + 6].sum()) / 10.0 - kappa / 10.0


def kappa_of(n, R):
    return 55.0 * R * (2 * np.pi / n) ** 2


# ------------------------------------------------------------------------------------------------ routes
OCT_M1, OCT_M2 = 226, 158                               # octagon of 1536 points: segments 1 and 4 hold a whole axis wall (271..496, 1039..1264)
OCT_N = 4 * (OCT_M1 + OCT_M2)


def tiled(pattern, n, phase=0):
    return np.array([pattern[(i - phase) % len(pattern)] for i in range(n)], np.int64)


def twin_bumps(offs, pattern_len, first, apart, height, walls, n_seg_bounds):
    """on every axis wall that lies inside one segment: two bumps of one height `apart` points apart, at places where the tiled pattern
    is in one phase: equal curvatures, nothing else as large"""
    for w0, w1, kind in walls:
        if kind != "axis" or w1 - w0 < apart + 20:
            continue
        if not any(sp <= w0 and w1 - 1 <= ep for sp, ep in n_seg_bounds):
            continue
        a = w0 + 8
        a += (first - a) % pattern_len
        offs[a] = height; offs[a + apart] = height


def routes_cases():
    out = []
    # untied: rough circles, the roughness decides how many points are corner candidates (random floats: no two curvatures equal)
    rng = np.random.default_rng(11)
    sig = [0.0, 0.006, 0.012, 0.02, 0.03, 0.03, 0.05, 0.05, 0.2, 0.2, 0.0, 0.012, 0.03, 0.05, 0.2, 0.3]
    out.append(_case("routes-untied", "routes", [vlp_ring(k, 6.0 + s * rng.standard_normal(EXT_N)) for k, s in enumerate(sig)]))
    # tied: exact octagons.  The tiled patterns make one, two or all three points of a period corner candidates of EQUAL curvature
    # (sums of eleven taps: (3,0,..,0): -30 at the bump; (3,0,0): -24; (0,6,3): 36, -36, 0; (0,4): 24, -24; x^2 / 4096 > 0.1 from |x| = 21 on);
    # twin bumps 64 candidates apart are the largest of their segment and tie in ONE lane of two rows
    walls = octagon_walls(OCT_M1, OCT_M2)
    segs = seg_bounds(OCT_N)
    rings = []
    for k in range(RINGS):
        kind = (5, 0, 1, 2, 3, 4, 6, 7, 7, 6, 4, 3, 2, 1, 0, 5)[k]       # the roughest octagons in the middle rings, whose bins are wide
        if kind == 0:                                                   # at most 64 candidates, all tied, the picks too
            offs = tiled([3] + [0] * 11, OCT_N)
        elif kind == 1:                                                 # at most 64 candidates, two of them tied, behind the break: untied picks
            offs = np.zeros(OCT_N, np.int64)
            offs[segs[0][0] + 6] = offs[segs[0][0] + 17] = 3
        elif kind == 2:
            offs = tiled([3, 0, 0], OCT_N); twin_bumps(offs, 3, 0, 192, 5, walls, segs)
            for a in (walls[2][0] + 30, walls[6][0] + 30):                  # twin dents 64 points apart: the two smallest curvatures of their
                assert a % 3 and (a + 64) % 3                               # segment (12 - 10 = 2 against 12 everywhere else), one lane, two rows
                offs[a] = offs[a + 64] = 1
        elif kind == 3:
            offs = tiled([0, 6, 3], OCT_N); twin_bumps(offs, 3, 1, 96, 12, walls, segs)
        elif kind == 4:
            offs = tiled([0, 4], OCT_N); twin_bumps(offs, 2, 0, 64, 8, walls, segs)
        elif kind == 5:                                                 # random small offsets: ties of every kind
            offs = rng.integers(-3, 4, OCT_N)
        elif kind == 6:
            offs = rng.integers(-5, 6, OCT_N)
        else:
            offs = rng.integers(-12, 13, OCT_N)
        ring = octagon_ring(k, OCT_M1, OCT_M2, offs)
        if kind == 1:                                                   # twenty float bumps per segment, all different; segment 0 also has two
            for s_i, (sp, ep) in enumerate(segs):                           # equal small ones, which the walk reaches only as its 21st candidate
                for t in range(20):
                    ring[sp + 30 + 11 * t, :2] *= 1.0 + rng.uniform(0.012, 0.02)
        rings.append(ring)
    out.append(_case("routes-tied", "routes", rings))
    return out


# ------------------------------------------------------------------------------------------------ caps
CAPS_CORNERS = (0, 1, 2, 3, 19, 20, 21, 23)             # eligible corner candidates in visiting order, per segment
CAPS_FLATS = (0, 1, 3, 4, 5)                            # flat candidates of a segment (a smooth segment has hundreds)


def caps_cases():
    """smooth segments with a counted number of isolated spikes (eleven apart: no pick marks another spike), and zigzag segments (every
    point a corner candidate, twenty larger spikes take the picks and mark q < 226) whose last points hold a counted number of dents: the
    segment's only flat candidates, their curvatures in ascending order of index.  A zigzag segment with four dents, the fourth within
    five points of the segment's end, is followed by a smooth segment whose second point is its smallest curvature: the fourth flat
    pick does not mark it."""
    rng = np.random.default_rng(5)
    n = EXT_N
    segs = seg_bounds(n)
    kap = kappa_of(n, 6.0)
    plan = [[("c", c) for c in CAPS_CORNERS[:6]], [("c", 21), ("c", 23), ("f", 0), ("f", 1), ("f", 3), ("c", 2)],
            [("f", 4), ("c", 1), ("f", 5), ("c", 3), ("f4", 4), ("c0dent", 0)]]
    rings = []
    for k in range(RINGS):
        r = np.full(n, 6.0)
        dents = []
        for (what, cnt), (sp, ep) in zip(plan[k % len(plan)], segs):
            if what.startswith("c"):
                for t in range(cnt):
                    r[sp + 5 + 11 * t] += rng.uniform(0.05, 0.2)
                if what == "c0dent":
                    dents.append((sp + 1, 0.0))
            else:
                r[sp:ep + 1] += 0.04 * (1.0 - 2.0 * (np.arange(sp, ep + 1) % 2))
                for t in range(20):
                    r[sp + 5 + 11 * t] += 0.1 if r[sp + 5 + 11 * t] > 6.0 else -0.1
                last = ep - 1 if what == "f4" else ep - 3
                for t in range(cnt):
                    dents.append((last - 6 * (cnt - 1 - t), 0.01 * (t + 1)))       # six apart: no dent marks another
        for li, extra in dents:
            dent(r, li, kap)
            r[li] += extra / 10.0
        rings.append(vlp_ring(k, r))
    return [_case("caps", "caps", rings)]


# ------------------------------------------------------------------------------------------------ lengths
LENGTH_SEGS = (63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 319, 320, 321, 382)
LENGTH_RINGS = tuple(n for ln in LENGTH_SEGS for n in range(11 + 6 * ln, 11 + 6 * ln + 6) if n <= 2304)
LENGTH_SHORT = (0, 1, 16, 17, 18, 22, 23)


def rough_ring(k, n, rng, seam_segs=(), R=None):
    """a ring with corners and flats: a smooth circle whose radius wanders a little, one point in twelve pushed out; at segment position
    190 of the segments in seam_segs a spike and behind it a quiet stretch with a dent at 196: picks on both sides of a tile seam"""
    if n == 0:
        return None
    R = base_radius(n) if R is None else R
    r = R * (1.0 + 0.0015 * rng.standard_normal(n) + np.where(rng.random(n) < 0.08, rng.uniform(0.01, 0.03, n), 0.0))
    kap = kappa_of(n, R)
    for j, (sp, ep) in enumerate(seg_bounds(n)):
        if j in seam_segs:
            for m in range(1, 8):
                q = 192 * m
                if q + 12 <= ep - sp and (m - 1) % SEGS == j:                # seam m in segment (m - 1) mod 6: at most two dents per segment, the two smallest
                    r[sp + q - 8:sp + q + 13] = R
                    r[sp + q - 2] = R * 1.05
                    dent(r, sp + q + 4, kap)
    return vlp_ring(k, r)


def lengths_cases():
    """every ring length 11 + 6 len + d next to a different one, seven scans; the short rings and the full ring ride among them"""
    rng = np.random.default_rng(3)
    todo = list(LENGTH_RINGS)
    todo = todo[0::3] + todo[1::3] + todo[2::3]                             # neighbours in a scan differ by a row or more
    out = []
    for i, n in enumerate(LENGTH_SHORT + (2304,)):                           # the short rings and the full ring between the others
        todo.insert(5 + 12 * i, n)
    while todo:
        take, todo = todo[:RINGS], todo[RINGS:]
        take += [40] * (RINGS - len(take))
        out.append(_case(f"lengths-{len(out)}", "lengths", [rough_ring(k, n, rng, seam_segs=range(6)) for k, n in enumerate(take)]))
    return out


# ------------------------------------------------------------------------------------------------ imports
def imports_cases():
    rng = np.random.default_rng(9)
    # (a) short rings: segments of 1 .. 12 points, a pick's marks run through whole segments
    short = [17 + 6 * m + (m % 3) for m in range(1, 13)] + [19, 25, 31, 83]
    rings = []
    for k, n in enumerate(short):
        R = base_radius(n)
        r = R * (1.0 + 0.002 * rng.standard_normal(n)) * np.where(rng.random(n) < 0.25, 1.0 + rng.uniform(0.05, 0.3, n), 1.0)
        rings.append(vlp_ring(k, r))
    out = [_case("imports-short", "imports", rings)]
    # (b) ordinary rings: a corner of segment j that only a corner mark from segment j - 1 keeps out; a flat pick of segment j whose marks
    # reach 1 .. 5 points into segment j + 1 and cover a corner and a flat candidate there; a ring of 161 points whose segment 0 ends
    # at local index 29, so that the marks beyond it straddle a word of the bitmap
    rings = []
    for k in range(RINGS):
        n = 161 if k == 15 else 11 + 6 * 70 + (k % 6)
        R = base_radius(n)
        kap = kappa_of(n, R)
        r = np.full(n, R)
        segs = seg_bounds(n)
        for j in range(SEGS - 1):
            ep = segs[j][1]
            if (j + k) % 2 == 0 and n != 161:
                r[ep - 1] += 0.12 * R / 6; r[ep + 3] += 0.08 * R / 6       # the larger spike is the last segment's, it marks the smaller
            else:
                reach = 5 if n == 161 else 1 + (j + k) % 5
                r[ep + reach] += 0.08 * R / 6                               # a corner at the far end of the reach, flats before it
                dent(r, ep - 5 + reach, kap)
        rings.append(vlp_ring(k, r))
    out.append(_case("imports-marks", "imports", rings))
    return out


# ------------------------------------------------------------------------------------------------ tiers
def tiers_cases():
    """rings for the 8-, 12- and 22-row kernels next to short and empty ones: rough circles with picks at every tile seam, and exact
    zigzag octagons whose segments hold more than 192 tied candidates and twin bumps in one lane of two rows"""
    rng = np.random.default_rng(21)
    out = []
    for name, cap, lens in (("tiers-4608", 4608, [2305, 40, 3072, 0, 3073, 17, 4608, 700, 3072, 2304, 0, 4608, 16, 2305, 100, 4604]),
                            ("tiers-8192", 8192, [4609, 0, 2305, 30, 8192, 3073, 16, 8192, 0, 4609, 700, 8192, 0, 0, 5000, 23])):
        rings = []
        for k, n in enumerate(lens):
            if n >= 2305 and n % 4 == 0 and k in (2, 6, 7, 8, 11):                  # exact octagons (their bins are wide enough in these rings)
                m1 = int(round(n / 4 * 0.5885 / 2)) * 2
                m2 = n // 4 - m1
                offs = tiled([0, 4], n)
                twin_bumps(offs, 2, 0, 64, 8, octagon_walls(m1, m2), seg_bounds(n))
                for sp, ep in seg_bounds(n):                                    # and twin bumps either side of every tile seam of the segment
                    for m in range(1, 8):
                        if 192 * m + 70 < ep - sp:
                            offs[sp + 192 * m - 2 - (sp % 2)] = 9 + m; offs[sp + 192 * m + 62 - (sp % 2)] = 9 + m
                rings.append(octagon_ring(k, m1, m2, offs))
            else:
                rings.append(rough_ring(k, n, rng, seam_segs=range(6), R=None if n < 400 else 20.0))
        out.append(_case(name, "tiers", rings, max_ring=cap))
    return out


# ------------------------------------------------------------------------------------------------ thresholds
def ulp_step(x, k):
    """the f32 k ulps above (k > 0) or below x"""
    return (np.array([x], F32).view(np.uint32) + np.uint32(k)).view(F32)[0] if k >= 0 else (np.array([x], F32).view(np.uint32) - np.uint32(-k)).view(F32)[0]


def find_z(v, target, times):
    """an f32 z with  f32(v) + (times * z)^2 == target  in f32 arithmetic (v: an exact multiple of 2^-12 below the target)"""
    v, target, times = F32(v), F32(target), F32(times)
    z0 = F32(np.sqrt(float(target) - float(v)) / float(times))
    cand = (np.array([z0], F32).view(np.uint32)[0] + np.arange(-4000, 4000)).astype(np.uint32).view(F32)
    d = times * cand
    hit = np.flatnonzero((v + d * d).view(np.uint32) == np.array([target], F32).view(np.uint32)[0])
    assert len(hit), ("no z for", v, target)
    return cand[hit[len(hit) // 2]]


def isolated(offs, z, i, sign, o, nb, zeta):
    """point i alone between two gaps: a step of 32 / 64 before it and another behind it (sign: up or down), the point itself o / 64
    off the middle level, its successor nb / 64 off the level behind, its z zeta: the eleven-tap sum of its normal coordinate is
    nb - 10 o (+ 4 per zigzag point that stands out among its neighbours), of its z -10 zeta.  No neighbour's mark can reach it."""
    offs[i] += sign * 32 + o
    offs[i + 1:] += sign * 64
    offs[i + 1] += nb
    z[i] = zeta


def thresholds_cases():
    """Ring 8 (elevation 0 .. 2 degrees) is an exact octagon in the plane z = 0; the special points stand alone between two gaps, so only
    their own comparison decides their label.  In a segment without other corners a curvature above the threshold makes them a sharp
    point; in a zigzag segment (every other point a corner candidate, the walk breaks long before it gets to them) a curvature below
    the threshold makes them the segment's flat pick.  Gap specials: two neighbours of large, equal curvature either side of a step; the
    one picked first marks the other exactly when the step is no gap."""
    out = []
    walls = octagon_walls(OCT_M1, OCT_M2)
    segs = seg_bounds(OCT_N)
    rng = np.random.default_rng(4)
    for name, curv, gap in (("thresholds-default", 0.1, 0.05), ("thresholds-eighth", 0.125, 0.0625)):
        offs = np.zeros(OCT_N, np.int64); tang = np.zeros(OCT_N, np.int64); z = np.zeros(OCT_N, F32)
        spec = {}
        if name == "thresholds-default":
            # curvature 400 / 4096 + (10 zeta)^2 on an axis wall: f32(0.1) is above the double 0.1 (a corner, no flat), its predecessor below
            at, below = F32(0.1), ulp_step(F32(0.1), -1)
            v, plain_o, plain_nb = 400.0 / 4096, 2, 0
            plain_wall = walls[2]
        else:
            # curvature 2 * 256 / 4096 = 0.125 exactly on a diagonal wall, and 2 * 225 / 4096 + (10 zeta)^2 one ulp either side of it
            at, below = F32(0.125), ulp_step(F32(0.125), -1)
            v = 450.0 / 4096
            plain_wall = walls[3]
        above = ulp_step(at, 1)
        # segment 0, a zigzag on an axis wall: curvature 400 / 4096 + (10 zeta)^2 at either threshold
        zig_lo = segs[0][0]
        offs[segs[0][0]:segs[0][1] + 1] = tiled([0, 4], OCT_N)[segs[0][0]:segs[0][1] + 1]
        for tag, val, i, sign in (("zig_below", below, zig_lo + 9, 1), ("zig_at", at, zig_lo + 23, -1)):
            assert offs[i + 1] - offs[i] == 4 == offs[i - 1] - offs[i]                      # six of its neighbours stand 4 / 64 out: 24 + 6 - 10 = 20
            isolated(offs, z, i, sign, 1, 6, find_z(400.0 / 4096, val, 10)); spec[tag] = i
        if name == "thresholds-default":
            w0 = plain_wall[0]
            for tag, val, i, sign in (("plain_below", below, w0 + 30, 1), ("plain_at", at, w0 + 60, -1), ("plain_above", above, w0 + 90, 1)):
                isolated(offs, z, i, sign, plain_o, plain_nb, find_z(v, val, 10)); spec[tag] = i
            offs[w0 + 120:] -= 64
        else:
            w0 = plain_wall[0]                                             # diagonal wall 497 .. 654, in segment 2 from 513 on
            for tag, val, i, sign, o, nb in (("plain_below", below, w0 + 30, 1, 2, 5), ("plain_at", at, w0 + 60, -1, 2, 4), ("plain_above", above, w0 + 90, 1, 2, 5)):
                isolated(offs, z, i, sign, o, nb, 0.0 if val == at else find_z(v, val, 10)); spec[tag] = i
            offs[w0 + 120:] -= 64
        # gap specials on the axis wall of segment 4: steps in z (and, for 0.0625 itself, a step of exactly 16 / 64 with no move along the wall)
        w0 = walls[6][0]
        gat = F32(0.05) if name == "thresholds-default" else F32(0.0625)
        steps = [("gap_below", ulp_step(gat, -1), w0 + 40), ("gap_above", ulp_step(gat, 1), w0 + 100)]
        steps.append(("gap_at", gat, w0 + 160))
        for tag, val, i in steps:
            if tag == "gap_at" and name != "thresholds-default":
                offs[i + 1:] += 16; tang[i + 1] = -2                       # exactly 0.25 apart
                offs[i + 12:] -= 8; offs[i + 24:] -= 8
            else:
                dz = find_z((4.0 + 196.0) / 4096, val, 1)                  # 14 / 64 across, 2 / 64 along, the rest in z
                offs[i + 1:] += 14
                offs[i + 12:] -= 7; offs[i + 24:] -= 7
                z[i + 1:i + 13] = dz; z[i + 13:i + 25] = dz / F32(2)          # and down again in two steps that are no gaps
            spec[tag] = i
        rings = []
        for k in range(RINGS):
            if k == 8:
                rings.append(octagon_ring(k, OCT_M1, OCT_M2, offs, tang, z))
            else:
                rings.append(octagon_ring(k, OCT_M1, OCT_M2, rng.integers(-2, 3, OCT_N)))
        c = _case(name, "thresholds", rings, curv=curv, gap=gap)
        c["spec"] = {t: int(c["off"][8] + i) for t, i in spec.items()}
        c["spec_values"] = dict(below=below, at=at, above=above, gap_below=ulp_step(gat, -1), gap_at=gat, gap_above=ulp_step(gat, 1))
        out.append(c)
    return out


# ------------------------------------------------------------------------------------------------ the cases
def extents_cases():
    return [extents_corner_case("extents-corner-walk", 0.0002, 0.3, 0.1, 0.05), extents_corner_case("extents-corner-rows", 0.03, 1.0, 0.5, 0.5),
            extents_corner_case("extents-corner-own", 0.15, 2.0, 1.0, 2.0), extents_flat_case("extents-flat")]


FAMILIES = ("routes", "caps", "extents", "lengths", "imports", "tiers", "thresholds")


@functools.lru_cache(maxsize=None)
def cases():
    """name -> case: dict(name, family, scan (N x 4 f32, ring-major), off (RINGS + 1 ring offsets), curv, gap (the two float parameters),
    max_ring (max_ring_points of the context))"""
    out = {}
    for make in (routes_cases, caps_cases, extents_cases, lengths_cases, imports_cases, tiers_cases, thresholds_cases):
        for c in make():
            assert c["name"] not in out and c["family"] in FAMILIES
            out[c["name"]] = c
    return out


NAMES = tuple(cases())


def is_default(c):
    return c["curv"] == 0.1 and c["gap"] == 0.05


@functools.lru_cache(maxsize=None)
def reference(name):
    """np_pick of a case, computed once and shared; nobody changes it"""
    c = cases()[name]
    return np_pick(c["scan"], c["off"], c["curv"], c["gap"])


@functools.lru_cache(maxsize=None)
def case_census(name):
    return census(reference(name))


def family_census(family):
    return [dict(s, case=n) for n in NAMES if cases()[n]["family"] == family for s in case_census(n)]
