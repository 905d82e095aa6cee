"""Crafted inputs for the MAPPING stage's correspondence vote, and an independent reference of it.

A plain helper module (not a conftest): test_map_vote_cases.py checks np_map_vote and the generators on the CPU,
test_gpu_map_vote.py runs the same cases through ll_map_vote_host (k_map_vote) and the maps.

np_map_vote restates laserMapping.cpp:836-1030 (called with corner_case = true at :2059) in vectorised float32 numpy: 20 regions
of n // 20 correspondences, the last one takes the remainder; correctly rounded square roots; a pair is incompatible when
(double)expf(-gap * gap) < 0.95 -- as the bit-exact threshold on the gap, with glibc's expf as the witness for every pair within
64 ulp of it -- and an entry is selected iff (float)count < 0.75f * (float)m, strict.
"""
import ctypes as C
import ctypes.util

import numpy as np

REGIONS = 20                                            # :841
GAP2_BITS = 0x3d5218e6                                  # LL_MAP_VOTE_GAP2_BITS: the smallest f32 gap^2 with (double)expf(-gap^2) < 0.95
GAP_BITS = 0x3e67ea6c                                   # LL_MAP_VOTE_GAP_BITS: the smallest f32 gap whose rounded square reaches it
G_T = np.array([GAP_BITS], np.uint32).view(np.float32)[0]
F32 = np.float32
NT = 256                                                # threads of a k_map_vote workgroup: a region above it is walked in strides

_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.expf.restype = C.c_float
_libm.expf.argtypes = [C.c_float]


def incompatible_by_expf(gap):
    """the reference's own test of one f32 gap: score = expf(-(gap * gap) / (1 * 1)) as a float, compared with the double 0.95"""
    g2 = F32(F32(gap) * F32(gap))
    return float(_libm.expf(F32(-g2) / F32(1.0))) < 0.95


def f4(xyz):
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    out = np.zeros((len(xyz), 4), np.float32)
    out[:, :3] = xyz.astype(np.float32)
    return out


def _ubits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.int64)


def pair_roots(p):
    """Distance() (:250) of every pair of the (m, >= 3) float32 points p: f32 sqrt of (dx*dx + dy*dy) + dz*dz"""
    p = np.ascontiguousarray(p, np.float32)
    with np.errstate(all="ignore"):
        dx = p[:, None, 0] - p[None, :, 0]; dy = p[:, None, 1] - p[None, :, 1]; dz = p[:, None, 2] - p[None, :, 2]
        return np.sqrt((dx * dx + dy * dy) + dz * dz)


def region_bounds(n):
    """[b0, b1) of the 20 regions: n // 20 each, the last runs to n (:884-893); n < 20: everything is in the last"""
    chunk = n // REGIONS
    return [(chunk * r, n if r == REGIONS - 1 else chunk * (r + 1)) for r in range(REGIONS)]


def _ulp_step(a, k):
    b = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    ok = np.isfinite(a) & (b + k >= 0)
    return np.where(ok, b + k, b).astype(np.int32).view(np.float32)


def np_map_vote(src, tgt, perturb=None, stats=None):
    """-> (count int32[n], selected bool[n]).
    perturb: a numpy Generator; every root of every pair is then moved by +1 or -1 ulp at random (what an approximate square
    root may do) -- used only to show that a case can tell such a root from the exact one.
    stats: a dict that receives near64, the pairs whose gap is within 64 ulp of the threshold (all expf-confirmed)."""
    src = np.ascontiguousarray(src, np.float32); tgt = np.ascontiguousarray(tgt, np.float32)
    n = len(src)
    cnt = np.zeros(n, np.int32); sel = np.zeros(n, bool)
    near64 = 0
    for b0, b1 in region_bounds(n):
        m = b1 - b0
        if m <= 0:
            continue
        s1 = pair_roots(src[b0:b1]); s2 = pair_roots(tgt[b0:b1])
        if perturb is not None:
            for s in (s1, s2):
                k = np.triu(perturb.choice(np.array([-1, 1]), size=(m, m)), 1)
                s[...] = _ulp_step(s, k + k.T)
        with np.errstate(all="ignore"):
            gap = np.abs(s1 - s2)
        inc = (_ubits(gap) >= GAP_BITS) & ~np.isnan(gap)
        near = (np.abs(_ubits(gap) - GAP_BITS) <= 64) & ~np.isnan(gap)
        for i, j in np.argwhere(near):
            assert bool(inc[i, j]) == incompatible_by_expf(gap[i, j]), (float(gap[i, j]), "the gap threshold disagrees with expf")
        near64 += int(np.triu(near, 1).sum())
        np.fill_diagonal(inc, False)
        c = inc.sum(axis=1).astype(np.int32)
        cnt[b0:b1] = c
        sel[b0:b1] = c.astype(np.float32) < F32(0.75) * F32(m)                       # :969-970, :996
    if stats is not None:
        stats["near64"] = near64
    return cnt, sel


def anchor_gap_ulps(src, tgt):
    """for every (anchor = first entry of a region, partner) pair: (gap - g_T) in ulps of the larger root, and the decision"""
    out_d, out_inc = [], []
    for b0, b1 in region_bounds(len(src)):
        if b1 - b0 < 2:
            continue
        s1 = pair_roots(src[b0:b1])[0, 1:]; s2 = pair_roots(tgt[b0:b1])[0, 1:]
        with np.errstate(all="ignore"):
            gap = np.abs(s1 - s2)
            big = np.maximum(s1, s2)
            d = (gap.astype(np.float64) - float(G_T)) / np.spacing(big).astype(np.float64)
        out_d.append(d); out_inc.append((_ubits(gap) >= GAP_BITS) & ~np.isnan(gap))
    return np.concatenate(out_d), np.concatenate(out_inc)


# ------------------------------------------------------------------------------------------------ families
def consistent(n, rng, outliers):
    """consistent correspondences plus outliers whose target is displaced by 0.1 .. 3 m (gaps on both sides of the threshold)"""
    src = rng.uniform(-15, 15, (n, 3)); tgt = src + rng.normal(0, 0.03, (n, 3))
    if outliers:
        bad = rng.choice(n, outliers, replace=False)
        tgt[bad] += rng.uniform(0.1, 3.0, (outliers, 1)) * rng.standard_normal((outliers, 3))
    return f4(src), f4(tgt)


SIZES = (0, 1, 19, 20, 21, 39, 40, 41, 419,
         20 * (NT + 1), 20 * (NT + 2), 20 * (NT + 1) + 19)      # regions of 257 (odd) and 258 (even) entries; a last region of 276


def size_cases():
    return {f"n{n}": consistent(n, np.random.default_rng(1000 + n), min(n, max(1, n // 3)) if n > 1 else 0) for n in SIZES}


def _gap_of(s0, sj, t0, tj):
    a = pair_roots(np.stack([s0, sj]))[0, 1]; b = pair_roots(np.stack([t0, tj]))[0, 1]
    return np.abs(a - b)


def place_partner(src0, tgt0, tgtj, k, direction):
    """a source point for the partner whose target is tgtj, so that the anchor pair's gap is g_T + k half-ulps of the larger root:
    placed in f64 along `direction` from the anchor's source, rounded to f32, then walked by single-ulp steps of its coordinates
    towards that gap (the coordinates' own rounding is coarser than the root's ulp)"""
    src0 = np.asarray(src0, np.float32); tgt0 = np.asarray(tgt0, np.float32); tgtj = np.asarray(tgtj, np.float32)
    s2 = float(pair_roots(np.stack([tgt0, tgtj]))[0, 1])
    s1 = s2 + float(G_T)
    half = 0.5 * k * float(np.spacing(F32(s1)))
    want = float(G_T) + half
    p = (src0.astype(np.float64) + (s1 + half) * np.asarray(direction, np.float64)).astype(np.float32)
    err = lambda q: abs(float(_gap_of(src0, q, tgt0, tgtj)) - want)
    best = err(p)
    for _ in range(48):
        moved = False
        for ax in range(3):
            for to in (np.inf, -np.inf):
                q = p.copy(); q[ax] = np.nextafter(q[ax], F32(to))
                e = err(q)
                if e < best:
                    best, p, moved = e, q, True
        if not moved:
            break
    return p


def borderline(scale, rng, m=12, kmax=6):
    """20 regions x m correspondences; entry 0 of each region is the anchor, every partner has its target scale * U(0.5, 1) from the
    anchor's along a random direction and its source along the same direction at s2 + g_T + k * ulp / 2, k in -kmax .. kmax.
    scale 0: all partners share the anchor's target point (the gap is the source distance)."""
    n = REGIONS * m
    src = np.zeros((n, 3), np.float32); tgt = np.zeros((n, 3), np.float32)
    for r in range(REGIONS):
        b0 = r * m
        tgt[b0] = rng.uniform(-2, 2, 3); src[b0] = tgt[b0].astype(np.float64) + rng.normal(0, 0.03, 3)
        ks = rng.permutation(np.arange(-kmax, kmax + 1))
        for j in range(1, m):
            d = rng.standard_normal(3); d /= np.linalg.norm(d)
            tgt[b0 + j] = tgt[b0].astype(np.float64) + scale * rng.uniform(0.5, 1.0) * d
            src[b0 + j] = place_partner(src[b0], tgt[b0], tgt[b0 + j], int(ks[(j - 1) % len(ks)]), d)
    return f4(src), f4(tgt)


def ladder(kmax=40):
    """the exact ladder: one shared target point per region, the anchor's source at the origin, partner k at g_T + k ulp along one
    axis: the gap of anchor pair k IS that float (sqrt(fl(d * d)) == d), 41 incompatible of 81.  20 regions of 2 * kmax + 3
    (anchor, 81 partners, one filler that coincides with the anchor)."""
    m = 2 * kmax + 3
    src = np.zeros((REGIONS * m, 3), np.float32); tgt = np.zeros((REGIONS * m, 3), np.float32)
    steps = _ulp_step(np.full(2 * kmax + 1, G_T, np.float32), np.arange(-kmax, kmax + 1))
    for r in range(REGIONS):
        b0 = r * m
        tgt[b0:b0 + m] = [3.0 + r, -1.5, 0.25]
        src[b0 + 1:b0 + m - 1, r % 3] = steps * (1 if r % 2 == 0 else -1)
    return f4(src), f4(tgt)


BORDERLINE_SCALES = (0, 1, 10, 100)


def borderline_cases():
    out = {f"borderline-scale{s}": borderline(s, np.random.default_rng(300 + s)) for s in BORDERLINE_SCALES}
    out["ladder"] = ladder()
    return out


def extreme_cases():
    """160 correspondences (regions of 8) with non-finite coordinates and overflowing squares"""
    rng = np.random.default_rng(17)
    out = {}
    src, tgt = consistent(160, rng, 30)
    src[1, 0] = 1e20                                       # dx * dx overflows: one infinite root, gap = inf -> incompatible
    src[9, 1] = -1e20; tgt[9, 1] = -1e20                   # both roots infinite: gap = NaN -> compatible
    src[18, 2] = 1e20; tgt[18, 0] = 1e20
    src[25, 0] = 1e19; src[26, 0] = -1e19                  # finite squares whose sum overflows
    out["overflow"] = (src, tgt)
    src, tgt = consistent(160, rng, 30)
    src[2, 0] = np.nan; tgt[11, 2] = np.nan; src[20, :3] = np.nan; tgt[20, :3] = np.nan
    src[33, 1] = np.inf; tgt[50, 1] = -np.inf; src[41, 0] = np.inf; tgt[41, 0] = np.inf
    out["nan"] = (src, tgt)
    src, tgt = consistent(160, rng, 0)
    src[8:12] = src[8]; tgt[8:12] = tgt[8]                 # coincident correspondences
    src[16:20] = src[16]                                   # coincident sources, distinct targets
    tgt[24:28] = tgt[24]                                   # coincident targets, distinct sources
    out["coincident"] = (src, tgt)
    return out


def groups_region(sizes, rng, far=1000.0):
    """one region whose entries fall into groups: within a group every pair is consistent (one common displacement), across
    groups every pair is incompatible (displacements `far` apart): an entry of group k has count m - sizes[k]"""
    m = sum(sizes)
    src = rng.uniform(-15, 15, (m, 3)); tgt = src.copy()
    order = rng.permutation(m); at = 0
    group = np.zeros(m, np.int64)
    for k, sz in enumerate(sizes):
        ix = order[at:at + sz]; at += sz
        v = np.zeros(3); v[k % 3] = far * (1 + k // 3) * (1 if k % 2 == 0 else -1)
        tgt[ix] += v
        group[ix] = k
    return src, tgt, group


def selection_cases():
    """name -> (src, tgt, expect) with expect = {index: (count, selected)}"""
    out = {}
    rng = np.random.default_rng(23)
    # regions of 20: 0.75f * 20 = 15.0f -- count 15 is AT the bound and dropped (strict <), 14 kept, 16 dropped.  Region 3 holds the
    # groups, region 7 is all compatible (identical displacement), region 19 (the last) all incompatible
    src = rng.uniform(-15, 15, (400, 3)); tgt = src.copy()
    s, t, grp = groups_region((5, 6, 4, 5), rng); src[60:80] = s; tgt[60:80] = t
    exp = {60 + i: ((15, False), (14, True), (16, False), (15, False))[g] for i, g in enumerate(grp)}
    tgt[140:160] += [0.0, 0.0, 7.0]
    exp.update({i: (0, True) for i in range(140, 160)})
    s, t, grp = groups_region((1,) * 20, rng); src[380:400] = s; tgt[380:400] = t
    exp.update({i: (19, False) for i in range(380, 400)})
    out["m20-count14-15-16"] = (f4(src), f4(tgt), exp)
    # regions of 22: 0.75f * 22 = 16.5f -- 16 kept, 17 dropped; of 21 + 19 = 40 in the last region of n = 439: 30.0f -- 29 kept, 30 and 31 dropped
    src = rng.uniform(-15, 15, (440, 3)); tgt = src.copy()
    s, t, grp = groups_region((6, 5, 11), rng); src[22:44] = s; tgt[22:44] = t
    exp = {22 + i: ((16, True), (17, False), (11, True))[g] for i, g in enumerate(grp)}
    out["m22-count16-17"] = (f4(src), f4(tgt), exp)
    src = rng.uniform(-15, 15, (439, 3)); tgt = src.copy()
    s, t, grp = groups_region((11, 10, 9, 10), rng); src[399:439] = s; tgt[399:439] = t
    exp = {399 + i: ((29, True), (30, False), (31, False), (30, False))[g] for i, g in enumerate(grp)}
    out["last40-count29-30-31"] = (f4(src), f4(tgt), exp)
    return out


SIZE_NAMES = tuple(f"n{n}" for n in SIZES)
BORDERLINE_NAMES = tuple(f"borderline-scale{s}" for s in BORDERLINE_SCALES) + ("ladder",)
EXTREME_NAMES = ("overflow", "nan", "coincident")
SELECTION_NAMES = ("m20-count14-15-16", "m22-count16-17", "last40-count29-30-31")
CASE_NAMES = SIZE_NAMES + BORDERLINE_NAMES + EXTREME_NAMES + SELECTION_NAMES             # (for parametrize: builds nothing)

_ALL = None
_REF = {}


def all_cases():
    """name -> (src, tgt): every family, built once on first use"""
    global _ALL
    if _ALL is None:
        c = {}
        c.update(size_cases()); c.update(borderline_cases()); c.update(extreme_cases())
        c.update({k: v[:2] for k, v in selection_cases().items()})
        assert tuple(c) == CASE_NAMES
        _ALL = c
    return _ALL


def reference(name):
    """np_map_vote of a case of all_cases(), computed once and shared"""
    if name not in _REF:
        _REF[name] = np_map_vote(*all_cases()[name])
    return _REF[name]
