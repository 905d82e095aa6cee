"""Crafted inputs for the correspondence vote and compaction, and an independent reference of the vote.

A plain helper module (not a conftest): test_vote_cases.py checks the generators and np_vote against the oracle on the CPU,
test_gpu_vote.py runs the same cases through ll_vote_host, the hot path's k_vote and the fused k_vote_lm_rows.

np_vote restates laserOdometry.cpp:153-342 in vectorised float32 numpy: correctly rounded square roots, the bit-exact gap
threshold of ll_exact_math.h, and glibc's expf as the witness for every pair near the threshold.
"""
import ctypes as C
import ctypes.util

import numpy as np

GAP_BITS = 0x3e4ee4cd                                   # LL_VOTE_GAP_BITS: the smallest f32 gap with expf(-gap * gap) < 0.96f
G_T = np.array([GAP_BITS], np.uint32).view(np.float32)[0]
F32 = np.float32

_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.expf.restype = C.c_float
_libm.expf.argtypes = [C.c_float]


def f4(xyz, intensity=0.0):
    """(n, 3) -> (n, 4) float32 points"""
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    out = np.zeros((len(xyz), 4), np.float32)
    out[:, :3] = xyz.astype(np.float32)
    out[:, 3] = intensity
    return out


def _ubits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.int64)


def pair_roots(p):
    """Distance() (:153-162) of every pair of the (m, >= 3) float32 points p: f32 sqrt of (dx*dx + dy*dy) + dz*dz"""
    p = np.ascontiguousarray(p, np.float32)
    with np.errstate(all="ignore"):
        dx = p[:, None, 0] - p[None, :, 0]; dy = p[:, None, 1] - p[None, :, 1]; dz = p[:, None, 2] - p[None, :, 2]
        return np.sqrt((dx * dx + dy * dy) + dz * dz)


def region_bounds(n, regions):
    """[b0, b1) of every region: n // regions each, the last takes the remainder (:202-211)"""
    chunk = n // regions
    return [(chunk * r, n if r == regions - 1 else chunk * (r + 1)) for r in range(regions)]


def _ulp_step(a, k):
    """the float32 array a moved by k[i] ulps (through the bit pattern; a >= 0 and finite where k != 0)"""
    b = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    ok = np.isfinite(a) & (b + k >= 0)
    return np.where(ok, b + k, b).astype(np.int32).view(np.float32)


def np_vote(src, tgt, regions, perturb=None, stats=None):
    """-> (count int32[n], selected bool[n], weight float32[n]).
    perturb: a numpy Generator; every root of every pair is then moved by +1 or -1 ulp at random (what an approximate
    square root may do) -- used only to show that a case can tell such a root from the exact one.
    stats: a dict that receives near64 (pairs whose gap is within 64 ulp of the threshold, all expf-confirmed)."""
    src = np.ascontiguousarray(src, np.float32); tgt = np.ascontiguousarray(tgt, np.float32)
    n = len(src)
    cnt = np.zeros(n, np.int32); sel = np.ones(n, bool); w = np.ones(n, np.float32)
    near64 = 0
    for b0, b1 in region_bounds(n, regions):
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
        near = np.abs(_ubits(gap) - GAP_BITS) <= 64
        for i, j in np.argwhere(near):
            g = float(gap[i, j])
            g2 = F32(F32(g) * F32(g))
            assert bool(inc[i, j]) == (F32(_libm.expf(-g2)) < F32(0.96)), (g, "the gap threshold disagrees with expf")
        near64 += int(np.triu(near, 1).sum())
        np.fill_diagonal(inc, False)
        c = inc.sum(axis=1).astype(np.int32)
        cnt[b0:b1] = c
        sel[b0:b1] = ~(c.astype(np.float32) > F32(0.9) * F32(m))                     # :299-316
        w[b0:b1] = np.where(c <= 50, F32(5.0), F32(1.0))                             # :317-322
    if stats is not None:
        stats["near64"] = near64
    return cnt, sel, w


def orc_vote(orc, src, tgt, corner_case):
    """the oracle's answer in np_vote's shape (the weight of a dropped entry is what the kernels write: by count)"""
    cnt, idx, w = orc.vote(src, tgt, corner_case)
    sel = np.zeros(len(cnt), bool); sel[idx] = True
    ww = np.where(cnt <= 50, F32(5.0), F32(1.0)).astype(np.float32)
    assert (ww[idx] == w).all()
    return cnt.astype(np.int32), sel, ww


def anchor_gap_ulps(src, tgt, regions=10):
    """for every (anchor = first entry of a region, partner) pair: (gap - g_T) in ulps of the larger root, and the decision"""
    out_d, out_inc = [], []
    for b0, b1 in region_bounds(len(src), regions):
        if b1 - b0 < 2:
            continue
        s1 = pair_roots(src[b0:b1])[0, 1:]; s2 = pair_roots(tgt[b0:b1])[0, 1:]
        with np.errstate(all="ignore"):
            gap = np.abs(s1 - s2)
            big = np.maximum(s1, s2)
            d = (gap.astype(np.float64) - float(G_T)) / np.spacing(big).astype(np.float64)
        out_d.append(d); out_inc.append((_ubits(gap) >= GAP_BITS) & ~np.isnan(gap))
    return np.concatenate(out_d), np.concatenate(out_inc)


# ------------------------------------------------------------------------------------------------ borderline families
def _gap_of(s0, sj, t0, tj):
    a = pair_roots(np.stack([s0, sj]))[0, 1]; b = pair_roots(np.stack([t0, tj]))[0, 1]
    return np.abs(a - b), max(a, b)


def place_partner(src0, tgt0, tgtj, k, direction=None):
    """a source point for the partner whose target is tgtj, so that the anchor pair's gap is g_T + k half-ulps of the larger
    root: placed in f64 along `direction` (default: anchor target -> partner target) from the anchor's source at distance
    s2 + g_T + k * ulp / 2, rounded to f32, then walked by single-ulp steps of its coordinates towards that gap (the
    coordinates' own rounding is coarser than the root's ulp)."""
    src0 = np.asarray(src0, np.float32); tgt0 = np.asarray(tgt0, np.float32); tgtj = np.asarray(tgtj, np.float32)
    s2 = float(pair_roots(np.stack([tgt0, tgtj]))[0, 1])
    if direction is None:
        direction = (tgtj.astype(np.float64) - tgt0.astype(np.float64)) / s2
    s1 = s2 + float(G_T)
    want = float(G_T) + 0.5 * k * float(np.spacing(F32(s1)))
    p = (src0.astype(np.float64) + (s1 + 0.5 * k * float(np.spacing(F32(s1)))) * np.asarray(direction, np.float64)).astype(np.float32)
    err = lambda q: abs(float(_gap_of(src0, q, tgt0, tgtj)[0]) - want)
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


def borderline(scale, rng, m=12, regions=10, kmax=6):
    """regions x m correspondences; entry 0 of each region is the anchor, every partner j has its target L_j ~ scale * U(0.5, 1)
    from the anchor's along a random direction and its source along the same direction at s2_j + g_T + k_j * ulp / 2,
    k_j in -kmax .. kmax.  scale 0: all partners share the anchor's target point (s2 == 0: the gap is the source distance)."""
    n = regions * m
    src = np.zeros((n, 3), np.float32); tgt = np.zeros((n, 3), np.float32)
    for r in range(regions):
        b0 = r * m
        tgt[b0] = rng.uniform(-2, 2, 3); src[b0] = tgt[b0].astype(np.float64) + rng.normal(0, 0.03, 3)
        ks = rng.permutation(np.arange(-kmax, kmax + 1))
        for j in range(1, m):
            d = rng.standard_normal(3); d /= np.linalg.norm(d)
            tgt[b0 + j] = tgt[b0].astype(np.float64) + scale * rng.uniform(0.5, 1.0) * d
            src[b0 + j] = place_partner(src[b0], tgt[b0], tgt[b0 + j], int(ks[(j - 1) % len(ks)]), d)
    return f4(src), f4(tgt)


def ladder(kmax=40):
    """the exact ladder: one shared target point, the anchor's source at the origin, partner k at (g_T + k ulp, 0, 0): the gap
    of anchor pair k IS that float (sqrt(fl(d * d)) == d), 41 incompatible of 81.  Ten regions of 2 * kmax + 3 (anchor, 81 partners, one filler)."""
    m = 2 * kmax + 3
    src = np.zeros((10 * m, 3), np.float32); tgt = np.zeros((10 * m, 3), np.float32)
    steps = _ulp_step(np.full(2 * kmax + 1, G_T, np.float32), np.arange(-kmax, kmax + 1))
    for r in range(10):
        b0 = r * m
        tgt[b0:b0 + m] = [3.0 + r, -1.5, 0.25]
        src[b0 + 1:b0 + m - 1, r % 3] = steps * (1 if r % 2 == 0 else -1)        # along +-x, +-y, +-z in turn
        src[b0 + m - 1] = src[b0]                                                # the filler coincides with the anchor
    return f4(src), f4(tgt)


BORDERLINE_SCALES = (0, 1, 10, 100)


_BORDER = None


def borderline_cases():
    global _BORDER
    if _BORDER is not None:
        return _BORDER
    out = {f"borderline-scale{s}": borderline(s, np.random.default_rng(100 + s)) for s in BORDERLINE_SCALES}
    out["ladder"] = ladder()
    _BORDER = out
    return out


# ------------------------------------------------------------------------------------------------ other families
def consistent(n, rng, outliers):
    """consistent correspondences plus outliers whose target is displaced by 0.1 .. 3 m (gaps on both sides of the threshold)"""
    src = rng.uniform(-15, 15, (n, 3)); tgt = src + rng.normal(0, 0.03, (n, 3))
    if outliers:
        bad = rng.choice(n, outliers, replace=False)
        tgt[bad] += rng.uniform(0.1, 3.0, (outliers, 1)) * rng.standard_normal((outliers, 3))
    return f4(src), f4(tgt)


REGION_SIZES = (1, 2, 3, 9, 10, 11, 19, 20, 21, 99, 100, 101, 255, 256, 257, 511, 512, 513, 1535, 1536, 1537, 5849, 5850)


def region_cases():
    return {f"n{n}": consistent(n, np.random.default_rng(n), min(n, max(1, n // 4)) if n > 1 else 0) for n in REGION_SIZES}


def extreme_cases():
    rng = np.random.default_rng(7)
    out = {}
    src, tgt = consistent(40, rng, 6)
    src[1, 0] = 1e20                                       # dx * dx overflows: one infinite root, gap = inf -> incompatible
    src[5, 1] = -1e20; tgt[5, 1] = -1e20                   # both roots infinite: gap = NaN -> compatible
    src[6, 2] = 1e20; tgt[6, 0] = 1e20
    src[9, 0] = 1e19; src[10, 0] = -1e19                   # finite squares whose sum overflows
    out["overflow"] = (src, tgt)
    src, tgt = consistent(40, rng, 6)
    src[2, 0] = np.nan; tgt[7, 2] = np.nan; src[13, :3] = np.nan; tgt[13, :3] = np.nan
    src[21, 1] = np.inf; tgt[22, 1] = -np.inf
    out["nan"] = (src, tgt)
    src, tgt = consistent(40, rng, 0)
    for r, step in enumerate((1e-41, 1e-39, 1e-20, 1e-19, 3e-23)):        # denormal differences, denormal sums of squares
        b0 = 4 * r
        src[b0:b0 + 4, :3] = 0; tgt[b0:b0 + 4, :3] = 0
        src[b0:b0 + 4, 0] = np.arange(4) * np.float32(step); tgt[b0:b0 + 4, 1] = np.arange(4) * np.float32(2 * step)
    src[20:24, :3] = 0; src[20:24, 0] = np.arange(4) * np.float32(1e-20)
    tgt[20:24, :3] = 0; tgt[20:24, 0] = np.float32(G_T) * np.arange(4)         # gap = k * g_T minus a denormal-scale root
    out["denormal"] = (src, tgt)
    src, tgt = consistent(40, rng, 4)
    src[4:8] = src[4]; tgt[4:8] = tgt[4]                   # coincident correspondences
    src[12:16] = src[12]                                   # coincident sources, distinct targets
    tgt[24:28] = tgt[24]                                   # coincident targets, distinct sources
    src[30] = tgt[30]
    out["coincident"] = (src, tgt)
    return out


def groups_region(sizes, rng, far=1000.0):
    """one region whose entries fall into groups: within a group every pair is consistent (one common displacement), across
    groups every pair is incompatible (displacements `far` apart): an entry of group k has count m - sizes[k]"""
    m = sum(sizes)
    src = rng.uniform(-15, 15, (m, 3)); tgt = src.copy()
    order = rng.permutation(m); at = 0
    for k, sz in enumerate(sizes):
        ix = order[at:at + sz]; at += sz
        v = np.zeros(3); v[k % 3] = far * (1 + k // 3) * (1 if k % 2 == 0 else -1)
        tgt[ix] += v
    group = np.zeros(m, np.int64); at = 0
    for k, sz in enumerate(sizes):
        group[order[at:at + sz]] = k; at += sz
    return src, tgt, group


def selection_cases():
    """name -> (src, tgt, expect) with expect = {index: (count, selected, weight)} for the ten-region vote"""
    out = {}
    rng = np.random.default_rng(11)
    # ten regions of 10, in region 3 one entry against the nine others: 9 > 0.9f * 10 == 9.0f is false -> kept
    src = rng.uniform(-15, 15, (100, 3)); tgt = src.copy(); tgt[34] += [0, 1000.0, 0]
    exp = {34: (9, True, 5.0)}; exp.update({i: (1, True, 5.0) for i in range(30, 40) if i != 34})
    out["m10-count9"] = (f4(src), f4(tgt), exp)
    # a region of 60 with groups of 10 / 9 / 41: counts 50 (weight 5), 51 (weight 1) and 19, all selected (<= 54)
    src = rng.uniform(-15, 15, (600, 3)); tgt = src.copy()
    s, t, grp = groups_region((10, 9, 41), rng)
    src[120:180] = s; tgt[120:180] = t
    exp = {120 + i: ((50, True, 5.0), (51, True, 1.0), (19, True, 5.0))[g] for i, g in enumerate(grp)}
    out["m60-count50-51"] = (f4(src), f4(tgt), exp)
    # regions of 20: count 19 = floor(0.9 m) + 1 is dropped, count 18 is kept; of 60: 55 dropped (weight 1), 54 kept
    src = rng.uniform(-15, 15, (200, 3)); tgt = src.copy()
    s, t, grp = groups_region((1, 19), rng); src[40:60] = s; tgt[40:60] = t
    exp = {40 + i: ((19, False, 5.0), (1, True, 5.0))[g] for i, g in enumerate(grp)}
    s, t, grp = groups_region((2, 18), rng); src[100:120] = s; tgt[100:120] = t
    exp.update({100 + i: ((18, True, 5.0), (2, True, 5.0))[g] for i, g in enumerate(grp)})
    out["m20-count18-19"] = (f4(src), f4(tgt), exp)
    src = rng.uniform(-15, 15, (600, 3)); tgt = src.copy()
    s, t, grp = groups_region((5, 6, 49), rng); src[0:60] = s; tgt[0:60] = t
    exp = {i: ((55, False, 1.0), (54, True, 1.0), (11, True, 5.0))[g] for i, g in enumerate(grp)}
    out["m60-count54-55"] = (f4(src), f4(tgt), exp)
    return out


EXTREME_NAMES = ("overflow", "nan", "denormal", "coincident")
SELECTION_NAMES = ("m10-count9", "m60-count50-51", "m20-count18-19", "m60-count54-55")
BORDERLINE_NAMES = tuple(f"borderline-scale{s}" for s in BORDERLINE_SCALES) + ("ladder",)
CASE_NAMES = BORDERLINE_NAMES + EXTREME_NAMES + tuple(f"n{n}" for n in REGION_SIZES) + SELECTION_NAMES    # (for parametrize: builds nothing)

_ALL = None


def all_cases():
    """name -> (src, tgt): every family, built once on first use"""
    global _ALL
    if _ALL is None:
        c = {}
        c.update(borderline_cases()); c.update(extreme_cases()); c.update(region_cases())
        c.update({k: v[:2] for k, v in selection_cases().items()})
        assert tuple(c) == CASE_NAMES
        _ALL = c
    return _ALL


_REF = {}


def reference(name, corner_case):
    """np_vote of a case of all_cases(), computed once and shared"""
    key = (name, bool(corner_case))
    if key not in _REF:
        src, tgt = all_cases()[name]
        _REF[key] = np_vote(src, tgt, 5 if corner_case else 10)
    return _REF[key]


# ------------------------------------------------------------------------------------------------ the lattice (hot path)
PER_RING = 32


def lattice(rings):
    """a ring-ordered target: ring r at y = r, PER_RING points 1 m apart in x, intensity r, z gently non-planar.
    Point (r, i) has index r * PER_RING + i."""
    r, i = np.meshgrid(np.arange(rings), np.arange(PER_RING), indexing="ij")
    z = 0.08 * np.sin(0.9 * i + 0.5 * r) + 0.05 * np.cos(1.3 * r + 0.2 * i)
    out = np.zeros((rings * PER_RING, 4), np.float32)
    out[:, 0] = i.ravel(); out[:, 1] = r.ravel(); out[:, 2] = z.ravel(); out[:, 3] = r.ravel()
    return out


def offsets(n, rng, lo=0.02, hi=0.29):
    d = rng.standard_normal((n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    return d * rng.uniform(lo, hi, (n, 1))


def queries(lat, idx, off, holes=None):
    """query i = lattice point idx[i] + off[i] (its ring as intensity); a hole is lifted 50 m and finds no neighbour"""
    idx = np.asarray(idx, np.int64)
    q = np.zeros((len(idx), 4), np.float32)
    if len(idx):
        q[:, :3] = (lat[idx, :3].astype(np.float64) + off).astype(np.float32)
        q[:, 3] = lat[idx, 3]
        if holes is not None:
            q[np.asarray(holes, bool), 2] += 50.0
    return q


HOLE_PATTERNS = ("none", "all", "every-second", "first-per", "last-thread-only", "only-0", "only-last")


def hole_mask(pattern, n, nt=512):
    """which of n queries are holes; `per` is ll_block_compact's share of a thread, ceil(n / nt)"""
    h = np.zeros(n, bool)
    if n == 0:
        return h
    per = -(-n // nt)
    if pattern == "all":
        h[:] = True
    elif pattern == "every-second":
        h[1::2] = True
    elif pattern == "first-per":
        h[:per] = True
    elif pattern == "last-thread-only":                    # only the share of the last thread that has one survives
        h[:] = True; h[((n - 1) // per) * per:] = False
    elif pattern == "only-0":
        h[1:] = True
    elif pattern == "only-last":
        h[:-1] = True
    return h


def lattice_borderline(lat, rng, scale, m=12, regions=10, kmax=6):
    """a borderline family on the lattice: query 0 of each region is the anchor at a lattice point plus a small offset; the
    partners sit at the same lattice point (scale 0) or at lattice points within 2 m (scale 1), their sources placed so that
    the anchor pair's gap is g_T + k half-ulps.  Every query stays within 0.3 m of its lattice point.  -> (idx, queries)"""
    rings = len(lat) // PER_RING
    idx = np.zeros(regions * m, np.int64); q = np.zeros((regions * m, 4), np.float32)
    for r in range(regions):
        b0 = r * m
        ring0 = int(rng.integers(2, rings - 2)); i0 = int(rng.integers(2, PER_RING - 2))
        a = ring0 * PER_RING + i0
        idx[b0] = a
        src0 = (lat[a, :3].astype(np.float64) + offsets(1, rng, 0.01, 0.08)[0]).astype(np.float32)
        q[b0, :3] = src0; q[b0, 3] = lat[a, 3]
        ks = rng.permutation(np.arange(-kmax, kmax + 1))
        for j in range(1, m):
            if scale == 0:
                b = a; d = rng.standard_normal(3); d /= np.linalg.norm(d)
            else:
                dr, di = [(0, 1), (0, -1), (1, 0), (-1, 0), (1, 1), (-1, 1), (1, -1), (-1, -1), (0, 2), (0, -2), (2, 0), (-2, 0)][(j - 1) % 12]
                b = (ring0 + dr) * PER_RING + i0 + di; d = None
            idx[b0 + j] = b
            q[b0 + j, :3] = place_partner(src0, lat[a, :3], lat[b, :3], int(ks[(j - 1) % len(ks)]), d)
            q[b0 + j, 3] = lat[b, 3]
    assert np.linalg.norm(q[:, :3].astype(np.float64) - lat[idx, :3], axis=1).max() < 0.3
    return idx, q
