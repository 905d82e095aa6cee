"""An independent numpy restatement of ll_places (include/lightloam_hip.h) and the inputs of its tests.

np_describe is the descriptor in float32 numpy, operation by operation as the header states it; its angles come from the host
atan2f (oracle.orc.libm), to which tests/test_exact_math.py pins ll_atan2f -- np.arctan2 may be routed through a SIMD library with
other roundings.  np_distances is the distance in float64 from the float32 descriptors, all 60 shifts.  No expected value of any
test comes from the library.  tests/test_place_cases.py checks, without a GPU, that the inputs stay inside their own preconditions.
"""
import numpy as np

RINGS, SECTORS = 20, 60
TWO_PI_F = np.float32(6.2831855)
K_F = np.float32(60.0 / (2.0 * np.pi))


def np_describe(points, max_radius=80.0, z_offset=2.0):
    """points (n, >= 3) -> desc[20][60] float32"""
    from oracle import orc
    p = np.asarray(points, np.float32)
    p = p.reshape(-1, p.shape[-1] if p.ndim == 2 else 4)
    desc = np.zeros((RINGS, SECTORS), np.float32)
    if len(p) == 0:
        return desc
    x, y, z = (np.ascontiguousarray(p[:, k]) for k in range(3))
    R = np.float32(max_radius)
    with np.errstate(all="ignore"):
        r = np.sqrt(x * x + y * y)                                  # float32 throughout: every product and sum rounded
        keep = r < R                                                # a NaN fails
        x, y, z, r = x[keep], y[keep], z[keep], r[keep]
        if len(r) == 0:
            return desc
        w = R / np.float32(20.0)
        i = np.minimum(RINGS - 1, (r / w).astype(np.int32))
        a = orc.libm(1, y, x)
        a = np.where(a < 0, a + TWO_PI_F, a).astype(np.float32)
        j = np.minimum(SECTORS - 1, (a * K_F).astype(np.int32))
        v = z + np.float32(z_offset)
    flat = np.full(RINGS * SECTORS, -np.inf, np.float32)
    hit = np.zeros(RINGS * SECTORS, bool)
    np.maximum.at(flat, i * SECTORS + j, v)
    hit[i * SECTORS + j] = True
    return np.where(hit, flat, np.float32(0)).astype(np.float32).reshape(RINGS, SECTORS)


def np_unit(desc):
    """float64 unit columns and which columns are not empty"""
    d = np.asarray(desc, np.float32).astype(np.float64).reshape(RINGS, SECTORS)
    nrm = np.sqrt((d * d).sum(axis=0))
    full = nrm != 0
    return np.where(full, d / np.where(full, nrm, 1.0), 0.0), full


def np_distances(q, c):
    """d(s), s = 0 .. 59, in float64: query q against candidate c"""
    uq, fq = np_unit(q)
    uc, fc = np_unit(c)
    G = uq.T @ uc                                                   # G[i][j] = query column i . candidate column j
    j = np.arange(SECTORS)
    d = np.ones(SECTORS)
    for s in range(SECTORS):
        i = (j + s) % SECTORS
        both = fq[i] & fc[j]
        n = int(both.sum())
        if n:
            d[s] = 1.0 - G[i, j][both].sum() / n
    return d


def np_best(q, c):
    d = np_distances(q, c)
    s = int(np.argmin(d))                                           # the first minimum: the lower shift
    return d[s], s, d


# ---------------------------------------------------------------------------------------------- crafted descriptor clouds
def _pt(x, y, z):
    return [np.float32(x), np.float32(y), np.float32(z), np.float32(0)]


def _inside(rng, n, max_radius=80.0):
    """n points at least 5 % of a bin away from every bin edge, random bins, z in -4 .. 6 (some below -z_offset)"""
    w = max_radius / RINGS
    i = rng.integers(0, RINGS, n); j = rng.integers(0, SECTORS, n)
    r = (i + rng.uniform(0.05, 0.95, n)) * w
    a = (j + rng.uniform(0.05, 0.95, n)) * (2 * np.pi / SECTORS)
    z = rng.uniform(-4.0, 6.0, n)
    return np.stack([r * np.cos(a), r * np.sin(a), z, np.zeros(n)], axis=1).astype(np.float32)


def describe_cases():
    """name -> (points (n, 4) float32, on_edge (n,) bool: the point lies on a bin edge ON PURPOSE)"""
    below = np.nextafter(np.float32(80.0), np.float32(0.0))
    cases = {}
    # r exactly k * w on the x axis (also a sector edge) and, off the axes, on 3-4-5 triangles
    pts = [_pt(4.0 * k, 0.0, 0.25 * k - 1.0) for k in range(RINGS)] + [_pt(12, 16, 1.0), _pt(24, 32, 2.0), _pt(36, 48, 3.0), _pt(-16, 12, 1.5)]
    cases["ring_edges"] = (pts, [True] * len(pts))
    pts = [_pt(80.0, 0.0, 5.0), _pt(below, 0.0, 1.0), _pt(0.0, 80.0, 5.0), _pt(0.0, -below, 2.0), _pt(48.0, 64.0, 7.0), _pt(100.0, 3.0, 9.0),
           _pt(np.nan, 1.0, 9.0), _pt(1.0, np.inf, 9.0)]
    cases["max_radius"] = (pts, [True] * len(pts))
    cases["origin"] = ([_pt(0.0, 0.0, 0.5)], [True])
    pts = [_pt(10, 0, 0.1), _pt(0, 10, 0.2), _pt(-10, 0, 0.3), _pt(0, -10, 0.4), _pt(-10, -0.0, 0.6)]
    cases["axes"] = (pts, [True] * len(pts))
    # a barely negative angle becomes 6.2831855f, and 6.2831855f * k is above 60
    pts = [_pt(10, -1e-30, 0.7), _pt(30, -1e-7, 0.8), _pt(50, -1e-20, 0.9)]
    cases["sector_clamp"] = (pts, [True] * len(pts))
    mid = lambda i, j, z: _pt((i + 0.5) * 4.0 * np.cos((j + 0.5) * np.pi / 30), (i + 0.5) * 4.0 * np.sin((j + 0.5) * np.pi / 30), z)  # noqa: E731
    pts = [mid(3, 7, 1.0), mid(3, 7, 2.5), mid(9, 40, 4.0), mid(9, 40, -1.0), mid(19, 59, 0.0), mid(0, 0, -0.5)]
    cases["two_in_a_bin"] = (pts, [False] * len(pts))
    pts = [mid(5, 5, -5.0), mid(5, 5, -3.0), mid(6, 5, -2.5), mid(7, 5, -2.0)]          # -3, -1, -0.5 and an exact 0 with a point
    cases["below_ground"] = (pts, [False] * len(pts))
    rng = np.random.default_rng(20260101)
    for n in (0, 1, 255, 256, 257, 4097):
        cases["n%d" % n] = (_inside(rng, n), [False] * n)
    return {k: (np.asarray(p, np.float32).reshape(-1, 4), np.asarray(e, bool)) for k, (p, e) in cases.items()}


# ---------------------------------------------------------------------------------------------- one-hot match cases
def onehot(ring_of_column, value=1.0):
    """desc with one cell `value` per column: ring_of_column[j] = the ring, or -1 for an empty column"""
    d = np.zeros((RINGS, SECTORS), np.float32)
    for j, r in enumerate(ring_of_column):
        if r >= 0:
            d[r, j] = value
    return d


def onehot_expected(q, c):
    """(distance float32, shift) of two one-hot descriptors in exact arithmetic: unit columns are exactly 1, sim is an integer"""
    rq = np.where(q.any(axis=0), q.argmax(axis=0), -1); rc = np.where(c.any(axis=0), c.argmax(axis=0), -1)
    j = np.arange(SECTORS)
    best = (np.float32(np.inf), 0)
    for s in range(SECTORS):
        i = (j + s) % SECTORS
        both = (rq[i] >= 0) & (rc[j] >= 0)
        n = int(both.sum()); sim = int((both & (rq[i] == rc[j])).sum())
        d = np.float32(1.0) - np.float32(sim) / np.float32(n) if n else np.float32(1.0)
        if d < best[0]:
            best = (d, s)
    return best


def onehot_cases():
    """name -> (query desc, candidate desc, the shift the case is about or None).  The query is the candidate turned by +s sectors:
    its column (j + s) mod 60 is the candidate's column j."""
    rng = np.random.default_rng(7)
    base = rng.integers(0, RINGS, SECTORS)
    turn = lambda rings, s: np.roll(rings, s)                      # noqa: E731  out[(j + s) % 60] = rings[j]
    cases = {}
    for s in (0, 1, 30, 59):
        cases["shift%d" % s] = (onehot(turn(base, s), 3.0), onehot(base, 0.5), s)
    cases["asymmetric7"] = (onehot(turn(base, 7)), onehot(base), 7)          # rows and columns swapped would answer 53
    eq = base.copy(); eq[[2, 3, 17, 44]] = -1
    ec = base.copy(); ec[[5, 17, 29, 30, 31]] = -1
    cases["empty_in_q"] = (onehot(turn(eq, 11)), onehot(base), 11)
    cases["empty_in_c"] = (onehot(turn(base, 11)), onehot(ec), 11)
    cases["empty_in_both"] = (onehot(turn(eq, 42)), onehot(ec), 42)           # count changes with the shift
    half = base.copy(); half[30:] = -1
    cases["half_empty"] = (onehot(turn(half, 20)), onehot(half), 20)
    part = base.copy(); part[::2] = (part[::2] + 1) % RINGS                  # half of the columns disagree at the best shift: d = 0.5
    cases["half_agree"] = (onehot(turn(part, 3)), onehot(base), 3)
    zero = np.zeros((RINGS, SECTORS), np.float32)
    cases["all_empty_both"] = (zero, zero, 0)
    cases["all_empty_q"] = (zero, onehot(base), 0)
    cases["all_empty_c"] = (onehot(base), zero, 0)
    return cases


# ---------------------------------------------------------------------------------------------- random match cases
MATCH_SIZES = [(1, 1), (3, 33), (33, 65), (2, 130)]


def random_descriptor(rng):
    """non-negative heights, about 30 % of the bins empty, a few whole columns empty"""
    d = rng.uniform(0.05, 6.0, (RINGS, SECTORS)).astype(np.float32)
    d[rng.random((RINGS, SECTORS)) < 0.3] = 0
    d[:, rng.choice(SECTORS, 4, replace=False)] = 0
    return d


def random_match_case(nq, nc, seed=None):
    """(queries [nq], candidates [nc], turned [nq]): query i is candidate i mod nc turned by turned[i] sectors with 5 % noise on its
    heights, so every query has one revisit with a clear heading; every other pair is unrelated"""
    rng = np.random.default_rng(1000 * nq + nc if seed is None else seed)
    cand = [random_descriptor(rng) for _ in range(nc)]
    turned = rng.integers(0, SECTORS, nq)
    qs = [np.roll(cand[i % nc] * rng.uniform(0.95, 1.05, (RINGS, SECTORS)).astype(np.float32), int(turned[i]), axis=1) for i in range(nq)]
    return qs, cand, turned


MATCH_K = (1, 3, 8)
MATCH_NC = 70


def topk_case():
    """5 queries over 70 candidates with clear ranks: per query ten copies of its own descriptor under growing noise (5 %, 10 %,
    ... 50 % on the heights, each turned by some sectors), so its first ten distances rise in steps far above any rounding; twenty
    unrelated candidates; all in a shuffled order.  Candidate 41 is a copy of candidate 12, query 0's second best: a tie."""
    rng = np.random.default_rng(4242)
    qs = [random_descriptor(rng) for _ in range(5)]
    cand, tag = [], []
    for i, q in enumerate(qs):
        for level in range(10):
            n = 0.05 * (level + 1)
            cand.append(np.roll(q * rng.uniform(1 - n, 1 + n, (RINGS, SECTORS)).astype(np.float32), -int(rng.integers(0, SECTORS)), axis=1))
            tag.append((i, level))
    for _ in range(MATCH_NC - len(cand)):
        cand.append(random_descriptor(rng)); tag.append((-1, 0))
    order = rng.permutation(MATCH_NC)
    cand = [cand[k] for k in order]; tag = [tag[k] for k in order]
    for want, at in (((0, 1), 12), ((-1, 0), 41)):                 # query 0's second best to place 12, an unrelated one to 41
        k = tag.index(want)
        cand[k], cand[at] = cand[at], cand[k]; tag[k], tag[at] = tag[at], tag[k]
    cand[41] = cand[12].copy()
    return qs, cand


def np_ranking(qs, cand):
    """float64 best distance [nq][nc]"""
    return np.array([[np_best(q, c)[0] for c in cand] for q in qs])


# ---------------------------------------------------------------------------------------------- the lap
LAP_DB = list(range(0, 600, 40))                                    # scans 0, 40, ..., 560
LAP_QUERIES = [628, 708, 828, 948]                                  # the circle of 100 m closes every 628.3 scans


def quarter_turn(scan):
    """(x, y) -> (-y, x): the scan turned by +90 degrees about z, exact in floats"""
    t = np.array(scan, np.float32, copy=True)
    t[:, 0], t[:, 1] = -scan[:, 1], scan[:, 0].copy()
    return t


def lap_scans(synth, rings=16):
    """(database scans, query scans, expected database index per query, expected shift per query)"""
    cfg = synth.default_cfg(rings)
    db = [synth.scan(cfg, k) for k in LAP_DB]
    plain = [synth.scan(cfg, k) for k in LAP_QUERIES]
    queries = plain + [quarter_turn(s) for s in plain]
    want = [LAP_DB.index(k - 628) for k in LAP_QUERIES] * 2
    shift = [0] * len(plain) + [15] * len(plain)
    return db, queries, want, shift
