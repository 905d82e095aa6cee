"""ll_pcm's contract restated in numpy, independent of the library: the pair arithmetic in the operation order the header fixes (numpy's
f64 + - * round as C's do, one operation at a time), the greedy clique on Python big-int bitsets, and the generators of the tests' graphs
and of the double-lap scene."""
import numpy as np

DEFAULT = dict(rot_tol=0.05, trans_tol=0.5, rot_rate=2e-4, trans_rate=0.02)
GRID = 2.0 ** -10


# ------------------------------------------------------------------ pose algebra, arrays [..., 7] = (qx, qy, qz, qw, tx, ty, tz)
def qmul(a, b):
    ax, ay, az, aw = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
    bx, by, bz, bw = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    return np.stack([aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw,
                     aw * bw - ax * bx - ay * by - az * bz], axis=-1)


def rotate(q, v):
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    r00 = 1.0 - 2.0 * (y * y + z * z); r01 = 2.0 * (x * y - z * w); r02 = 2.0 * (x * z + y * w)
    r10 = 2.0 * (x * y + z * w); r11 = 1.0 - 2.0 * (x * x + z * z); r12 = 2.0 * (y * z - x * w)
    r20 = 2.0 * (x * z - y * w); r21 = 2.0 * (y * z + x * w); r22 = 1.0 - 2.0 * (x * x + y * y)
    v0, v1, v2 = v[..., 0], v[..., 1], v[..., 2]
    return np.stack([(r00 * v0 + r01 * v1) + r02 * v2, (r10 * v0 + r11 * v1) + r12 * v2, (r20 * v0 + r21 * v1) + r22 * v2], axis=-1)


def compose(a, b):
    a, b = np.broadcast_arrays(a, b)
    return np.concatenate([qmul(a[..., :4], b[..., :4]), rotate(a[..., :4], b[..., 4:]) + a[..., 4:]], axis=-1)


def inverse(a):
    qc = a[..., :4] * np.array([-1.0, -1.0, -1.0, 1.0])
    return np.concatenate([qc, -rotate(qc, a[..., 4:])], axis=-1)


def normalise(p):
    p = np.array(p, np.float64).reshape(-1, 7)
    x, y, z, w = p[:, 0], p[:, 1], p[:, 2], p[:, 3]
    n = np.sqrt((x * x + y * y) + (z * z + w * w))
    out = p.copy()
    out[:, :4] = p[:, :4] / n[:, None]
    return out


def path_length(P):
    s = np.zeros(len(P))
    with np.errstate(all="ignore"):
        for k in range(1, len(P)):
            dx, dy, dz = P[k, 4] - P[k - 1, 4], P[k, 5] - P[k - 1, 5], P[k, 6] - P[k - 1, 6]
            s[k] = s[k - 1] + np.sqrt((dx * dx + dy * dy) + dz * dz)
    return s


def split(cands):
    """(i [C], j [C], Z [C, 7]) of a list of tuples starting with (i, j, Z)"""
    i = np.array([int(c[0]) for c in cands], np.int64); j = np.array([int(c[1]) for c in cands], np.int64)
    Z = np.array([np.asarray(c[2], np.float64) for c in cands], np.float64).reshape(-1, 7)
    return i, j, Z


def pair_terms(poses, cands, params=None):
    """(rot2, trans2, ar2, at2), each [C, C], entry (c, d) evaluated as the header evaluates the pair (c, d) -- meaningful for c < d"""
    p = dict(DEFAULT); p.update(params or {})
    P = normalise(poses); s = path_length(P)
    i, j, Z = split(cands)
    Z = normalise(Z)
    with np.errstate(all="ignore"):
        B = compose(Z, inverse(P[j]))
        Ai = compose(compose(P[j], inverse(Z)), inverse(P[i]))
        E = compose(compose(B[:, None, :], Ai[None, :, :]), P[i][:, None, :])
        rot2 = 4.0 * ((E[..., 0] * E[..., 0] + E[..., 1] * E[..., 1]) + E[..., 2] * E[..., 2])
        trans2 = (E[..., 4] * E[..., 4] + E[..., 5] * E[..., 5]) + E[..., 6] * E[..., 6]
        L = np.abs(s[i][:, None] - s[i][None, :]) + np.abs(s[j][:, None] - s[j][None, :])
        ar = p["rot_tol"] + p["rot_rate"] * L; at = p["trans_tol"] + p["trans_rate"] * L
        return rot2, trans2, ar * ar, at * at


def adjacency(poses, cands, params=None):
    """the consistency matrix, bool [C, C]: the upper triangle evaluated, mirrored; zero diagonal"""
    C = len(cands)
    if C == 0:
        return np.zeros((0, 0), bool)
    rot2, trans2, ar2, at2 = pair_terms(poses, cands, params)
    with np.errstate(all="ignore"):
        finite = (rot2 - rot2 == 0.0) & (trans2 - trans2 == 0.0) & (ar2 - ar2 == 0.0) & (at2 - at2 == 0.0)
        ok = finite & (rot2 <= ar2) & (trans2 <= at2)
    up = np.triu(ok, 1)
    return up | up.T


def _bitset(row):
    return int.from_bytes(np.packbits(row, bitorder="little").tobytes(), "little")


def select(adj):
    """(selected bool [C], degree [C], record dict): every start, no pruning"""
    adj = np.asarray(adj, bool); C = len(adj)
    if C == 0:
        return np.zeros(0, bool), np.zeros(0, np.int32), dict(n_candidates=0, n_selected=0, start=-1, max_degree=0, n_consistent_pairs=0)
    deg = adj.sum(1).astype(np.int32)
    order = sorted(range(C), key=lambda c: (-int(deg[c]), c))
    rel = adj[np.ix_(order, order)]
    N = [_bitset(rel[r]) for r in range(C)]
    best, best_M, best_v = 0, 0, -1
    for v in range(C):
        M, U, size = 1 << v, N[v], 1
        while U:
            u = (U & -U).bit_length() - 1
            M |= 1 << u; U &= N[u]; size += 1
        if size > best:
            best, best_M, best_v = size, M, v
    sel = np.zeros(C, bool)
    for r in range(C):
        if (best_M >> r) & 1:
            sel[order[r]] = True
    return sel, deg, dict(n_candidates=C, n_selected=best, start=order[best_v], max_degree=int(deg.max()), n_consistent_pairs=int(deg.sum()) // 2)


def pcm(poses, cands, params=None):
    adj = adjacency(poses, cands, params)
    return (adj,) + select(adj)


def record_tuple(r):
    """a PcmRecord or a record dict as a comparable tuple"""
    get = (lambda k: r[k]) if isinstance(r, dict) else (lambda k: getattr(r, k))
    return tuple(int(get(k)) for k in ("n_candidates", "n_selected", "start", "max_degree", "n_consistent_pairs"))


# ------------------------------------------------------------------ generators
def quat_z(a):
    return np.array([0.0, 0.0, np.sin(a / 2), np.cos(a / 2)])


def quat_rv(v):
    v = np.asarray(v, np.float64); a = np.linalg.norm(v)
    if a == 0.0:
        return np.array([0.0, 0.0, 0.0, 1.0])
    return np.concatenate([np.sin(a / 2) * v / a, [np.cos(a / 2)]])


def pose(q, t):
    return np.concatenate([np.asarray(q, np.float64), np.asarray(t, np.float64)])


def relative(Pi, Pj):
    return compose(inverse(np.asarray(Pi, np.float64)), np.asarray(Pj, np.float64))


def chain(steps, start=None):
    P = [pose([0, 0, 0, 1], [0, 0, 0]) if start is None else np.asarray(start, np.float64)]
    for d in steps:
        n = compose(P[-1], d); n[:4] /= np.linalg.norm(n[:4])
        P.append(n)
    return np.array(P)


def random_graph(seed, N, C, p_true=0.6):
    """a wandering trajectory of N poses and C candidates: true ones (the poses' own relative pose plus noise of the thresholds' size, so
    pairs fall on both sides) and random ones; un-normalised quaternions on purpose"""
    rng = np.random.default_rng(seed)
    steps = [pose(quat_rv(rng.normal(0, 0.08, 3)), [1.0 + rng.normal(0, 0.1), rng.normal(0, 0.05), rng.normal(0, 0.02)]) for _ in range(N - 1)]
    P = chain(steps)
    cands = []
    for _ in range(C):
        i, j = rng.choice(N, 2, replace=False)
        if rng.random() < p_true:
            noise = pose(quat_rv(rng.normal(0, 0.02, 3)), rng.normal(0, 0.25, 3))
            Z = compose(relative(P[i], P[j]), noise)
        else:
            Z = pose(quat_rv(rng.normal(0, 1.0, 3)), rng.normal(0, 5.0, 3))
        Z[:4] *= rng.uniform(0.5, 2.0)
        cands.append((int(i), int(j), Z))
    P = P.copy(); P[:, :4] *= rng.uniform(0.5, 2.0, (N, 1))
    return P, cands


# exact-arithmetic graphs: identity and 180-degree quaternions, translations on the 2^-10 grid, thresholds on the grid: every product
# and sum below is exact, so the expected bit is known without any arithmetic of doubt
Q_ID = [0.0, 0.0, 0.0, 1.0]
Q_X, Q_Y, Q_Z = [1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0]
EXACT_PARAMS = dict(rot_tol=0.0, trans_tol=0.5, rot_rate=0.0, trans_rate=2.0 ** -6)


def exact_line(N=40, step=1.0):
    """N identity poses a step apart along x: s[k] = k * step exactly"""
    return np.array([pose(Q_ID, [k * step, 0.0, 0.0]) for k in range(N)])


def exact_candidate(P, i, j, off=(0.0, 0.0, 0.0), q=Q_ID):
    """Z = (q, R(q) u), u = the true translation from pose i to pose j (identity rotations) plus off: against the candidate (i, j) with
    the true Z the cycle is (q*, -off)"""
    u = P[j, 4:] - P[i, 4:] + np.asarray(off, np.float64)
    return (i, j, pose(q, rotate(np.asarray(q, np.float64), u)))


def exact_cases():
    """[(name, poses, candidates, params, expected bool matrix)] -- pairs of candidates on a line of identity poses.  For candidates
    (i, j, off_c) and (i', j', off_d) with identity rotations the cycle's translation is off_c - off_d and its rotation zero, L =
    |i - i'| + |j - j'| steps; a 180-degree turn q in the second one leaves the translation and gives |vec(q_E)| = 1, rot2 = 4"""
    P = exact_line()
    cases = []

    def two(name, c, d, params, want):
        cases.append((name, P, [c, d], params, np.array([[False, want], [want, False]])))

    g = GRID
    # L = 0 (same endpoints): at = trans_tol = 0.5 exactly; hit, one grid step inside, one outside
    for name, off, want in (("tol-hit", 0.5, True), ("tol-inside", 0.5 - g, True), ("tol-outside", 0.5 + g, False)):
        two("L0-" + name, exact_candidate(P, 3, 20), exact_candidate(P, 3, 20, (off, 0.0, 0.0)), EXACT_PARAMS, want)
    # L = 32 + 32 = 64 steps of 1 m: at = 0.5 + 64 / 64 = 1.5: only the rate term admits 1.5
    for name, off, want in (("rate-hit", 1.5, True), ("rate-inside", 1.5 - g, True), ("rate-outside", 1.5 + g, False)):
        two("L64-" + name, exact_candidate(P, 0, 5), exact_candidate(P, 32, 37, (0.0, off, 0.0)), EXACT_PARAMS, want)
    two("L64-without-rate", exact_candidate(P, 0, 5), exact_candidate(P, 32, 37, (0.0, 1.5, 0.0)), dict(EXACT_PARAMS, trans_rate=0.0), False)
    # rotation: a 180-degree turn in one candidate: |vec(q_E)| = 1, rot2 = 4: ar = 2 hits, anything below fails
    turned = exact_candidate(P, 3, 20, q=Q_Z)
    two("rot-hit", exact_candidate(P, 3, 20), turned, dict(EXACT_PARAMS, rot_tol=2.0), True)
    two("rot-outside", exact_candidate(P, 3, 20), turned, dict(EXACT_PARAMS, rot_tol=2.0 - g), False)
    two("rot-inside", exact_candidate(P, 3, 20), turned, dict(EXACT_PARAMS, rot_tol=2.0 + g), True)
    # L = 64: ar = 1 + 64 / 64 = 2 admits the turn only through the rate; at L = 63 it does not
    two("rot-by-rate", exact_candidate(P, 0, 5), exact_candidate(P, 32, 37, q=Q_X), dict(EXACT_PARAMS, rot_tol=1.0, rot_rate=2.0 ** -6), True)
    two("rot-by-rate-short", exact_candidate(P, 0, 5), exact_candidate(P, 31, 37, q=Q_X), dict(EXACT_PARAMS, rot_tol=1.0, rot_rate=2.0 ** -6), False)
    # passes rotation, fails translation -- and the reverse
    two("rot-ok-trans-bad", exact_candidate(P, 3, 20), exact_candidate(P, 3, 20, (0.0, 0.0, 1.0)), dict(EXACT_PARAMS, rot_tol=2.0), False)
    two("trans-ok-rot-bad", exact_candidate(P, 3, 20), turned, dict(EXACT_PARAMS, rot_tol=1.0), False)
    # two candidates on the same (i, j), the same Z: the cycle is the identity
    two("duplicate", exact_candidate(P, 7, 30, (0.25, 0.0, 0.0)), exact_candidate(P, 7, 30, (0.25, 0.0, 0.0)), dict(EXACT_PARAMS, trans_tol=0.0, trans_rate=0.0), True)
    # N = 2: (0, 1) and its reverse (1, 0) agree (L = 2); (0, 1) off by 0.5 + g fails against (0, 1) at L = 0 and passes against (1, 0), where
    # L = 2 gives at = 0.5 + 2 / 64
    P2 = exact_line(2)
    cases.append(("N2", P2, [exact_candidate(P2, 0, 1), exact_candidate(P2, 1, 0), exact_candidate(P2, 0, 1, (0.5 + g, 0.0, 0.0))], EXACT_PARAMS,
                  np.array([[False, True, False], [True, False, True], [False, True, False]])))
    # coordinates of 1e200: trans2 overflows against the near candidate, and the path length itself is infinite from node 30 on, so L of the
    # two far duplicates is inf - inf: every pair is inconsistent, none is decided by a NaN comparison
    far = exact_line(); far = far.copy(); far[30:, 5] = 1e200
    cases.append(("huge", far, [exact_candidate(far, 3, 20), (3, 35, pose(Q_ID, [32.0, 0.0, 0.0])), (3, 35, pose(Q_ID, [32.0, 0.0, 0.0]))], EXACT_PARAMS,
                  np.zeros((3, 3), bool)))
    # the same with finite path lengths (the jump is one step of 1e200, s stays finite): the far duplicates agree exactly, the near one
    # is 1e200 away from them
    far2 = exact_line().copy(); far2[30:, 5] = 1e150
    cases.append(("huge-finite", far2, [exact_candidate(far2, 3, 20), exact_candidate(far2, 3, 35), exact_candidate(far2, 3, 35), (3, 35, pose(Q_ID, [32.0, 0.0, 0.0]))],
                  EXACT_PARAMS, np.array([[False, True, True, False], [True, False, True, False], [True, True, False, False], [False, False, False, False]])))
    return cases


def graph_matrix(kind, C, seed=0):
    """adjacency matrices for the selection's direct tests"""
    rng = np.random.default_rng(seed)
    a = np.zeros((C, C), bool)
    if kind == "empty":
        pass
    elif kind == "complete":
        a[:] = True
    elif kind == "two-cliques":                                      # two disjoint cliques of equal size: the tie goes to the earliest start
        h = C // 2
        idx = rng.permutation(C)
        for part in (idx[:h], idx[h:2 * h]):
            a[np.ix_(part, part)] = True
    elif kind == "star":
        a[0, :] = True; a[:, 0] = True
    elif kind == "path":
        k = np.arange(C - 1); a[k, k + 1] = True; a[k + 1, k] = True
    elif kind == "gnp":
        u = np.triu(rng.random((C, C)) < 0.1, 1); a = u | u.T
    elif kind == "planted":                                          # a clique of 40 in a sparse random graph
        u = np.triu(rng.random((C, C)) < 0.002, 1); a = u | u.T
        part = rng.choice(C, 40, replace=False)
        a[np.ix_(part, part)] = True
    else:
        raise ValueError(kind)
    np.fill_diagonal(a, False)
    return a


# ------------------------------------------------------------------ the double-lap scene
def double_lap(N=80, seed=7, n_true=24, n_false=16, n_alias=6, radius=20.0, scale=1.02, yaw_bias=3.3e-3, noise=(2e-4, 5e-3)):
    """Two laps of a circle in N poses.  Ground truth gt; odometry est = the truth's own steps with a scale error, a yaw bias per step and
    noise, integrated from the true start.  Candidates measure the truth (plus noise): n_true real revisits (k, k + N / 2), n_false random
    pairs with random measurements, and n_alias that all tell one and the same wrong story -- a look-alike place: a stretch of the second
    lap is taken for the stretch a quarter lap before it, by every one of them with the same wrong world offset -- so they are consistent
    among themselves.  Returns dict(gt, est, cands, true, false, alias: index arrays, odom: [(k, k + 1, Z)])"""
    rng = np.random.default_rng(seed)
    half = N // 2
    dth = 2.0 * np.pi / half
    step = pose(quat_z(dth), [2.0 * radius * np.sin(dth / 2) * np.cos(dth / 2), 2.0 * radius * np.sin(dth / 2) * np.sin(dth / 2), 0.0])
    gt = chain([step] * (N - 1))
    odom = []
    for k in range(N - 1):
        d = relative(gt[k], gt[k + 1])
        e = pose(quat_rv(np.array([0.0, 0.0, yaw_bias]) + rng.normal(0, noise[0], 3)), rng.normal(0, noise[1], 3))
        z = compose(d, e); z[4:] = z[4:] * scale; z[:4] /= np.linalg.norm(z[:4])
        odom.append((k, k + 1, z))
    est = chain([z for _, _, z in odom])
    cands, kind = [], []
    meas = lambda: pose(quat_rv(rng.normal(0, 2e-3, 3)), rng.normal(0, 0.02, 3))
    for k in rng.choice(half, n_true, replace=False):
        cands.append((int(k), int(k + half), compose(relative(gt[k], gt[k + half]), meas()))); kind.append(0)
    for _ in range(n_false):
        i, j = rng.choice(N, 2, replace=False)
        cands.append((int(i), int(j), pose(quat_rv(rng.normal(0, 0.5, 3)), rng.normal(0, 4.0, 3)))); kind.append(1)
    quarter = half // 4
    for m in range(n_alias):                                         # j is a quarter lap past i's place; the measurement says "the same place"
        cands.append((2 + m, half + quarter + 2 + m, meas())); kind.append(2)
    perm = rng.permutation(len(cands))
    cands = [cands[p] for p in perm]; kind = np.array(kind)[perm]
    return dict(gt=gt, est=est, cands=cands, true=np.flatnonzero(kind == 0), false=np.flatnonzero(kind == 1), alias=np.flatnonzero(kind == 2), odom=odom)


def ate(P, gt):
    """translational ATE: the RMS distance of the positions, no alignment (node 0 is fixed at the truth)"""
    d = np.asarray(P)[:, 4:] - np.asarray(gt)[:, 4:]
    return float(np.sqrt((d * d).sum(1).mean()))
