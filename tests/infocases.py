"""A numpy float64 restatement of what the information feature adds, on top of tests/posegraphcases.py (imported, not edited):
edge_from_info as include/lightloam_hip.h specifies it, the pose-graph residual with a FULL square-root information, its cost, its
linearisation by central differences and a dense Levenberg-Marquardt on it.  Nothing here comes from the library.

An edge is posegraphcases' tuple (i, j, Z[7], s, a) whose weight s is either the six diagonal entries or a 6 x 6 matrix S:
    e = [2 sgn(w_e) vec(q_e) ; t_e] of E = Z^-1 P_i^-1 P_j,   r = S e   (S = diag(s) for six entries)."""
import numpy as np

import posegraphcases as pc


def weight(s):
    """the 6 x 6 matrix an edge's weight stands for"""
    s = np.asarray(s, float)
    return s if s.ndim == 2 else np.diag(np.broadcast_to(s, (6,)))


# ------------------------------------------------------------------------------------------------ record -> edge
def information(H, X, sigma, floor=0.0):
    """Lambda = M^-T H M^-1 / sigma^2 + floor I with M^-1 = blkdiag(R(X) / 2, R(X)): the information in the tangent of the edge error"""
    R = pc.qmat(np.asarray(X, float)[:4])
    Mi = np.zeros((6, 6)); Mi[:3, :3] = 0.5 * R; Mi[3:, 3:] = R
    L = Mi.T @ np.asarray(H, float).reshape(6, 6) @ Mi / (sigma * sigma)
    return 0.5 * (L + L.T) + floor * np.eye(6)


def edge_from_info(H, X, sigma, floor=0.0):
    """the upper-triangular S with S^T S = information(...); numpy raises LinAlgError when it is not positive definite"""
    return np.linalg.cholesky(information(H, X, sigma, floor)).T


def spd(rng, lo=0.5, hi=50.0):
    """a random symmetric positive definite 6 x 6 with eigenvalues in [lo, hi]"""
    Q, _ = np.linalg.qr(rng.normal(size=(6, 6)))
    return Q @ np.diag(rng.uniform(lo, hi, 6)) @ Q.T


# ------------------------------------------------------------------------------------------------ residual, cost, linearisation
def residual(Pi, Pj, edge):
    unit = (edge[0], edge[1], edge[2], np.ones(6), edge[4])
    return weight(edge[3]) @ pc.residual(Pi, Pj, unit)


# The same over all edges of a graph at once (arrays [E, ...]): posegraphcases' formulas, restated for stacked operands, so that the
# central differences of a 300-node graph cost 24 array passes and not 7200 calls.  test_info_cases.py holds the two against each other.
def _qmul(a, b):
    ax, ay, az, aw = np.moveaxis(a, -1, 0); bx, by, bz, bw = np.moveaxis(b, -1, 0)
    return np.stack([aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw,
                     aw * bw - ax * bx - ay * by - az * bz], -1)


def _qconj(q):
    return q * np.array([-1.0, -1.0, -1.0, 1.0])


def _rot(q, v):
    """R(q / |q|) v, through the matrix of posegraphcases.qmat"""
    x, y, z, w = np.moveaxis(q / np.linalg.norm(q, axis=-1, keepdims=True), -1, 0)
    R = np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], -1),
                  np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], -1),
                  np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1)], -2)
    return np.einsum("...ab,...b->...a", R, v)


def _compose(P, Z):
    return np.concatenate([_qmul(P[..., :4], Z[..., :4]), P[..., 4:] + _rot(P[..., :4], Z[..., 4:])], -1)


def _inverse(P):
    qc = _qconj(P[..., :4])
    return np.concatenate([qc, -_rot(qc, P[..., 4:])], -1)


def _plus(P, d):
    n = np.linalg.norm(d[..., :3], axis=-1, keepdims=True)
    safe = np.where(n == 0.0, 1.0, n)
    qd = np.concatenate([np.where(n == 0.0, d[..., :3], np.sin(n) / safe * d[..., :3]), np.where(n == 0.0, 1.0, np.cos(n))], -1)
    return np.concatenate([_qmul(qd, P[..., :4]), P[..., 4:] + d[..., 3:]], -1)


def residuals(Pi, Pj, Z, S):
    """[E, 6]: r = S e of every edge; Pi, Pj, Z [E, 7], S [E, 6, 6]"""
    E = _compose(_inverse(Z), _compose(_inverse(Pi), Pj))
    sgn = np.where(E[..., 3:4] >= 0.0, 1.0, -1.0)
    e = np.concatenate([2.0 * sgn * E[..., :3], E[..., 4:]], -1)
    return np.einsum("eab,eb->ea", S, e)


def _stacked(edges):
    i = np.array([e[0] for e in edges], int); j = np.array([e[1] for e in edges], int)
    Z = np.array([np.asarray(e[2], float) for e in edges]).reshape(-1, 7)
    S = np.array([weight(e[3]) for e in edges]).reshape(-1, 6, 6)
    a = np.array([e[4] for e in edges], float)
    return i, j, Z, S, a


def _huber(sq, a):
    """(rho, rho') of ceres::HuberLoss(a) per edge"""
    out = (a > 0.0) & (sq > a * a)
    r = np.sqrt(np.where(out, sq, 1.0))
    return np.where(out, 2.0 * a * r - a * a, sq), np.where(out, a / r, 1.0)


def cost(poses, edges):
    x = np.array([pc.normalized(p) for p in poses])
    if not len(edges):
        return 0.0
    i, j, Z, S, a = _stacked(edges)
    r = residuals(x[i], x[j], Z, S)
    return float(0.5 * _huber(np.sum(r * r, -1), a)[0].sum())


def edge_jacobians(Pi, Pj, edge, h=pc.H_STEP):
    Ji = np.empty((6, 6)); Jj = np.empty((6, 6))
    for k in range(6):
        d = np.zeros(6); d[k] = h
        Ji[:, k] = (residual(pc.plus(Pi, d), Pj, edge) - residual(pc.plus(Pi, -d), Pj, edge)) / (2 * h)
        Jj[:, k] = (residual(Pi, pc.plus(Pj, d), edge) - residual(Pi, pc.plus(Pj, -d), edge)) / (2 * h)
    return Ji, Jj


def linearize(poses, edges, fixed=None, h=pc.H_STEP):
    """(cost, g [N, 6], H [6 N, 6 N]) of the robustified problem: residuals and central-difference Jacobians scaled by sqrt(rho'), fixed
    nodes' rows and columns zero; H = J^T J summed edge by edge"""
    x = np.array([pc.normalized(p) for p in poses])
    n = len(x)
    fixed = pc.default_fixed(n) if fixed is None else np.asarray(fixed, bool)
    i, j, Z, S, a = _stacked(edges)
    r = residuals(x[i], x[j], Z, S)
    rho, rho1 = _huber(np.sum(r * r, -1), a)
    w = np.sqrt(rho1)
    Ji = np.empty((len(edges), 6, 6)); Jj = np.empty((len(edges), 6, 6))
    for k in range(6):
        d = np.zeros(6); d[k] = h
        Ji[:, :, k] = (residuals(_plus(x[i], d), x[j], Z, S) - residuals(_plus(x[i], -d), x[j], Z, S)) / (2 * h)
        Jj[:, :, k] = (residuals(x[i], _plus(x[j], d), Z, S) - residuals(x[i], _plus(x[j], -d), Z, S)) / (2 * h)
    Ji *= (w * ~fixed[i])[:, None, None]; Jj *= (w * ~fixed[j])[:, None, None]
    r = r * w[:, None]
    H = np.zeros((6 * n, 6 * n)); g = np.zeros((n, 6))
    for k in range(len(edges)):
        a_, b_ = 6 * i[k], 6 * j[k]
        H[a_:a_ + 6, a_:a_ + 6] += Ji[k].T @ Ji[k]; H[b_:b_ + 6, b_:b_ + 6] += Jj[k].T @ Jj[k]
        H[a_:a_ + 6, b_:b_ + 6] += Ji[k].T @ Jj[k]; H[b_:b_ + 6, a_:a_ + 6] += Jj[k].T @ Ji[k]
        g[i[k]] += Ji[k].T @ r[k]; g[j[k]] += Jj[k].T @ r[k]
    return float(0.5 * rho.sum()), g, H


def gradient(poses, edges, fixed=None):
    return linearize(poses, edges, fixed)[1]


def dense_lm(poses, edges, fixed=None, tol=1e-12, max_iterations=200):
    """posegraphcases.dense_lm on this module's cost and linearisation -> (poses [N, 7], gradient max-norm, iterations)"""
    x = np.array([pc.normalized(p) for p in poses])
    n = len(x)
    fixed = pc.default_fixed(n) if fixed is None else np.asarray(fixed, bool)
    free = np.repeat(~fixed, 6)
    lam = 1e-4
    c, g, H = linearize(x, edges, fixed)
    it = 0
    for it in range(1, max_iterations + 1):
        if np.abs(g).max() < tol:
            break
        Hf = H[np.ix_(free, free)]
        d = np.zeros(6 * n)
        d[free] = np.linalg.solve(Hf + lam * np.diag(np.maximum(np.diag(Hf), 1e-6)), -g.reshape(-1)[free])
        cand = _plus(x, d.reshape(n, 6))
        cc = cost(cand, edges)
        if cc <= c:
            x = cand
            c, g, H = linearize(x, edges, fixed)
            lam = max(lam / 10.0, 1e-12)
            if np.abs(d).max() < 1e-14:
                break
        else:
            lam *= 10.0
            if lam > 1e12:
                break
    return x, float(np.abs(g).max()), it


# ------------------------------------------------------------------------------------------------ graphs with full weights
def with_full_loops(edges, seed, lo=0.5, hi=3.0):
    """the edges with a random NON-symmetric full S on every edge that is no odometry edge (|i - j| > 1, or all of a graph of <= 3 nodes)"""
    rng = np.random.default_rng(seed)
    small = max(max(e[0], e[1]) for e in edges) <= 2
    out = []
    for e in edges:
        if small or abs(e[0] - e[1]) > 1:
            S = rng.uniform(-hi, hi, (6, 6)) + np.diag(rng.uniform(lo, hi, 6))
            out.append((e[0], e[1], e[2], S, e[4]))
        else:
            out.append(e)
    return out


def anisotropic(strong=30.0, ratio=1e-4):
    """a translation information whose principal axes are turned 45 degrees about z against the edge frame: strong across, ratio * strong
    along the turned x axis; rotations at `strong`.  -> (S upper triangular, the weak axis in the edge frame, Lambda)"""
    c = np.sqrt(0.5)
    Q = np.array([[c, -c, 0.0], [c, c, 0.0], [0.0, 0.0, 1.0]])
    L = np.zeros((6, 6))
    L[:3, :3] = strong ** 2 * np.eye(3)
    L[3:, 3:] = Q @ np.diag([(ratio * strong) ** 2, strong ** 2, strong ** 2]) @ Q.T
    return np.linalg.cholesky(L).T, Q[:, 0].copy(), L


def weak_axis_chain(off=0.4):
    """(truth, start, edges_full, edges_diag, edges_free, weak axis): posegraphcases' exact 40-node chain whose loop measurements are pushed
    `off` metres ALONG the weak axis of their information and `off` across it.  edges_full carry anisotropic()'s S on the loops,
    edges_diag its best diagonal approximation sqrt(diag(Lambda)), edges_free no loop edges at all"""
    truth, edges = pc.chain(s_min=5.0, s_max=15.0)
    S, weak, L = anisotropic()
    across = np.array([-weak[1], weak[0], 0.0])
    full, diag, free = [], [], []
    for e in edges:
        if abs(e[0] - e[1]) <= 1:
            full.append(e); diag.append(e); free.append(e)
            continue
        Z = e[2].copy()
        Z[4:] += pc.qmat(Z[:4]) @ (off * weak + 0.25 * off * across)           # E's translation at the truth is R(Z)^T of what is added
        full.append((e[0], e[1], Z, S, 0.0))
        diag.append((e[0], e[1], Z, np.sqrt(np.diag(L)), 0.0))
    return truth, pc.start_of(truth), full, diag, free, weak
