"""An independent numpy restatement of ll_posegraphs' chain preconditioner, and the graphs and systems its tests use.  Nothing here comes
from the library and nothing here is a cyclic reduction: M is put together from the restatement's Jacobians (posegraphcases.linearize,
central differences) edge by edge, systems are solved by numpy.linalg.solve on the dense matrix, and PCG is the textbook recursion.

For a graph at the radius `radius`, A = H + D / radius with H = J^T J and D = clip(diag H, min_diag, max_diag) as the kernel has it.
M keeps of A what the odometry chain explains:
    every edge between nodes n and n + 1, both free, contributes its whole J_e^T J_e (two diagonal blocks and the coupling);
    every other edge contributes the diagonal blocks of its J_e^T J_e alone;  D / radius is added as it is.
So M is a sum of positive semi-definite matrices and a positive diagonal: symmetric positive definite.  It is the block-tridiagonal part
of A in node order, and A - M holds the two off-diagonal blocks of every other edge between free nodes: rank at most 12 each."""
import numpy as np

import posegraphcases as pc

EPS = np.finfo(np.float64).eps


# ------------------------------------------------------------------------------------------------ A and M of a graph
def chain_edge(e, fixed):
    """is edge e one the chain matrix keeps whole: endpoints n, n + 1 and both free"""
    return abs(e[0] - e[1]) == 1 and not fixed[e[0]] and not fixed[e[1]]


def other_edges(edges, fixed):
    """L: the edges between two free nodes that are not chain edges -- what A - M is made of"""
    return sum(1 for e in edges if not fixed[e[0]] and not fixed[e[1]] and abs(e[0] - e[1]) != 1)


def chain_matrix(poses, edges, fixed=None, radius=1e4, min_diag=1e-6, max_diag=1e32):
    """(A, M), dense, over the free nodes' unknowns in node order"""
    n = len(poses)
    fixed = pc.default_fixed(n) if fixed is None else np.asarray(fixed, bool)
    _, _, J, _ = pc.linearize(poses, edges, fixed)
    H = J.T @ J
    D = np.clip(np.diag(H), min_diag, max_diag) / radius
    A = H + np.diag(D)
    M = np.diag(D)
    for k, e in enumerate(edges):
        Je = J[6 * k:6 * k + 6]
        He = Je.T @ Je                                              # zero outside the blocks of e's two nodes
        if chain_edge(e, fixed):
            M += He
        else:
            for a in (e[0], e[1]):
                M[6 * a:6 * a + 6, 6 * a:6 * a + 6] += He[6 * a:6 * a + 6, 6 * a:6 * a + 6]
    free = np.repeat(~fixed, 6)
    ix = np.ix_(free, free)
    return A[ix], M[ix]


def tridiagonal_part(A, fixed):
    """the blocks (a, b), |a - b| <= 1 in NODE order, of a matrix over the free nodes"""
    nodes = np.flatnonzero(~np.asarray(fixed, bool))
    T = np.zeros_like(A)
    for p, a in enumerate(nodes):
        for q in (p - 1, p, p + 1):
            if 0 <= q < len(nodes) and abs(int(nodes[q]) - int(a)) <= 1:
                T[6 * p:6 * p + 6, 6 * q:6 * q + 6] = A[6 * p:6 * p + 6, 6 * q:6 * q + 6]
    return T


def right_hand_side(poses, edges, fixed=None):
    n = len(poses)
    fixed = pc.default_fixed(n) if fixed is None else np.asarray(fixed, bool)
    return -pc.gradient(poses, edges, fixed).reshape(-1)[np.repeat(~fixed, 6)]


def dense_solve(M, b):
    return np.linalg.solve(M, b)


def pcg_count(A, M, b, eta, max_iterations=5000):
    """iterations of preconditioned conjugate gradients on A x = b from x = 0 until |r| <= eta |b|"""
    Mi = np.linalg.inv(M)
    x = np.zeros_like(b); r = b.copy(); z = Mi @ r; p = z.copy(); rz = r @ z
    stop = eta * np.linalg.norm(b)
    for k in range(1, max_iterations + 1):
        Ap = A @ p
        alpha = rz / (p @ Ap)
        x += alpha * p; r -= alpha * Ap
        if np.linalg.norm(r) <= stop:
            return k
        z = Mi @ r
        rz2 = r @ z
        p = z + (rz2 / rz) * p
        rz = rz2
    return max_iterations


# ------------------------------------------------------------------------------------------------ block-tridiagonal systems
def dense_of(diag, upper):
    """the dense matrix of diagonal blocks diag [N, 6, 6] and couplings upper[n] = M[n][n+1] (the last one is ignored)"""
    n = len(diag)
    M = np.zeros((6 * n, 6 * n))
    for k in range(n):
        M[6 * k:6 * k + 6, 6 * k:6 * k + 6] = diag[k]
        if k + 1 < n:
            M[6 * k:6 * k + 6, 6 * k + 6:6 * k + 12] = upper[k]
            M[6 * k + 6:6 * k + 12, 6 * k:6 * k + 6] = upper[k].T
    return M


def _thomas(diag, upper, b):
    """block forward elimination and back substitution, for the condition number of the large systems only"""
    n = len(diag)
    Dk = [None] * n; y = [None] * n
    Dk[0] = diag[0]; y[0] = b[0]
    for k in range(1, n):
        W = np.linalg.solve(Dk[k - 1], upper[k - 1]).T              # M[k][k-1] D_{k-1}^-1
        Dk[k] = diag[k] - W @ upper[k - 1]
        y[k] = b[k] - W @ y[k - 1]
    x = np.zeros((n, 6))
    x[n - 1] = np.linalg.solve(Dk[n - 1], y[n - 1])
    for k in range(n - 2, -1, -1):
        x[k] = np.linalg.solve(Dk[k], y[k] - upper[k] @ x[k + 1])
    return x


def _apply(diag, upper, v):
    out = np.einsum("nab,nb->na", diag, v)
    if len(diag) > 1:
        out[:-1] += np.einsum("nab,nb->na", upper[:-1], v[1:])
        out[1:] += np.einsum("nba,nb->na", upper[:-1], v[:-1])
    return out


def condition_number(diag, upper, dense_limit=3100):
    """lambda_max / lambda_min of the system.  Up to dense_limit unknowns: numpy.linalg.eigvalsh of the dense matrix.  Above: Rayleigh
    quotients after 60 power iterations (a lower bound of lambda_max) and 60 inverse iterations (an upper bound of lambda_min), so the
    figure never exceeds the condition number and a bound that is proportional to it only gets tighter."""
    n = len(diag)
    if 6 * n <= dense_limit:
        w = np.linalg.eigvalsh(dense_of(diag, upper))
        return float(w[-1] / w[0])
    rng = np.random.default_rng(99)
    v = rng.normal(size=(n, 6)); u = v.copy()
    for _ in range(60):
        v = _apply(diag, upper, v); v /= np.linalg.norm(v)
        u = _thomas(diag, upper, u); u /= np.linalg.norm(u)
    return float(np.vdot(v, _apply(diag, upper, v)) / np.vdot(u, _apply(diag, upper, u)))


def random_system(n, seed, delta=1e-3, scale=1.0):
    """(diag [n, 6, 6], upper [n, 6, 6], cond): M = sum_k G_k^T G_k + delta I with G_k a random 6 x 12 block on the nodes k, k + 1 --
    the shape of an odometry edge's J^T J.  upper[n - 1] is zeros"""
    rng = np.random.default_rng(seed)
    diag = np.tile(delta * np.eye(6), (n, 1, 1)); upper = np.zeros((n, 6, 6))
    for k in range(n - 1):
        G = scale * rng.normal(size=(6, 12))
        GG = G.T @ G
        diag[k] += GG[:6, :6]; diag[k + 1] += GG[6:, 6:]; upper[k] = GG[:6, 6:]
    return diag, upper, condition_number(diag, upper)


# ------------------------------------------------------------------------------------------------ the graphs
LAP_NODES = 65                                                      # the laps that are solved against the dense LM


def circle_lap(n=257, loops=1, yaw_bias=2e-4, radius=30.0):
    """posegraphcases.lap on a circle driven once: one loop edge last -> first; loops == 2 adds one from three quarters of the lap back
    to one quarter, from the truth.  The fixed node is the one half way round, so that every loop edge joins two free nodes and
    counts towards the rank of A - M (an edge at a fixed node has no off-diagonal block)"""
    th = 2.0 * np.pi * np.arange(n) / n
    truth, start, edges = pc.lap([(radius * np.sin(t), radius * (1.0 - np.cos(t)), t) for t in th], yaw_bias)
    if loops == 2:
        a, b = (3 * n) // 4, n // 4
        edges.append(pc.edge(a, b, pc.relative(truth[a], truth[b]), (20.0,) * 3 + (5.0,) * 3))
    fixed = np.zeros(n, np.uint8); fixed[n // 2] = 1
    return start, edges, fixed


def _plain_chain(n=40):
    truth, edges = pc.chain(n=n, sig_rot=0.005, sig_t=0.01, loops=(), s_min=5.0, s_max=15.0)
    return truth, pc.start_of(truth), edges


def loop_free_chain():
    _, start, edges = _plain_chain()
    return start, edges


def reversed_chain():
    """the loop-free chain with every third edge stated from n + 1 to n"""
    _, start, edges = _plain_chain()
    return start, [pc.edge(e[1], e[0], pc.inverse(e[2]), e[3], e[4]) if k % 3 == 1 else e for k, e in enumerate(edges)]


def doubled_chain():
    """noisy_chain("cm") with every odometry edge a second time, the copy with noise and weights of its own, stated backwards for odd n"""
    truth, start, edges = pc.noisy_chain("cm")
    rng = np.random.default_rng(21)
    out = []
    for e in edges:
        out.append(e)
        if abs(e[0] - e[1]) == 1:
            Z = pc.noisy(pc.relative(truth[e[0]], truth[e[1]]), rng, 0.005, 0.01)
            w = rng.uniform(5.0, 15.0, 6)
            out.append(pc.edge(e[1], e[0], pc.inverse(Z), w) if e[0] % 2 else pc.edge(e[0], e[1], Z, w))
    return start, out


FIXED_NODES = (0, 17, 39)


def fixed_chain():
    """noisy_chain("cm") with fixed nodes at 0, in the middle and at the end"""
    _, start, edges = pc.noisy_chain("cm")
    fixed = np.zeros(len(start), np.uint8); fixed[list(FIXED_NODES)] = 1
    return start, edges, fixed


def star_graph():
    truth, edges = pc.star()
    start = pc.perturbed(truth, np.random.default_rng(11), 0.05, np.deg2rad(1.0))
    start[0] = truth[0]
    return start, edges


def graphs():
    """name -> (start poses, edges, fixed flags).  Built anew at every call; the tests share them through a cache of their own"""
    out = {}
    for level in ("tiny", "cm"):
        _, start, edges = pc.noisy_chain(level)
        out["chain_" + level] = (start, edges)
    _, start, edges = pc.huber_chain()
    out["chain_huber"] = (start, edges)
    out["lap_1"] = circle_lap(LAP_NODES, loops=1, yaw_bias=1e-3)
    out["lap_2"] = circle_lap(LAP_NODES, loops=2, yaw_bias=1e-3)
    out["loop_free"] = loop_free_chain()
    out["reversed"] = reversed_chain()
    out["doubled"] = doubled_chain()
    out["fixed"] = fixed_chain()
    out["star"] = star_graph()
    out["lap257_1"] = circle_lap(257, loops=1)
    out["lap257_2"] = circle_lap(257, loops=2)
    return {k: (g[0], g[1], (np.asarray(g[2], np.uint8) if len(g) > 2 else pc.default_fixed(len(g[0])).astype(np.uint8))) for k, g in out.items()}


GRAPH_NAMES = ("chain_tiny", "chain_cm", "chain_huber", "lap_1", "lap_2", "loop_free", "reversed", "doubled", "fixed", "star")   # solved against the dense LM
COUNT_NAMES = ("lap257_1", "lap257_2")                              # 257 nodes: the iteration counts (the dense LM would take ten seconds there)
LOOPS = {"lap257_1": 1, "lap257_2": 2}


def cost_floor(poses, edges):
    """what rounding alone leaves of a cost that is zero in exact arithmetic: a residual entry is a weight times a difference of
    coordinates of size `extent`, each a few roundings (taken as 64) off, so |r| errs by about 64 eps w extent and the cost,
    1/2 sum of 6 E squares, by at most 3 E times its square.  Below this a relative comparison of two costs compares noise"""
    extent = max(1.0, float(np.abs(np.asarray(poses)[:, 4:]).max()))
    w = max(float(np.abs(np.asarray(e[3])).max()) for e in edges)
    return 3.0 * len(edges) * (64.0 * EPS * w * extent) ** 2
