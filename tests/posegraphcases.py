"""An independent numpy float64 restatement of the pose-graph problem ll_posegraphs solves, and the graphs the tests use.  Nothing here
comes from the library: its own quaternion algebra (x, y, z, w), the residual, its own `plus`, Ceres' Huber cost, a Jacobian by central
differences of the residual through `plus` (h = 1e-6) -- a different route than the kernel's closed forms --, and a dense
Levenberg-Marquardt over the 6 N unknowns with numpy.linalg.solve.

A pose is (qx, qy, qz, qw, tx, ty, tz), world from body.  An edge is the tuple (i, j, Z[7], s[6], a): Z measures P_i^-1 P_j, s is the
diagonal square-root information (rotation rows first), a the Huber width (a <= 0: no loss).
    E = Z^-1 P_i^-1 P_j,   r = s o [2 sgn(w_e) vec(q_e) ; t_e],   cost = 1/2 sum_e rho_a(|r_e|^2)."""
import numpy as np

H_STEP = 1e-6


# ------------------------------------------------------------------------------------------------ quaternions and poses
def qmul(a, b):
    ax, ay, az, aw = a; bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw,
                     aw * bw - ax * bx - ay * by - az * bz])


def qconj(q):
    return np.array([-q[0], -q[1], -q[2], q[3]])


def qmat(q):
    x, y, z, w = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def qexp(d):
    """[sin|d| d / |d|, cos|d|]: d is the HALF-angle vector"""
    n = np.linalg.norm(d)
    if n == 0.0:
        return np.array([d[0], d[1], d[2], 1.0])
    return np.concatenate([np.sin(n) / n * np.asarray(d, float), [np.cos(n)]])


def axis_angle(axis, angle):
    axis = np.asarray(axis, float)
    return qexp(0.5 * angle * axis / np.linalg.norm(axis))


def normalized(pose):
    p = np.array(pose, float)
    p[:4] /= np.linalg.norm(p[:4])
    return p


def plus(pose, d):
    """q <- exp(d[:3]) (x) q, t <- t + d[3:]"""
    out = np.empty(7)
    out[:4] = qmul(qexp(d[:3]), pose[:4])
    out[4:] = pose[4:] + d[3:]
    return out


def compose(P, Z):
    """P Z"""
    return np.concatenate([qmul(P[:4], Z[:4]), P[4:] + qmat(P[:4]) @ Z[4:]])


def inverse(P):
    return np.concatenate([qconj(P[:4]), -(qmat(P[:4]).T @ P[4:])])


def relative(Pi, Pj):
    """P_i^-1 P_j"""
    return compose(inverse(Pi), Pj)


# ------------------------------------------------------------------------------------------------ residual, cost, gradient
def residual(Pi, Pj, edge):
    _, _, Z, s, _ = edge
    E = compose(inverse(np.asarray(Z, float)), relative(Pi, Pj))
    sgn = 1.0 if E[3] >= 0.0 else -1.0
    return np.asarray(s, float) * np.concatenate([2.0 * sgn * E[:3], E[4:]])


def huber(sq, a):
    """(rho, rho') of ceres::HuberLoss(a) at the squared norm sq"""
    if a <= 0.0 or sq <= a * a:
        return sq, 1.0
    r = np.sqrt(sq)
    return 2.0 * a * r - a * a, a / r


def cost(poses, edges):
    poses = [normalized(p) for p in poses]
    c = 0.0
    for e in edges:
        r = residual(poses[e[0]], poses[e[1]], e)
        c += 0.5 * huber(float(r @ r), e[4])[0]
    return c


def edge_jacobians(Pi, Pj, edge, h=H_STEP):
    """(J_i, J_j), 6 x 6 each: central differences of the residual through plus"""
    Ji = np.empty((6, 6)); Jj = np.empty((6, 6))
    for k in range(6):
        d = np.zeros(6); d[k] = h
        Ji[:, k] = (residual(plus(Pi, d), Pj, edge) - residual(plus(Pi, -d), Pj, edge)) / (2 * h)
        Jj[:, k] = (residual(Pi, plus(Pj, d), edge) - residual(Pi, plus(Pj, -d), edge)) / (2 * h)
    return Ji, Jj


def default_fixed(n):
    f = np.zeros(n, bool); f[0] = True
    return f


def linearize(poses, edges, fixed=None):
    """(cost, g [N, 6], J [6 E, 6 N], r [6 E]) with residual and Jacobian scaled by sqrt(rho'); fixed nodes' columns are zero"""
    poses = [normalized(p) for p in poses]
    n = len(poses)
    fixed = default_fixed(n) if fixed is None else np.asarray(fixed, bool)
    J = np.zeros((6 * len(edges), 6 * n)); rr = np.zeros(6 * len(edges)); c = 0.0
    for k, e in enumerate(edges):
        i, j = e[0], e[1]
        r = residual(poses[i], poses[j], e)
        rho, rho1 = huber(float(r @ r), e[4])
        c += 0.5 * rho
        Ji, Jj = edge_jacobians(poses[i], poses[j], e)
        w = np.sqrt(rho1)
        rr[6 * k:6 * k + 6] = w * r
        if not fixed[i]:
            J[6 * k:6 * k + 6, 6 * i:6 * i + 6] = w * Ji
        if not fixed[j]:
            J[6 * k:6 * k + 6, 6 * j:6 * j + 6] = w * Jj
    return c, (J.T @ rr).reshape(n, 6), J, rr


def gradient(poses, edges, fixed=None):
    return linearize(poses, edges, fixed)[1]


def dense_lm(poses, edges, fixed=None, tol=1e-12, max_iterations=200):
    """Levenberg-Marquardt on the dense normal equations until the max-norm of the gradient is below tol.
    -> (poses [N, 7], gradient max-norm, iterations); the caller asserts on the norm"""
    x = np.array([normalized(p) for p in poses])
    n = len(x)
    fixed = default_fixed(n) if fixed is None else np.asarray(fixed, bool)
    free = np.repeat(~fixed, 6)
    lam = 1e-4
    c, g, J, rr = linearize(x, edges, fixed)
    it = 0
    for it in range(1, max_iterations + 1):
        if np.abs(g).max() < tol:
            break
        Hf = (J.T @ J)[np.ix_(free, free)]
        d = np.zeros(6 * n)
        d[free] = np.linalg.solve(Hf + lam * np.diag(np.maximum(np.diag(Hf), 1e-6)), -g.reshape(-1)[free])
        cand = np.array([plus(x[k], d[6 * k:6 * k + 6]) for k in range(n)])
        cc = cost(cand, edges)
        if cc <= c:
            x = cand
            c, g, J, rr = linearize(x, edges, fixed)
            lam = max(lam / 10.0, 1e-12)
            if np.abs(d).max() < 1e-14:                            # steps below the rounding of the poses: nothing more to gain
                break
        else:
            lam *= 10.0
            if lam > 1e12:
                break
    return x, float(np.abs(g).max()), it


# ------------------------------------------------------------------------------------------------ graphs (fixed seeds)
def random_pose(rng, spread=5.0, max_angle=np.pi):
    return np.concatenate([axis_angle(rng.normal(size=3), rng.uniform(-max_angle, max_angle)), rng.uniform(-spread, spread, 3)])


def perturbed(poses, rng, dt, drot):
    """every pose moved by up to dt metres per axis and turned by drot radians about a random axis (plus's convention)"""
    out = []
    for p in poses:
        ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
        out.append(plus(np.asarray(p, float), np.concatenate([0.5 * drot * ax, rng.uniform(-dt, dt, 3)])))
    return np.array(out)


def noisy(Z, rng, sig_rot, sig_t):
    return plus(Z, np.concatenate([0.5 * rng.normal(0.0, sig_rot, 3), np.zeros(3)])) + np.concatenate([np.zeros(4), rng.normal(0.0, sig_t, 3)])


def edge(i, j, Z, s=(1.0,) * 6, a=0.0):
    return (int(i), int(j), np.array(Z, float), np.array(s, float), float(a))


def two_node(seed=1):
    """(start poses, edges, Z): node 0 fixed; the solution is P_1 = P_0 Z"""
    rng = np.random.default_rng(seed)
    P0 = random_pose(rng); Z = random_pose(rng, 2.0, 1.0)
    start = np.array([P0, perturbed([compose(P0, Z)], rng, 0.3, np.deg2rad(5.0))[0]])
    return start, [edge(0, 1, Z, (3.0, 2.0, 4.0, 1.5, 1.0, 2.5))], Z


def triangle(seed=2):
    """three nodes, three edges whose measurements do not compose to the identity"""
    rng = np.random.default_rng(seed)
    truth = np.array([random_pose(rng, 3.0) for _ in range(3)])
    edges = [edge(a, b, noisy(relative(truth[a], truth[b]), rng, 0.05, 0.2), rng.uniform(0.5, 20.0, 6)) for a, b in ((0, 1), (1, 2), (2, 0))]
    return perturbed(truth, rng, 0.3, np.deg2rad(5.0)), edges


def helix(n, radius=2.0, rise=0.02):
    """n poses along a rising circle, heading along the tangent with a slow roll: a full turn, so that the last poses see the first"""
    out = []
    for k in range(n):
        th = 2.0 * np.pi * k / n
        q = qmul(axis_angle([0, 0, 1], th + 0.5 * np.pi), axis_angle([1, 0, 0], 0.2 * np.sin(3 * th)))
        out.append(np.concatenate([q, [radius * np.cos(th), radius * np.sin(th), rise * k]]))
    return np.array(out)


CHAIN_LOOPS = ((39, 0), (30, 5), (12, 27))


def chain(n=40, seed=3, sig_rot=0.0, sig_t=0.0, loops=CHAIN_LOOPS, s_min=1.0, s_max=3.0, huber_loops=0.0):
    """(truth, edges): n - 1 odometry edges and the loop edges of a helix; noise 0 gives a consistent graph"""
    rng = np.random.default_rng(seed)
    truth = helix(n)
    edges = []
    for a, b in [(k, k + 1) for k in range(n - 1)] + [l for l in loops if max(l) < n]:
        Z = relative(truth[a], truth[b])
        if sig_rot or sig_t:
            Z = noisy(Z, rng, sig_rot, sig_t)
        edges.append(edge(a, b, Z, rng.uniform(s_min, s_max, 6), huber_loops if abs(a - b) > 1 else 0.0))
    return truth, edges


def star(seed=4, degree=100):
    """node 0 joined to `degree` others, by edges in both directions, weights up to 100"""
    rng = np.random.default_rng(seed)
    truth = np.array([random_pose(rng, 6.0) for _ in range(degree + 1)])
    edges = []
    for k in range(1, degree + 1):
        a, b = (0, k) if k % 2 else (k, 0)
        edges.append(edge(a, b, noisy(relative(truth[a], truth[b]), rng, 0.02, 0.1), rng.uniform(0.5, 100.0, 6), 1.0 if k % 5 == 0 else 0.0))
    return truth, edges


def false_loop(truth, a=20, b=2, off=5.0, width=0.5, s=1.0):
    """a loop edge whose measurement is `off` metres away from the truth, with Huber width `width`"""
    Z = relative(truth[a], truth[b])
    Z[4] += off
    return edge(a, b, Z, (s,) * 6, width)


def ring_graph(n, seed):
    """(start, edges) of any size >= 2: a noisy closed chain, for the batch test (no reference solve needed)"""
    rng = np.random.default_rng(seed)
    truth = helix(n, radius=0.2 * n + 2.0, rise=0.01)
    pairs = [(k, k + 1) for k in range(n - 1)] + ([(n - 1, 0)] if n > 2 else [])
    edges = [edge(a, b, noisy(relative(truth[a], truth[b]), rng, 0.002, 0.01), rng.uniform(1.0, 5.0, 6), 0.0 if abs(a - b) == 1 else 1.0)
             for a, b in pairs]
    return perturbed(truth, rng, 0.05, np.deg2rad(1.0)), edges


def ate(poses, truth):
    """translational RMSE without alignment (node 0 is fixed at the truth in the tests that use it)"""
    return float(np.sqrt(np.mean(np.sum((np.asarray(poses)[:, 4:] - np.asarray(truth)[:, 4:]) ** 2, axis=1))))


# ------------------------------------------------------------------------------------------------ the solves the tests share
TIGHT = dict(function_tolerance=0.0, gradient_tolerance=1e-12, parameter_tolerance=0.0)
NOISE = {"tiny": (1e-5, 1e-5), "cm": (0.005, 0.01)}                 # (rad, m) on every measurement


def start_of(truth, seed=7):
    """the truth perturbed by 0.3 m and 5 degrees, node 0 (fixed) left where it is"""
    start = perturbed(truth, np.random.default_rng(seed), 0.3, np.deg2rad(5.0))
    start[0] = truth[0]
    return start


def consistent_chain():
    """(truth, start, edges): exact measurements"""
    truth, edges = chain()
    return truth, start_of(truth), edges


def noisy_chain(level):
    """(truth, start, edges): the 40-node chain with 3 loops, Gaussian noise NOISE[level] on Z, odometry stiff against the false loop
    of huber_chain (weights 5 .. 15)"""
    truth, edges = chain(sig_rot=NOISE[level][0], sig_t=NOISE[level][1], s_min=5.0, s_max=15.0)
    return truth, start_of(truth), edges


def huber_chain(width=0.5):
    """noisy_chain("cm") with one false loop edge, 5 m off; width 0 turns the loss off"""
    truth, start, edges = noisy_chain("cm")
    return truth, start, edges + [false_loop(truth, width=width)]


def lap(poses_xyyaw, yaw_bias):
    """(truth [N, 7], start [N, 7], edges) of a planar lap: odometry edges from the truth with a constant yaw bias per step, one loop
    edge (last -> first) from the truth; the start is the biased odometry chained up from node 0"""
    truth = np.array([np.concatenate([axis_angle([0, 0, 1], yaw), [x, y, 0.0]]) for x, y, yaw in poses_xyyaw])
    bias = np.concatenate([axis_angle([0, 0, 1], yaw_bias), np.zeros(3)])
    n = len(truth)
    edges = [edge(k, k + 1, compose(relative(truth[k], truth[k + 1]), bias), (20.0,) * 3 + (5.0,) * 3) for k in range(n - 1)]
    start = [truth[0]]
    for e in edges:
        start.append(compose(start[-1], e[2]))
    edges.append(edge(n - 1, 0, relative(truth[n - 1], truth[0]), (20.0,) * 3 + (5.0,) * 3))
    return truth, np.array(start), edges
