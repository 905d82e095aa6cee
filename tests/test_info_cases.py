"""tests/infocases.py against itself, and the library's host function ll_pg_edge_from_info against it; no GPU.

The geometry first: for Z = P_i^-1 X the edge error at X' = plus(X, d) is e = M d to first order, and e(0) = 0, so the Hessian of
d -> 1/2 |S e(plus(X, d))|^2 at d = 0 is exactly J^T J with J the Jacobian of S e there.  With S from edge_from_info(H, X, sigma) it
must be H / sigma^2: that pins the factor 2 of the rotation rows, the transpose of R(X) and the sign convention of q_e.

Tolerance of that comparison.  J comes from central differences with h = 1e-5: the truncation is h^2 / 6 times a third derivative of
order |J| (2 sin h for the rotation rows, none for the translation rows), 2e-11 |J|; the rounding is ulp(1) / 2h = 1.1e-11 per entry of e
for coordinates below 2 (the poses here keep |t| <= 1).  An entry of J^T J sums six products, so its error stays below
2 * 6 * 3e-11 |J|^2 < 1e-9 max|Lambda|: the 1e-9 tests/test_posegraph_cases.py asks of its central-difference Jacobians, here relative
to max|Lambda| because Lambda is not of order one."""
import ctypes as C

import numpy as np
import pytest

import infocases as ic
import posegraphcases as pc

H_FD = 1e-5


def fd_hessian(Pi, X, Z, S):
    """J^T J of d -> S e(P_i, plus(X, d)) at d = 0, J by central differences"""
    e = (0, 1, Z, S, 0.0)
    J = np.empty((6, 6))
    for k in range(6):
        d = np.zeros(6); d[k] = H_FD
        J[:, k] = (ic.residual(Pi, pc.plus(X, d), e) - ic.residual(Pi, pc.plus(X, -d), e)) / (2 * H_FD)
    assert np.abs(ic.residual(Pi, X, e)).max() < 1e-14             # e(0) = 0: the Gauss-Newton Hessian is the Hessian
    return J.T @ J


def poses_for(seed, max_angle=np.pi):
    rng = np.random.default_rng(seed)
    Pi = pc.random_pose(rng, 1.0)
    X = pc.random_pose(rng, 1.0, max_angle)
    return rng, Pi, X


@pytest.mark.parametrize("seed", range(8))
def test_the_edge_information_is_h_over_sigma2_in_the_increment_of_x(seed):
    rng, Pi, X = poses_for(seed)
    H = ic.spd(rng); sigma = float(rng.uniform(0.05, 2.0))
    Z = pc.relative(Pi, X)
    S = ic.edge_from_info(H, X, sigma)
    got = fd_hessian(Pi, X, Z, S)
    want = H / sigma ** 2
    err = np.abs(got - want).max() / np.abs(ic.information(H, X, sigma)).max()
    print(f"seed {seed}: |J^T J - H / sigma^2| / max|Lambda| = {err:.3g}")
    assert err <= 1e-9


def test_the_sign_convention_holds_when_q_e_comes_out_with_negative_w():
    """X and -X are one pose; with Z from X and the graph holding -X, q_e = (0, 0, 0, -1) and sgn(w_e) = -1 enters e"""
    rng, Pi, X = poses_for(100)
    H = ic.spd(rng)
    Z = pc.relative(Pi, X)
    Xn = X * np.array([-1, -1, -1, -1, 1, 1, 1.0])
    E = pc.compose(pc.inverse(Z), pc.relative(Pi, Xn))
    assert E[3] < 0.0
    S = ic.edge_from_info(H, Xn, 0.5)
    assert np.array_equal(S, ic.edge_from_info(H, X, 0.5))          # R(-q) = R(q)
    got = fd_hessian(Pi, Xn, Z, S)
    err = np.abs(got - H / 0.25).max() / np.abs(ic.information(H, X, 0.5)).max()
    print(f"negative w: {err:.3g}")
    assert err <= 1e-9


def test_a_diagonal_weight_is_the_diagonal_matrix():
    rng, Pi, X = poses_for(5)
    Pj = pc.random_pose(rng, 1.0)
    s = rng.uniform(0.5, 3.0, 6)
    e = (0, 1, pc.random_pose(rng, 1.0), s, 0.0)
    assert np.array_equal(ic.residual(Pi, Pj, e), ic.residual(Pi, Pj, (0, 1, e[2], np.diag(s), 0.0)))
    assert np.allclose(ic.residual(Pi, Pj, e), pc.residual(Pi, Pj, e), rtol=0, atol=1e-15)
    truth, start, edges = pc.noisy_chain("cm")
    assert ic.cost(start, edges) == pytest.approx(pc.cost(start, edges), rel=1e-14)


def test_the_stacked_restatement_is_the_per_edge_one():
    """residuals / linearize work on all edges at once; they must be posegraphcases' numbers, and residual()'s for full weights"""
    _, start, edges = pc.huber_chain()
    full = ic.with_full_loops(edges, 24, 0.5, 1.5)
    assert any(np.ndim(e[3]) == 2 for e in full) and any(np.ndim(e[3]) == 1 for e in full)
    x = np.array([pc.normalized(p) for p in start])
    i, j, Z, S, a = ic._stacked(full)
    r = ic.residuals(x[i], x[j], Z, S)
    for k, e in enumerate(full):
        assert np.allclose(r[k], ic.residual(x[e[0]], x[e[1]], e), rtol=0, atol=1e-13)
    c, g, H = ic.linearize(start, edges)
    c_pc, g_pc, J_pc, _ = pc.linearize(start, edges)
    assert c == pytest.approx(c_pc, rel=1e-14)
    assert np.abs(g - g_pc).max() <= 1e-8 * np.abs(g_pc).max()      # two central differences of the same function
    assert np.abs(H - J_pc.T @ J_pc).max() <= 1e-8 * np.abs(H).max()
    assert not H[:6].any() and not H[:, :6].any() and not g[0].any()    # node 0 is fixed
    d = np.random.default_rng(1).normal(0.0, 0.1, (len(x), 6)); d[3, :3] = 0.0
    assert np.allclose(ic._plus(x, d), [pc.plus(x[k], d[k]) for k in range(len(x))], rtol=0, atol=1e-15)


def test_the_dense_lm_lands_on_z_whatever_s():
    start, edges, Z = pc.two_node()
    S = np.random.default_rng(3).uniform(-2.0, 2.0, (6, 6)) + 3.0 * np.eye(6)
    x, gmax, it = ic.dense_lm(start, [(0, 1, edges[0][2], S, 0.0)])
    assert gmax < 1e-12
    assert np.allclose(x[1], pc.compose(pc.normalized(start[0]), Z), rtol=0, atol=1e-12)


# ------------------------------------------------------------------------------------------------ the library's host function
def record(api, H, sigma2=0.0, flags=0, rows=100):
    r = api.PoseInfo()
    for k, v in enumerate(np.asarray(H, float).reshape(36)):
        r.H[k] = v
    r.sigma2 = sigma2; r.flags = flags; r.rows = rows
    return r


def raw(api, info, X, sigma, floor, out=True):
    S = np.full((6, 6), 7.0)
    x = None if X is None else np.ascontiguousarray(X, np.float64)
    rc = api.load_library().ll_pg_edge_from_info(None if info is None else C.addressof(info), None if x is None else x.ctypes.data,
                                                 float(sigma), float(floor), S.ctypes.data if out else None)
    return rc, S


@pytest.mark.parametrize("seed", range(6))
def test_the_library_agrees_with_the_restatement(api, seed):
    rng, _, X = poses_for(200 + seed)
    X[:4] *= 1.0 + 0.5 * seed                                       # the quaternion is normalised inside
    H = ic.spd(rng, 1e-2, 1e6); sigma = float(rng.uniform(0.01, 3.0)); floor = float(seed % 2) * 1e-3
    S = api.edge_from_info(record(api, H), X, sigma, floor)
    L = ic.information(H, X, sigma, floor)
    err = np.abs(S.T @ S - L).max() / np.abs(L).max()
    print(f"seed {seed}: |S^T S - Lambda| / max|Lambda| = {err:.3g}")
    assert err <= 1e-12
    assert np.array_equal(S, np.triu(S)) and (np.diag(S) > 0.0).all()
    assert np.abs(S - ic.edge_from_info(H, X, sigma, floor)).max() <= 1e-9 * np.abs(S).max()


def test_sigma_at_or_below_zero_uses_sigma2(api):
    rng, _, X = poses_for(300)
    H = ic.spd(rng)
    for sigma in (0.0, -1.0):
        S = api.edge_from_info(record(api, H, sigma2=0.25), X, sigma)
        assert np.array_equal(S, api.edge_from_info(record(api, H), X, 0.5))      # 0.5 * 0.5 is exact
    rc, S = raw(api, record(api, H, sigma2=0.0), X, 0.0, 0.0)
    assert rc == -7 and (S == 7.0).all()                            # LL_ERR_STATE, the output untouched


def test_floor_rescues_a_rank_five_hessian(api):
    H = np.diag([4.0, 9.0, 1.0, 25.0, 16.0, 0.0])                   # nothing known along z
    X = np.array([0, 0, 0, 1.0, 1.0, 2.0, 3.0])
    rc, _ = raw(api, record(api, H), X, 1.0, 0.0)
    assert rc == -7
    S = api.edge_from_info(record(api, H), X, 1.0, floor=1e-6)
    assert np.allclose(S.T @ S, ic.information(H, X, 1.0, 1e-6), rtol=0, atol=1e-12 * 25.0)
    assert S[5, 5] == pytest.approx(1e-3, rel=1e-12)
    rng = np.random.default_rng(9)                                  # and a turned one: rank 5 in no axis of the edge frame
    Q, _ = np.linalg.qr(rng.normal(size=(6, 6)))
    H5 = Q @ np.diag([0.0, 1.0, 2.0, 3.0, 4.0, 5.0]) @ Q.T
    Xr = pc.random_pose(rng, 1.0)
    S = api.edge_from_info(record(api, H5), Xr, 1.0, floor=1e-4)
    L = ic.information(H5, Xr, 1.0, 1e-4)
    assert np.abs(S.T @ S - L).max() <= 1e-12 * np.abs(L).max()


def test_every_error_of_the_host_function(api):
    rng, _, X = poses_for(400)
    H = ic.spd(rng)
    ok = record(api, H, sigma2=1.0)
    assert raw(api, ok, X, 1.0, 0.0)[0] == 0
    assert raw(api, None, X, 1.0, 0.0)[0] == -2                     # NULL pointers
    assert raw(api, ok, None, 1.0, 0.0)[0] == -2
    assert raw(api, ok, X, 1.0, 0.0, out=False)[0] == -2
    for bad in (np.nan, np.inf):                                    # non-finite arguments
        assert raw(api, ok, X, bad, 0.0)[0] == -2
        assert raw(api, ok, X, 1.0, bad)[0] == -2
        Xb = X.copy(); Xb[5] = bad
        assert raw(api, ok, Xb, 1.0, 0.0)[0] == -2
    assert raw(api, ok, X, 1.0, -1e-3)[0] == -2                     # floor >= 0
    Xz = X.copy(); Xz[:4] = 0.0
    assert raw(api, ok, Xz, 1.0, 0.0)[0] == -2                      # zero quaternion
    assert raw(api, record(api, H, sigma2=1.0, flags=1), X, 1.0, 0.0)[0] == -7     # H was not finite
    assert raw(api, record(api, H, flags=2), X, 1.0, 0.0)[0] == 0                  # few rows alone do not stop it
    assert raw(api, record(api, -H), X, 1.0, 0.0)[0] == -7          # not positive definite
    Hn = H.copy(); Hn[2, 3] = Hn[3, 2] = np.nan
    rc, S = raw(api, record(api, Hn), X, 1.0, 0.0)
    assert rc == -7 and (S == 7.0).all()
    with pytest.raises(api.LightLoamError) as ei:
        api.edge_from_info(record(api, -H), X, 1.0)
    assert ei.value.code == -7
    with pytest.raises(api.LightLoamError) as ei:
        api.edge_from_info(ok, Xz, 1.0)
    assert ei.value.code == -2


def test_edges_are_promoted_only_when_one_is_full(api):
    rng, Pi, X = poses_for(500)
    S = rng.normal(size=(6, 6))
    d = api.pg_edges([(0, 1, Pi, 2.0, 0.5), (1, 0, X, np.arange(6.0))])
    assert d.dtype == api.PG_EDGE
    f = api.pg_edges([(0, 1, Pi, 2.0, 0.5), (1, 0, X, S)])
    assert f.dtype == api.PG_EDGE6 and np.array_equal(f["S"][0], 2.0 * np.eye(6)) and np.array_equal(f["S"][1], S)
    assert f["huber"].tolist() == [0.5, 0.0] and np.array_equal(f["Z_w7"][1], X)
    p = api.pg_edges6(d)
    assert p.dtype == api.PG_EDGE6 and np.array_equal(p["S"][1], np.diag(np.arange(6.0)))
    poses = np.stack([Pi, X])
    assert api.PoseGraphs._pack([(poses, d)])[4].dtype == api.PG_EDGE
    no, eo, _, _, e = api.PoseGraphs._pack([(poses, d), (poses, f[1:])])
    assert e.dtype == api.PG_EDGE6 and eo.tolist() == [0, 2, 3] and np.array_equal(e["S"][0], 2.0 * np.eye(6))
