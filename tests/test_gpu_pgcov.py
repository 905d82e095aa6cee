"""ll_posegraphs_covariances on the GPU against the numpy restatement of tests/pgcovcases.py (dense H from closed-form Jacobians,
numpy.linalg.inv): every graph and size that takes another path, under both preconditioners, held to

    max |S_dev - S_ref| <= (tolerance + 100 eps cond(H_ref)) * ||H_ref^-1||_2

with cond and the norm from the dense eigenvalues (the stop rule |r| <= tolerance gives |x - x*| <= ||H^-1|| |r|; 100 eps cond is the
rounding margin ll_posegraphs_chain_solve's tests grant); then the shapes of a query, the records, batch independence bit for bit, every
host-side refusal, the solves' bits around a covariance call, and the gate on device covariances.  No expected value comes from the library."""
import ctypes as C

import numpy as np
import pytest

import pgchaincases as cc
import pgcovcases as cv
import posegraphcases as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(api):
    c = api.Context(api.default_params(16, batch=2, max_points=4096))
    yield c
    c.close()


@pytest.fixture(scope="module")
def pg(ctx):
    """block-Jacobi unless a test switches, and every test that switches switches back"""
    p = ctx.posegraphs(16, 3000, 3600)
    yield p
    p.close()


@pytest.fixture()
def chain(pg, api):
    pg.set_preconditioner(api.PG_PRECOND_CHAIN)
    yield pg
    pg.set_preconditioner(api.PG_PRECOND_BLOCK_JACOBI)


@pytest.fixture(params=["jacobi", "chain"])
def either(request, pg, api):
    pg.set_preconditioner(request.param)
    yield pg
    pg.set_preconditioner(api.PG_PRECOND_BLOCK_JACOBI)


# ------------------------------------------------------------------------------------------------ graphs and references, built once
def full_chain():
    """the 40-node chain with ll_pg_edge6 edges: S = diag(s) (I + a strictly upper-triangular part), one edge with a Huber width"""
    _, start, edges = pc.noisy_chain("cm")
    rng = np.random.default_rng(31)
    out = []
    for k, e in enumerate(edges):
        S = np.diag(e[3]) @ (np.eye(6) + 0.3 * np.triu(rng.normal(size=(6, 6)), 1))
        out.append((e[0], e[1], e[2], S, 0.05 if k == 41 else 0.0))
    return start, out


def _build(name):
    if name == "two_node":
        poses, edges, _ = pc.two_node(); return poses, edges, None
    if name == "triangle":
        poses, edges = pc.triangle(); return poses, edges, None
    if name == "star":
        truth, edges = pc.star()
        return pc.perturbed(truth, np.random.default_rng(11), 0.3, np.deg2rad(5.0)), edges, None
    if name == "chain40":
        truth, edges = pc.chain(); return pc.start_of(truth), edges, None
    if name == "huber_chain":
        _, start, edges = pc.huber_chain(); return start, edges, None
    if name == "full_chain":
        return full_chain() + (None,)
    if name.startswith("lap"):
        return cc.circle_lap(int(name[3:]))
    g = {"loop_free": cc.loop_free_chain, "reversed": cc.reversed_chain, "doubled": cc.doubled_chain, "fixed": cc.fixed_chain,
         "star_graph": cc.star_graph}[name]()
    return g[0], g[1], (g[2] if len(g) > 2 else None)


_GRAPHS, _REF = {}, {}


def graph(name):
    """(poses, edges, fixed uint8 [N])"""
    if name not in _GRAPHS:
        poses, edges, fixed = _build(name)
        fixed = pc.default_fixed(len(poses)) if fixed is None else np.asarray(fixed, bool)
        _GRAPHS[name] = (np.asarray(poses, float), edges, fixed.astype(np.uint8))
    return _GRAPHS[name]


def reference(name):
    """(Sigma [6 N, 6 N], eigenvalues of H_free) of the restatement, computed once and left alone"""
    if name not in _REF:
        poses, edges, fixed = graph(name)
        S, w = cv.sigma(poses, edges, fixed)
        S.setflags(write=False)
        _REF[name] = (S, w)
    return _REF[name]


def queries_of(name):
    """sources at node 1, N - 1 and inside the chain (not a fixed node), alone and in pairs, both ways round, b == a"""
    poses, _, fixed = graph(name)
    n = len(poses)
    mid = n // 3 if n > 3 else n - 1
    assert n < 3 or not fixed[mid]
    q = [(0, 1, -1), (0, n - 1, -1), (0, mid, -1), (0, mid, mid), (0, 1, n - 1), (0, n - 1, 1), (0, mid, n - 1), (0, 0, 1)]
    return q


def check_against_the_restatement(pg, api, name, options, tolerance):
    poses, edges, fixed = graph(name)
    S, w = reference(name)
    bound, cond = cv.bound(w, tolerance)
    q = queries_of(name)
    joint, rec = pg.covariances([(poses, edges, fixed)], q, options)
    worst = 0.0
    for k, (_, a, b) in enumerate(q):
        worst = max(worst, float(np.abs(joint[k] - cv.joint(S, a, b)).max()))
    its = max(r.pcg_iterations for r in rec)
    print(f"{name}: N {len(poses)}, cond {cond:.3g}, |H^-1| {1.0 / w[0]:.3g}, max error {worst:.3g}, bound {bound:.3g}, error / bound {worst / bound:.3g}, "
          f"most PCG iterations of a query {its}, largest residual {max(r.residual for r in rec):.3g}")
    assert [r.status for r in rec] == [0] * len(q)
    assert all(r.residual <= tolerance for r in rec)
    assert worst <= bound
    return rec, q


# ------------------------------------------------------------------------------------------------ 1: accuracy
JACOBI = ["two_node", "triangle", "star", "chain40", "huber_chain", "full_chain"]
CHAIN = ["loop_free", "reversed", "doubled", "fixed", "star_graph", "lap255", "lap256", "lap257", "lap513"]


@pytest.mark.parametrize("name", JACOBI)
def test_block_jacobi_against_the_restatement(pg, api, name):
    n = len(graph(name)[0])
    o = api.pg_cov_options(max_pcg_iterations=20 * 6 * n)
    check_against_the_restatement(pg, api, name, o, o.tolerance)


@pytest.mark.parametrize("name", CHAIN)
def test_chain_preconditioner_against_the_restatement(chain, api, name):
    rec, q = check_against_the_restatement(chain, api, name, None, api.pg_cov_options().tolerance)
    poses, edges, fixed = graph(name)
    L = cc.other_edges(edges, fixed.astype(bool))
    if L == 0:                                                      # M = H: one iteration in exact arithmetic, a second for its rounding
        for r, (_, a, b) in zip(rec, q):
            columns = 6 * sum(1 for n in {a, b} if n >= 0 and not fixed[n])
            assert r.pcg_iterations <= columns * (12 * L + 2), (a, b, r.pcg_iterations)


# ------------------------------------------------------------------------------------------------ 2: the shape of a query
def test_single_node_queries_and_fixed_nodes(either):
    poses, edges, fixed = graph("fixed")
    q = [(0, 20, -1), (0, 20, 20), (0, 17, -1), (0, 17, 20), (0, 20, 17), (0, 0, 39), (0, 20)]
    joint, rec = either.covariances([(poses, edges, fixed)], q)
    assert joint[0].tobytes() == joint[1].tobytes() == joint[6].tobytes()
    assert not joint[0][6:].any() and not joint[0][:, 6:].any() and joint[0][:6, :6].any()
    assert not joint[2].any() and not joint[5].any()                # fixed nodes: exact zeros
    assert not joint[3][:6].any() and not joint[3][:, :6].any()
    assert joint[3][6:, 6:].tobytes() == joint[0][:6, :6].tobytes() == joint[4][:6, :6].tobytes()
    assert not joint[4][6:].any() and not joint[4][:, 6:].any()
    assert (rec[2].status, rec[2].pcg_iterations, rec[2].residual) == (0, 0, 0.0)
    assert rec[3].pcg_iterations == rec[0].pcg_iterations > 0
    assert np.array_equal(joint[0], joint[0].T)                     # (X + X^T) / 2


def test_swapped_queries_are_exact_permutations(either):
    poses, edges, fixed = graph("doubled")
    joint, rec = either.covariances([(poses, edges, fixed)], [(0, 5, 30), (0, 30, 5)])
    swap = np.r_[6:12, 0:6]
    assert joint[0].tobytes() == np.ascontiguousarray(joint[1][np.ix_(swap, swap)]).tobytes()
    assert np.array_equal(joint[0], joint[0].T) and joint[0][:6, 6:].any()
    assert bytes(memoryview(rec[0])) == bytes(memoryview(rec[1]))


def test_a_source_shared_by_several_queries_is_solved_once(either):
    poses, edges, fixed = graph("doubled")
    joint, rec = either.covariances([(poses, edges, fixed)], [(0, 5, 10), (0, 5, 20), (0, 5, -1), (0, 20, 5)])
    assert joint[0][:6, :6].tobytes() == joint[1][:6, :6].tobytes() == joint[2][:6, :6].tobytes() == joint[3][6:, 6:].tobytes()
    t = either.cov_timing()
    assert (t["queries"], t["sources"]) == (4, 3)
    alone = either.covariances([(poses, edges, fixed)], [(0, 5, -1)])[1][0].pcg_iterations
    assert rec[2].pcg_iterations == alone and t["pcg_iterations"] >= alone
    assert t["ms"][0] > 0.0 and t["ms"][1] > 0.0


def test_no_queries_launch_nothing(pg):
    poses, edges, fixed = graph("triangle")
    joint, rec = pg.covariances([(poses, edges, fixed)], [])
    assert joint.shape == (0, 12, 12) and rec == []
    t = pg.cov_timing()
    assert (t["queries"], t["sources"], t["pcg_iterations"], t["ms"]) == (0, 0, 0, [0.0, 0.0])
    assert pg.covariances([], [])[0].shape == (0, 12, 12)


# ------------------------------------------------------------------------------------------------ 3: the same bits in any company
def rec_bytes(r):
    return bytes(memoryview(r))


def test_a_query_has_the_same_bits_alone_and_in_any_batch(either):
    names = ["triangle", "doubled", "two_node", "lap257", "fixed", "star"]
    graphs = [graph(n) for n in names]
    own = {"triangle": (1, 2), "doubled": (5, 30), "two_node": (1, -1), "lap257": (3, 250), "fixed": (20, 38), "star": (7, 50)}
    alone = {}
    for n, g in zip(names, graphs):
        j, r = either.covariances([g], [(0,) + own[n]])
        alone[n] = (j[0].tobytes(), rec_bytes(r[0]))
    # every graph but one queried (lap257 has none), the queries in another order than the graphs, with company
    q = [(4, 20, 38), (0, 1, 2), (5, 7, 50), (1, 5, 30), (1, 6, 5), (2, 1, -1), (4, 38, 2), (1, 5, 30)]
    j, r = either.covariances(graphs, q)
    for k, n in ((0, "fixed"), (1, "triangle"), (2, "star"), (3, "doubled"), (5, "two_node"), (7, "doubled")):
        assert (j[k].tobytes(), rec_bytes(r[k])) == alone[n], n
    # the batch reversed, lap257 queried this time
    back = graphs[::-1]
    q = [(len(names) - 1 - names.index(n),) + own[n] for n in names]
    j, r = either.covariances(back, q)
    for k, n in enumerate(names):
        assert (j[k].tobytes(), rec_bytes(r[k])) == alone[n], n


# ------------------------------------------------------------------------------------------------ 4: the records
def test_the_iteration_limit_is_status_1_with_finite_blocks(pg, api):
    poses, edges, fixed = graph("chain40")
    joint, rec = pg.covariances([(poses, edges, fixed)], [(0, 20, -1), (0, 20, 39)], api.pg_cov_options(max_pcg_iterations=1))
    assert [r.status for r in rec] == [1, 1] and [r.pcg_iterations for r in rec] == [6, 12]
    assert np.isfinite(joint).all() and joint[0][:6, :6].any() and all(r.residual > 1e-10 for r in rec)


def test_a_singular_but_connected_graph_is_status_2_with_zeros(either):
    """node 2 hangs on an all-zero S: connected, so the host lets it through, but its block of H is zero"""
    poses, edges = pc.triangle()
    e6 = [(0, 1, edges[0][2], np.diag(edges[0][3]), 0.0), (1, 2, edges[1][2], np.zeros((6, 6)), 0.0)]
    joint, rec = either.covariances([(poses, e6)], [(0, 2, -1), (0, 1, 2), (0, 1, -1)])
    assert [r.status for r in rec] == [2, 2, 0]
    assert not joint[0].any() and not joint[1].any() and np.isfinite(joint).all()
    _, Jj = cv.edge_jacobians(pc.normalized(poses[0]), pc.normalized(poses[1]), e6[0])
    want = np.linalg.inv(Jj.T @ Jj)                                 # node 1 is held by its one edge alone
    assert np.abs(joint[2][:6, :6] - want).max() <= 1e-9 * np.abs(want).max()


# ------------------------------------------------------------------------------------------------ 5: refusals leave the outputs alone
def raw(pg, api, graphs, q, options=None, fixed_null=False, joint_null=False):
    no, eo, poses, fixed, edges = pg._pack(graphs)
    qa = np.zeros(len(q), api.PG_COV_QUERY)
    for k, t in enumerate(q):
        qa[k] = t
    joint = np.full((max(len(q), 1), 144), -7.0); rec = (api.PgCovRecord * max(len(q), 1))()
    for r in rec:
        r.status = -7
    fn = pg.lib.ll_posegraphs_covariances6 if edges.dtype == api.PG_EDGE6 else pg.lib.ll_posegraphs_covariances
    rc = fn(pg.h, len(graphs), no.ctypes.data, eo.ctypes.data, poses.ctypes.data, None if fixed_null else fixed.ctypes.data, edges.ctypes.data,
            len(q), qa.ctypes.data, None if options is None else C.addressof(options), None if joint_null else joint.ctypes.data, C.addressof(rec))
    return rc, bool((joint == -7.0).all() and all(r.status == -7 for r in rec)), pg.lib.ll_posegraphs_last_error(pg.h).decode()


def test_host_errors_leave_the_outputs_untouched(pg, api):
    tri = graph("triangle")
    poses, edges, fixed = tri
    island = (np.vstack([poses, poses[:2] + 1.0]), list(edges) + [pc.edge(3, 4, pc.relative(poses[0], poses[1]))], None)   # 3 - 4: no fixed node
    lonely = (np.vstack([poses, poses[:1] + 1.0]), edges, None)                                                          # 3: no edge
    nan_pose = poses.copy(); nan_pose[2, 5] = np.nan
    cases = [
        ([tri], [(1, 1, -1)], None, "graph 1"), ([tri], [(-1, 1, -1)], None, "graph -1"),
        ([tri], [(0, 3, -1)], None, "node 3"), ([tri], [(0, -1, 1)], None, "node -1"), ([tri], [(0, 1, 3)], None, "node 3"),
        ([tri, island], [(0, 1, 2), (1, 1, 4)], None, "query 1: node 4 of graph 1 is not connected"),
        ([lonely], [(0, 3, -1)], None, "query 0: node 3 of graph 0 is not connected"),
        ([tri], [(0, 1, 2)], api.pg_cov_options(max_pcg_iterations=0), "options"),
        ([tri], [(0, 1, 2)], api.pg_cov_options(tolerance=-1.0), "options"),
        ([tri], [(0, 1, 2)], api.pg_cov_options(tolerance=float("nan")), "options"),
        ([(nan_pose, edges, fixed)], [(0, 1, 2)], None, "not finite"),
        ([(poses, edges, np.zeros(3, np.uint8))], [(0, 1, 2)], None, "no fixed node"),
        ([(poses, [pc.edge(0, 3, edges[0][2])], fixed)], [(0, 1, -1)], None, "outside the graph"),
    ]
    for graphs, q, o, text in cases:
        rc, untouched, err = raw(pg, api, graphs, q, o)
        assert rc == -2 and untouched and text in err and err.startswith("posegraphs: covariances: "), (text, rc, err)
    rc, untouched, err = raw(pg, api, [tri], [(0, 1, 2)], joint_null=True)
    assert rc == -2 and "joint144" in err
    rc, untouched, err = raw(pg, api, [tri] * 17, [(0, 1, 2)])
    assert rc == -4 and untouched and "max_graphs" in err
    rc, untouched, err = raw(pg, api, [island], [(0, 1, 2)])        # a singular island nobody asks about is nobody's error
    assert rc == 0 and not untouched
    rc, untouched, _ = raw(pg, api, [tri], [(0, 1, 2)], fixed_null=True)                 # fixed == NULL: node 0
    assert rc == 0 and not untouched
    with pytest.raises(api.LightLoamError) as ei:
        pg.covariances([tri], [(0, 9, -1)])
    assert ei.value.code == -2 and "node 9" in str(ei.value)


# ------------------------------------------------------------------------------------------------ 6: the solves do not notice
@pytest.mark.parametrize("kind", ["jacobi", "chain"])
def test_solve_agrees_bit_for_bit_before_and_after(pg, api, kind):
    pg.set_preconditioner(kind)
    try:
        graphs = [graph("doubled"), graph("lap257"), graph("huber_chain")]
        x0, r0 = pg.solve(graphs)
        c0, g0 = pg.evaluate(graphs)
        pg.covariances(graphs, [(0, 5, 30), (1, 3, 250), (2, 20, 2)])
        x1, r1 = pg.solve(graphs)
        c1, g1 = pg.evaluate(graphs)
        for a, b in zip(x0 + g0, x1 + g1):
            assert a.tobytes() == b.tobytes()
        assert [rec_bytes(r) for r in r0] == [rec_bytes(r) for r in r1] and c0.tobytes() == c1.tobytes()
    finally:
        pg.set_preconditioner(api.PG_PRECOND_BLOCK_JACOBI)


# ------------------------------------------------------------------------------------------------ 7: the gate on device covariances
def test_the_gate_on_a_solved_chain(chain, api):
    """the levels of tests/test_pgcov_cases.py, on the device's solve and covariances: a closure measured from the truth stays below the
    median of chi-square(6), 5.35; posegraphcases.false_loop at s = 5 lies above its 0.999 quantile, 22.46"""
    truth, start, edges = pc.noisy_chain("cm")
    x, rec = chain.solve([(start, edges)], api.pg_options(**pc.TIGHT))
    x = x[0]
    fl = pc.false_loop(truth, s=5.0)
    joint, crec = chain.covariances([(x, edges)], [(0, 35, 3), (0, fl[0], fl[1])])
    assert [r.status for r in crec] == [0, 0]
    good = api.edge_gate(x[35], x[3], pc.relative(truth[35], truth[3]), (10.0,) * 6, joint[0])
    bad = api.edge_gate(x[fl[0]], x[fl[1]], fl[2], fl[3], joint[1])
    print(f"gate on the device: chi2 {good:.4g} for a true closure, {bad:.4g} for the false loop")
    assert good < 5.35 and bad > cv.CHI2_6_999
