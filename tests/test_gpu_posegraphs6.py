"""ll_posegraphs_evaluate6 / _solve6 -- pose-graph edges with a full 6 x 6 square-root information -- against the numpy restatement of
tests/infocases.py: cost and gradient, solves against its dense LM, a loop information that a diagonal weight cannot express, batch
independence bit for bit, diagonal weights through the full path, the host-side errors, and one end-to-end case in which no weight is
hand-picked: localize_slots(info=True) -> edge_from_info -> solve.  Tolerances are those of tests/test_gpu_posegraphs.py.  No expected
value comes from the library."""
import numpy as np
import pytest

import infocases as ic
import posegraphcases as pc
from test_gpu_localize import World
from test_gpu_posegraphs import pose_diff, rec_bytes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(api):
    c = api.Context(api.default_params(16, batch=2, max_points=4096))
    yield c
    c.close()


@pytest.fixture(scope="module")
def pg(ctx):
    p = ctx.posegraphs(8, 2000, 2500)
    yield p
    p.close()


@pytest.fixture(scope="module")
def tight(api):
    return api.pg_options(**pc.TIGHT)


def some_full(edges, seed, every=7):
    """every `every`-th edge and every loop edge gets a random non-symmetric full S"""
    rng = np.random.default_rng(seed)
    out = []
    for k, e in enumerate(edges):
        if k % every == 0 or abs(e[0] - e[1]) > 1:
            s = np.asarray(e[3], float).mean()
            out.append((e[0], e[1], e[2], s * (np.eye(6) + rng.uniform(-0.3, 0.3, (6, 6))), e[4]))
        else:
            out.append(e)
    return out


def cases():
    """name -> (start, edges): the graphs both the evaluate and the solve tests use"""
    two, two_edges, _ = pc.two_node()
    tri, tri_edges = pc.triangle()
    tri[1, :4] *= 2.0                                               # quaternions are normalised on entry
    _, chain_start, chain_edges = pc.noisy_chain("cm")
    _, hub_start, hub_edges = pc.huber_chain()
    return {"two_node": (two, ic.with_full_loops(two_edges, 21)), "triangle": (tri, ic.with_full_loops(tri_edges, 22)),
            "chain": (chain_start, ic.with_full_loops(chain_edges, 23)), "huber_chain": (hub_start, ic.with_full_loops(hub_edges, 24, 0.5, 1.5))}


_REF = {}


def reference(name, start, edges):
    """the restatement's dense LM, computed once per case: (poses, gradient max-norm at the start)"""
    if name not in _REF:
        x, _, _ = ic.dense_lm(start, edges)
        _REF[name] = (x, float(np.abs(ic.gradient(start, edges)).max()))
    return _REF[name]


def has_full(edges):
    return any(np.ndim(e[3]) == 2 for e in edges)


# ------------------------------------------------------------------------------------------------ evaluate6
@pytest.mark.parametrize("huber", [False, True])
@pytest.mark.parametrize("name", ["two_node", "triangle", "chain"])
def test_evaluate6_against_the_restatement(pg, name, huber):
    poses, edges = cases()[name]
    assert has_full(edges)
    if huber:                                                       # a width every residual of the start exceeds somewhere, and some do not
        edges = [(e[0], e[1], e[2], e[3], 0.3) for e in edges]
        sq = [float(np.sum(ic.residual(pc.normalized(poses[e[0]]), pc.normalized(poses[e[1]]), e) ** 2)) for e in edges]
        assert max(sq) > 0.09
    else:
        edges = [(e[0], e[1], e[2], e[3], 0.0) for e in edges]
    cost, grad = pg.evaluate([(poses, edges)])
    want_c, want_g = ic.cost(poses, edges), ic.gradient(poses, edges)
    rel = abs(cost[0] - want_c) / want_c
    err = np.abs(grad[0] - want_g).max() / np.abs(want_g).max()
    print(f"{name} huber {huber}: cost {cost[0]!r} vs {want_c!r} (rel {rel:.3g}), gradient error / max|g| {err:.3g}")
    assert rel <= 1e-12
    assert err <= 1e-6
    assert not grad[0][0].any()


# ------------------------------------------------------------------------------------------------ solve6
def test_two_nodes_land_on_z_whatever_s(pg, tight):
    start, edges = cases()["two_node"]
    _, _, Z = pc.two_node()
    x, rec = pg.solve([(start, edges)], tight)
    want = pc.compose(pc.normalized(start[0]), Z)
    print("two nodes:", pose_diff(x[0][1:], want[None]), rec[0].cost, rec[0].lm_iterations, rec[0].termination)
    assert pose_diff(x[0][1:], want[None]) <= 1e-12
    assert x[0][0].tobytes() == start[0].tobytes()


def check_against_dense_lm(pg, tight, name, start, edges):
    ref, g0 = reference(name, start, edges)
    x, rec = pg.solve([(start, edges)], tight)
    g1 = float(np.abs(ic.gradient(x[0], edges)).max())
    r = rec[0]
    print(f"{name}: gradient {g1:.3g} of {g0:.3g} at the start, distance to the dense LM {pose_diff(x[0], ref):.3g}, cost {r.cost0:.6g} -> {r.cost:.6g}, "
          f"LM {r.lm_iterations}, PCG {r.pcg_iterations}, termination {r.termination}")
    assert g1 <= 1e-6 * g0
    assert pose_diff(x[0], ref) <= 1e-7
    assert r.cost == pytest.approx(ic.cost(x[0], edges), rel=1e-9)
    return x[0], ref


def test_huber_chain_with_full_s(pg, tight):
    start, edges = cases()["huber_chain"]
    assert has_full(edges) and edges[-1][4] == 0.5
    check_against_dense_lm(pg, tight, "huber_chain", start, edges)


def test_a_star_of_degree_100(pg, tight):
    truth, edges = pc.star(degree=100)
    start = pc.perturbed(truth, np.random.default_rng(11), 0.3, np.deg2rad(5.0))
    edges = some_full(edges, 31, every=3)
    check_against_dense_lm(pg, tight, "star", start, edges)


def test_a_ring_of_300_walks_the_strided_loops_twice(pg, api):
    """a closed chain of 300 poses on a circle of 62 m is what block-Jacobi PCG is slowest at (the stronger preconditioner is not built):
    the default 1000 PCG iterations per LM step end every step early, so the step gets room to reach eta"""
    start, edges = pc.ring_graph(300, 400)
    edges = some_full(edges, 32)
    assert len(start) > 256 and len(edges) > 256
    opt = api.pg_options(max_pcg_iterations=20000, max_lm_iterations=100, **pc.TIGHT)
    check_against_dense_lm(pg, opt, "ring", start, edges)


def test_a_weak_axis_turned_against_the_edge_frame_keeps_the_odometry(pg, tight):
    """The loops' information is strong across and 1e-4 of that (1e-8 in information) along an axis turned 45 degrees against the edge
    frame, and their measurements are 0.4 m off along that axis, 0.1 m across it.  Along the weak axis the loop has nothing to set against
    odometry weights of 5 .. 15, so the solution keeps what the odometry says there -- at least half of the 0.4 m stays in the loops'
    error -- while across it the loop (30) outweighs a chain of at most 15 per edge over at least 15 edges by more than 60 to 1, so at
    most a tenth of the 0.1 m stays.  The best diagonal approximation sqrt(diag(Lambda)) weighs x and y alike and must land elsewhere."""
    truth, start, full, diag, free, weak = ic.weak_axis_chain()
    x, ref = check_against_dense_lm(pg, tight, "weak axis", start, full)
    ref_diag, _ = reference("weak axis, diagonal", start, diag)
    xd, _ = pg.solve([(start, diag)], tight)
    assert pose_diff(xd[0], ref_diag) <= 1e-7
    apart = pose_diff(x, ref_diag)
    print(f"weak axis: the full solution is {apart:.3g} from the best diagonal one")
    assert apart > 1e-3                                             # four orders above the tolerance: no diagonal-only path passes
    across = np.array([-weak[1], weak[0], 0.0])
    for e in full:
        if abs(e[0] - e[1]) > 1:
            r = pc.residual(x[e[0]], x[e[1]], (e[0], e[1], e[2], np.ones(6), 0.0))
            print(f"loop {e[0]} -> {e[1]}: error along the weak axis {r[3:] @ weak:.4f}, across {r[3:] @ across:.5f}")
            assert abs(r[3:] @ weak) >= 0.2 and abs(r[3:] @ across) <= 0.01


# ------------------------------------------------------------------------------------------------ bits
def test_a_graphs_bits_do_not_depend_on_the_batch(pg, api):
    """graphs with full edges, with full and diagonal edges (promoted by the wrapper) and all-diagonal ones (promoted because another
    graph of the call is full), sizes round the 256 threads; bounded work keeps the runs short"""
    graphs = []
    for k, n in enumerate([2, 3, 40, 257, 300]):
        start, edges = pc.ring_graph(n, 500 + n)
        graphs.append((start, edges if k == 2 else some_full(edges, 600 + n, every=1 if k == 0 else 5)))
    assert not has_full(graphs[2][1])
    opt = api.pg_options(max_lm_iterations=6, max_pcg_iterations=100)
    alone = [pg.solve([(g[0], api.pg_edges6(g[1]))], opt) for g in graphs]
    batch = pg.solve(graphs, opt)
    back = pg.solve(graphs[::-1], opt)
    rot = pg.solve(graphs[2:] + graphs[:2], opt)                    # every graph somewhere else: first, last, in the middle
    for k, g in enumerate(graphs):
        x1, r1 = alone[k][0][0], alone[k][1][0]
        assert x1.tobytes() == batch[0][k].tobytes() == back[0][len(graphs) - 1 - k].tobytes() == rot[0][(k - 2) % len(graphs)].tobytes(), k
        assert rec_bytes(r1) == rec_bytes(batch[1][k]) == rec_bytes(back[1][len(graphs) - 1 - k]) == rec_bytes(rot[1][(k - 2) % len(graphs)]), k
        assert r1.lm_successes > 0 and r1.cost < r1.cost0 and r1.termination != 5, (k, r1.termination)
    c_batch, g_batch = pg.evaluate(graphs)
    for k, g in enumerate(graphs):
        c1, g1 = pg.evaluate([(g[0], api.pg_edges6(g[1]))])
        assert c1.tobytes() == c_batch[k:k + 1].tobytes() and g1[0].tobytes() == g_batch[k].tobytes(), k


# ------------------------------------------------------------------------------------------------ diagonal weights through the full path
def test_diagonal_s_through_solve6_meets_solve(pg, api, tight):
    _, start, edges = pc.noisy_chain("cm")
    d = api.pg_edges(edges)
    f = api.pg_edges6(edges)
    assert d.dtype == api.PG_EDGE and f.dtype == api.PG_EDGE6
    c_d, _ = pg.evaluate([(start, d)])
    c_f, _ = pg.evaluate([(start, f)])
    assert abs(c_d[0] - c_f[0]) <= 1e-12 * c_d[0]
    x_d, r_d = pg.solve([(start, d)], tight)
    x_f, r_f = pg.solve([(start, f)], tight)
    print(f"diagonal through solve6: {pose_diff(x_f[0], x_d[0]):.3g} from solve, cost {r_f[0].cost!r} / {r_d[0].cost!r}")
    assert pose_diff(x_f[0], x_d[0]) <= 1e-7


# ------------------------------------------------------------------------------------------------ errors
def test_a_nan_in_s_is_refused_and_a_zero_s_says_nothing(pg, api, tight):
    tri, tri_edges = cases()["triangle"]
    start, edges = cases()["two_node"]
    bad = edges[0][3].copy(); bad[4, 2] = np.nan
    graphs = [(tri, tri_edges), (start, [(0, 1, edges[0][2], bad, 0.0)])]
    no, eo, poses, fixed, packed = api.PoseGraphs._pack(graphs)
    assert packed.dtype == api.PG_EDGE6
    before = poses.copy()
    for solve in (True, False):
        cost = np.zeros(2); grad = np.zeros((len(poses), 6))
        if solve:
            rc = pg.lib.ll_posegraphs_solve6(pg.h, 2, api._ptr(no), api._ptr(eo), api._ptr(poses), api._ptr(fixed), api._ptr(packed), None, None)
        else:
            rc = pg.lib.ll_posegraphs_evaluate6(pg.h, 2, api._ptr(no), api._ptr(eo), api._ptr(poses), api._ptr(fixed), api._ptr(packed), api._ptr(cost), api._ptr(grad))
        msg = pg.lib.ll_posegraphs_last_error(pg.h).decode()
        assert rc == -2 and "graph 1, edge 0" in msg and poses.tobytes() == before.tobytes(), (solve, rc, msg)
    for inf in (np.inf, -np.inf):
        bad = edges[0][3].copy(); bad[0, 5] = inf
        with pytest.raises(api.LightLoamError) as ei:
            pg.solve([(start, [(0, 1, edges[0][2], bad, 0.0)])])
        assert ei.value.code == -2
    # an all-zero S: an edge that says nothing -- cost, gradient and solution are those of the graph without it
    _, cstart, cedges = pc.noisy_chain("cm")
    full = ic.with_full_loops(cedges, 23)
    silent = full + [(3, 30, pc.random_pose(np.random.default_rng(5)), np.zeros((6, 6)), 0.0)]
    c0, g0 = pg.evaluate([(cstart, full)])
    c1, g1 = pg.evaluate([(cstart, silent)])
    assert c0[0] == c1[0] and np.array_equal(g0[0], g1[0])
    x0, _ = pg.solve([(cstart, full)], tight)
    x1, r1 = pg.solve([(cstart, silent)], tight)
    assert r1[0].termination != 5 and pose_diff(x1[0], x0[0]) <= 1e-12


# ------------------------------------------------------------------------------------------------ end to end: no hand-picked weight
def test_a_measured_edge_from_localisation_to_the_graph(api, synth, pg):
    """sequences 1 and 2 localise frames of drive A in map 0; each localisation becomes an edge (0 -> q, Z = P_0^-1 X_q) whose weight is
    edge_from_info of its own record, sigma from the record.  At the measured poses every edge error is zero, so 2 * cost is 0 -- up to
    rounding: the rotation part of E = Z^-1 P_0^-1 P_q cancels exactly, its translation is R(a) (t_q - t_0) - R(q_z)^T t_z through two
    different formulas of one rotation, which differ by a few ulp of |t| ~ 10 m, 1e-15 m; times |S| < 1e5 and squared that stays below
    1e-18 (measured: 5.6e-26).  Moved away, the solve comes back to the measured poses"""
    w = World(api, synth, 16)
    frames, guess, slots = w.call(1)
    poses, ran, fit, info = w.many.localize_slots(guess, slots, [0] * w.S, info=True)
    assert ran[1] and ran[2]
    P0 = np.array([0, 0, 0, 1.0, 0, 0, 0])
    edges, nodes = [], [P0]
    for q in (1, 2):
        S = api.edge_from_info(info[q], poses[q], floor=1e-6)
        eig = np.array(info[q].eig[:])
        print(f"sequence {q}: eig {eig[0]:.4g} .. {eig[5]:.4g}, sigma {np.sqrt(info[q].sigma2):.4g} m, |S| {np.abs(S).max():.4g}")
        assert eig[0] > 0.0 and np.array_equal(S, np.triu(S))
        edges.append((0, q, api.relative_pose(P0, poses[q]), S, 1.0))
        nodes.append(poses[q])
    nodes = np.array(nodes)
    cost, grad = pg.evaluate([(nodes, edges)])
    print(f"end to end: 2 * cost at the measured poses {2.0 * cost[0]!r}")
    assert 2.0 * cost[0] <= 1e-18
    moved = pc.perturbed(nodes, np.random.default_rng(8), 0.05, np.deg2rad(0.5)); moved[0] = P0
    x, rec = pg.solve([(moved, edges)], api.pg_options(**pc.TIGHT))
    print(f"end to end: cost {rec[0].cost0:.6g} -> {rec[0].cost:.3g}, back within {pose_diff(x[0], nodes):.3g}")
    assert rec[0].cost < 1e-12 * rec[0].cost0 and pose_diff(x[0], nodes) <= 1e-7
    w.close()
