"""ll_posegraphs on the GPU against the numpy restatement of tests/posegraphcases.py: cost and gradient (the kernel's closed-form
Jacobians against central differences), closed-form and consistent solves, noisy and robust solves against the restatement's dense LM,
fixed nodes, batch independence bit for bit, bounded failure, every host-side error, a synthetic lap and the timing counters.  The
shapes are the smallest that reach every path: sizes round the workgroup's 256 threads, one graph that walks the strided loops more
than once, a node of degree 100.  No expected value comes from the library."""
import ctypes as C

import numpy as np
import pytest

import posegraphcases as pc

pytestmark = pytest.mark.gpu

BATCH_SIZES = [2, 3, 40, 255, 256, 257, 600]


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


_REF = {}


def reference(name):
    """the restatement's dense LM on a shared case, computed once: (truth, start, edges, poses, gradient max-norm at the start)"""
    if name not in _REF:
        truth, start, edges = pc.huber_chain() if name == "huber" else pc.noisy_chain(name)
        x, _, _ = pc.dense_lm(start, edges)
        _REF[name] = (truth, start, edges, x, float(np.abs(pc.gradient(start, edges)).max()))
    return _REF[name]


def pose_diff(a, b):
    """max over nodes of the coordinate difference, q and -q being the same rotation"""
    a = np.asarray(a); b = np.asarray(b)
    flip = np.concatenate([-a[:, :4], a[:, 4:]], axis=1)
    return float(np.minimum(np.abs(a - b).max(axis=1), np.abs(flip - b).max(axis=1)).max())


def rec_bytes(r):
    return bytes(memoryview(r))


def evaluate_cases():
    two, two_edges, _ = pc.two_node()
    tri, tri_edges = pc.triangle()
    tri[1, :4] *= 2.0                                               # quaternions are normalised on entry
    _, chain_start, chain_edges = pc.noisy_chain("cm")
    star_truth, star_edges = pc.star()
    star_start = pc.perturbed(star_truth, np.random.default_rng(11), 0.3, np.deg2rad(5.0))
    return {"two_node": (two, two_edges), "triangle": (tri, tri_edges), "chain": (chain_start, chain_edges), "star": (star_start, star_edges)}


# ------------------------------------------------------------------------------------------------ 1: evaluate
@pytest.mark.parametrize("name", ["two_node", "triangle", "chain", "star"])
def test_evaluate_against_the_restatement(pg, name):
    poses, edges = evaluate_cases()[name]
    cost, grad = pg.evaluate([(poses, edges)])
    want_c = pc.cost(poses, edges)
    want_g = pc.gradient(poses, edges)
    rel = abs(cost[0] - want_c) / want_c
    err = np.abs(grad[0] - want_g).max() / np.abs(want_g).max()
    print(f"{name}: cost {cost[0]!r} vs {want_c!r} (rel {rel:.3g}), gradient error / max|g| {err:.3g}, max|g| {np.abs(want_g).max():.3g}")
    assert rel <= 1e-12
    assert err <= 1e-6
    assert not grad[0][0].any()                                     # zeros at the fixed node


def test_evaluate_in_a_batch_has_the_same_bits(pg):
    cases = list(evaluate_cases().values())
    cost, grad = pg.evaluate(cases)
    for k, g in enumerate(cases):
        c1, g1 = pg.evaluate([g])
        assert c1.tobytes() == cost[k:k + 1].tobytes() and g1[0].tobytes() == grad[k].tobytes(), k


# ------------------------------------------------------------------------------------------------ 2, 3: closed form, consistent graph
def test_two_nodes_solve_to_p0_z(pg, tight):
    start, edges, Z = pc.two_node()
    x, rec = pg.solve([(start, edges)], tight)
    want = pc.compose(pc.normalized(start[0]), Z)
    print("two nodes:", pose_diff(x[0][1:], want[None]), rec[0].cost, rec[0].lm_iterations, rec[0].termination)
    assert pose_diff(x[0][1:], want[None]) <= 1e-12
    assert x[0][0].tobytes() == start[0].tobytes()


def test_a_consistent_graph_recovers_the_truth(pg, tight):
    truth, start, edges = pc.consistent_chain()
    x, rec = pg.solve([(start, edges)], tight)
    r = rec[0]
    print("consistent:", pose_diff(x[0], truth), r.cost0, r.cost, r.grad_max, r.lm_iterations, r.lm_successes, r.pcg_iterations, r.termination)
    assert pose_diff(x[0], truth) <= 1e-7
    assert r.cost < 1e-18 and r.termination == 0
    assert r.cost0 == pytest.approx(pc.cost(start, edges), rel=1e-12)


# ------------------------------------------------------------------------------------------------ 4, 5: noise, Huber
@pytest.mark.parametrize("level", ["tiny", "cm"])
def test_a_noisy_graph_meets_the_restatements_optimum(pg, tight, level):
    truth, start, edges, ref, g0 = reference(level)
    x, rec = pg.solve([(start, edges)], tight)
    g1 = float(np.abs(pc.gradient(x[0], edges)).max())
    r = rec[0]
    print(f"noisy {level}: gradient {g1:.3g} of {g0:.3g} at the start, distance to the dense LM {pose_diff(x[0], ref):.3g}, cost {r.cost0:.6g} -> "
          f"{r.cost:.6g}, LM {r.lm_iterations}, PCG {r.pcg_iterations}, termination {r.termination}")
    assert g1 <= 1e-6 * g0
    assert pose_diff(x[0], ref) <= 1e-7
    assert r.cost == pytest.approx(pc.cost(x[0], edges), rel=1e-9)


def test_huber_holds_a_false_loop_off(pg, tight):
    truth, start, edges, ref, _ = reference("huber")
    plain = edges[:-1] + [pc.false_loop(truth, width=0.0)]
    x, rec = pg.solve([(start, edges), (start, plain)], tight)
    print(f"huber: distance to the robust dense LM {pose_diff(x[0], ref):.3g}, ATE robust {pc.ate(x[0], truth):.4g}, plain {pc.ate(x[1], truth):.4g}, "
          f"LM {rec[0].lm_iterations}, termination {rec[0].termination}")
    assert pose_diff(x[0], ref) <= 1e-7
    assert pc.ate(x[0], truth) < pc.ate(x[1], truth)


# ------------------------------------------------------------------------------------------------ 6: fixed nodes
def test_fixed_and_unconnected_nodes_come_back_bit_for_bit(pg):
    _, start, edges = pc.noisy_chain("cm")
    poses = np.concatenate([start, [pc.random_pose(np.random.default_rng(3))]])         # node 40: free, no edge
    poses[17, :4] *= 1.0000001                                                          # a fixed node is not even normalised
    fixed = np.zeros(41, np.uint8); fixed[[0, 17, 33]] = 1
    x, rec = pg.solve([(poses, edges, fixed)])
    for k in (0, 17, 33, 40):
        assert x[0][k].tobytes() == poses[k].tobytes(), k
    moved = np.abs(x[0] - poses).max(axis=1) > 0
    assert moved[[k for k in range(40) if k not in (0, 17, 33)]].all() and rec[0].lm_successes > 0 and rec[0].cost < rec[0].cost0
    x, rec = pg.solve([(poses, edges, np.ones(41, np.uint8))])
    assert rec[0].lm_iterations == 0 and rec[0].lm_successes == 0 and x[0].tobytes() == poses.tobytes()
    assert rec[0].cost == rec[0].cost0 == pytest.approx(pc.cost(poses, edges), rel=1e-12)


# ------------------------------------------------------------------------------------------------ 7: batch independence
def test_a_graphs_bits_do_not_depend_on_the_batch(pg, api):
    """bounded work per graph (8 LM iterations of at most 150 PCG iterations) keeps the three runs short; every loop is still walked"""
    graphs = [pc.ring_graph(n, 100 + n) for n in BATCH_SIZES]
    opt = api.pg_options(max_lm_iterations=8, max_pcg_iterations=150)
    alone = [pg.solve([g], opt) for g in graphs]
    batch = pg.solve(graphs, opt)
    back = pg.solve(graphs[::-1], opt)
    for k, n in enumerate(BATCH_SIZES):
        x1, r1 = alone[k][0][0], alone[k][1][0]
        assert x1.tobytes() == batch[0][k].tobytes() == back[0][len(graphs) - 1 - k].tobytes(), n
        assert rec_bytes(r1) == rec_bytes(batch[1][k]) == rec_bytes(back[1][len(graphs) - 1 - k]), n
        assert r1.lm_successes > 0 and r1.cost < r1.cost0 and r1.termination != 5, (n, r1.termination)
        assert np.isfinite(x1).all() and (n <= 2 or np.abs(x1[1:] - graphs[k][0][1:]).max() > 0)


# ------------------------------------------------------------------------------------------------ 8: bounded failure
def test_iteration_limits_end_the_solve(pg, api):
    _, start, edges = pc.noisy_chain("cm")
    x, rec = pg.solve([(start, edges)], api.pg_options(max_pcg_iterations=1, max_lm_iterations=2))
    r = rec[0]
    assert r.termination == 3 and r.lm_iterations == 2 and r.pcg_iterations <= 2
    assert np.isfinite(x[0]).all() and r.cost <= r.cost0


def test_an_overflowing_cost_returns_the_input(pg):
    _, start, edges = pc.noisy_chain("cm")
    edges = [pc.edge(e[0], e[1], e[2], (1e200,) * 6, e[4]) for e in edges]
    x, rec = pg.solve([(start, edges)])
    assert rec[0].termination == 5 and rec[0].lm_successes == 0
    assert x[0].tobytes() == start.tobytes()


# ------------------------------------------------------------------------------------------------ 9: errors
def _raw_solve(api, pg, graphs, options=None, nulls=(), n_graphs=None, node_off=None):
    """ll_posegraphs_solve itself -> (status, poses unchanged?, last error)"""
    no, eo, poses, fixed, edges = api.PoseGraphs._pack(graphs)
    if node_off is not None:
        no = np.array(node_off, np.int32)
    before = poses.copy()
    args = {"node_off": no, "edge_off": eo, "poses": poses, "fixed": fixed, "edges": edges}
    p = {k: (None if k in nulls else api._ptr(v)) for k, v in args.items()}
    rc = pg.lib.ll_posegraphs_solve(pg.h, len(graphs) if n_graphs is None else n_graphs, p["node_off"], p["edge_off"], p["poses"], p["fixed"],
                                    p["edges"], None if options is None else C.addressof(options), None)
    return rc, poses.tobytes() == before.tobytes(), pg.lib.ll_posegraphs_last_error(pg.h).decode()


def _bad_graphs():
    """name -> graphs, each with one defect"""
    start, edges, _ = pc.two_node()
    tri, tri_edges = pc.triangle()
    e = edges[0]

    def with_edge(**kw):
        f = dict(i=e[0], j=e[1], Z=e[2].copy(), s=e[3].copy(), a=e[4]); f.update(kw)
        return [(tri, tri_edges), (start, [(f["i"], f["j"], f["Z"], f["s"], f["a"])])]

    def with_pose(k, v):
        p = start.copy(); p[1, k] = v
        return [(p, edges)]

    nan_s = e[3].copy(); nan_s[4] = np.nan
    inf_z = e[2].copy(); inf_z[5] = np.inf
    zero_z = e[2].copy(); zero_z[:4] = 0.0
    zero_q = start.copy(); zero_q[1, :4] = 0.0
    return {"index above": with_edge(j=2), "index below": with_edge(i=-1), "i == j": with_edge(i=1, j=1),
            "pose nan": with_pose(5, np.nan), "pose inf": with_pose(2, np.inf), "measurement inf": with_edge(Z=inf_z),
            "weight nan": with_edge(s=nan_s), "huber inf": with_edge(a=np.inf), "zero measurement quaternion": with_edge(Z=zero_z),
            "zero pose quaternion": [(zero_q, edges)], "no fixed node": [(tri, tri_edges), (start, edges, [0, 0])]}


@pytest.mark.parametrize("name", sorted(_bad_graphs()))
def test_bad_graphs_are_refused_on_the_host(api, pg, name):
    rc, untouched, msg = _raw_solve(api, pg, _bad_graphs()[name])
    assert rc == -2 and untouched and msg, (name, rc, msg)
    if "edge" in msg:
        assert "graph 1, edge 0" in msg, msg                       # the message names the graph and the edge
    with pytest.raises(api.LightLoamError) as ei:
        pg.solve(_bad_graphs()[name])
    assert ei.value.code == -2
    with pytest.raises(api.LightLoamError):
        pg.evaluate(_bad_graphs()[name])


def test_bad_calls_are_refused_on_the_host(api, ctx, pg):
    start, edges, _ = pc.two_node()
    g = [(start, edges)]
    for nulls in (("node_off",), ("edge_off",), ("poses",), ("edges",)):
        rc, untouched, msg = _raw_solve(api, pg, g, nulls=nulls)
        assert rc == -2 and untouched and msg, nulls
    rc, untouched, msg = _raw_solve(api, pg, g + g, node_off=[0, 3, 2])
    assert rc == -2 and untouched and "ascend" in msg
    rc, untouched, msg = _raw_solve(api, pg, g, node_off=[1, 2])
    assert rc == -2 and untouched and msg
    rc, untouched, msg = _raw_solve(api, pg, g, n_graphs=-1)
    assert rc == -2 and untouched and msg
    for bad in (dict(eta=0.0), dict(eta=1.0), dict(max_pcg_iterations=0), dict(max_lm_iterations=-1), dict(gradient_tolerance=-1.0),
                dict(initial_radius=0.0), dict(min_lm_diagonal=0.0), dict(function_tolerance=float("nan")), dict(max_radius=1.0)):
        rc, untouched, msg = _raw_solve(api, pg, g, options=api.pg_options(**bad))
        assert rc == -2 and untouched and "options" in msg, bad
    small = ctx.posegraphs(2, 5, 4)
    tri, tri_edges = pc.triangle()
    for graphs, what in ((g * 3, "graphs"), ([(tri, tri_edges)] * 2, "nodes"), ([(start, edges * 5)], "edges")):
        rc, untouched, msg = _raw_solve(api, small, graphs)
        assert rc == -4 and untouched and what in msg, (what, rc, msg)
    x, rec = small.solve(g + [(tri, tri_edges)])                    # exactly the totals (2 graphs, 5 nodes, 4 edges) is within them
    assert len(x) == 2 and rec[1].cost <= rec[1].cost0
    small.close()


def test_create_refuses_bad_totals(api, ctx):
    for args in ((0, 10, 10), (1, 0, 10), (1, 10, -1)):
        with pytest.raises(api.LightLoamError) as ei:
            ctx.posegraphs(*args)
        assert ei.value.code == -2


# ------------------------------------------------------------------------------------------------ 10: a lap
def test_a_loop_edge_pulls_a_drifting_lap_back(pg, synth):
    cfg = synth.default_cfg(16)
    truth, start, edges = pc.lap([synth.pose(cfg, 3 * k) for k in range(200)], yaw_bias=0.002)
    before = pc.ate(start, truth)
    x, rec = pg.solve([(start, edges)])
    after = pc.ate(x[0], truth)
    print(f"lap: ATE {before:.3f} m -> {after:.3f} m, LM {rec[0].lm_iterations}, PCG {rec[0].pcg_iterations}, termination {rec[0].termination}")
    assert before > 1.0 and after < before and rec[0].cost < rec[0].cost0


# ------------------------------------------------------------------------------------------------ 11: timing
def test_timing_counts_the_records(pg, api):
    graphs = [pc.ring_graph(n, 200 + n) for n in (3, 40, 257)]
    pg.evaluate(graphs)
    x, rec = pg.solve(graphs, api.pg_options(max_lm_iterations=8, max_pcg_iterations=150))
    t = pg.timing()
    assert t["ms"][0] > 0.0 and t["ms"][1] > 0.0
    assert t["graphs"] == 3
    assert t["lm_iterations"] == sum(r.lm_iterations for r in rec) > 0
    assert t["pcg_iterations"] == sum(r.pcg_iterations for r in rec) > 0
