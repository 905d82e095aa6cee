"""ll_posegraphs' chain preconditioner on the GPU against the numpy restatement of tests/pgchaincases.py and posegraphcases.py:
ll_posegraphs_chain_solve against numpy.linalg.solve at every size that takes another path through the cyclic reduction, solves under
the chain preconditioner against the restatement's dense LM on every graph of pgchaincases.graphs() and both edge types, the PCG
iteration counts the rank argument promises, batch independence bit for bit, the default preconditioner's bits before and after a
switch, and every host-side refusal.  No expected value comes from the library."""
import ctypes as C

import numpy as np
import pytest

import pgchaincases as cc
import posegraphcases as pc

pytestmark = pytest.mark.gpu

# a lone node, every ragged-end shape of the first levels, the workgroup's 256 threads from both sides, more than one node per thread
SIZES = [1, 2, 3, 4, 5, 7, 8, 9, 255, 256, 257, 513, 1000]
EPS = cc.EPS


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


_SYSTEMS, _GRAPHS, _REF = {}, {}, {}


def system(n):
    """(diag, upper, cond, rhs, the dense solution) of the random system of n nodes, computed once"""
    if n not in _SYSTEMS:
        diag, upper, cond = cc.random_system(n, 100 + n)
        rhs = np.random.default_rng(200 + n).normal(size=(n, 6))
        _SYSTEMS[n] = (diag, upper, cond, rhs, cc.dense_solve(cc.dense_of(diag, upper), rhs.reshape(-1)).reshape(n, 6))
    return _SYSTEMS[n]


def graph(name):
    if not _GRAPHS:
        _GRAPHS.update(cc.graphs())
    return _GRAPHS[name]


def reference(name):
    """the restatement's dense LM on a graph, computed once: (poses, gradient max-norm at the start)"""
    if name not in _REF:
        start, edges, fixed = graph(name)
        x, _, _ = pc.dense_lm(start, edges, fixed)
        _REF[name] = (x, float(np.abs(pc.gradient(start, edges, fixed)).max()))
    return _REF[name]


def pose_diff(a, b):
    a = np.asarray(a); b = np.asarray(b)
    flip = np.concatenate([-a[:, :4], a[:, 4:]], axis=1)
    return float(np.minimum(np.abs(a - b).max(axis=1), np.abs(flip - b).max(axis=1)).max())


def rec_bytes(r):
    return bytes(memoryview(r))


# ------------------------------------------------------------------------------------------------ 1: the solver alone
@pytest.mark.parametrize("n", SIZES)
def test_chain_solve_against_the_dense_solve(pg, n):
    diag, upper, cond, rhs, want = system(n)
    x, status = pg.chain_solve([(diag, upper, rhs)])
    err = np.abs(x[0] - want).max() / np.abs(want).max()
    print(f"N {n}: cond {cond:.3g}, relative max-norm error {err:.3g}, bound {100 * EPS * cond:.3g}")
    assert status.tolist() == [0]
    assert err <= 100 * EPS * cond


def test_zero_couplings_give_the_blocks_own_solves(pg):
    diag, _, _, rhs, _ = system(257)
    upper = np.zeros_like(diag)
    x, status = pg.chain_solve([(diag, upper, rhs)])
    want = np.array([np.linalg.solve(d, r) for d, r in zip(diag, rhs)])
    cond = max(np.linalg.cond(d) for d in diag)
    err = np.abs(x[0] - want).max() / np.abs(want).max()
    print(f"zero couplings: relative max-norm error {err:.3g}, bound {100 * EPS * cond:.3g}")
    assert status.tolist() == [0] and err <= 100 * EPS * cond


def test_the_last_coupling_is_ignored(pg):
    diag, upper, _, rhs, _ = system(9)
    junk = upper.copy(); junk[-1] = np.nan
    a, _ = pg.chain_solve([(diag, upper, rhs)])
    b, status = pg.chain_solve([(diag, junk, rhs), (diag[:1], junk[-1:], rhs[:1])])
    assert status.tolist() == [0, 0] and a[0].tobytes() == b[0].tobytes()
    assert np.allclose(b[1][0], np.linalg.solve(diag[0], rhs[0]), rtol=1e-9)


def test_a_batch_of_ragged_systems_has_each_systems_bits(pg):
    systems = [system(n)[:2] + (system(n)[3],) for n in SIZES]
    alone = [pg.chain_solve([s])[0][0] for s in systems]
    batch, status = pg.chain_solve(systems)
    back, _ = pg.chain_solve(systems[::-1])
    assert not status.any()
    for k, n in enumerate(SIZES):
        assert alone[k].tobytes() == batch[k].tobytes() == back[len(SIZES) - 1 - k].tobytes(), n


@pytest.mark.parametrize("n,node", [(1, 0), (9, 0), (9, 4), (9, 8), (257, 128), (257, 255)])
def test_an_indefinite_block_fails_its_system_alone(pg, n, node):
    """the node is eliminated at level 0 (odd), at a higher level or is node 0, the last one to be factored"""
    diag, upper, _, rhs, _ = system(n)
    bad = diag.copy(); bad[node] = -bad[node]
    good = [system(m)[:2] + (system(m)[3],) for m in (5, 256)]
    alone = [pg.chain_solve([s])[0][0] for s in good]
    x, status = pg.chain_solve([good[0], (bad, upper, rhs), good[1]])
    assert status.tolist() == [0, 1, 0]
    assert not x[1].any() and x[1].shape == (n, 6)
    assert x[0].tobytes() == alone[0].tobytes() and x[2].tobytes() == alone[1].tobytes()


def _raw_chain(api, pg, no, diag, upper, rhs, n_systems=None, nulls=()):
    """ll_posegraphs_chain_solve itself -> (status, out and status untouched?, last error)"""
    no = np.array(no, np.int32)
    n = max(int(no.max()), 1)
    out = np.full((n, 6), 7.0); st = np.full(max(len(no) - 1, 1), 7, np.int32)
    args = {"node_off": no, "diag": np.ascontiguousarray(diag), "upper": np.ascontiguousarray(upper), "rhs": np.ascontiguousarray(rhs), "out": out, "status": st}
    p = {k: (None if k in nulls else api._ptr(v)) for k, v in args.items()}
    rc = pg.lib.ll_posegraphs_chain_solve(pg.h, len(no) - 1 if n_systems is None else n_systems, p["node_off"], p["diag"], p["upper"], p["rhs"],
                                          p["out"], p["status"])
    return rc, bool((out == 7.0).all() and (st == 7).all()), pg.lib.ll_posegraphs_last_error(pg.h).decode()


def test_bad_chain_solves_are_refused_on_the_host(api, ctx, pg):
    diag, upper, _, rhs, _ = system(9)
    d, u, r = diag.reshape(9, 36), upper.reshape(9, 36), rhs
    for nulls in (("node_off",), ("diag",), ("upper",), ("rhs",), ("out",), ("status",)):
        rc, untouched, msg = _raw_chain(api, pg, [0, 9], d, u, r, nulls=nulls)
        assert rc == -2 and untouched and msg, nulls
    for no, what in (([0, 5, 3], "ascend"), ([1, 9], "start at 0")):
        rc, untouched, msg = _raw_chain(api, pg, no, d, u, r)
        assert rc == -2 and untouched and what in msg, (no, msg)
    rc, untouched, msg = _raw_chain(api, pg, [0, 9], d, u, r, n_systems=-1)
    assert rc == -2 and untouched and msg
    for which, k in (("diag", 5 * 36 + 7), ("upper", 7 * 36 + 35), ("rhs", 8 * 6 + 5)):      # nodes 5, 7 and 8: system 1 of [0, 4, 9]
        for v in (np.nan, np.inf):
            arrs = {"diag": d.copy(), "upper": u.copy(), "rhs": r.copy()}
            arrs[which].reshape(-1)[k] = v
            rc, untouched, msg = _raw_chain(api, pg, [0, 4, 9], arrs["diag"], arrs["upper"], arrs["rhs"])
            assert rc == -2 and untouched and "system 0" not in msg and "system 1" in msg, (which, v, msg)
    small = ctx.posegraphs(2, 5, 4)
    rc, untouched, msg = _raw_chain(api, small, [0, 1, 2, 3], d, u, r)
    assert rc == -4 and untouched and "systems" in msg
    rc, untouched, msg = _raw_chain(api, small, [0, 6], d, u, r)
    assert rc == -4 and untouched and "nodes" in msg
    rc, untouched, msg = _raw_chain(api, small, [0, 2, 5], d, u, r)      # exactly the totals is within them
    assert rc == 0 and not untouched
    rc, _, _ = _raw_chain(api, small, [0], d, u, r)                     # no system: nothing to do
    assert rc == 0
    assert small.preconditioner == api.PG_PRECOND_BLOCK_JACOBI          # chain_solve does not switch the solves
    small.close()
    with pytest.raises(ValueError):
        pg.chain_solve([(diag, upper[:5], rhs)])


# ------------------------------------------------------------------------------------------------ 2: solves against the dense LM
@pytest.mark.parametrize("full", [False, True], ids=["diagonal", "full"])
@pytest.mark.parametrize("name", cc.GRAPH_NAMES)
def test_a_solve_with_the_chain_meets_the_restatements_optimum(chain, api, name, full):
    start, edges, fixed = graph(name)
    ref, g0 = reference(name)
    given = api.pg_edges6(api.pg_edges(edges)) if full else edges      # solve6 with diag(sqrt_info) written as full matrices
    x, rec = chain.solve([(start, given, fixed)], api.pg_options(max_lm_iterations=200, **pc.TIGHT))
    r = rec[0]
    g1 = float(np.abs(pc.gradient(x[0], edges, fixed)).max())
    want = pc.cost(x[0], edges)
    stats = chain.precond_stats()
    print(f"{name} {'full' if full else 'diagonal'}: gradient {g1:.3g} of {g0:.3g} at the start, distance to the dense LM {pose_diff(x[0], ref):.3g}, "
          f"cost {r.cost0:.6g} -> {r.cost!r} (restatement {want!r}), LM {r.lm_iterations}, PCG {r.pcg_iterations}, termination {r.termination}, {stats}")
    assert g1 <= 1e-6 * g0
    assert pose_diff(x[0], ref) <= 1e-7
    assert r.cost == pytest.approx(want, rel=1e-9, abs=cc.cost_floor(start, edges))
    assert stats == {"factorisations": r.lm_iterations, "fallbacks": 0}
    for k in np.flatnonzero(fixed):
        assert x[0][k].tobytes() == np.asarray(start)[k].tobytes(), k


# ------------------------------------------------------------------------------------------------ 3: iteration counts
def test_a_loop_free_chain_takes_one_pcg_iteration_per_lm_iteration(chain, api):
    opt = api.pg_options(eta=1e-6)
    for name in ("loop_free", "reversed", "star"):                     # M = A on all three: the star's edges all end at the fixed node
        start, edges, fixed = graph(name)
        x, rec = chain.solve([(start, edges, fixed)], opt)
        r = rec[0]
        print(f"{name}: LM {r.lm_iterations}, PCG {r.pcg_iterations}, termination {r.termination}, cost {r.cost0:.6g} -> {r.cost:.6g}")
        assert r.lm_iterations > 0 and r.pcg_iterations == r.lm_iterations, name
        assert chain.precond_stats() == {"factorisations": r.lm_iterations, "fallbacks": 0}


@pytest.mark.parametrize("name", cc.COUNT_NAMES)
def test_a_lap_stays_within_the_rank_bound_and_below_block_jacobi(pg, api, name):
    start, edges, fixed = graph(name)
    L = cc.LOOPS[name]
    opt = api.pg_options(eta=1e-6, max_lm_iterations=6, max_pcg_iterations=3000)
    xj, rj = pg.solve([(start, edges, fixed)], opt)
    assert pg.precond_stats() == {"factorisations": 0, "fallbacks": 0}
    pg.set_preconditioner("chain")
    try:
        xc, rc = pg.solve([(start, edges, fixed)], opt)
        stats = pg.precond_stats()
    finally:
        pg.set_preconditioner("jacobi")
    j, c = rj[0], rc[0]
    print(f"{name}: chain LM {c.lm_iterations}, PCG {c.pcg_iterations} (bound {c.lm_iterations * (12 * L + 1)}), cost {c.cost0:.6g} -> {c.cost:.6g}; "
          f"block-Jacobi LM {j.lm_iterations}, PCG {j.pcg_iterations}, cost -> {j.cost:.6g}; {stats}")
    assert c.lm_iterations > 0 and c.pcg_iterations <= c.lm_iterations * (12 * L + 1)
    assert c.pcg_iterations < j.pcg_iterations
    assert stats["factorisations"] >= c.lm_iterations and stats["fallbacks"] == 0
    assert c.cost < c.cost0


# ------------------------------------------------------------------------------------------------ 4: bits
def test_a_graphs_bits_do_not_depend_on_the_batch_under_the_chain(chain, api):
    sizes = [2, 3, 40, 255, 256, 257, 600]
    others = [pc.ring_graph(n, 100 + n) for n in sizes]
    opt = api.pg_options(max_lm_iterations=8, max_pcg_iterations=150)
    alone = [chain.solve([g], opt) for g in others]
    batch = chain.solve(others, opt)
    back = chain.solve(others[::-1], opt)
    for k, n in enumerate(sizes):
        x1, r1 = alone[k][0][0], alone[k][1][0]
        assert x1.tobytes() == batch[0][k].tobytes() == back[0][len(sizes) - 1 - k].tobytes(), n
        assert rec_bytes(r1) == rec_bytes(batch[1][k]) == rec_bytes(back[1][len(sizes) - 1 - k]), n
        assert r1.lm_successes > 0 and r1.cost < r1.cost0 and r1.termination != 5, (n, r1.termination)
    assert chain.precond_stats()["factorisations"] == sum(r.lm_iterations for r in back[1])


def test_the_default_keeps_its_bits_across_a_switch(pg, api):
    graphs = [graph("chain_cm")[:2], graph("lap_2"), pc.ring_graph(257, 357)]
    opt = api.pg_options(max_lm_iterations=8, max_pcg_iterations=150)
    assert pg.preconditioner == api.PG_PRECOND_BLOCK_JACOBI
    x0, r0 = pg.solve(graphs, opt)
    c0, g0 = pg.evaluate(graphs)
    pg.set_preconditioner(api.PG_PRECOND_CHAIN)
    try:
        assert pg.preconditioner == api.PG_PRECOND_CHAIN
        x1, r1 = pg.solve(graphs, opt)
        c1, g1 = pg.evaluate(graphs)
    finally:
        pg.set_preconditioner(api.PG_PRECOND_BLOCK_JACOBI)
    x2, r2 = pg.solve(graphs, opt)
    c2, g2 = pg.evaluate(graphs)
    assert c0.tobytes() == c1.tobytes() == c2.tobytes()
    for k in range(len(graphs)):
        assert x0[k].tobytes() == x2[k].tobytes() and rec_bytes(r0[k]) == rec_bytes(r2[k]), k
        assert g0[k].tobytes() == g1[k].tobytes() == g2[k].tobytes(), k
    assert any(rec_bytes(a) != rec_bytes(b) for a, b in zip(r0, r1))   # the switch did switch


# ------------------------------------------------------------------------------------------------ 5: the switch
def test_a_bad_kind_is_refused_and_changes_nothing(pg, api):
    for start_kind in (api.PG_PRECOND_BLOCK_JACOBI, api.PG_PRECOND_CHAIN):
        pg.set_preconditioner(start_kind)
        try:
            for kind in (-1, 2, 7):
                assert pg.lib.ll_posegraphs_set_preconditioner(pg.h, kind) == -2
                assert "kind" in pg.lib.ll_posegraphs_last_error(pg.h).decode()
                assert pg.preconditioner == start_kind
                with pytest.raises(api.LightLoamError) as ei:
                    pg.set_preconditioner(kind)
                assert ei.value.code == -2
        finally:
            pg.set_preconditioner(api.PG_PRECOND_BLOCK_JACOBI)


def test_fixed_and_unconnected_nodes_come_back_bit_for_bit_under_the_chain(chain):
    _, start, edges = pc.noisy_chain("cm")
    poses = np.concatenate([start, [pc.random_pose(np.random.default_rng(3))]])         # node 40: free, no edge
    poses[17, :4] *= 1.0000001                                                          # a fixed node is not even normalised
    fixed = np.zeros(41, np.uint8); fixed[[0, 17, 33]] = 1
    x, rec = chain.solve([(poses, edges, fixed)])
    for k in (0, 17, 33, 40):
        assert x[0][k].tobytes() == poses[k].tobytes(), k
    moved = np.abs(x[0] - poses).max(axis=1) > 0
    assert moved[[k for k in range(40) if k not in (0, 17, 33)]].all() and rec[0].lm_successes > 0 and rec[0].cost < rec[0].cost0
    assert chain.precond_stats()["fallbacks"] == 0
    x, rec = chain.solve([(poses, edges, np.ones(41, np.uint8))])
    assert rec[0].lm_iterations == 0 and rec[0].lm_successes == 0 and x[0].tobytes() == poses.tobytes()
    assert chain.precond_stats() == {"factorisations": 0, "fallbacks": 0}
