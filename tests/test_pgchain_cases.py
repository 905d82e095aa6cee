"""The chain preconditioner's restatement on its own (tests/pgchaincases.py, no device): on every graph the GPU tests use, M is symmetric
positive definite, is the block-tridiagonal part of A in node order and is A itself on a loop-free chain; A - M has rank at most 12 per
other edge; preconditioned conjugate gradients with M stay within 12 L + 1 iterations at eta = 1e-6 (1 on the loop-free chain) and well
below block-Jacobi on the laps; the random block-tridiagonal systems have the condition numbers the GPU test's bound assumes.  So the
conditions the GPU tests put on the library hold for the reference alone."""
import numpy as np
import pytest

import pgchaincases as cc

ETA = 1e-6
_SYS = {}


def system(name):
    """(A, M, b, fixed, L) of a graph at its start and the initial radius, computed once"""
    if name not in _SYS:
        if "graphs" not in _SYS:
            _SYS["graphs"] = cc.graphs()
        start, edges, fixed = _SYS["graphs"][name]
        A, M = cc.chain_matrix(start, edges, fixed)
        _SYS[name] = (A, M, cc.right_hand_side(start, edges, fixed), fixed, cc.other_edges(edges, fixed))
    return _SYS[name]


def test_the_graphs_are_the_ones_listed():
    g = cc.graphs()
    assert tuple(g) == cc.GRAPH_NAMES + cc.COUNT_NAMES
    L = {k: cc.other_edges(v[1], v[2]) for k, v in g.items()}
    assert (L["lap257_1"], L["lap257_2"]) == (1, 2) == (cc.LOOPS["lap257_1"], cc.LOOPS["lap257_2"])
    assert (L["lap_1"], L["lap_2"], L["loop_free"], L["reversed"], L["chain_cm"], L["chain_huber"], L["doubled"]) == (1, 2, 0, 0, 2, 3, 2)
    assert L["fixed"] == 2                                           # the loop 39 -> 0 ends at a fixed node in all of them: no off-diagonal block
    assert any(e[0] == e[1] + 1 for e in g["reversed"][1]) and any(e[0] + 1 == e[1] for e in g["reversed"][1])
    assert len(g["doubled"][1]) == len(g["chain_cm"][1]) + 39
    assert g["fixed"][2].nonzero()[0].tolist() == list(cc.FIXED_NODES)
    assert sum(1 for e in g["star"][1] if abs(e[0] - e[1]) == 1) == 1 and L["star"] == 0          # every edge of the star touches node 0, fixed
    assert len(g["lap_1"][0]) == cc.LAP_NODES and len(g["lap257_1"][0]) == len(g["lap257_2"][0]) == 257


@pytest.mark.parametrize("name", cc.GRAPH_NAMES + cc.COUNT_NAMES)
def test_m_is_spd_and_the_tridiagonal_part_of_a(name):
    A, M, b, fixed, L = system(name)
    scale = np.abs(A).max()
    assert np.abs(M - M.T).max() <= 1e-13 * scale
    w = np.linalg.eigvalsh(0.5 * (M + M.T))
    print(f"{name}: {len(b)} unknowns, L {L}, eigenvalues of M {w[0]:.3g} .. {w[-1]:.3g}")
    assert w[0] > 0.0
    assert np.abs(M - cc.tridiagonal_part(A, fixed)).max() <= 1e-12 * scale
    if L == 0:
        assert np.abs(M - A).max() <= 1e-12 * scale
    rank = np.linalg.matrix_rank(A - M, tol=1e-10 * scale)
    print(f"{name}: rank(A - M) {rank}, bound {12 * L}")
    assert rank <= 12 * L


@pytest.mark.parametrize("name", cc.GRAPH_NAMES + cc.COUNT_NAMES)
def test_pcg_with_m_stays_within_the_rank_bound(name):
    A, M, b, fixed, L = system(name)
    k = cc.pcg_count(A, M, b, ETA)
    print(f"{name}: PCG iterations with M {k}, bound {12 * L + 1}")
    assert k <= 12 * L + 1
    if L == 0:
        assert k == 1


@pytest.mark.parametrize("name", cc.COUNT_NAMES)
def test_block_jacobi_needs_more_on_a_lap(name):
    A, M, b, fixed, L = system(name)
    BJ = np.zeros_like(A)
    for k in range(len(b) // 6):
        BJ[6 * k:6 * k + 6, 6 * k:6 * k + 6] = A[6 * k:6 * k + 6, 6 * k:6 * k + 6]
    kj, kc = cc.pcg_count(A, BJ, b, ETA), cc.pcg_count(A, M, b, ETA)
    print(f"{name}: block-Jacobi {kj}, chain {kc}")
    assert kc < kj


def test_dense_solve_and_the_condition_number_agree_with_numpy():
    diag, upper, cond = cc.random_system(9, 5)
    M = cc.dense_of(diag, upper)
    assert cond == pytest.approx(np.linalg.cond(M), rel=1e-6)
    b = np.random.default_rng(1).normal(size=54)
    assert np.abs(M @ cc.dense_solve(M, b) - b).max() <= 1e-9 * np.abs(b).max()
    lower = cc.condition_number(diag, upper, dense_limit=0)          # the iteration's figure never exceeds the condition number
    assert 0.5 * cond <= lower <= cond * (1 + 1e-9)
    assert np.allclose(cc._thomas(diag, upper, b.reshape(9, 6)).reshape(-1), cc.dense_solve(M, b), rtol=0, atol=1e-9 * np.abs(b).max() * cond)


@pytest.mark.parametrize("n", [1, 2, 9, 257, 1000])
def test_random_systems_are_well_enough_conditioned(n):
    diag, upper, cond = cc.random_system(n, 100 + n)
    print(f"N {n}: cond {cond:.3g}")
    assert 1.0 <= cond <= 1e6
    assert not upper[-1].any()
