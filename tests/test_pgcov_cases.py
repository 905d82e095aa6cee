"""The covariance restatement (tests/pgcovcases.py) against what is known without it, on the CPU: its closed-form Jacobians against the
central differences of posegraphcases, Sigma symmetric positive definite, the one closed-form covariance there is (two nodes), drift
along a loop-free chain and what a loop edge does to it, and the gate's two levels on the graphs the GPU tests gate."""
import numpy as np
import pytest

import pgchaincases as cc
import pgcovcases as cv
import posegraphcases as pc


@pytest.fixture(scope="module")
def solved_chain():
    """noisy_chain("cm") at the restatement's own optimum: (truth, poses, edges, Sigma)"""
    truth, start, edges = pc.noisy_chain("cm")
    x, gmax, _ = pc.dense_lm(start, edges)
    assert gmax < 1e-8
    return truth, x, edges, cv.sigma(x, edges)[0]


@pytest.mark.parametrize("name", ["two_node", "triangle", "chain", "star", "full"])
def test_closed_form_jacobians_against_central_differences(name):
    """posegraphcases.test line: atol 1e-9 on entries of size <= 6 (h = 1e-6: truncation h^2 and rounding eps / h, both relative to the
    entries); here relative to the largest entry of the pair, which reaches 1e3 on the star (weights up to 100, arms of 10 m)"""
    if name == "two_node":
        poses, edges, _ = pc.two_node()
    elif name == "triangle":
        poses, edges = pc.triangle()
    elif name == "chain":
        _, poses, edges = pc.noisy_chain("cm")
    elif name == "star":
        truth, edges = pc.star()
        poses = pc.perturbed(truth, np.random.default_rng(11), 0.3, np.deg2rad(5.0))
    else:
        poses, edges = pc.triangle()
        rng = np.random.default_rng(5)
        edges = [(e[0], e[1], e[2], rng.normal(size=(6, 6)), e[4]) for e in edges]
    worst = 0.0
    for e in edges:
        Pi, Pj = pc.normalized(poses[e[0]]), pc.normalized(poses[e[1]])
        Ji, Jj = cv.edge_jacobians(Pi, Pj, e)
        if np.ndim(e[3]) == 2:                                      # posegraphcases.residual takes diagonal weights: difference e, then S
            unit = (e[0], e[1], e[2], np.ones(6), e[4])
            Di, Dj = pc.edge_jacobians(Pi, Pj, unit)
            Di, Dj = e[3] @ Di, e[3] @ Dj
        else:
            Di, Dj = pc.edge_jacobians(Pi, Pj, e)
        scale = max(1.0, np.abs(Di).max(), np.abs(Dj).max())
        worst = max(worst, np.abs(Ji - Di).max() / scale, np.abs(Jj - Dj).max() / scale)
    print(f"{name}: worst |closed form - central difference| / max(1, max|J|) = {worst:.3g}")
    assert worst <= 1e-9


def test_the_error_is_the_unweighted_residual():
    poses, edges = pc.triangle()
    for e in edges:
        err, _, _ = cv.error_and_jacobians(poses[e[0]], poses[e[1]], e[2])
        want = pc.residual(pc.normalized(poses[e[0]]), pc.normalized(poses[e[1]]), e) / e[3]
        assert np.allclose(err, want, rtol=0, atol=1e-14)


@pytest.mark.parametrize("name", ["triangle", "chain_cm", "fixed", "star"])
def test_sigma_is_symmetric_positive_definite(name):
    if name == "triangle":
        poses, edges = pc.triangle(); fixed = None
    else:
        poses, edges, fixed = cc.graphs()[name]
    S, w = cv.sigma(poses, edges, fixed)
    fixed = pc.default_fixed(len(poses)) if fixed is None else np.asarray(fixed, bool)
    free = np.repeat(~fixed, 6)
    Sf = S[np.ix_(free, free)]
    assert w[0] > 0.0
    assert np.abs(Sf - Sf.T).max() <= 1e-12 * np.abs(Sf).max()
    assert np.linalg.eigvalsh(0.5 * (Sf + Sf.T))[0] > 0.0
    assert not S[~free].any() and not S[:, ~free].any()             # zeros at the fixed nodes


def test_two_node_has_the_closed_form():
    """one edge to a fixed node: H = J_j^T J_j, so S_bb = (J_j^T J_j)^-1 and the joint with the fixed node has nothing else"""
    poses, edges, _ = pc.two_node()
    S, _ = cv.sigma(poses, edges)
    _, Jj = cv.edge_jacobians(pc.normalized(poses[0]), pc.normalized(poses[1]), edges[0])
    want = np.linalg.inv(Jj.T @ Jj)
    assert np.allclose(S[6:, 6:], want, rtol=1e-12, atol=0)
    J = cv.joint(S, 0, 1)
    assert not J[:6].any() and not J[:, :6].any() and np.array_equal(J[6:, 6:], S[6:, 6:])
    assert np.array_equal(cv.joint(S, 1), cv.joint(S, 1, 1)) and not cv.joint(S, 1)[6:].any()
    Jba = cv.joint(S, 1, 0)
    assert np.array_equal(Jba[:6, :6], S[6:, 6:]) and not Jba[6:].any()


def test_drift_grows_along_a_chain_and_a_loop_edge_takes_it_back():
    """Along a loop-free chain S_(n+1)(n+1) = A S_nn A^T + Q with Q the edge's own covariance and A the unit-determinant map that carries
    node n's increment to node n + 1 (the rotation as it is, the translation plus the lever arm 2 w x (t_(n+1) - t_n)).  So the rotation
    block's trace and det S_nn grow strictly with n.  The plain trace of S_nn does not on this helix: the lever arm is measured from the
    fixed node, and the second half of the turn comes back towards it; it is asserted end against start.  A loop edge only adds
    information: every node's trace falls, the far end's by far the most"""
    start, edges = cc.loop_free_chain()
    n = len(start)
    S, _ = cv.sigma(start, edges)
    blocks = [S[6 * k:6 * k + 6, 6 * k:6 * k + 6] for k in range(n)]
    tr = np.array([np.trace(b) for b in blocks])
    rot = np.array([np.trace(b[:3, :3]) for b in blocks])
    logdet = np.array([np.linalg.slogdet(b)[1] for b in blocks[1:]])
    assert tr[0] == 0.0 and (np.diff(rot) > 0.0).all() and (np.diff(logdet) > 0.0).all()
    assert tr[-1] > 100.0 * tr[1]
    loop = pc.edge(n - 1, 0, pc.relative(start[n - 1], start[0]), (10.0,) * 6)
    S2, _ = cv.sigma(start, edges + [loop])
    tr2 = np.array([np.trace(S2[6 * k:6 * k + 6, 6 * k:6 * k + 6]) for k in range(n)])
    print(f"trace of S_nn at the far end: {tr[-1]:.4g} without the loop edge, {tr2[-1]:.4g} with it; at node 1: {tr[1]:.4g}")
    assert tr2[-1] < 0.1 * tr[-1] and (tr2[1:] < tr[1:]).all()


def test_the_gate_passes_a_true_closure_and_stops_the_false_loop(solved_chain):
    """The levels were fixed on the restatement alone.  A candidate measured from the truth, on the 40-node chain solved with cm noise:
    chi2 about 0.01, held below 5.35, the MEDIAN of chi-square(6) -- a consistent candidate must not look worse than half of all honest
    ones.  posegraphcases.false_loop, 5 m off: above the 0.999 quantile 22.46 against the graph's covariance alone (about 107) and with
    the edge's own information at s = 5 (a 0.2 m claim, what the odometry claims; about 70).  At s = 1 the edge itself claims a standard
    deviation of a metre and 5 m is chi2 = 17.5: an edge that vague is not refutable by 5 m, so that level is not a case"""
    truth, x, edges, S = solved_chain
    for a, b in ((20, 2), (35, 3), (10, 30)):
        Z = pc.relative(truth[a], truth[b])
        for info in (None, (1.0,) * 6, (10.0,) * 6):
            chi2, C = cv.gate(x[a], x[b], Z, info, cv.joint(S, a, b))
            assert np.linalg.eigvalsh(C)[0] > 0.0
            assert chi2 < 5.35, (a, b, info, chi2)
    fl = pc.false_loop(truth, s=5.0)
    J = cv.joint(S, fl[0], fl[1])
    with_info = cv.gate(x[fl[0]], x[fl[1]], fl[2], fl[3], J)[0]
    alone = cv.gate(x[fl[0]], x[fl[1]], fl[2], None, J)[0]
    print(f"false loop: chi2 {with_info:.4g} with its information, {alone:.4g} against the graph alone")
    assert with_info > cv.CHI2_6_999 and alone > with_info

