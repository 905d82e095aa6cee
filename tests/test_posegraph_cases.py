"""The numpy restatement of tests/posegraphcases.py against closed forms, without a GPU: it is what test_gpu_posegraphs.py measures the
kernels with, so its conventions, its central-difference Jacobian and its dense LM are pinned here first."""
import numpy as np
import pytest

import posegraphcases as pc


def test_plus_is_the_left_half_angle_update_of_ll_pose_plus():
    """q <- exp(d) (x) q with d the HALF-angle vector.  By hand: a quarter turn about x, then d = (0, 0, pi / 4) -- a quarter turn about z
    applied on the LEFT -- is (1/2, 1/2, 1/2, 1/2); on the right it would be (1/2, -1/2, 1/2, 1/2).  Translation is added."""
    s = np.sqrt(0.5)
    got = pc.plus(np.array([s, 0, 0, s, 1.0, 2.0, 3.0]), np.array([0, 0, np.pi / 4, 0.5, -0.25, 4.0]))
    assert np.allclose(got, [0.5, 0.5, 0.5, 0.5, 1.5, 1.75, 7.0], rtol=0, atol=1e-15)
    assert pc.plus(np.array([s, 0, 0, s, 1.0, 2.0, 3.0]), np.zeros(6)).tolist() == [s, 0, 0, s, 1.0, 2.0, 3.0]


def test_residual_by_hand():
    """P_i = identity, P_j = a turn of 0.2 rad about z at (1, 2, 3), Z = identity: r = s o [2 sin(0.1) e_z ; (1, 2, 3)]; the opposite sign
    of the error quaternion gives the same residual"""
    Pi = np.array([0, 0, 0, 1.0, 0, 0, 0]); Pj = np.concatenate([pc.axis_angle([0, 0, 1], 0.2), [1.0, 2.0, 3.0]])
    e = pc.edge(0, 1, Pi, (1, 2, 3, 4, 5, 6))
    want = np.array([0, 0, 3 * 2 * np.sin(0.1), 4, 10, 18])
    assert np.allclose(pc.residual(Pi, Pj, e), want, rtol=0, atol=1e-14)
    assert np.allclose(pc.residual(Pi, Pj * np.array([-1, -1, -1, -1, 1, 1, 1]), e), want, rtol=0, atol=1e-14)
    Ji, Jj = pc.edge_jacobians(Pi, Pi, e)                           # at the identity: d r / d (w_j, t_j) = S diag(2, 2, 2, 1, 1, 1)
    assert np.allclose(Jj, np.diag([2, 4, 6, 4, 5, 6]), rtol=0, atol=1e-9) and np.allclose(Ji, -Jj, rtol=0, atol=1e-9)


def test_huber_is_ceres_huber_loss():
    assert pc.huber(0.2, 0.5) == (0.2, 1.0) and pc.huber(9.0, 0.0) == (9.0, 1.0)
    rho, rho1 = pc.huber(4.0, 0.5)                                  # |r| = 2: 2 a |r| - a^2, a / |r|
    assert rho == 1.75 and rho1 == 0.25


def test_two_nodes_solve_to_p0_z():
    start, edges, Z = pc.two_node()
    x, gmax, _ = pc.dense_lm(start, edges)
    assert gmax < 1e-12
    want = pc.compose(pc.normalized(start[0]), Z)
    assert np.allclose(x[1], want, rtol=0, atol=1e-12) and x[0].tolist() == pc.normalized(start[0]).tolist()


def test_a_consistent_graph_rests_at_the_truth():
    truth, start, edges = pc.consistent_chain()
    assert pc.cost(truth, edges) < 1e-28
    assert np.abs(pc.gradient(truth, edges)).max() < 1e-12
    assert pc.cost(start, edges) > 1.0 and np.abs(pc.gradient(start, edges)).max() > 1.0
    assert pc.gradient(start, edges)[0].tolist() == [0.0] * 6       # the fixed node


def test_the_dense_lm_converges_on_the_noisy_chains():
    """The GPU tests take this solve as their reference.  At measurement noise of 1e-5 the LM meets its own stopping rule, a gradient
    max-norm below 1e-12.  At centimetre noise that rule is out of reach of ANY graph with residuals that do not vanish: a central
    difference with h = 1e-6 of a translation of up to 4 m carries a rounding of ulp(4) / 2h = 4.4e-10 per Jacobian entry, which the
    weighted residuals (s^2 |e| <= 225 x 0.03) turn into a gradient noise of about 3e-9 per term.  The LM then stops where its steps fall
    below the rounding of the poses; 1e-8 bounds that floor.  H's smallest eigenvalue (checked below) says how far such a gradient can
    leave the poses from the exact optimum in the worst direction; the GPU test measures the distance between this solve and the
    kernel's, whose Jacobians are closed forms, against the 1e-7 it has to meet."""
    _, start, edges = pc.noisy_chain("tiny")
    x, gmax, it = pc.dense_lm(start, edges)
    assert gmax < 1e-12 and it < 50
    _, start, edges = pc.noisy_chain("cm")
    x, gmax, it = pc.dense_lm(start, edges)
    assert gmax < 1e-8 and it < 100
    H = pc.linearize(x, edges)[2]
    assert np.linalg.eigvalsh((H.T @ H)[6:, 6:]).min() > 0.05


def test_the_false_loop_is_an_outlier_of_the_huber_chain():
    truth, start, edges = pc.huber_chain()
    r = pc.residual(truth[edges[-1][0]], truth[edges[-1][1]], edges[-1])
    assert edges[-1][4] == 0.5 and abs(np.linalg.norm(r) - 5.0) < 1e-9
    assert len(edges) == 39 + 3 + 1


@pytest.mark.parametrize("n", [2, 3, 40, 257])
def test_ring_graphs_are_valid(n):
    start, edges = pc.ring_graph(n, n)
    assert start.shape == (n, 7) and len(edges) == (n if n > 2 else 1)
    assert all(0 <= e[0] < n and 0 <= e[1] < n and e[0] != e[1] for e in edges)
