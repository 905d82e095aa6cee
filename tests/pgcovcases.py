"""An independent numpy restatement of ll_posegraphs_covariances and ll_pg_edge_gate.  Nothing here comes from the library: the edge
Jacobians are closed forms written with rotation matrices (the kernel builds its rotation block column by column from quaternion
products), H is the dense J^T J, Sigma is numpy.linalg.inv of its free part padded with zeros at the fixed nodes, and the gate is the
textbook Mahalanobis distance.

Why closed forms and not posegraphcases.edge_jacobians: those are central differences with a relative error near 1e-10, and an error
of H enters H^-1 times cond(H) -- it would swamp the comparison with the device at the condition numbers of these graphs.

The tangent is the increments' own: per node d = (w, dt), q <- exp(w) (x) q with w the HALF-angle vector, t <- t + dt.  With
E = Z^-1 P_i^-1 P_j = (q_e, t_e), q_e = (v_e, w_e), a = q_z* (x) q_i*, R_a = R(a) = R(q_z)^T R(q_i)^T and v = t_j - t_i:
    q_j <- [w, 1] (x) q_j changes q_e by a (x) [w, 0] (x) q_j = [R_a w, 0] (x) q_e, whose vector part is w_e (R_a w) + (R_a w) x v_e:
        d e_rot / d w_j = 2 sgn(w_e) (w_e I - [v_e]x) R_a = A,      d e_rot / d w_i = -A,
    t_e = R_a v - R(q_z)^T t_z:   d t_e / d t_j = R_a,  d t_e / d t_i = -R_a,  and R(q_i)^T <- R(q_i)^T (I - 2 [w]x):  d t_e / d w_i = 2 R_a [v]x."""
import numpy as np

import posegraphcases as pc

CHI2_6_999 = 22.46                                                  # the 0.999 quantile of chi-square with 6 degrees of freedom


def skew(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def error_and_jacobians(Pi, Pj, Z):
    """(e [6], Je_i [6, 6], Je_j [6, 6]): the UNWEIGHTED error of the edge and its Jacobians; poses and Z are normalised here"""
    Pi = pc.normalized(Pi); Pj = pc.normalized(Pj); Z = pc.normalized(Z)
    E = pc.compose(pc.inverse(Z), pc.relative(Pi, Pj))
    sgn = 1.0 if E[3] >= 0.0 else -1.0
    e = np.concatenate([2.0 * sgn * E[:3], E[4:]])
    Ra = pc.qmat(Z[:4]).T @ pc.qmat(Pi[:4]).T
    A = 2.0 * sgn * (E[3] * np.eye(3) - skew(E[:3])) @ Ra
    v = Pj[4:] - Pi[4:]
    Ji = np.zeros((6, 6)); Jj = np.zeros((6, 6))
    Ji[:3, :3] = -A; Jj[:3, :3] = A
    Ji[3:, :3] = 2.0 * Ra @ skew(v); Ji[3:, 3:] = -Ra; Jj[3:, 3:] = Ra
    return e, Ji, Jj


def weight_matrix(s):
    s = np.asarray(s, float)
    return s.reshape(6, 6) if s.size == 36 else np.diag(s)


def edge_jacobians(Pi, Pj, edge):
    """(J_i, J_j) of the weighted residual r = S e, without the Huber scale: what posegraphcases.edge_jacobians differentiates"""
    _, Ji, Jj = error_and_jacobians(Pi, Pj, edge[2])
    S = weight_matrix(edge[3])
    return S @ Ji, S @ Jj


def dense_H(poses, edges, fixed=None):
    """(H [6 N, 6 N] with zero rows and columns at fixed nodes, free [6 N] bool): J^T J with the Huber scale, no damping"""
    poses = [pc.normalized(p) for p in poses]
    n = len(poses)
    fixed = pc.default_fixed(n) if fixed is None else np.asarray(fixed, bool)
    J = np.zeros((6 * len(edges), 6 * n))
    for k, ed in enumerate(edges):
        i, j = ed[0], ed[1]
        e, Ji, Jj = error_and_jacobians(poses[i], poses[j], ed[2])
        S = weight_matrix(ed[3])
        r = S @ e
        w = np.sqrt(pc.huber(float(r @ r), ed[4])[1])
        if not fixed[i]:
            J[6 * k:6 * k + 6, 6 * i:6 * i + 6] = w * (S @ Ji)
        if not fixed[j]:
            J[6 * k:6 * k + 6, 6 * j:6 * j + 6] = w * (S @ Jj)
    return J.T @ J, np.repeat(~fixed, 6)


def sigma(poses, edges, fixed=None):
    """(Sigma [6 N, 6 N], eigenvalues of H_free ascending): inv(H_free) padded with zeros at the fixed nodes"""
    H, free = dense_H(poses, edges, fixed)
    ix = np.ix_(free, free)
    Hf = H[ix]
    S = np.zeros_like(H)
    S[ix] = np.linalg.inv(Hf)
    return S, np.linalg.eigvalsh(Hf)


def joint(Sigma, a, b=-1):
    """the 12 x 12 [[S_aa, S_ab], [S_ba, S_bb]]; b < 0 or b == a: S_aa in the top-left block, zeros elsewhere"""
    out = np.zeros((12, 12))
    ia = slice(6 * a, 6 * a + 6)
    out[:6, :6] = Sigma[ia, ia]
    if b >= 0 and b != a:
        ib = slice(6 * b, 6 * b + 6)
        out[:6, 6:] = Sigma[ia, ib]; out[6:, :6] = Sigma[ib, ia]; out[6:, 6:] = Sigma[ib, ib]
    return out


def gate(Pa, Pb, Z, S, joint144):
    """(chi2, C): e^T C^-1 e with C = J Sigma J^T + (S^T S)^-1 (no second term for S None) of the candidate edge a -> b"""
    e, Ja, Jb = error_and_jacobians(Pa, Pb, Z)
    J = np.hstack([Ja, Jb])
    Cm = J @ np.asarray(joint144, float).reshape(12, 12) @ J.T
    if S is not None:
        W = weight_matrix(S)
        Cm = Cm + np.linalg.inv(W.T @ W)
    return float(e @ np.linalg.solve(Cm, e)), Cm


def bound(eigenvalues, tolerance, eps=np.finfo(np.float64).eps):
    """the accuracy a device column may be held to: (tolerance + 100 eps cond(H)) ||H^-1||_2.  The stop rule |r| <= tolerance gives
    |x - x*| <= ||H^-1|| |r|; 100 eps cond is the rounding margin the chain solver's tests already grant"""
    cond = eigenvalues[-1] / eigenvalues[0]
    return (tolerance + 100.0 * eps * cond) / eigenvalues[0], cond
