"""The numpy model of the trust-region step policy and the scripted scenarios of lmcases.py, checked on the CPU: every scenario
reaches exactly the branches it is named for (so that test_gpu_lm_steps.py cannot pass without the device taking them), with
every decision at least a factor 2 from its threshold; wrong policies are told apart by the scenarios meant for them; the model
solves a small analytic problem; and it agrees with the oracle's lm_core under three option sets."""
import numpy as np
import pytest

import lmcases as lc

SCENARIOS = lc.scenarios()


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_scenario_reaches_its_branches(name):
    sc = SCENARIOS[name]
    m, stages = lc.play(sc)
    print(name, m.log, [t["radius"] for t in m.trace], "kappa", [float("%.3g" % t["kappa"]) for t in m.trace])
    assert m.log == sc.branches
    if sc.radii is not None:
        assert np.allclose([t["radius"] for t in m.trace], sc.radii, rtol=1e-9, atol=0.0)
    for what, lhs, rhs in m.margins:                    # a factor 2 from every threshold (equality counts: 5e-4 against 1e-3)
        if rhs > 0.0 and np.isfinite(lhs):
            assert not 0.5 * (1 + 1e-6) < lhs / rhs < 2.0 * (1 - 1e-6), (what, lhs, rhs)
    for t in m.trace:                                   # well conditioned everywhere but in the min clamp
        assert t["kappa"] < (3e6 if name.startswith("clamp_min") else 20.0), t["kappa"]
    assert [s.branch for s in stages] == m.log


def _candidates(name, mutant=None):
    sc = SCENARIOS[name]
    m, stages = lc.play(sc, model=lc.LmModel(sc.opt, mutant))
    return m, [s for s in stages if s.branch == "candidate"]


def test_clamps_show_in_the_step():
    for mn, dz in ((1e-6, -1e-3), (1e-3, -1e-6)):
        m, c = _candidates(f"clamp_min_{mn:g}")
        assert c[0].tr["clamped"] == "min"
        assert abs(c[0].tr["d"][5] - dz) <= 1e-9 * abs(dz)
        assert abs((c[0].ref[6] - SCENARIOS[f"clamp_min_{mn:g}"].pose0[6]) - dz) <= 1e-9 * abs(dz) + 8 * lc.EPS
    on, off = _candidates("clamp_max_0.5_jacobi_1")[1][0], _candidates("clamp_max_0.5_jacobi_0")[1][0]
    assert on.tr["clamped"] == off.tr["clamped"] == "max"
    assert np.abs(on.ref - off.ref).max() > 1e6 * (lc.candidate_bound(on.tr, on.ref) + lc.candidate_bound(off.tr, off.ref))
    mid = _candidates("clamp_max_0.9_jacobi_1")[1][0]
    on, off = _candidates("clamp_max_1e+32_jacobi_1")[1][0], _candidates("clamp_max_1e+32_jacobi_0")[1][0]
    assert mid.tr["clamped"] == "" and lc.same_bits(mid.ref, on.ref) and _candidates("clamp_max_0.9_jacobi_0")[1][0].tr["clamped"] == "max"
    assert on.tr["clamped"] == off.tr["clamped"] == ""                          # diagonal damping is scale invariant
    assert np.abs(on.ref - off.ref).max() <= lc.candidate_bound(on.tr, on.ref) + lc.candidate_bound(off.tr, off.ref)


def test_scale_kept_sees_a_tenfold_diagonal():
    m, c = _candidates("scale_kept")
    sc = SCENARIOS["scale_kept"]
    ratio = np.diag(sc.steps[0].rec.H) / np.diag(sc.rec0.H)
    assert (ratio > 5).all() and (ratio < 20).all()
    assert c[1].tr["clamped"] == "max" and lc.same_bits(c[1].tr["scale"], c[0].tr["scale"])


def test_stops_are_the_ones_named():
    m, _ = lc.play(SCENARIOS["stop_function"])
    (_, diff, tol), = [x for x in m.margins if x[0] == "function"]
    assert diff / m.mcc > 2.0 * m.o["min_relative_decrease"]                    # rho would have accepted the candidate
    m, _ = lc.play(SCENARIOS["stop_parameter"])
    assert [x[0] for x in m.margins if x[0] == "function"] == []                # the function test was never reached ...
    sc = SCENARIOS["stop_parameter"]
    assert sc.steps[0].record(m).cost == sc.rec0.cost                           # ... and would have fired: the cost did not change
    m, _ = lc.play(SCENARIOS["plus_far_start_parameter_stop"])
    (_, step, tol), = [x for x in m.margins if x[0] == "parameter"]
    assert np.linalg.norm(m.x) > 1e3 and step > 2.0 * 1e-4 * (1.0 + 1e-4)       # |x| makes the stop: at |x| = 1 the step is no stop


def test_pose_composition_cases():
    m, c = _candidates("plus_large_rotation")
    assert 0.5 < np.linalg.norm(c[0].tr["d"][:3]) < 1.5
    assert abs(np.linalg.norm(c[0].ref[:4]) - 1.0) < 1e-14
    m, c = _candidates("plus_zero_rotation")
    assert (c[0].tr["d"][:3] == 0.0).all() and (c[0].tr["d"][3:] != 0.0).all()
    assert lc.same_bits(c[0].ref[:4], SCENARIOS["plus_zero_rotation"].pose0[:4])
    # Plus against an independent statement: the rotation matrix of q+ is that of the increment times that of q, and the
    # increment [sin|w| w/|w|, cos|w|] turns by 2 |w| about w
    rng = np.random.default_rng(3)
    x = lc._pose(rng); d = rng.standard_normal(6)
    y = lc.plus(x, d)
    w = d[:3]; n = np.linalg.norm(w); k = w / n
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    Rw = np.eye(3) + np.sin(2 * n) * K + (1 - np.cos(2 * n)) * K @ K
    assert np.abs(_rotmat(y[:4]) - Rw @ _rotmat(x[:4])).max() < 1e-14 and lc.same_bits(y[4:], x[4:] + d[3:])


@pytest.mark.parametrize("mutant", list(lc.MUTANTS))
def test_wrong_policies_are_told_apart(mutant):
    """each wrong policy of lmcases.MUTANTS gives, on the scenarios meant for it, another branch sequence or a pose further
    from the right one than 1000 times the bound test_gpu_lm_steps.py allows the device"""
    for name in lc.MUTANTS[mutant]:
        sc = SCENARIOS[name]
        right, a = lc.play(sc)
        wrong, b = lc.play(sc, model=lc.LmModel(sc.opt, mutant))
        if wrong.log != right.log:
            continue
        far = False
        for s, w in zip(a, b):
            bound = lc.candidate_bound(s.tr, s.ref) if s.tr is not None and s.branch == "candidate" else 8 * lc.EPS * np.abs(s.ref).max()
            far = far or np.abs(s.ref - w.ref).max() > 1000.0 * bound
        assert far, (mutant, name)


def _rotmat(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _point_problem():
    """twelve point-to-point residuals R(q) p_i + t - y_i with y from a known transform.  The increment of Plus turns by 2 |w|
    about w, so d(R p)/dw = -2 [R p]x"""
    rng = np.random.default_rng(12)
    P = 2.0 * rng.standard_normal((12, 3))
    truth = lc.plus(np.array([0, 0, 0, 1.0, 0, 0, 0]), np.array([0.2, -0.15, 0.25, 0.7, -0.4, 0.3]))
    Y = P @ _rotmat(truth[:4]).T + truth[4:]

    def residuals(x):
        return (P @ _rotmat(x[:4]).T + x[4:] - Y).ravel()

    def evaluate(x):
        Rp = P @ _rotmat(x[:4]).T
        J = np.zeros((36, 6))
        for i, v in enumerate(Rp):
            J[3 * i:3 * i + 3, :3] = -2.0 * np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])
            J[3 * i:3 * i + 3, 3:] = np.eye(3)
        return lc.Record.from_jacobian(J, residuals(x))
    return truth, residuals, evaluate


def test_model_solves_an_analytic_problem():
    truth, residuals, evaluate = _point_problem()
    x0 = np.array([0, 0, 0, 1.0, 0, 0, 0])
    J = evaluate(x0).J                                  # the analytic Jacobian against central differences through Plus
    for k in range(6):
        e = np.zeros(6); e[k] = 1e-6
        fd = (residuals(lc.plus(x0, e)) - residuals(lc.plus(x0, -e))) / 2e-6
        assert np.abs(fd - J[:, k]).max() < 1e-8
    x, m = lc.solve(evaluate, x0, lc.options(max_num_iterations=50))
    print(m.log, m.costs)
    assert (np.diff(m.costs) < 0).all() and m.successes >= 3
    assert m.log[-1].startswith("stop:") and m.log[-1] != "stop:max_iterations"
    assert np.abs(x - truth).max() < 1e-8 and m.costs[-1] < 1e-16 * m.costs[0]


ORACLE_SETS = {"defaults": ({}, None), "all_reject": (dict(min_relative_decrease=10.0), (4, 0)), "function_stop": (dict(function_tolerance=1.0), (1, 0))}


@pytest.mark.parametrize("name", list(ORACLE_SETS))
def test_model_agrees_with_the_oracle(orc, synth, name):
    from test_oracle import _pair
    kw, summary = ORACLE_SETS[name]
    opt = lc.options(**kw)
    cfg, e0, e1 = _pair(orc, synth)
    q = np.array([0, 0, 0, 1.0]); t = np.array([0.5, 0.1, 0.0])
    es, ea, eb = orc.associate_corner(q, t, e1["sharp"], e0["less_sharp"])
    ps, pa, pb, pc = orc.associate_plane(q, t, e1["flat"], e0["less_flat"])
    args = (e1["sharp"], es, e0["less_sharp"], ea, eb, e1["flat"], ps, e0["less_flat"], pa, pb, pc, np.ones(len(ps), np.float32))

    def evaluate(x):
        H, g, cost = orc.normal_equations(x[:4], x[4:], *args)
        return lc.Record(H, g, cost, 3 * len(es) + len(ps))
    x, m = lc.solve(evaluate, np.concatenate([q, t]), opt)
    qo, to, summ = orc.lm_solve(q, t, *args, opt=lc.fill(orc.lm_options(), opt))
    print(name, m.log, summ)
    assert np.abs(x[:4] - qo).max() < 1e-9 and np.abs(x[4:] - to).max() < 1e-9
    assert (m.iterations, m.successes) == (int(summ[2]), int(summ[3]))
    assert abs(m.costs[-1] - summ[1]) <= 1e-9 * summ[0]
    if summary is not None:
        assert (m.iterations, m.successes) == summary and lc.same_bits(x, np.concatenate([q, t])) and lc.same_bits(np.concatenate([qo, to]), x)
    else:
        assert m.successes >= 1 and "accept" in m.log
