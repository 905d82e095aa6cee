"""The trust-region step policy on the device, branch by branch.

(a) The stepwise kernels (k_lm_begin, k_lm_propose, k_lm_accept through ll_map_lm_begin / ll_map_lm_propose / ll_map_lm_accept)
    on the scripted records of lmcases.py, the pose read back after every call: bit for bit where the policy leaves or restores
    x (a stop, an invalid step, a rejection), the accepted pose bit for bit the candidate read after the propose, and a
    candidate within 64 eps kappa |d|_inf + 8 eps |pose|_inf of the numpy model's (lmcases.candidate_bound).  test_lm_cases.py
    shows on the CPU that every scenario reaches the branches it is named for.
(b) The fused kernels under options that force the same branches: Map.solve (k_map_lm_solve) against the stepwise calls bit for
    bit, ll_lm_solve_batch (k_lm_solve) against the oracle, ll_odometry_sequences (k_vote_lm_rows) against ll_odometry_frames
    bit for bit -- with the numpy model replaying the evaluated records as the witness that the branch was taken.
"""
import numpy as np
import pytest

import lmcases as lc

pytestmark = pytest.mark.gpu

SCENARIOS = lc.scenarios()


def _opt(api, opt):
    return lc.fill(api.LmOptions(), opt)


@pytest.fixture(scope="module")
def rig(api):
    ctx = api.Context(api.default_params(16, batch=1, max_points=4096))
    m = api.Map(ctx, 1, 1, 1, 1)                       # the smallest capacities ll_map_create accepts: no cloud is needed
    yield api, ctx, m
    m.close(); ctx.close()


# ----------------------------------------------------------------------------- (a) the stepwise kernels, every scenario
@pytest.mark.parametrize("name", list(SCENARIOS))
def test_stepwise_kernels_follow_the_policy(rig, name):
    api, ctx, m = rig
    sc = SCENARIOS[name]
    model, stages = lc.play(sc, m, _opt(api, sc.opt))
    assert model.log == sc.branches                    # the model took the scenario's branches with the device's poses as well
    worst = lc.check_stages(sc, stages)
    print(f"{name}: largest candidate error / bound = {worst:.3g}")


def test_begin_resets_what_a_stopped_solve_left(rig):
    """stop_min_radius leaves the done flag set, the decrease factor at 8 and the radius at 1/8; set_pose and lm_begin on the
    same map then give, call by call, what a fresh map gives"""
    api, ctx, m = rig
    first, again = SCENARIOS["stop_min_radius"], SCENARIOS["after_restart"]
    lc.check_stages(first, lc.play(first, m, _opt(api, first.opt))[1])
    _, used = lc.play(again, m, _opt(api, again.opt))
    fresh_map = api.Map(ctx, 1, 1, 1, 1)
    _, fresh = lc.play(again, fresh_map, _opt(api, again.opt))
    fresh_map.close()
    lc.check_stages(again, fresh)
    assert [s.branch for s in used] == [s.branch for s in fresh] == again.branches
    for k, (a, b) in enumerate(zip(used, fresh)):
        assert lc.same_bits(a.got, b.got), (k, a.call, a.got, b.got)


# ----------------------------------------------------------------------------- (b) Map.solve against the stepwise calls
@pytest.fixture(scope="module")
def map_scene(api):
    """the smallest scene of test_gpu_map_neq_paths.py (half = 1.2: fewer than 256 edge and plane blocks), associated once"""
    from test_gpu_map_neq_paths import LINE_RES, PLANE_RES, T_TRUE, _apply, _inverse, _scene
    half = 1.2
    rng = np.random.default_rng(int(half * 10))
    r = 0.5 * half + 0.07
    map_c, map_s = [g.astype(np.float32) for g in _scene(rng, half + 2.0, 0.0, r)]
    Ti = _inverse(T_TRUE)
    scan_c, scan_s = [np.concatenate([_apply(Ti, g[:, :3]), g[:, 3:]], 1).astype(np.float32) for g in _scene(rng, half, 0.13, r)]
    pose0 = T_TRUE.copy()
    pose0[4:] += (0.10, -0.08, 0.05)
    ctx = api.Context(api.default_params(16, batch=1, max_points=4096))
    many = api.CubeMaps(ctx, 1, len(map_c) + 64, len(map_s) + 64, pool_points=1 << 16, line_res=LINE_RES, plane_res=PLANE_RES)
    _, ran = many.process(np.array([[0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]]), [map_c], [map_s])
    assert not ran[0]
    _, ran = many.process(pose0[None, :], [scan_c], [scan_s])
    assert ran[0]
    cl = [many.cloud(0, w) for w in range(4)]
    m = api.Map(ctx, len(cl[0]), len(cl[1]), len(cl[2]), len(cl[3]))
    m.set_map(cl[0], cl[1])
    m.set_scan(cl[2], cl[3])
    m.associate(pose0)
    ne, npl = m.counts()
    assert 1 <= ne <= 255 and 1 <= npl <= 255, (ne, npl)
    yield m, pose0
    m.close(); many.close(); ctx.close()


def _stepwise(m, pose, o, n_it):
    """test_gpu_map_neq_paths._stepwise under options, keeping what it evaluated"""
    m.set_pose(pose)
    records = [m.evaluate()]
    m.lm_begin(records[0], o)
    for _ in range(n_it):
        m.lm_propose(o)
        records.append(m.evaluate())
        m.lm_accept(records[-1], o)
    return m.pose(), records


# option set -> what the model's replay of the evaluated records must show
MAP_SETS = {
    "defaults": (dict(), lambda m: "accept" in m.log),
    "all_reject": (dict(min_relative_decrease=10.0), lambda m: m.log.count("reject") == 4 and m.successes == 0),
    # radius 1e-3, 5e-4, 1.25e-4 over three rejections, then 1.6e-5 < min_radius at the fourth propose
    "min_radius": (dict(initial_radius=1e-3, min_radius=1e-4, min_relative_decrease=10.0),
                   lambda m: m.log[-2:] == ["stop:min_radius", "done"] and m.log.count("reject") == 3),
    # the same radii without the forced rejections: small damped steps, all good ones
    "small_radius": (dict(initial_radius=1e-3, min_radius=1e-4), lambda m: "accept" in m.log and all(t["radius"] < 1.0 for t in m.trace)),
    "function_stop": (dict(function_tolerance=0.5), lambda m: "stop:function" in m.log),
    "clamp_max": (dict(max_lm_diagonal=0.5), lambda m: "accept" in m.log and all(t["clamped"] == "max" for t in m.trace)),
    "no_jacobi_scaling": (dict(jacobi_scaling=0), lambda m: "accept" in m.log and all((t["scale"] == 1.0).all() for t in m.trace)),
}


@pytest.mark.parametrize("name", list(MAP_SETS))
def test_map_solve_takes_the_stepwise_branches(api, map_scene, name):
    from test_gpu_map_neq_paths import _same
    m, pose0 = map_scene
    kw, shows = MAP_SETS[name]
    opt = lc.options(**kw)
    o = _opt(api, opt)
    a = m.solve(pose0, o)                                          # k_map_lm_solve
    b, records = _stepwise(m, pose0, o, opt["max_num_iterations"])
    model = lc.replay(opt, pose0, records)
    print(name, model.log, [t["radius"] for t in model.trace], a)
    assert not np.isnan(a).any()
    assert _same(a, b), (a, b)
    assert shows(model), model.log                                 # the branch this option set is here for
    assert np.abs(model.x - b).max() < 1e-9
    if model.successes == 0:
        assert _same(a, pose0)
    else:
        assert not _same(a, pose0)


# ----------------------------------------------------------------------------- (b) ll_lm_solve_batch against the oracle
def test_lm_solve_under_options_matches_the_oracle(api, orc, synth):
    """the pair of test_gpu_odometry.test_lm_solve_parity_single_pair: all steps rejected, a function stop at the first step
    (both leave the input pose, bit for bit), and a solve from initial_radius = 1"""
    cfg = synth.default_cfg(16)
    scans = [synth.scan(cfg, k) for k in range(2)]
    P = orc.params(16)
    e0, e1 = orc.extract(scans[0], P), orc.extract(scans[1], P)
    pose = np.array([0.0, 0.0, 0.0, 1.0, 0.5, 0.1, 0.0])
    q, t = pose[:4], pose[4:]
    es, ea, eb = orc.associate_corner(q, t, e1["sharp"], e0["less_sharp"])
    ps, pa, pb, pc = orc.associate_plane(q, t, e1["flat"], e0["less_flat"])
    cnt, sidx, sw = orc.vote(e1["flat"][ps], e0["less_flat"][pa])
    order = np.sort(sidx); wmap = np.ones(len(ps), np.float32); wmap[sidx] = sw
    args = (e1["sharp"], es, e0["less_sharp"], ea, eb, e1["flat"], ps[order], e0["less_flat"], pa[order], pb[order], pc[order], wmap[order])
    ctx = api.Context(api.default_params(16, batch=2, max_points=max(map(len, scans))))
    ctx.upload_scan(0, scans[0]); ctx.upload_scan(1, scans[1])
    ctx.extract(0, 2)
    ctx.set_target_from_slot(0)
    got, ref = {}, {}
    sets = {"all_reject": dict(min_relative_decrease=10.0), "function_stop": dict(function_tolerance=1.0), "radius_1": dict(initial_radius=1.0)}
    for name, kw in sets.items():
        opt = lc.options(**kw)
        ctx.associate(1, 1, pose)
        ctx.vote(1, 1, True)
        ctx.lm_solve(1, 1, _opt(api, opt))
        got[name] = ctx.pose(1)
        qo, to, summ = orc.lm_solve(q, t, *args, opt=lc.fill(orc.lm_options(), opt))
        ref[name] = (np.concatenate([qo, to]), summ)
        print(name, got[name], summ)
    ctx.close()
    assert tuple(ref["all_reject"][1][2:4]) == (4, 0) and tuple(ref["function_stop"][1][2:4]) == (1, 0)
    for name in ("all_reject", "function_stop"):
        assert lc.same_bits(got[name], pose) and lc.same_bits(ref[name][0], pose), name
    x, summ = ref["radius_1"]
    assert summ[3] >= 1 and summ[1] < summ[0]
    assert np.abs(got["radius_1"] - x).max() < 1e-9
    assert np.abs(x - pose).max() > 1e-3                           # and it moved


# ----------------------------------------------------------------------------- (b) ll_odometry_sequences against ll_odometry_frames
def test_sequences_equal_the_single_sequence_loop_under_rejections(api, orc, synth):
    """two sequences of four frames with min_relative_decrease = 1.2.  The Huber-weighted Gauss-Newton model underestimates
    the decrease here (rho 1.3 .. 1.7 at the first steps, nearer 1 for the short steps after a rejection), so sequence 0 takes
    some steps and rejects others and sequence 1 rejects all of its: the model, run as the solver of the oracle's frame loop,
    says so, with rho no nearer than 1e-3 to the threshold.  Compared as test_gpu_sequences.py compares at the defaults."""
    from test_gpu_sequences import drives, lockstep_ctx, pair_counts
    rings, n_seq, n_frames = 16, 2, 4
    opt = lc.options(min_relative_decrease=1.2)
    o = _opt(api, opt)
    _, scans, pose0 = drives(synth, rings, n_seq, n_frames)
    ctx, L = lockstep_ctx(api, rings, scans, n_frames)
    rel = ctx.odometry_sequences(n_seq, n_frames, 1, n_frames - 1, pose0=pose0, opt=o)
    counts = [pair_counts(ctx, L, range(1, n_frames), q) for q in range(n_seq)]
    ctx.close()
    assert rel.shape == (n_frames - 1, n_seq, 7)
    P = orc.params(rings)
    for q in range(n_seq):
        one = api.Context(api.default_params(rings, batch=n_frames, max_points=max(len(s) for s in scans[q])))
        for k in range(n_frames):
            one.upload_scan(k, scans[q][k])
        one.extract(0, n_frames)
        one.set_target_from_slot(0)
        ref = one.odometry_frames(1, n_frames - 1, pose0=pose0[q], n_outer=3, first_frame_index=1, opt=o)
        ref_counts = [(p.n_edge, p.n_plane, p.n_plane_selected) for p in (one.pair_info(k) for k in range(1, n_frames))]
        one.close()
        assert np.array_equal(rel[:, q], ref), (q, np.abs(rel[:, q] - ref).max())
        assert counts[q] == ref_counts, q
        # the witness: the oracle's frame loop (no vote before the sixth frame) with the model as its solver
        ex = [orc.extract(s, P) for s in scans[q]]
        orc.set_nn_mode(1)
        x = pose0[q].copy(); log = []; rel_m = []
        for k in range(1, n_frames):
            for outer in range(3):
                es, ea, eb = orc.associate_corner(x[:4], x[4:], ex[k]["sharp"], ex[k - 1]["less_sharp"])
                ps, pa, pb, pc = orc.associate_plane(x[:4], x[4:], ex[k]["flat"], ex[k - 1]["less_flat"])
                args = (ex[k]["sharp"], es, ex[k - 1]["less_sharp"], ea, eb, ex[k]["flat"], ps, ex[k - 1]["less_flat"], pa, pb, pc, np.ones(len(ps), np.float32))
                x, m = lc.solve(lambda y: lc.Record(*orc.normal_equations(y[:4], y[4:], *args)), x, opt)
                log += m.log
                assert all(abs(lhs / rhs - 1.0) > 1e-4 for what, lhs, rhs in m.margins if what == "rho")
            rel_m.append(x.copy())
        orc.set_nn_mode(0)
        print(q, log.count("accept"), "accepted,", log.count("reject"), "rejected")
        assert log.count("reject") >= 4 and (q != 0 or log.count("accept") >= 2)
        assert np.abs(rel[:, q] - np.array(rel_m)).max() < 1e-6
