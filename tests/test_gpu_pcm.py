"""ll_pcm on the GPU.  Adjacency, degrees, selection and records equal the numpy restatement of tests/pcmcases.py bit for bit with no
pair excluded -- the device uses only + - * and comparisons in f64 after the host's normalisation -- on crafted exact-arithmetic graphs
and random ones at sizes round the 64-bit word and the 256-row workgroup; the selection alone on supplied matrices; run against
ll_pcm_host byte for byte; a graph's bytes alone, first, last and in the middle of a batch that also holds graphs of 0 and 4096
candidates; every refusal; and the double-lap scene through PoseGraphs.solve.  No expected value comes from the device."""
import ctypes as C

import numpy as np
import pytest

import pcmcases as pc

pytestmark = pytest.mark.gpu

RANDOM_C = (1, 2, 63, 64, 65, 127, 128, 129, 300)
SELECT_CASES = [("empty", 1), ("empty", 70), ("complete", 64), ("complete", 65), ("complete", 300), ("two-cliques", 10), ("two-cliques", 130), ("star", 9),
                ("star", 200), ("path", 9), ("path", 129), ("gnp", 300), ("planted", 4096)]


@pytest.fixture(scope="module")
def ctx(api):
    c = api.Context(api.default_params(16, batch=2, max_points=4096))
    yield c
    c.close()


@pytest.fixture(scope="module")
def pcm(ctx):
    p = ctx.pcm(16, 4000, 12000)
    yield p
    p.close()


def rec_bytes(r):
    return bytes(memoryview(r))


def check_graph(api, pcm, poses, cands, params=None):
    """one graph alone through run: matrix, degrees, selection and record against the restatement"""
    adj, sel, deg, rec = pc.pcm(poses, cands, params)
    gsel, gdeg, grec = pcm.run([(poses, cands)], None if params is None else api.pcm_params(**params))
    assert pcm.adjacency_words(0).tobytes() == api.pcm_pack_bits(adj).tobytes(), "the bit matrix"
    assert (pcm.adjacency(0) == adj).all()
    assert (gdeg[0] == deg).all() and (gsel[0] == sel).all()
    assert pc.record_tuple(grec[0]) == pc.record_tuple(rec)
    return adj


@pytest.mark.parametrize("case", pc.exact_cases(), ids=lambda c: c[0])
def test_crafted_exact_graphs(api, pcm, case):
    name, poses, cands, params, want = case
    adj = check_graph(api, pcm, poses, cands, params)
    assert (adj == want).all(), name


@pytest.mark.parametrize("C_", RANDOM_C)
def test_random_graphs(api, pcm, C_):
    poses, cands = pc.random_graph(1000 + C_, 50, C_)
    check_graph(api, pcm, poses, cands)


def test_all_crafted_graphs_in_one_call_under_one_parameter_set(api, pcm):
    cases = [c for c in pc.exact_cases() if c[3] == pc.EXACT_PARAMS]
    sel, deg, rec = pcm.run([(c[1], c[2]) for c in cases], api.pcm_params(**pc.EXACT_PARAMS))
    for g, c in enumerate(cases):
        assert (pcm.adjacency(g) == c[4]).all(), c[0]


_SELECT_REF = {}


def select_reference(kind, n):
    if (kind, n) not in _SELECT_REF:
        a = pc.graph_matrix(kind, n, seed=n)
        _SELECT_REF[(kind, n)] = (a,) + pc.select(a)
    return _SELECT_REF[(kind, n)]


@pytest.mark.parametrize("kind,n", SELECT_CASES)
def test_select_on_supplied_matrices(api, pcm, kind, n):
    a, sel, deg, rec = select_reference(kind, n)
    gsel, gdeg, grec = pcm.select([a])
    assert (gsel[0] == sel).all() and (gdeg[0] == deg).all() and pc.record_tuple(grec[0]) == pc.record_tuple(rec)
    assert (pcm.adjacency(0) == a).all()
    if kind == "planted":
        assert rec["n_selected"] == 40
    if kind == "two-cliques":
        assert rec["n_selected"] == n // 2 and sel[rec["start"]]


def test_select_batch_and_empty_graphs(api, pcm):
    cases = [("gnp", 300), ("empty", 1), ("complete", 65), ("path", 129), ("star", 9)]
    mats = [select_reference(k, n)[0] for k, n in cases]
    mats.insert(2, np.zeros((0, 0), bool))
    gsel, gdeg, grec = pcm.select(mats)
    assert pc.record_tuple(grec[2]) == (0, 0, -1, 0, 0) and len(gsel[2]) == 0
    del gsel[2], gdeg[2], grec[2]
    for (k, n), s, d, r in zip(cases, gsel, gdeg, grec):
        _, sel, deg, rec = select_reference(k, n)
        assert (s == sel).all() and (d == deg).all() and pc.record_tuple(r) == pc.record_tuple(rec), (k, n)
    sel, deg, rec = pcm.select([])
    assert sel == [] and rec == []
    sel, deg, rec = pcm.select([np.zeros((0, 0), bool)] * 3)
    assert [pc.record_tuple(r) for r in rec] == [(0, 0, -1, 0, 0)] * 3
    assert pcm.timing()["ms"] == [0.0] * 5 and pcm.timing()["candidates"] == 0, "a call without a candidate launches nothing"


_BIG = {}


def big_graph(api):
    """4096 candidates on 500 poses, and ll_pcm_host's answer for it (the restatement's full matrix would take minutes)"""
    if not _BIG:
        poses, cands = pc.random_graph(77, 500, 4096, p_true=0.5)
        _BIG["g"] = (poses, api.pcm_candidates(cands))
        _BIG["host"] = api.pcm_host(*_BIG["g"])
    return _BIG["g"], _BIG["host"]


def test_run_equals_the_host_function_byte_for_byte(api, pcm):
    for C_ in (65, 300):
        poses, cands = pc.random_graph(2000 + C_, 60, C_)
        words, sel, deg, rec = api.pcm_host(poses, cands)
        gsel, gdeg, grec = pcm.run([(poses, cands)])
        assert pcm.adjacency_words(0).tobytes() == words.tobytes() and gsel[0].tobytes() == sel.tobytes() and gdeg[0].tobytes() == deg.tobytes()
        assert rec_bytes(grec[0]) == rec_bytes(rec)


def test_batch_independence_and_repetition(api, pcm):
    """a graph's words, selection, degrees and record: the same bytes alone, first, last and in the middle of a batch that also holds
    graphs of 0 and 4096 candidates, and on repetition"""
    big, host = big_graph(api)
    probe = pc.random_graph(31, 40, 129)
    others = [pc.random_graph(32, 30, 64), pc.random_graph(33, 2, 5), (pc.exact_line(3), [])]

    def take(graphs, g):
        sel, deg, rec = pcm.run(graphs)
        return pcm.adjacency_words(g).tobytes(), sel[g].tobytes(), deg[g].tobytes(), rec_bytes(rec[g]), (sel, deg, rec)

    alone = take([probe], 0)[:4]
    assert alone == take([probe], 0)[:4], "repetition"
    first = take([probe, big, others[0], others[2]], 0)
    assert first[:4] == alone
    sel, deg, rec = first[4]
    assert len(sel[3]) == 0 and pc.record_tuple(rec[3]) == (0, 0, -1, 0, 0)
    assert sel[1].tobytes() == host[1].tobytes() and deg[1].tobytes() == host[2].tobytes() and rec_bytes(rec[1]) == rec_bytes(host[3]), "4096 candidates against ll_pcm_host"
    assert pcm.adjacency_words(1).tobytes() == host[0].tobytes()
    assert take([others[2], others[0], big, probe], 3)[:4] == alone, "last"
    assert take([others[1], others[2], probe, big, others[0]], 2)[:4] == alone, "middle"
    t = pcm.timing()
    assert t["graphs"] == 5 and t["candidates"] == 5 + 129 + 4096 + 64 and t["pairs"] == 25 + 129 * 129 + 4096 * 4096 + 64 * 64
    assert all(m > 0.0 for m in t["ms"]) and t["clique_steps"] > 0


def test_refusals_leave_the_outputs_untouched(api, ctx, pcm):
    lib = api.load_library()
    fresh = ctx.pcm(2, 100, 200)
    w = np.zeros(4, np.uint64)
    assert lib.ll_pcm_adjacency(fresh.h, 0, w.ctypes.data) == -7, "adjacency before any run is LL_ERR_STATE"
    poses, cands = pc.random_graph(2, 6, 4)
    P = np.ascontiguousarray(poses); cd = api.pcm_candidates(cands)
    sel = np.full(8, 7, np.uint8); deg = np.full(8, 7, np.int32); rec = (api.PcmRecord * 2)()
    rec[0].start = 77
    no = np.array([0, 6], np.int32); co = np.array([0, 4], np.int32)

    def run(P=P, cd=cd, no=no, co=co, n=1, prm=None, h=fresh.h, sel_=sel):
        return lib.ll_pcm_run(h, n, no.ctypes.data, co.ctypes.data, None if P is None else P.ctypes.data, cd.ctypes.data, None if prm is None else C.addressof(prm),
                              None if sel_ is None else sel_.ctypes.data, deg.ctypes.data, C.addressof(rec))

    def mod(field, k, value):
        bad = cd.copy(); bad[field][k] = value
        return bad

    zq = cd.copy(); zq["Z_w7"][0, :4] = 0.0
    nf = cd.copy(); nf["Z_w7"][3, 5] = np.inf
    badP = P.copy(); badP[2, 0] = np.nan
    zeroP = P.copy(); zeroP[1, :4] = 0.0
    arg = [dict(cd=mod("i", 1, 6)), dict(cd=mod("j", 1, -1)), dict(cd=mod("j", 2, cd["i"][2])), dict(cd=zq), dict(cd=nf), dict(P=badP), dict(P=zeroP), dict(P=None),
           dict(sel_=None), dict(prm=api.pcm_params(trans_rate=-1e-3)), dict(prm=api.pcm_params(rot_tol=np.inf)), dict(no=np.array([1, 6], np.int32)),
           dict(co=np.array([0, -1], np.int32)), dict(no=np.array([0, 6, 5], np.int32), co=np.array([0, 4, 4], np.int32), n=2), dict(n=-1)]
    for kw in arg:
        assert run(**kw) == -2, kw
        assert fresh.lib.ll_pcm_last_error(fresh.h)
    assert run(cd=mod("i", 1, 6)) == -2 and b"graph 0, candidate 1" in lib.ll_pcm_last_error(fresh.h), "last_error names the graph and the candidate"
    cap = [dict(n=3, no=np.array([0, 6, 6, 6], np.int32), co=np.array([0, 4, 4, 4], np.int32)),        # graphs beyond max_graphs
           dict(no=np.array([0, 101], np.int32)),                                                       # nodes beyond max_nodes_total
           dict(co=np.array([0, 201], np.int32))]                                                       # candidates beyond max_candidates_total
    for kw in cap:
        assert run(**kw) == -4, kw
    many = np.zeros(4097, api.PCM_CANDIDATE); many["j"] = 1; many["Z_w7"][:, 3] = 1.0
    bigsel = np.full(4097, 7, np.uint8)
    assert lib.ll_pcm_run(pcm.h, 1, no.ctypes.data, np.array([0, 4097], np.int32).ctypes.data, P.ctypes.data, many.ctypes.data, None, bigsel.ctypes.data, None, None) == -4
    assert b"4097" in lib.ll_pcm_last_error(pcm.h) and (bigsel == 7).all()
    assert (sel == 7).all() and (deg == 7).all() and rec[0].start == 77, "a refused call leaves the outputs untouched"
    assert lib.ll_pcm_adjacency(fresh.h, 0, w.ctypes.data) == -7, "refused calls are no run"
    # select: not symmetric, a diagonal bit, a bit at or beyond C
    good = pc.graph_matrix("gnp", 70, 5)
    for what in ("asymmetric", "diagonal", "beyond"):
        words = api.pcm_pack_bits(good).copy()
        if what == "asymmetric":
            words[3, 1] ^= np.uint64(1) << np.uint64(2)                # (3, 66) without (66, 3)
        elif what == "diagonal":
            words[5, 0] |= np.uint64(1) << np.uint64(5)
        else:
            words[9, 1] |= np.uint64(1) << np.uint64(6)                # column 70 of 70
        with pytest.raises(api.LightLoamError) as e:
            fresh.select([words])
        assert e.value.code == -2, what
    with pytest.raises(api.LightLoamError) as e:
        fresh.select([np.zeros((201, 4), np.uint64)])
    assert e.value.code == -4
    assert run() == 0 and sel[:4].max() <= 1 and (sel[4:] == 7).all()
    assert lib.ll_pcm_adjacency(fresh.h, 1, w.ctypes.data) == -2 and lib.ll_pcm_adjacency(fresh.h, 0, None) == -2
    fresh.close()


def test_double_lap_scene_through_the_chain(api, ctx, pcm):
    """Pcm.run selects exactly the planted true set; PoseGraphs.solve with the selected candidates (Huber width 1) ends with a smaller
    translational ATE than with all candidates under the same Huber width and weights, and equals the solve with the true set bit for
    bit: it is the same edge list"""
    sc = pc.double_lap()
    sel, deg, rec = pcm.run([(sc["est"], sc["cands"])])
    assert sorted(np.flatnonzero(sel[0])) == sorted(sc["true"])
    odo_w, loop_w = [100.0] * 3 + [10.0] * 3, [100.0] * 3 + [20.0] * 3
    odom = [(i, j, Z, odo_w, 0.0) for i, j, Z in sc["odom"]]
    loop = lambda idx: [(sc["cands"][k][0], sc["cands"][k][1], sc["cands"][k][2], loop_w, 1.0) for k in idx]
    pg = ctx.posegraphs(3, 3 * 80, 3 * (79 + 46))
    graphs = [(sc["est"], odom + loop(np.flatnonzero(sel[0]))), (sc["est"], odom + loop(range(len(sc["cands"])))), (sc["est"], odom + loop(sorted(sc["true"])))]
    poses, recs = pg.solve(graphs)
    pg.close()
    a0, a_sel, a_all, a_true = pc.ate(sc["est"], sc["gt"]), pc.ate(poses[0], sc["gt"]), pc.ate(poses[1], sc["gt"]), pc.ate(poses[2], sc["gt"])
    print(f"double lap, translational ATE: odometry {a0:.3f} m, all 46 candidates under Huber 1 {a_all:.3f} m, the {int(sel[0].sum())} selected {a_sel:.3f} m, "
          f"the true set {a_true:.3f} m")
    assert poses[0].tobytes() == poses[2].tobytes(), "the selected set is the true set: the same edge list, the same bits"
    assert a_sel < a_all
