"""ll_pcm without a GPU: ll_pcm_host -- which runs the pair arithmetic text the kernels run (ll_pcm_math.h) and the selection as the header
states it -- against the independent numpy restatement of tests/pcmcases.py, bit for bit; and the restatement's own properties."""
import numpy as np
import pytest

import pcmcases as pc

RANDOM_C = (1, 2, 63, 64, 65, 127, 128, 129, 300)


def check_host(api, poses, cands, params=None):
    adj, sel, deg, rec = pc.pcm(poses, cands, params)
    words, hsel, hdeg, hrec = api.pcm_host(poses, cands, None if params is None else api.pcm_params(**params))
    C = len(cands)
    assert words.shape == (C, (C + 63) // 64)
    assert words.tobytes() == api.pcm_pack_bits(adj).tobytes(), "the bit matrix"
    assert (hdeg == deg).all() and (hsel == sel).all()
    assert pc.record_tuple(hrec) == pc.record_tuple(rec)
    return adj, sel, deg, rec


@pytest.mark.parametrize("case", pc.exact_cases(), ids=lambda c: c[0])
def test_crafted_exact_graphs(api, case):
    """identity and 180-degree quaternions, translations and thresholds on the 2^-10 grid: every product is exact, the expected bit is
    known by hand; the restatement and ll_pcm_host both give it"""
    name, poses, cands, params, want = case
    adj, _, _, _ = check_host(api, poses, cands, params)
    assert (adj == want).all(), (name, adj.astype(int).tolist())


@pytest.mark.parametrize("C", RANDOM_C)
def test_random_graphs_equal_the_restatement(api, C):
    poses, cands = pc.random_graph(1000 + C, 50, C)
    adj, sel, deg, rec = check_host(api, poses, cands)
    assert (adj == adj.T).all() and not adj.diagonal().any()
    assert sel.sum() == rec["n_selected"] and adj[np.ix_(sel, sel)].sum() == rec["n_selected"] * (rec["n_selected"] - 1), "the selection is a clique"
    if C >= 63:
        assert 0 < rec["n_consistent_pairs"] < C * (C - 1) // 2, "the generator must put pairs on both sides of the thresholds"


def test_other_parameters(api):
    poses, cands = pc.random_graph(5, 30, 90)
    a = check_host(api, poses, cands, dict(rot_tol=0.02, trans_tol=0.2, rot_rate=0.0, trans_rate=0.0))[0]
    b = check_host(api, poses, cands, dict(rot_tol=0.2, trans_tol=2.0, rot_rate=1e-3, trans_rate=0.05))[0]
    assert a.sum() < b.sum() and not (a & ~b).any()


def test_duplicates_of_one_candidate_are_consistent(api):
    poses, cands = pc.random_graph(11, 20, 12)
    cands = cands + [cands[3], cands[3]]
    adj = check_host(api, poses, cands, dict(rot_tol=1e-9, trans_tol=1e-9, rot_rate=0.0, trans_rate=0.0))[0]
    assert adj[3, 12] and adj[3, 13] and adj[12, 13]


def test_empty_and_single(api):
    poses, cands = pc.random_graph(3, 5, 1)
    words, sel, deg, rec = api.pcm_host(poses, [])
    assert words.shape == (0, 0) and len(sel) == 0 and pc.record_tuple(rec) == (0, 0, -1, 0, 0)
    words, sel, deg, rec = api.pcm_host(poses, cands)
    assert sel.tolist() == [True] and deg.tolist() == [0] and pc.record_tuple(rec) == (1, 1, 0, 0, 0)


def test_selection_rules_on_the_restatement():
    sel, deg, rec = pc.select(pc.graph_matrix("star", 9))
    assert rec["n_selected"] == 2 and rec["start"] == 0 and sel.tolist() == [True, True] + [False] * 7          # the hub, then the leaf earliest in the order
    sel, deg, rec = pc.select(pc.graph_matrix("path", 9))
    assert rec["n_selected"] == 2 and rec["start"] == 1 and sel.tolist() == [False, True, True] + [False] * 6   # inner nodes come first; node 1 prefers node 2 (degree 2) to node 0
    a = pc.graph_matrix("two-cliques", 10, seed=3)
    sel, deg, rec = pc.select(a)
    assert rec["n_selected"] == 5 and rec["start"] == 0 and sel[0], "equal cliques: the tie goes to the start earliest in the order, index 0"
    sel, deg, rec = pc.select(pc.graph_matrix("empty", 4))
    assert rec["n_selected"] == 1 and rec["start"] == 0 and sel.tolist() == [True, False, False, False]


def test_host_refusals(api):
    import ctypes as C
    lib = api.load_library()
    poses, cands = pc.random_graph(2, 6, 4)
    P = np.ascontiguousarray(poses); cd = api.pcm_candidates(cands)
    sel = np.full(4, 7, np.uint8)

    def call(P=P, cd=cd, n=len(P), c=4, prm=None):
        return lib.ll_pcm_host(n, P.ctypes.data, c, cd.ctypes.data, None if prm is None else C.addressof(prm), None, sel.ctypes.data, None, None)

    assert call() == 0 and sel.max() <= 1
    sel[:] = 7
    bad = cd.copy(); bad["i"][1] = 6
    assert call(cd=bad) == -2
    bad = cd.copy(); bad["j"][2] = bad["i"][2]
    assert call(cd=bad) == -2
    bad = cd.copy(); bad["Z_w7"][0, :4] = 0.0
    assert call(cd=bad) == -2
    bad = cd.copy(); bad["Z_w7"][3, 5] = np.inf
    assert call(cd=bad) == -2
    badP = P.copy(); badP[2, 0] = np.nan
    assert call(P=badP) == -2
    assert call(prm=api.pcm_params(trans_rate=-1e-3)) == -2
    assert call(prm=api.pcm_params(rot_tol=np.nan)) == -2
    assert lib.ll_pcm_host(len(P), None, 4, cd.ctypes.data, None, None, sel.ctypes.data, None, None) == -2
    many = np.zeros(4097, api.PCM_CANDIDATE); many["j"] = 1; many["Z_w7"][:, 3] = 1.0
    big = np.zeros(4097, np.uint8)
    assert lib.ll_pcm_host(len(P), P.ctypes.data, 4097, many.ctypes.data, None, None, big.ctypes.data, None, None) == -4
    assert (sel == 7).all(), "a refused call leaves the outputs untouched"


def test_double_lap_scene(api):
    """80 poses, two laps; the planted true revisits are recovered exactly; the aliased group agrees with itself in every pair and loses"""
    sc = pc.double_lap()
    adj, sel, deg, rec = check_host(api, sc["est"], sc["cands"])
    drift = float(np.linalg.norm(sc["est"][-1, 4:] - sc["gt"][-1, 4:]))
    alias_pairs = int(adj[np.ix_(sc["alias"], sc["alias"])].sum())
    rot2, trans2, ar2, at2 = pc.pair_terms(sc["est"], sc["cands"])
    iu = np.triu_indices(len(adj), 1)
    margin = float(np.minimum(np.abs(np.sqrt(rot2[iu] / ar2[iu]) - 1.0), np.abs(np.sqrt(trans2[iu] / at2[iu]) - 1.0)).min())
    print(f"double lap: {len(sc['gt'])} poses, end drift {drift:.2f} m, ATE of the odometry {pc.ate(sc['est'], sc['gt']):.2f} m; "
          f"{len(sc['true'])} true + {len(sc['false'])} random + {len(sc['alias'])} aliased candidates; selected {rec['n_selected']}, "
          f"consistent pairs {rec['n_consistent_pairs']}, aliased ordered pairs consistent {alias_pairs} of {len(sc['alias']) * (len(sc['alias']) - 1)}, "
          f"smallest relative distance of a pair to a threshold {margin:.1e}")
    assert len(sc["true"]) == 24 and len(sc["false"]) == 16 and len(sc["alias"]) == 6 and len(sc["gt"]) == 80
    assert sorted(np.flatnonzero(sel)) == sorted(sc["true"]), "exactly the planted set"
    assert alias_pairs == 30, "the aliased group is mutually consistent"
    assert not adj[np.ix_(sc["alias"], sc["true"])].any()
    assert 4.5 < drift < 5.5
