"""The inputs of tests/test_gpu_places.py against their own preconditions, without a GPU: what the numpy restatement
(tests/placecases.py) says about them holds by a margin far above any rounding, so a disagreement of the library is the library's."""
import numpy as np
import pytest

import placecases as pc


def test_crafted_points_are_on_an_intended_edge_or_clear_of_every_edge():
    w, sect = 80.0 / pc.RINGS, 2 * np.pi / pc.SECTORS
    for name, (pts, on_edge) in pc.describe_cases().items():
        assert len(pts) == len(on_edge), name
        p = pts[~on_edge].astype(np.float64)
        r = np.hypot(p[:, 0], p[:, 1])
        a = np.mod(np.arctan2(p[:, 1], p[:, 0]), 2 * np.pi)
        dr = np.abs(r - np.round(r / w) * w)
        da = np.abs(a - np.round(a / sect) * sect)
        assert (dr > 1e-3).all() and (da > 1e-4).all() and (r < 80.0 - 1e-3).all(), name
    assert [len(pc.describe_cases()["n%d" % n][0]) for n in (0, 1, 255, 256, 257, 4097)] == [0, 1, 255, 256, 257, 4097]


def test_the_restatement_puts_the_edge_points_where_the_contract_says(orc):
    cases = pc.describe_cases()
    d = pc.np_describe(cases["ring_edges"][0])
    for k in range(pc.RINGS):                                       # r = k * w exactly lands in ring k
        assert d[k, 0] == np.float32(0.25 * k - 1.0 + 2.0), k
    assert d[5, 8] == 3.0 and d[10, 8] == 4.0 and d[15, 8] == 5.0   # 3-4-5 triangles: r = 20, 40, 60
    d = pc.np_describe(cases["max_radius"][0])
    assert d[19, 0] == 3.0 and d[19, 45] == 4.0                     # the float below 80 is kept, 80 itself and beyond are dropped
    assert np.count_nonzero(d) == 2
    d = pc.np_describe(cases["origin"][0])
    assert d[0, 0] == 2.5 and np.count_nonzero(d) == 1
    d = pc.np_describe(cases["axes"][0])
    assert d[2, 0] == np.float32(2.1) and d[2, 15] == np.float32(2.2) and d[2, 30] == np.float32(2.6) and d[2, 45] == np.float32(2.4)
    d = pc.np_describe(cases["sector_clamp"][0])
    assert d[2, 59] == np.float32(2.7) and d[7, 59] == np.float32(2.8) and d[12, 59] == np.float32(2.9) and np.count_nonzero(d) == 3
    d = pc.np_describe(cases["two_in_a_bin"][0])
    assert d[3, 7] == 4.5 and d[9, 40] == 6.0 and d[19, 59] == 2.0 and d[0, 0] == 1.5
    d = pc.np_describe(cases["below_ground"][0])
    assert d[5, 5] == -1.0 and d[6, 5] == -0.5 and d[7, 5] == 0.0   # a bin of negative heights keeps its negative maximum
    assert pc.np_describe(np.zeros((0, 4), np.float32)).tolist() == np.zeros((20, 60)).tolist()


def test_onehot_cases_answer_the_shift_they_are_about():
    for name, (q, c, s) in pc.onehot_cases().items():
        d, got = pc.onehot_expected(q, c)
        assert got == s, name
        d64, s64, _ = pc.np_best(q, c)                              # the float64 restatement agrees with the exact one
        assert s64 == s and abs(d64 - float(d)) < 1e-7, name
    e = pc.onehot_expected
    cs = pc.onehot_cases()
    assert e(*cs["shift30"][:2])[0] == 0.0 and e(*cs["half_agree"][:2])[0] == 0.5 and e(*cs["all_empty_q"][:2]) == (1.0, 0)
    q, c, _ = cs["empty_in_both"]
    counts = {int((np.roll(q.any(axis=0), -s) & c.any(axis=0)).sum()) for s in range(60)}
    assert len(counts) > 1                                           # count varies with the shift
    q, c, _ = cs["asymmetric7"]
    assert e(c, q)[1] == 53                                          # what a kernel with the operands swapped would answer


@pytest.mark.parametrize("nq,nc", pc.MATCH_SIZES)
def test_random_match_cases_have_one_clear_heading_per_query(nq, nc):
    qs, cand, turned = pc.random_match_case(nq, nc)
    for d in qs + cand:
        assert (d >= 0).all() and 0.25 < (d == 0).mean() < 0.45
    for i, q in enumerate(qs):
        best, s, d = pc.np_best(q, cand[i % nc])
        assert s == turned[i] and np.sort(d)[1] - best > 1e-3 and best < 0.05, i


def test_topk_case_has_clear_ranks_and_one_tie():
    qs, cand = pc.topk_case()
    D = pc.np_ranking(qs, cand)
    assert (D[:, 12] == D[:, 41]).all()                              # the duplicate
    for i in range(len(qs)):
        d = np.delete(D[i], 41)                                      # apart from it, the first K + 1 ranks are 1e-4 apart
        gaps = np.diff(np.sort(d)[:max(pc.MATCH_K) + 1])
        assert (gaps > 1e-4).all(), (i, gaps)
    first = np.argsort(D[0], kind="stable")[:3]
    assert first[1] == 12 and first[2] == 41                        # the tie sits inside every K > 1


def test_lap_revisits_stand_out(synth, orc):
    db, queries, want, shift = pc.lap_scans(synth)
    D = [pc.np_describe(s) for s in db]
    for q, w, s in zip(queries, want, shift):
        dq = pc.np_describe(q)
        res = [pc.np_best(dq, d) for d in D]
        dist = np.array([r[0] for r in res])
        assert int(np.argmin(dist)) == w and res[w][1] == s
        assert dist[w] < 0.2 and (np.delete(dist, w) > 0.5).all(), (w, dist)
