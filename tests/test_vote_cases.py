"""The crafted vote inputs of votecases.py, checked on the CPU against the oracle alone: np_vote (vectorised numpy, correctly
rounded roots, glibc's expf as witness) equals orc.vote on every case, and the generators deliver what they promise -- pairs
within a few ulp of the gap threshold on both sides, so that a kernel deciding from approximate roots cannot pass them."""
import numpy as np
import pytest

import votecases as vc


@pytest.mark.parametrize("corner_case", [False, True], ids=["10-regions", "5-regions"])
@pytest.mark.parametrize("name", vc.CASE_NAMES)
def test_np_vote_equals_the_oracle(orc, name, corner_case):
    src, tgt = vc.all_cases()[name]
    cnt, sel, w = vc.reference(name, corner_case)
    ocnt, osel, ow = vc.orc_vote(orc, src, tgt, corner_case)
    assert (cnt == ocnt).all()
    assert (sel == osel).all()
    assert w.tobytes() == ow.tobytes()


@pytest.mark.parametrize("name", vc.BORDERLINE_NAMES)
def test_borderline_families_straddle_the_threshold(name):
    """at least 8 anchor pairs within 4 ulp (of the larger root) of g_T, both outcomes among them; moving every root by +-1 ulp
    at random changes a count in at least half of 20 trials"""
    src, tgt = vc.borderline_cases()[name]
    d, inc = vc.anchor_gap_ulps(src, tgt)
    close = np.abs(d) <= 4
    print(name, "anchor pairs within 4 ulp:", int(close.sum()), "of", len(d), "incompatible among them:", int(inc[close].sum()))
    assert close.sum() >= 8
    assert inc[close].any() and (~inc[close]).any()
    cnt, _, _ = vc.np_vote(src, tgt, 10)
    rng = np.random.default_rng(5)
    changed = sum(int((vc.np_vote(src, tgt, 10, perturb=rng)[0] != cnt).any()) for _ in range(20))
    print(name, "trials in which +-1 ulp roots change a count:", changed, "of 20")
    assert changed >= 10


def test_the_exact_ladder_counts_41_of_81():
    src, tgt = vc.ladder()
    cnt, sel, w = vc.np_vote(src, tgt, 10)
    for r in range(10):
        assert cnt[83 * r] == 41 and cnt[83 * r + 82] == 41
        assert cnt[83 * r + 1:83 * r + 82].tolist() == [0] * 40 + [2] * 41        # k < 0 compatible, k >= 0 against anchor and filler
    d, inc = vc.anchor_gap_ulps(src, tgt)
    assert np.array_equal(d.reshape(10, 82)[:, :81], np.tile(np.arange(-40.0, 41.0), (10, 1)))              # exactly k ulp from g_T


def test_extreme_cases_hold_what_they_name():
    c = vc.extreme_cases()
    src, tgt = c["overflow"]
    s1 = vc.pair_roots(src[:4]); s2 = vc.pair_roots(tgt[:4])
    assert np.isinf(s1[1, 0]) and np.isfinite(s2[1, 0])                          # one infinite root
    a = vc.pair_roots(src[4:8]); b = vc.pair_roots(tgt[4:8])
    with np.errstate(all="ignore"):
        assert np.isinf(a[1, 0]) and np.isinf(b[1, 0]) and np.isnan(a[1, 0] - b[1, 0])   # both infinite: NaN gap
    cnt, sel, w = vc.np_vote(src, tgt, 10)
    assert cnt[1] == 3 and cnt[5] == 0                                           # inf gap: incompatible; NaN gap: compatible
    src, tgt = c["nan"]
    cnt, _, _ = vc.np_vote(src, tgt, 10)
    assert cnt[2] == 0 and cnt[7] == 0 and cnt[13] == 0                          # a NaN gap is compatible
    src, tgt = c["denormal"]
    d = src[1, 0] - src[0, 0]
    assert 0 < d < np.finfo(np.float32).tiny                                     # a denormal coordinate difference


def test_selection_cases_hit_their_edges():
    for name, (src, tgt, expect) in vc.selection_cases().items():
        cnt, sel, w = vc.np_vote(src, tgt, 10)
        for i, (c, s, ww) in expect.items():
            assert (int(cnt[i]), bool(sel[i]), float(w[i])) == (c, s, ww), (name, i)


@pytest.mark.parametrize("n", [0, 1, 7, 512, 513, 1025])
@pytest.mark.parametrize("pattern", vc.HOLE_PATTERNS)
def test_hole_patterns(n, pattern):
    h = vc.hole_mask(pattern, n)
    assert len(h) == n
    if n == 0:
        return
    per = -(-n // 512)
    keep = np.flatnonzero(~h)
    want = {"none": n, "all": 0, "every-second": (n + 1) // 2, "first-per": n - per, "only-0": 1, "only-last": 1}
    if pattern in want:
        assert len(keep) == want[pattern]
    else:
        assert len(keep) >= 1 and keep[-1] == n - 1 and keep[0] // per == (n - 1) // per     # one thread's share


def test_lattice_queries_associate_as_intended(orc):
    """every non-hole query finds the chosen lattice point as its closest point, for planes and for corners, and gets a
    correspondence; the lists are the non-hole indices in order"""
    rng = np.random.default_rng(3)
    lat = vc.lattice(64)
    n = 1537
    idx = rng.integers(0, len(lat), n)
    holes = np.zeros(n, bool); holes[rng.choice(n, 100, replace=False)] = True
    q = vc.queries(lat, idx, vc.offsets(n, rng), holes)
    ident = (np.array([0, 0, 0, 1.0]), np.zeros(3))
    ps, pa, pb, pc = orc.associate_plane(*ident, q, lat)
    es, ea, eb = orc.associate_corner(*ident, q, lat)
    keep = np.flatnonzero(~holes)
    assert len(keep) == 1437
    assert np.array_equal(ps, keep) and np.array_equal(pa, idx[keep])
    assert np.array_equal(es, keep) and np.array_equal(ea, idx[keep])


@pytest.mark.parametrize("scale", [0, 1])
def test_lattice_borderline_survives_association(orc, scale):
    lat = vc.lattice(64)
    idx, q = vc.lattice_borderline(lat, np.random.default_rng(40 + scale), scale)
    ps, pa, pb, pc = orc.associate_plane(np.array([0, 0, 0, 1.0]), np.zeros(3), q, lat)
    assert np.array_equal(ps, np.arange(len(q))) and np.array_equal(pa, idx)
    d, inc = vc.anchor_gap_ulps(q[ps], lat[pa])
    close = np.abs(d) <= 4
    print("lattice scale", scale, "within 4 ulp:", int(close.sum()), "incompatible:", int(inc[close].sum()))
    assert close.sum() >= 8 and inc[close].any() and (~inc[close]).any()
