"""The mapping vote's threshold constants against the host libm, and the crafted inputs of mapvotecases.py checked on the CPU:
np_map_vote equals a plain pair-by-pair restatement that calls expf for EVERY pair, and the generators deliver what they promise --
the region sizes, pairs within a few ulp of the gap threshold on both sides, non-finite gaps, counts at / below / above 0.75f * m."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mapvotecases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "map_vote_host.cpp")
OUT = os.path.join(ROOT, "tests", "native", "_build", "libmap_vote_host.so")


@pytest.fixture(scope="module")
def mv():
    hdr = os.path.join(ROOT, "light-loam_amd", "csrc", "ll_exact_math.h")
    if not os.path.exists(OUT) or max(os.path.getmtime(SRC), os.path.getmtime(hdr)) > os.path.getmtime(OUT):
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-fopenmp", "-ffp-contract=off", "-fno-fast-math",
                               "-I", os.path.dirname(hdr), "-o", OUT, SRC, "-lm"])
    lib = C.CDLL(OUT)
    for f in (lib.mv_check_vote, lib.mv_check_vote_gap):
        f.restype = C.c_longlong
        f.argtypes = [C.c_ulonglong, C.c_ulonglong]
    lib.mv_first_incompatible_gap2.restype = C.c_uint
    return lib


# ------------------------------------------------------------------------------------------------ the constants
def test_gap2_threshold_all_non_negative_floats(mv):
    """(double)expf(-g2) < 0.95  <=>  bits(g2) >= 0x3d5218e6 for EVERY non-negative f32 (2^31 inputs, +inf included)"""
    assert mv.mv_check_vote(0, 1) == 0
    assert mv.mv_first_incompatible_gap2() == mc.GAP2_BITS == 0x3d5218e6


def test_gap_threshold_all_non_negative_floats(mv):
    """RN(g * g) >= 0x3d5218e6  <=>  bits(g) >= 0x3e67ea6c for EVERY non-negative f32"""
    assert mv.mv_check_vote_gap(0, 1) == 0
    assert mc.GAP_BITS == 0x3e67ea6c


def test_the_double_literal_matters():
    """0.95 is a double at laserMapping.cpp:937: scores between 0.95 and 0.95f are incompatible there, and the constants say so"""
    lo = np.array([mc.GAP2_BITS], np.uint32).view(np.float32)[0]
    below = np.array([mc.GAP2_BITS - 1], np.uint32).view(np.float32)[0]
    e = lambda g2: float(mc._libm.expf(np.float32(-g2)))
    assert e(lo) < 0.95 and not e(below) < 0.95
    assert not np.float32(e(lo)) < np.float32(0.95)                  # the 0.95f reading would still call this pair compatible
    g = mc.G_T; gb = np.array([mc.GAP_BITS - 1], np.uint32).view(np.float32)[0]
    assert mc.incompatible_by_expf(g) and not mc.incompatible_by_expf(gb)


# ------------------------------------------------------------------------------------------------ np_map_vote itself
def loop_map_vote(src, tgt):
    """laserMapping.cpp:836-1030 pair by pair, every decision by expf (slow: small cases only)"""
    src = np.ascontiguousarray(src, np.float32); tgt = np.ascontiguousarray(tgt, np.float32)
    n = len(src)
    cnt = np.zeros(n, np.int32); sel = np.zeros(n, bool)
    for b0, b1 in mc.region_bounds(n):
        m = b1 - b0
        if m <= 0:
            continue
        s1 = mc.pair_roots(src[b0:b1]); s2 = mc.pair_roots(tgt[b0:b1])
        with np.errstate(all="ignore"):
            gap = np.abs(s1 - s2)
        for i in range(m):
            for j in range(i + 1, m):
                if mc.incompatible_by_expf(gap[i, j]):
                    cnt[b0 + i] += 1; cnt[b0 + j] += 1
        sel[b0:b1] = cnt[b0:b1].astype(np.float32) < np.float32(0.75) * np.float32(m)
    return cnt, sel


SMALL = tuple(n for n in mc.CASE_NAMES if n not in ("n5140", "n5160", "n5159", "ladder"))


@pytest.mark.parametrize("name", SMALL)
def test_np_map_vote_equals_the_pair_loop(name):
    src, tgt = mc.all_cases()[name]
    cnt, sel = mc.reference(name)
    lcnt, lsel = loop_map_vote(src, tgt)
    assert (cnt == lcnt).all() and (sel == lsel).all()


def test_region_bounds():
    for n in mc.SIZES + (439, 440):
        b = mc.region_bounds(n)
        assert len(b) == 20 and b[0][0] == 0 and b[-1][1] == n
        assert all(b[r][1] == b[r + 1][0] for r in range(19))
        assert all(b1 - b0 == n // 20 for b0, b1 in b[:-1]) and b[-1][1] - b[-1][0] == n // 20 + n % 20
    assert mc.region_bounds(19)[-1] == (0, 19) and mc.region_bounds(0)[-1] == (0, 0)


def test_size_cases_cover_the_workgroup_edges():
    """a region with one entry more than the workgroup has threads (odd) and two more (even), and a longer last region; every small
    size has both kept and dropped entries where its regions are large enough to drop any"""
    sizes = {n: [b1 - b0 for b0, b1 in mc.region_bounds(n)] for n in mc.SIZES}
    assert set(sizes[20 * (mc.NT + 1)]) == {mc.NT + 1} and set(sizes[20 * (mc.NT + 2)]) == {mc.NT + 2}
    assert sizes[20 * (mc.NT + 1) + 19][-1] == mc.NT + 20
    for n in (419, 20 * (mc.NT + 1), 20 * (mc.NT + 2), 20 * (mc.NT + 1) + 19):
        cnt, sel = mc.reference(f"n{n}")
        assert sel.any() and (~sel).any() and cnt.max() > 0, n
    for n in (0, 1):
        cnt, sel = mc.reference(f"n{n}")
        assert len(cnt) == n and (cnt == 0).all() and sel.all()              # 0 < 0.75f * 1


@pytest.mark.parametrize("name", mc.BORDERLINE_NAMES)
def test_borderline_families_straddle_the_threshold(name):
    """at least 16 anchor pairs within 4 ulp (of the larger root) of g_T, both outcomes among them; moving every root by +-1 ulp
    at random changes a count in at least half of 20 trials"""
    src, tgt = mc.all_cases()[name]
    d, inc = mc.anchor_gap_ulps(src, tgt)
    close = np.abs(d) <= 4
    print(name, "anchor pairs within 4 ulp:", int(close.sum()), "of", len(d), "incompatible among them:", int(inc[close].sum()))
    assert close.sum() >= 16
    assert inc[close].any() and (~inc[close]).any()
    stats = {}
    cnt, _ = mc.np_map_vote(src, tgt, stats=stats)
    print(name, "pairs within 64 ulp of the GAP's threshold:", stats["near64"])
    if name in ("borderline-scale0", "borderline-scale1", "ladder"):         # at 10 m and 100 m one ulp of a root is 64 and 512 ulp of the gap
        assert stats["near64"] >= 16
    rng = np.random.default_rng(5)
    changed = sum(int((mc.np_map_vote(src, tgt, perturb=rng)[0] != cnt).any()) for _ in range(20))
    print(name, "trials in which +-1 ulp roots change a count:", changed, "of 20")
    assert changed >= 10


def test_the_exact_ladder_counts_41_of_81():
    src, tgt = mc.ladder()
    cnt, sel = mc.reference("ladder")
    for r in range(20):
        assert cnt[83 * r] == 41 and cnt[83 * r + 82] == 41
        assert cnt[83 * r + 1:83 * r + 82].tolist() == [0] * 40 + [2] * 41        # k < 0 compatible, k >= 0 against anchor and filler
    d, inc = mc.anchor_gap_ulps(src, tgt)
    assert np.array_equal(d.reshape(20, 82)[:, :81], np.tile(np.arange(-40.0, 41.0), (20, 1)))             # exactly k ulp from g_T


def test_extreme_cases_hold_what_they_name():
    c = mc.extreme_cases()
    src, tgt = c["overflow"]
    s1 = mc.pair_roots(src[:8]); s2 = mc.pair_roots(tgt[:8])
    assert np.isinf(s1[1, 0]) and np.isfinite(s2[1, 0])                          # one infinite root
    a = mc.pair_roots(src[8:16]); b = mc.pair_roots(tgt[8:16])
    with np.errstate(all="ignore"):
        assert np.isinf(a[1, 0]) and np.isinf(b[1, 0]) and np.isnan(a[1, 0] - b[1, 0])   # both infinite: NaN gap
    cnt, sel = mc.np_map_vote(src, tgt)
    assert cnt[1] == 7 and not sel[1]                                            # inf gap: incompatible with all of its region
    others = np.delete(np.arange(8, 16), 1)
    assert cnt[9] == 0 and sel[9] and (cnt[others] <= 6).all()                   # NaN gap: compatible
    src, tgt = c["nan"]
    cnt, sel = mc.np_map_vote(src, tgt)
    assert cnt[2] == 0 and cnt[11] == 0 and cnt[20] == 0 and cnt[41] == 0        # NaN gaps only
    assert cnt[33] == 7 and cnt[50] == 7                                         # one infinite root each


def test_selection_cases_hit_their_edges():
    for name, (src, tgt, expect) in mc.selection_cases().items():
        cnt, sel = mc.reference(name)
        for i, (c, s) in expect.items():
            assert (int(cnt[i]), bool(sel[i])) == (c, s), (name, i)
    _, _, exp = mc.selection_cases()["m20-count14-15-16"]
    assert {v for i, v in exp.items() if 60 <= i < 80} == {(15, False), (14, True), (16, False)}        # at, below, above 0.75f * 20
    assert all(exp[i] == (0, True) for i in range(140, 160)) and all(exp[i] == (19, False) for i in range(380, 400))
