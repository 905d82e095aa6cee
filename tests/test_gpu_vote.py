"""The correspondence vote (ll_vote_core in its three kernels) and the compaction (ll_block_compact) at crafted inputs.

Direct: ll_vote_host (k_vote_points, 256 threads) on every case of votecases.py against np_vote and the oracle.
The hot path's kernels: k_associate and k_vote (512 threads) through the staged calls, on a lattice target where the association
is known in advance, at the sizes where a thread's share of the compaction changes and with hole patterns that empty whole
shares.  (ll_hot_path_batch extracts its slots from raw scans, so it cannot take crafted features.)
Fused: k_vote_lm_rows (ll_odometry_sequences) and ll_odometry_frames leave the lists and votes of the staged calls.
Normal equations at the row-count edges, from the device's own lists and weights.
All comparisons of counts, flags, indices and weights are exact."""
import ctypes as C

import numpy as np
import pytest

import votecases as vc
from test_gpu_parity import close

pytestmark = pytest.mark.gpu

IDENT = np.array([0, 0, 0, 1.0, 0, 0, 0])
RING_MODEL = {128: dict(ring_model=1, lower_bound=-25.0, up_bound=15.0, minimum_range=0.3)}


def same_vote(got, want, what):
    assert got[0].dtype == np.int32 and np.array_equal(got[0], want[0]), f"{what}: counts"
    assert np.array_equal(got[1], want[1]), f"{what}: selected"
    assert got[2].tobytes() == np.asarray(want[2], np.float32).tobytes(), f"{what}: weights"


# ------------------------------------------------------------------------------------------------ direct: ll_vote_host
@pytest.fixture(scope="module")
def vctx(api):
    ctx = api.Context(api.default_params(16, batch=1, max_points=4096))
    yield ctx
    ctx.close()


@pytest.mark.parametrize("corner_case", [False, True], ids=["10-regions", "5-regions"])
@pytest.mark.parametrize("name", vc.CASE_NAMES)
def test_vote_points_equals_the_references(vctx, orc, name, corner_case):
    src, tgt = vc.all_cases()[name]
    got = vctx.vote_points(src, tgt, corner_case)
    same_vote(got, vc.reference(name, corner_case), f"{name} vs np_vote")
    same_vote(got, vc.orc_vote(orc, src, tgt, corner_case), f"{name} vs the oracle")


def test_vote_points_selection_edges(vctx):
    for name, (src, tgt, expect) in vc.selection_cases().items():
        cnt, sel, w = vctx.vote_points(src, tgt)
        for i, (c, s, ww) in expect.items():
            assert (int(cnt[i]), bool(sel[i]), float(w[i])) == (c, s, ww), (name, i)


def test_vote_points_capacity_and_arguments(api, vctx):
    """5850 correspondences fill the 160 KB of LDS (a case above); 5851 are refused before any launch and the context goes on"""
    src, tgt = vc.consistent(5851, np.random.default_rng(1), 10)
    with pytest.raises(api.LightLoamError) as e:
        vctx.vote_points(src, tgt)
    assert e.value.code == -4 and "5850" in str(e.value)
    s, t = vc.all_cases()["n21"]
    same_vote(vctx.vote_points(s, t), vc.reference("n21", False), "after the refusal")
    cnt, sel, w = vctx.vote_points(np.zeros((0, 4), np.float32), np.zeros((0, 4), np.float32))
    assert cnt.shape == (0,) and cnt.dtype == np.int32 and sel.shape == (0,) and sel.dtype == bool and w.shape == (0,) and w.dtype == np.float32
    lib = api.load_library()
    out = np.zeros(8, np.int32); p = lambda a: a.ctypes.data_as(C.c_void_p)
    s8, t8 = np.ascontiguousarray(s[:8]), np.ascontiguousarray(t[:8])
    assert lib.ll_vote_host(vctx.h, None, p(t8), 8, 0, p(out), None, None) == -2
    assert lib.ll_vote_host(vctx.h, p(s8), None, 8, 0, p(out), None, None) == -2
    assert lib.ll_vote_host(vctx.h, p(s8), p(t8), -1, 0, p(out), None, None) == -2
    assert lib.ll_vote_host(None, p(s8), p(t8), 8, 0, p(out), None, None) == -2
    assert lib.ll_vote_host(vctx.h, None, None, 0, 0, None, None, None) == 0
    assert lib.ll_vote_host(vctx.h, p(s8), p(t8), 8, 0, p(out), None, None) == 0         # any output may be left out
    assert np.array_equal(out, vc.np_vote(s8, t8, 10)[0])


# ------------------------------------------------------------------------------------------------ the hot path's k_vote
class Lattice:
    """a context whose carry target is the lattice of its ring count, corner and surface alike"""

    def __init__(self, api, rings, batch=2):
        self.rings = rings
        self.lat = vc.lattice(rings)
        self.ctx = api.Context(api.default_params(rings, batch=batch, max_points=8192, **RING_MODEL.get(rings, {})))
        self.ctx.set_target(self.lat, self.lat)

    def make(self, n_sharp, n_flat, pattern, seed=0):
        rng = np.random.default_rng(1000 * n_flat + n_sharp + seed)
        out = {}
        for nm, n in (("sharp", n_sharp), ("flat", n_flat)):
            idx = rng.integers(0, len(self.lat), n)
            holes = vc.hole_mask(pattern, n)
            out[nm] = (idx, holes, vc.queries(self.lat, idx, vc.offsets(n, rng), holes))
        return out

    def upload(self, slot, sharp, flat):
        self.ctx.upload_features(slot, sharp, self.lat[:1], flat, self.lat[:1])

    def lists(self, slot):
        c = self.ctx
        pi = c.pair_info(slot)
        return dict(edge=c.edge_corr(slot), plane=c.plane_corr(slot), vote=c.vote_result(slot),
                    info=(pi.n_edge, pi.n_plane, pi.n_plane_selected))


def check_slot(L, orc, slot, q, enable=True):
    """the slot's lists against the oracle's association and the intended lattice points; its vote against np_vote"""
    got = L.lists(slot)
    (si, sh, sharp), (fi, fh, flat) = q["sharp"], q["flat"]
    qq, tt = IDENT[:4], IDENT[4:]
    want_e = orc.associate_corner(qq, tt, sharp, L.lat)
    want_p = orc.associate_plane(qq, tt, flat, L.lat)
    for g, w_, nm in zip(got["edge"] + got["plane"], want_e + want_p, ("e_src", "e_a", "e_b", "p_src", "p_a", "p_b", "p_c")):
        assert g.dtype == np.int32 and np.array_equal(g, w_), nm
    keep_s, keep_f = np.flatnonzero(~sh), np.flatnonzero(~fh)
    assert np.array_equal(got["edge"][0], keep_s) and np.array_equal(got["edge"][1], si[keep_s]), "corner queries -> lattice points"
    assert np.array_equal(got["plane"][0], keep_f) and np.array_equal(got["plane"][1], fi[keep_f]), "plane queries -> lattice points"
    ps, pa = got["plane"][0], got["plane"][1]
    n = len(ps)
    want_v = vc.np_vote(flat[ps], L.lat[pa], 10) if enable else (np.zeros(n, np.int32), np.ones(n, bool), np.ones(n, np.float32))
    same_vote(got["vote"], want_v, "vote_result")
    assert got["info"] == (len(keep_s), n, int(want_v[1].sum())), "pair_info"
    return got


def run_staged(L, orc, q):
    c = L.ctx
    L.upload(0, q["sharp"][2], q["flat"][2])
    c.associate(0, 1, IDENT)
    c.vote(0, 1, True)
    got = check_slot(L, orc, 0, q, True)
    c.vote(0, 1, False)                                   # the same per-query results compacted again, the vote switched off
    off = check_slot(L, orc, 0, q, False)
    assert off["info"][2] == off["info"][1]
    for a, b in zip(got["edge"] + got["plane"], off["edge"] + off["plane"]):
        assert np.array_equal(a, b)
    return got


@pytest.fixture(scope="module")
def L64(api):
    L = Lattice(api, 64)
    yield L
    L.ctx.close()


@pytest.fixture(scope="module")
def L16(api):
    L = Lattice(api, 16, batch=1)
    yield L
    L.ctx.close()


N_FLAT_64 = (0, 1, 9, 10, 11, 511, 512, 513, 1023, 1024, 1025, 1535, 1536)
N_SHARP_64 = (0, 1, 511, 512, 513, 767, 768)


@pytest.mark.parametrize("pattern", vc.HOLE_PATTERNS)
@pytest.mark.parametrize("k", range(len(N_FLAT_64)), ids=[f"flat{n}-sharp{N_SHARP_64[i % 7]}" for i, n in enumerate(N_FLAT_64)])
def test_k_vote_on_the_lattice_64_rings(L64, orc, k, pattern):
    got = run_staged(L64, orc, L64.make(N_SHARP_64[k % 7], N_FLAT_64[k], pattern))
    if pattern == "all":
        assert got["info"] == (0, 0, 0)


@pytest.mark.parametrize("pattern", vc.HOLE_PATTERNS)
@pytest.mark.parametrize("n_sharp,n_flat", [(0, 383), (1, 384), (191, 1), (192, 0), (97, 257)])
def test_k_vote_on_the_lattice_16_rings(L16, orc, n_sharp, n_flat, pattern):
    """cap_flat 384: fewer rows than the 512 threads of the compaction"""
    run_staged(L16, orc, L16.make(n_sharp, n_flat, pattern))


def test_k_vote_on_the_lattice_128_rings(api, orc):
    """cap_flat 3072: the 86 KB LDS vote, shares of up to 6 per thread"""
    L = Lattice(api, 128, batch=1)
    try:
        for n_sharp, n_flat, pattern in ((1536, 3072, "none"), (1535, 3071, "every-second"), (1, 2561, "last-thread-only"),
                                         (513, 2049, "first-per")):
            run_staged(L, orc, L.make(n_sharp, n_flat, pattern))
    finally:
        L.ctx.close()


@pytest.mark.parametrize("scale", [0, 1])
def test_borderline_pairs_through_k_vote(L64, orc, scale):
    """the near-threshold pairs survive the association (recounted from the device's own lists) and are decided exactly"""
    idx, flat = vc.lattice_borderline(L64.lat, np.random.default_rng(40 + scale), scale)
    q = dict(sharp=(np.zeros(0, np.int64), np.zeros(0, bool), np.zeros((0, 4), np.float32)), flat=(idx, np.zeros(len(idx), bool), flat))
    got = run_staged(L64, orc, q)
    ps, pa = got["plane"][0], got["plane"][1]
    d, inc = vc.anchor_gap_ulps(flat[ps], L64.lat[pa])
    near = np.abs(d) <= 4
    assert near.sum() >= 8 and inc[near].any() and (~inc[near]).any()


# ------------------------------------------------------------------------------------------------ fused paths
FUSED = [(0, 0, "none"), (1, 11, "none"), (257, 513, "every-second"), (768, 1536, "none"), (512, 1025, "first-per"), (0, -1, "none")]


@pytest.mark.parametrize("n_sharp,n_flat,pattern", FUSED, ids=[f"sharp{a}-flat{b}-{c}" if b >= 0 else "borderline" for a, b, c in FUSED])
def test_frame_loops_leave_the_staged_lists_and_votes(api, L64, orc, n_sharp, n_flat, pattern):
    """one frame with n_outer = 1 from the identity at a frame index above 5 (the vote is on): ll_odometry_frames (k_vote) and
    ll_odometry_sequences (k_vote_lm_rows, the lattice as the less-sharp / less-flat clouds of the predecessor slot) leave
    the correspondence lists and the vote of associate + vote, byte for byte, and solve to the same pose"""
    if n_flat < 0:
        idx, flat = vc.lattice_borderline(L64.lat, np.random.default_rng(41), 1)
        q = dict(sharp=(np.zeros(0, np.int64), np.zeros(0, bool), np.zeros((0, 4), np.float32)), flat=(idx, np.zeros(len(idx), bool), flat))
    else:
        q = L64.make(n_sharp, n_flat, pattern, seed=7)
    c = L64.ctx
    L64.upload(0, q["sharp"][2], q["flat"][2])
    c.associate(0, 1, IDENT)
    c.vote(0, 1, True)
    staged = check_slot(L64, orc, 0, q, True)

    def same(got, what):
        for k in ("edge", "plane", "vote"):
            for a, b in zip(got[k], staged[k]):
                assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), (what, k)
        assert got["info"] == staged["info"], what

    L64.upload(0, q["sharp"][2], q["flat"][2])            # fresh per-query results
    pose_f = c.odometry_frames(0, 1, pose0=IDENT, n_outer=1, first_frame_index=6)[0]
    same(L64.lists(0), "ll_odometry_frames")
    off = c.odometry_frames(0, 1, pose0=IDENT, n_outer=1, first_frame_index=5)[0]           # frame 5: no vote yet (:794)
    got = L64.lists(0)
    assert (got["vote"][0] == 0).all() and got["vote"][1].all() and (got["vote"][2] == 1).all() and got["info"][2] == got["info"][1]
    assert off.shape == (7,)

    empty = np.zeros((0, 4), np.float32)
    c.upload_features(0, empty, L64.lat, empty, L64.lat)             # the predecessor: its less-sharp / less-flat clouds are the target
    L64.upload(1, q["sharp"][2], q["flat"][2])
    pose_s = c.odometry_sequences(1, 2, 1, 1, frame_index0=6, pose0=IDENT, n_outer=1)[0, 0]
    same(L64.lists(1), "ll_odometry_sequences")
    assert pose_s.tobytes() == pose_f.tobytes()
    c.set_target(L64.lat, L64.lat)                                   # the carry target again, for the tests that follow


# ------------------------------------------------------------------------------------------------ normal equations
POSE_OFF = np.array([0.004, -0.003, 0.006, 1.0, 0.03, -0.02, 0.025])
POSE_OFF[:4] /= np.linalg.norm(POSE_OFF[:4])

NEQ = ([(0, 0, "none", True), (0, 7, "all", True), (0, 5, "only-last", True), (4, 0, "only-0", True), (1, 1, "none", True)] +
       [(0, n, "none", False) for n in (255, 256, 257, 511, 512, 513)] + [(n, 0, "none", True) for n in (255, 256, 257, 511, 512, 513)] +
       [(85, 1, "none", False), (85, 2, "none", False), (170, 1, "none", False), (171, 0, "none", False), (768, 1536, "none", True), (300, 700, "every-second", True)])


@pytest.mark.parametrize("n_sharp,n_flat,pattern,vote", NEQ)
def test_normal_equations_at_the_row_count_edges(L64, orc, n_sharp, n_flat, pattern, vote):
    """H, g, cost and the number of rows a few centimetres off the identity, from the device's own lists and vote weights;
    offsets up to 0.29 m put residuals on both sides of the Huber radius (0.1)"""
    q = L64.make(n_sharp, n_flat, pattern, seed=3)
    c = L64.ctx
    L64.upload(0, q["sharp"][2], q["flat"][2])
    c.associate(0, 1, IDENT)
    c.vote(0, 1, vote)
    got = check_slot(L64, orc, 0, q, vote)
    c.normal_equations(0, 1, POSE_OFF)
    H, g, cost = c.normal_equations_result(0)
    (es, ea, eb), (ps, pa, pb, pc), (cnt, sel, w) = got["edge"], got["plane"], got["vote"]
    o = np.flatnonzero(sel)
    sharp, flat = q["sharp"][2], q["flat"][2]
    Ho, go, co = orc.normal_equations(POSE_OFF[:4], POSE_OFF[4:], sharp, es, L64.lat, ea, eb, flat, ps[o], L64.lat, pa[o], pb[o], pc[o], w[o], 0.1)
    rows = 3 * len(es) + len(o)
    r, Jq, Jt = c.residual_jacobian(0, POSE_OFF)
    assert len(r) == rows
    if rows == 0:
        assert not H.any() and not g.any() and cost == 0.0
    else:
        assert H.any() and cost > 0
    if rows > 20:
        a = np.abs(r)
        assert (a > 0.1).any() and (a < 0.1).any()                   # both sides of the Huber radius
    close(H, Ho, "H"); close(g, go, "g"); close(cost, co, "cost")
