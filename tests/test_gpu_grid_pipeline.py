"""GPU parity of k_build_grid's two sweeps and the batches they share (through the public API only: the grid has no accessor, so
every case is judged by what k_associate finds in it -- the corner and plane index tuples must equal the oracle's exactly).

Each wave of the kernel walks its block of 64-point chunks in batches of 8.  The batches end-align with the block (the first may be
short); the histogram sweep leaves the wave's last two batches in registers, the scatter sweep starts with them and reads only the
batches in front of them again.  The shapes below are the smallest at which that can go wrong: fewer chunks than the sixteen waves;
exactly one batch per wave (16 * 8 chunks: nothing read twice); one chunk more (two batches, the first short, both kept); 17 and 25
chunks per wave (one and two batches read again, the loop in front of the kept ones runs once and twice); chunk ends at, one before
and one behind a multiple of 64; ring rows that are empty in the middle and at the end of a scan; a refused scan inside a batch that
is no multiple of 8; points in the border cells; ring values that run backwards.  Every target is searched twice: as the clouds of a
slot (slot k's target is slot k - 1) and as the carry (ll_set_target / ll_set_target_from_slot)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

POSE = np.array([0.001, -0.002, 0.004, 1.0, 0.8, 0.02, -0.01])
POSE[:4] /= np.linalg.norm(POSE[:4])
EMPTY = np.zeros((0, 4), np.float32)
CHUNK, WAVES, UN = 64, 16, 8                       # points per chunk, waves per workgroup, chunks per batch


def _corr(ctx, k):
    return tuple(ctx.edge_corr(k)) + tuple(ctx.plane_corr(k))


def _want(orc, pose, cur, corner, surf):
    q, t = pose[:4], pose[4:]
    return tuple(orc.associate_corner(q, t, cur["sharp"], corner)) + tuple(orc.associate_plane(q, t, cur["flat"], surf))


def _same(got, want, what):
    for g, w, nm in zip(got, want, ("e_src", "e_a", "e_b", "p_src", "p_a", "p_b", "p_c")):
        assert len(g) == len(w) and (g == w).all(), (what, nm)


@pytest.fixture(scope="module")
def pair(api, orc, synth):
    """Slot 1 holds the queries (scan 1's features) for good; slot 0 and the carry take the targets of the cases."""
    cfg = synth.default_cfg(64)
    s0, s1 = synth.scan(cfg, 0), synth.scan(cfg, 1)
    P = orc.params(64)
    e0, e1 = orc.extract(s0, P), orc.extract(s1, P)
    ctx = api.Context(api.default_params(64, batch=2, max_points=max(len(s0), len(s1))))
    ctx.upload_features(1, e1["sharp"], e1["less_sharp"], e1["flat"], e1["less_flat"])
    orc.set_nn_mode(1)
    yield dict(ctx=ctx, e0=e0, e1=e1, s0=s0, s1=s1)
    orc.set_nn_mode(0)
    ctx.close()


def both_ways(pair, orc, corner, surf, pose=POSE, what=""):
    """The target (corner, surf) as slot 0's clouds and as the carry; slot 1's correspondences against the oracle both times."""
    ctx, e0 = pair["ctx"], pair["e0"]
    want = _want(orc, pose, pair["e1"], corner, surf)
    ctx.set_target(EMPTY, EMPTY)                                      # slot 0's own target: nothing
    ctx.upload_features(0, e0["sharp"], corner, e0["flat"], surf)
    ctx.associate(0, 2, pose); ctx.vote(0, 2, True)
    _same(_corr(ctx, 1), want, what + " as a slot")
    assert ctx.pair_info(0).n_plane == 0 and ctx.pair_info(0).n_edge == 0
    ctx.set_target(corner, surf)
    ctx.associate(1, 1, pose); ctx.vote(1, 1, True)
    _same(_corr(ctx, 1), want, what + " as the carry")
    return want


def _spread(cloud, n):
    """n points of the cloud, evenly spread over it, order kept (so the rings stay sorted and the points cover the scene)."""
    return cloud[np.linspace(0, len(cloud) - 1, n).astype(np.int64)] if n else cloud[:0]


SIZES = [0, 1, 63, 64, 65, WAVES * CHUNK - 1, WAVES * CHUNK, WAVES * CHUNK + 1, UN * WAVES * CHUNK, UN * WAVES * CHUNK + 1,
         2 * UN * WAVES * CHUNK + 1, 3 * UN * WAVES * CHUNK + 1]


@pytest.mark.parametrize("n_flat", SIZES)
def test_uploaded_less_flat_clouds_of_exact_sizes(pair, orc, n_flat):
    """Contiguous less-flat clouds of 0 .. 3 * 8 * 16 * 64 + 1 points (1 .. 4 batches per wave), each with the less-sharp cloud empty, of one point and full
    (7680 points: 64 rings x 120, every point twice so that equal distances occur -- lowest index wins)."""
    e0 = pair["e0"]
    assert len(e0["less_flat"]) >= SIZES[-1] and 2 * len(e0["less_sharp"]) >= 7680
    surf = _spread(e0["less_flat"], n_flat)
    found = 0
    for corner in (EMPTY, e0["less_sharp"][len(e0["less_sharp"]) // 2:][:1], np.repeat(e0["less_sharp"], 2, axis=0)[:7680]):
        want = both_ways(pair, orc, corner, surf, what=f"{n_flat} less-flat, {len(corner)} less-sharp points")
        found = max(found, len(want[3]))
        if len(corner) == 7680:
            assert len(want[0]) > 100
    if n_flat >= WAVES * CHUNK:
        assert found > 50                           # the case does exercise the search: plane correspondences exist


def test_targets_beyond_the_grid(pair, orc):
    """x, y scaled by 1.5: returns out to 180 m saturate into the border cells of the 128 x 128 grid."""
    c = pair["e0"]["less_sharp"].copy(); s = pair["e0"]["less_flat"].copy()
    c[:, :2] *= 1.5; s[:, :2] *= 1.5
    assert np.abs(s[:, :2]).max() > 64.0
    for pose in ([0, 0, 0, 1, 0, 0, 0], [0, 0, 0.7071, 0.7071, 60, 40, 0], [0, 0, 0, 1, 150, 100, 0]):
        p = np.array(pose, float); p[:4] /= np.linalg.norm(p[:4])
        both_ways(pair, orc, c, s, pose=p, what=f"beyond the grid, pose {pose}")


def test_ring_values_decreasing_along_the_cloud(pair, orc):
    """Ring values that step DOWN along the cloud: the grid's "ring values never decrease" bit (flag bit 1) must come out clear -- with
    it set, k_associate would take a place window for a ring and name other points than the oracle.  Once with every second ring
    boundary a step down (rings stored 1, 0, 3, 2, ...: most queries still find their partners, a few no longer do), once with the
    whole cloud back to front (the reference's walks then meet no partner at all, although every query has a nearest neighbour)."""
    e0 = pair["e0"]

    def swapped(a):
        r = a[:, 3].astype(np.int32)
        return np.concatenate([a[r == (v ^ 1)] for v in range(64)])

    c, s = swapped(e0["less_sharp"]), swapped(e0["less_flat"])
    assert (np.diff(s[:, 3].astype(np.int32)) < 0).sum() >= 16
    want = both_ways(pair, orc, c, s, what="ring pairs swapped")
    assert len(want[0]) > 100 and len(want[3]) > 100
    c = e0["less_sharp"][::-1].copy(); s = e0["less_flat"][::-1].copy()
    assert (np.diff(s[:, 3].astype(np.int32)) < 0).any() and (np.diff(s[:, 3].astype(np.int32)) <= 0).all()
    want = both_ways(pair, orc, c, s, what="rings decreasing")
    assert len(want[0]) == 0 and len(want[3]) == 0


def test_sixteen_ring_batch_of_nine_with_a_refused_scan_and_empty_rows(api, orc):
    """Nine extracted 16-ring scans (no multiple of 8) whose ring rows are ragged: rows missing in the middle and at the end of a scan,
    rows ending on, before and behind a chunk edge.  Scan 4 has no point beyond the minimum range: refused, it is nobody's target and has
    no correspondences.  Slot k against slot k - 1 (ring rows, places), then every slot once more against the carry copy of its
    predecessor (contiguous)."""
    from test_gpu_parity import _vlp16_ring, _ring_scan
    rng = np.random.default_rng(707)
    counts = [3, 63, 64, 65, 127, 128, 129, 250, 400, 513]
    scans = []
    for s in range(9):
        rings = []
        for k in range(16):
            if k in ((5, 6, 9) if s % 2 else (2, 10)) or (s in (2, 7) and k >= 13):        # empty rows: middle / end of the scan
                continue
            n = int(rng.choice(counts))
            base = rng.uniform(2.0, 12.0)
            r = base * (1.0 + rng.uniform(0.0005, 0.01) * np.cumsum(rng.standard_normal(n)))
            r = np.where(rng.random(n) < rng.uniform(0.0, 0.3), r * rng.uniform(1.2, 2.0), r)
            rings.append(_vlp16_ring(-15 + 2 * k, n, np.abs(r) + 0.35, phase=rng.random()))
        scans.append(_ring_scan(rings))
    scans[4][:, :3] *= 0.2 / np.linalg.norm(scans[4][:, :3], axis=1).max()                   # everything inside the minimum range
    P = orc.params(16, minimum_range=0.3)
    refs = [orc.extract(sc, P) for sc in scans]
    assert refs[4]["rc"] != 0 and all(refs[k]["rc"] == 0 for k in range(9) if k != 4)
    none = dict(less_sharp=EMPTY, less_flat=EMPTY)
    pose = np.array([0.0, 0.0, 0.002, 1.0, 0.05, -0.02, 0.0]); pose[:4] /= np.linalg.norm(pose[:4])
    ctx = api.Context(api.default_params(16, batch=9, max_points=max(map(len, scans)) + 8, minimum_range=0.3))
    orc.set_nn_mode(1)
    try:
        for k, sc in enumerate(scans):
            ctx.upload_scan(k, sc)
        ctx.extract(0, 9)
        assert ctx.scan_info(4).status != 0
        ctx.set_target_from_slot(8)
        ctx.associate(0, 9, pose); ctx.vote(0, 9, False)
        planes = 0
        for k in range(9):
            if k == 4:
                continue
            tgt = refs[k - 1] if k != 5 else none                      # slot 0's target is the carry (slot 8's clouds)
            want = _want(orc, pose, refs[k], tgt["less_sharp"], tgt["less_flat"])
            _same(_corr(ctx, k), want, f"slot {k} against slot {k - 1}")
            planes += len(want[3])
        assert planes > 50
        for k in (1, 3, 5, 8):                                         # the same targets through the carry
            ctx.set_target_from_slot(k - 1)
            ctx.associate(k, 1, pose); ctx.vote(k, 1, False)
            tgt = refs[k - 1] if k != 5 else none
            _same(_corr(ctx, k), _want(orc, pose, refs[k], tgt["less_sharp"], tgt["less_flat"]), f"slot {k} against the carry of slot {k - 1}")
    finally:
        orc.set_nn_mode(0)
        ctx.close()


def test_two_stream_association_stage_gives_the_same_and_the_oracles_tuples(api, orc, synth):
    """ll_hot_path_batch over 520 scans (>= 512, no multiple of the piece size) with the association stage on two streams: the grids
    of one piece are built beside the search of the piece before.  Same tuples as kernel after kernel, and the oracle's."""
    rings, B = 16, 520
    cfg = synth.default_cfg(rings)
    scans = [synth.scan(cfg, k) for k in range(5)]
    P = orc.params(rings)
    refs = [orc.extract(s, P) for s in scans]
    ctx = api.Context(api.default_params(rings, batch=B + 1, max_points=max(map(len, scans))))
    ctx.upload_scan(B, scans[0]); ctx.extract(B, 1); ctx.set_target_from_slot(B)
    for i in range(B):
        ctx.upload_scan(i, scans[(i + 1) % 5])                          # slot i's target: slot i - 1 = scan i % 5 (slot 0: the carry = scan 0)
    pose = np.array([0, 0, 0, 1, 0.9, 0.0, 0.0])
    ctx.set_pose_guess(0, B, np.tile(pose, (B, 1)))
    look = (0, 1, 129, 130, 259, 260, 389, 390, B - 1)

    def run(on):
        ctx.set_two_stream(on)
        ctx.hot_path(0, B, None, vote=True); ctx.synchronize()
        return [_corr(ctx, i) for i in look]

    one, two = run(False), run(True)
    orc.set_nn_mode(1)
    try:
        for i, a, b in zip(look, one, two):
            want = _want(orc, pose, refs[(i + 1) % 5], refs[i % 5]["less_sharp"], refs[i % 5]["less_flat"])
            _same(a, want, f"slot {i}, one stream"); _same(b, want, f"slot {i}, two streams")
            assert len(want[0]) > 10 and len(want[3]) > 10
    finally:
        orc.set_nn_mode(0)
        ctx.close()


def test_extracted_sixty_four_and_128_ring_targets(api, orc, synth):
    """An extracted 64-ring pair (about 100 less-sharp and 520 less-flat chunks per scan, the headline's shape: 5 batches per wave, 3
    read again) and a 128-ring pair (twice the ring rows; its less-flat cloud is past 64 chunks per wave: 9 batches or more), slot
    against slot and against the carry.  Every less-sharp cloud stays within the two kept batches and is read once."""
    for rings, extra in ((64, {}), (128, dict(ring_model=1, lower_bound=-25.0, up_bound=15.0, minimum_range=0.3))):
        cfg = synth.default_cfg(rings)
        scans = [synth.scan(cfg, k) for k in range(3)]
        P = orc.params(rings, **extra)
        refs = [orc.extract(s, P) for s in scans]
        ctx = api.Context(api.default_params(rings, batch=3, max_points=max(map(len, scans)), **extra))
        orc.set_nn_mode(1)
        try:
            for k, sc in enumerate(scans):
                ctx.upload_scan(k, sc)
            ctx.extract(0, 3)
            ctx.set_target_from_slot(2)
            ctx.associate(0, 3, POSE); ctx.vote(0, 3, True)
            for k in range(3):
                tgt = refs[k - 1]                                        # slot 0: the carry = slot 2's clouds
                want = _want(orc, POSE, refs[k], tgt["less_sharp"], tgt["less_flat"])
                _same(_corr(ctx, k), want, f"{rings} rings, slot {k}")
                assert len(want[0]) > 100 and len(want[3]) > 100
            if rings == 128:
                assert min(len(r["less_flat"]) for r in refs) > 64 * WAVES * CHUNK
        finally:
            orc.set_nn_mode(0)
            ctx.close()
