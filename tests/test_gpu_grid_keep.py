"""GPU parity of what k_build_grid keeps of a wave's block of chunks between its two sweeps (through the public API only: the grid
has no accessor, so every case is judged by what k_associate finds in it -- the corner and plane index tuples must equal the
oracle's exactly; every target is searched once as a slot's clouds and once as the carry).

Each of the kernel's 16 waves walks its block of 64-point chunks in batches of 8, end-aligned with the block.  Of the block's end,
the last K chunks (three batches) stay in registers, narrowed to x, y, z and the low byte of int(w); the S chunks in front of them
wait in the wave's piece of LDS as whole points; only what lies in front of those is read again by the scatter sweep, in batches
end-aligned with the stash.  The ring tables and the out-of-range flag come from the full w in the histogram sweep.  The sizes
below put K, K + 1, K + S, K + S + 1 (nothing, then one chunk read again), K + S + 8 and K + S + 9 (one and two batches read
again) chunks on every wave, each also one point short of and one point past a whole chunk."""
import numpy as np
import pytest

from test_gpu_grid_pipeline import EMPTY, POSE, _corr, _same, _want, both_ways

pytestmark = pytest.mark.gpu

CHUNK, WAVES, UN = 64, 16, 8                       # points per chunk, waves per workgroup, chunks per batch
K = 3 * UN                                         # chunks per wave kept in registers between the sweeps (LL_GRID_KEEP batches)
S = 5                                              # chunks per wave stashed in LDS on MI355X: (160 KB - 68 KB histogram - 4.2 KB static) / 16 waves / 1 KB
PER_WAVE = [K, K + 1, K + S, K + S + 1, K + S + UN, K + S + UN + 1]
SIZES = [c * WAVES * CHUNK + d for c in PER_WAVE for d in (-1, 0, 1)]


def _chunks_per_wave(ring_counts):
    """of a ring-strided cloud: every ring row is ceil(n / 64) chunks, dealt to the waves in equal blocks"""
    nch = int(sum((int(n) + CHUNK - 1) // CHUNK for n in ring_counts))
    return (nch + WAVES - 1) // WAVES


@pytest.fixture(scope="module")
def pair(api, orc, synth):
    """Slot 1 holds the queries (scan 1's features) for good; slot 0 and the carry take the targets of the cases."""
    cfg = synth.default_cfg(64)
    s0, s1 = synth.scan(cfg, 0), synth.scan(cfg, 1)
    P = orc.params(64)
    e0, e1 = orc.extract(s0, P), orc.extract(s1, P)
    assert max(len(s0), len(s1)) >= SIZES[-1]
    ctx = api.Context(api.default_params(64, batch=2, max_points=max(len(s0), len(s1))))
    ctx.upload_features(1, e1["sharp"], e1["less_sharp"], e1["flat"], e1["less_flat"])
    orc.set_nn_mode(1)
    yield dict(ctx=ctx, e0=e0, e1=e1)
    orc.set_nn_mode(0)
    ctx.close()


@pytest.mark.parametrize("n_flat", SIZES)
def test_uploaded_less_flat_clouds_around_kept_and_stashed_chunks(pair, orc, n_flat):
    """Contiguous less-flat clouds of K .. K + S + 9 chunks per wave (+-1 point): the extracted cloud, every point repeated as often
    as the size needs (the rings stay sorted; equal distances resolve to the lowest index), each with an empty, a one-point and a
    full (7680-point) less-sharp cloud."""
    e0 = pair["e0"]
    lf = e0["less_flat"]
    rep = (n_flat + len(lf) - 1) // len(lf)
    surf = (np.repeat(lf, rep, axis=0) if rep > 1 else lf)
    surf = surf[np.linspace(0, len(surf) - 1, n_flat).astype(np.int64)]
    assert len(surf) == n_flat and (np.diff(surf[:, 3].astype(np.int32)) >= 0).all()
    found = 0
    for corner in (EMPTY, e0["less_sharp"][len(e0["less_sharp"]) // 2:][:1], np.repeat(e0["less_sharp"], 2, axis=0)[:7680]):
        want = both_ways(pair, orc, corner, surf, what=f"{n_flat} less-flat, {len(corner)} less-sharp points")
        found = max(found, len(want[3]))
        if len(corner) == 7680:
            assert len(want[0]) > 100
    assert found > 50                               # the case does exercise the search: plane correspondences exist


def _edge_rings(a, lowest):
    """ring r of an extracted 64-ring cloud -> 2 (r - lowest), at least 0; the last ring (63) -> 127; the fraction stays"""
    a = a.copy()
    r = a[:, 3].astype(np.int32)
    a[:, 3] = np.where(r == 63, 127, 2 * np.maximum(r - lowest, 0)).astype(np.float32) + (a[:, 3] - r)
    return a


def _ring_edge_cloud(lf, lowest, out_of_range):
    """The extracted less-flat cloud (33 chunks or so per wave as an upload: a few read again, 5 stashed, 24 kept) with its ring
    values moved to the edges of what the tables hold: its lowest ring becomes 0, the last one 127, the others even values between.
    out_of_range: values beyond the tables (160 and above, among them 256 and 300, whose low bytes 0 and 44 are ring values of the
    cloud) in a chunk that is read again, a stashed and a kept one of wave 8 and at the cloud's end, and a negative intensity in
    front."""
    s = _edge_rings(lf, lowest)
    if out_of_range:
        per_wave = ((len(s) + CHUNK - 1) // CHUNK + WAVES - 1) // WAVES
        assert per_wave > K + S
        c0 = 8 * per_wave
        front, stashed, kept = c0 + 1, c0 + per_wave - K - 2, c0 + per_wave - 5
        s[front * CHUNK + 10, 3] = 300.75
        s[stashed * CHUNK + 20, 3] = 256.0
        s[kept * CHUNK + 30, 3] = 161.5
        s[-3:, 3] = [160.25, 200.5, 255.0]
        s[0, 3] = -1.5
    return s


@pytest.mark.parametrize("out_of_range", [False, True], ids=["0..127", "beyond the tables"])
def test_ring_values_at_the_edges(pair, orc, out_of_range):
    """Ring values 0 and 127 leave the tables valid; values of 160 and more and a negative intensity clear the flag (the walks then
    scan the window point by point).  A table or a flag taken from the narrowed byte would see rings 0 and 44 where the cloud has
    256 and 300, and ring 255 for the negative intensity."""
    e0 = pair["e0"]
    lowest = int(e0["less_flat"][:, 3].min())
    surf = _ring_edge_cloud(e0["less_flat"], lowest, out_of_range)
    assert int(surf[1, 3]) == 0 and (surf[:, 3].astype(np.int32) == 127).any()
    corner = _edge_rings(e0["less_sharp"], lowest)
    if out_of_range:
        corner[len(corner) // 2, 3] = 256.0
        corner[-1, 3] = 300.75
        corner[0, 3] = -1.5
    ctx, e1 = pair["ctx"], pair["e1"]
    q = dict(e1, sharp=_edge_rings(e1["sharp"], lowest), flat=_edge_rings(e1["flat"], lowest))   # the queries' rings follow the targets'
    ctx.upload_features(1, q["sharp"], q["less_sharp"], q["flat"], q["less_flat"])
    try:
        shadow = dict(pair, e1=q)
        want = both_ways(shadow, orc, corner, surf, what="ring values at the edges" + (", out of range" if out_of_range else ""))
        if not out_of_range:
            assert len(want[0]) > 100 and len(want[3]) > 100
    finally:
        ctx.upload_features(1, e1["sharp"], e1["less_sharp"], e1["flat"], e1["less_flat"])


def test_extracted_sixty_four_and_128_ring_targets(api, orc, synth):
    """Extracted pairs, ring-strided rows: 64 rings (the headline's shape: more than K + S chunks per wave, one batch read again) and
    128 rings (past K + S + 2 UN: several batches read again), slot against slot and against the carry."""
    for rings, extra, least in ((64, {}, K + S + 1), (128, dict(ring_model=1, lower_bound=-25.0, up_bound=15.0, minimum_range=0.3), K + S + 2 * UN + 1)):
        cfg = synth.default_cfg(rings)
        scans = [synth.scan(cfg, k) for k in range(3)]
        P = orc.params(rings, **extra)
        refs = [orc.extract(s, P) for s in scans]
        for r in refs:
            cpw = _chunks_per_wave(np.bincount(r["less_flat"][:, 3].astype(np.int32), minlength=rings))
            print(f"{rings} rings: {cpw} less-flat chunks per wave")
            assert cpw >= least
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
        finally:
            orc.set_nn_mode(0)
            ctx.close()


def test_sixteen_ring_batch_of_eleven_with_a_refused_scan(api, orc):
    """Eleven extracted 16-ring scans (no multiple of 8) with ragged ring rows; scan 6 has no point beyond the minimum range: refused,
    it is nobody's target and has no correspondences.  Slot k against slot k - 1, then some slots against the carry copy."""
    from test_gpu_parity import _vlp16_ring, _ring_scan
    rng = np.random.default_rng(808)
    counts = [3, 63, 64, 65, 127, 128, 129, 250, 400, 513, 900]
    scans = []
    for s in range(11):
        rings = []
        for k in range(16):
            if k in ((4, 11) if s % 2 else (7,)) or (s == 3 and k >= 14):
                continue
            n = int(rng.choice(counts))
            base = rng.uniform(2.0, 12.0)
            r = base * (1.0 + rng.uniform(0.0005, 0.01) * np.cumsum(rng.standard_normal(n)))
            r = np.where(rng.random(n) < rng.uniform(0.0, 0.3), r * rng.uniform(1.2, 2.0), r)
            rings.append(_vlp16_ring(-15 + 2 * k, n, np.abs(r) + 0.35, phase=rng.random()))
        scans.append(_ring_scan(rings))
    scans[6][:, :3] *= 0.2 / np.linalg.norm(scans[6][:, :3], axis=1).max()
    P = orc.params(16, minimum_range=0.3)
    refs = [orc.extract(sc, P) for sc in scans]
    assert refs[6]["rc"] != 0 and all(refs[k]["rc"] == 0 for k in range(11) if k != 6)
    none = dict(less_sharp=EMPTY, less_flat=EMPTY)
    pose = np.array([0.0, 0.0, 0.002, 1.0, 0.05, -0.02, 0.0]); pose[:4] /= np.linalg.norm(pose[:4])
    ctx = api.Context(api.default_params(16, batch=11, max_points=max(map(len, scans)) + 8, minimum_range=0.3))
    orc.set_nn_mode(1)
    try:
        for k, sc in enumerate(scans):
            ctx.upload_scan(k, sc)
        ctx.extract(0, 11)
        assert ctx.scan_info(6).status != 0
        ctx.set_target_from_slot(10)
        ctx.associate(0, 11, pose); ctx.vote(0, 11, False)
        planes = 0
        for k in range(11):
            if k == 6:
                continue
            tgt = refs[k - 1] if k != 7 else none                      # slot 0's target is the carry (slot 10's clouds)
            want = _want(orc, pose, refs[k], tgt["less_sharp"], tgt["less_flat"])
            _same(_corr(ctx, k), want, f"slot {k} against slot {k - 1}")
            planes += len(want[3])
        assert planes > 50
        for k in (1, 7, 10):                                           # the same targets through the carry
            ctx.set_target_from_slot(k - 1)
            ctx.associate(k, 1, pose); ctx.vote(k, 1, False)
            tgt = refs[k - 1] if k != 7 else none
            _same(_corr(ctx, k), _want(orc, pose, refs[k], tgt["less_sharp"], tgt["less_flat"]), f"slot {k} against the carry of slot {k - 1}")
    finally:
        orc.set_nn_mode(0)
        ctx.close()
