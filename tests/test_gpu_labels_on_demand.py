"""cloudLabel is no longer stored by k_ring_pick: ll_download_labels rebuilds a slot's labels from the pick's per-ring lists
(ring_off, ring_rec, ring_cnt: per segment the first n_sharp less-sharp entries 2, the other less-sharp entries 1, the flat
entries -1, everything else 0) into a context-owned scratch and copies that out.  What ctx.labels(slot) returns must equal the
oracle's labels byte for byte -- the oracle's array is zero outside [5, n - 5), where the reference writes nothing, and so is the
device's -- whatever organise path, pick kernel (the common six-row launch or a tier's) and call order produced the lists."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _same_labels(ctx, slot, ref, what):
    lab = ctx.labels(slot)
    assert lab.dtype == np.int8 and len(lab) == len(ref["label"]), what
    want = ref["label"].astype(np.int8)
    assert (want[:5] == 0).all() and (want[len(want) - 5:] == 0).all()
    bad = np.flatnonzero(lab != want)
    assert len(bad) == 0, f"{what}: {len(bad)} labels differ, first at {bad[:5].tolist()}: {lab[bad[:5]].tolist()} vs {want[bad[:5]].tolist()}"
    return want


@pytest.fixture(scope="module")
def s64(orc, synth):
    cfg = synth.default_cfg(64)
    scans = [synth.scan(cfg, k) for k in range(2)]
    P = orc.params(64)
    return dict(scans=scans, refs=[orc.extract(s, P) for s in scans])


@pytest.fixture(scope="module")
def s16(orc, synth):
    cfg = synth.default_cfg(16)
    scans = [synth.scan(cfg, k) for k in range(3)]
    P = orc.params(16)
    return dict(scans=scans, refs=[orc.extract(s, P) for s in scans])


def test_sixty_four_ring_scans_in_one_small_call(api, s64):
    """At most 64 scans per call: the tile-parallel organise kernels."""
    scans, refs = s64["scans"], s64["refs"]
    ctx = api.Context(api.default_params(64, batch=2, max_points=max(map(len, scans))))
    try:
        for k, sc in enumerate(scans):
            ctx.upload_scan(k, sc)
        ctx.extract(0, 2)
        for k in (1, 0, 1):                                               # the scratch is one slot's: every download rebuilds it
            want = _same_labels(ctx, k, refs[k], f"64 rings, slot {k}")
            assert (want == 2).sum() > 100 and (want == 1).sum() > 1000 and (want == -1).sum() > 100
    finally:
        ctx.close()


def test_sixty_five_sixteen_ring_scans_in_one_call(api, s16):
    """65 scans in one call: k_organize, one workgroup per scan."""
    scans, refs = s16["scans"], s16["refs"]
    B = 65
    ctx = api.Context(api.default_params(16, batch=B, max_points=max(map(len, scans))))
    try:
        for k in range(B):
            ctx.upload_scan(k, scans[k % 3])
        ctx.extract(0, B)
        for k in (0, 1, 2, 31, 63, 64):
            want = _same_labels(ctx, k, refs[k % 3], f"16 rings, 65 scans, slot {k}")
            assert (want == 2).sum() > 20 and (want == -1).sum() > 20
    finally:
        ctx.close()


def test_rings_shorter_than_seventeen_points_and_empty_rings(api, orc):
    """Rings of 3 .. 16 points have no segment (their labels stay 0, their counts are written as 0), rings 2 and 10 are missing
    altogether, the others carry picks."""
    from test_gpu_parity import _vlp16_ring, _ring_scan
    rng = np.random.default_rng(88)
    lengths = [3, 16, 0, 17, 130, 9, 400, 11, 64, 12, 0, 250, 5, 65, 129, 47]
    rings = []
    for k, n in enumerate(lengths):
        if n == 0:
            continue
        base = rng.uniform(2.0, 10.0)
        r = base * (1.0 + 0.004 * np.cumsum(rng.standard_normal(n)))
        r = np.where(rng.random(n) < 0.15, r * 1.5, r)
        rings.append(_vlp16_ring(-15 + 2 * k, n, np.abs(r) + 0.35, phase=rng.random()))
    scan = _ring_scan(rings)
    ref = orc.extract(scan, orc.params(16, minimum_range=0.3))
    assert ref["rc"] == 0
    ctx = api.Context(api.default_params(16, batch=1, max_points=len(scan) + 8, minimum_range=0.3))
    try:
        ctx.upload_scan(0, scan)
        ctx.extract(0, 1)
        want = _same_labels(ctx, 0, ref, "short and empty rings")
        assert (want != 0).sum() > 20
        ss, se = ref["scan_start"], ref["scan_end"]
        assert sum(1 for a, b in zip(ss, se) if b - a < 6) >= 8           # rings without segments are in the scan
    finally:
        ctx.close()


def test_segments_with_equal_curvatures(api, orc):
    """The square room of the parity tests: hundreds of equal curvatures per segment, picks decided by the index."""
    from test_gpu_parity import _square_room_ring, _ring_scan
    rings = [_square_room_ring(z=round(8.0 * np.tan(np.deg2rad(-15 + 2 * k)) * 32) / 32, step=1.0 / 16) for k in range(16)]
    scan = _ring_scan(rings)
    ref = orc.extract(scan, orc.params(16, minimum_range=0.3))
    assert ref["rc"] == 0 and len(np.unique(ref["curv"][5:-5])) < 0.03 * len(ref["curv"])
    ctx = api.Context(api.default_params(16, batch=1, max_points=len(scan) + 8, minimum_range=0.3))
    try:
        ctx.upload_scan(0, scan)
        ctx.extract(0, 1)
        want = _same_labels(ctx, 0, ref, "equal curvatures")
        assert (want == 2).sum() > 50 and (want == -1).sum() > 100
    finally:
        ctx.close()


def test_hdl64_scan_through_the_tier_kernels(api, orc):
    """max_ring_points = 4608 and the HDL-64E table scan: rings beyond 2304 points are picked by the tier launches."""
    import scangen
    scan = scangen.hdl64_scan(0, order="kitti")
    ref = orc.extract(scan, orc.params(64))
    assert ref["rc"] == 0
    assert int((ref["scan_end"] - ref["scan_start"]).max()) + 11 > 2304   # a ring of a tier is in the scan
    ctx = api.Context(api.default_params(64, batch=1, max_points=len(scan) + 7, max_ring_points=4608))
    try:
        ctx.upload_scan(0, scan)
        ctx.extract(0, 1)
        assert ctx.scan_info(0).status == 0
        want = _same_labels(ctx, 0, ref, "hdl64, tiers")
        assert (want == 2).sum() > 100 and (want == -1).sum() > 100
    finally:
        ctx.close()


def test_slot_downloaded_after_a_later_hot_path_over_other_slots(api, s16):
    """Slot 0 is extracted, then slots 1 .. 3 go through the whole hot path (extract, grids, association, vote, solve): slot 0's
    lists are untouched and its labels come out as before; the later slots' labels are theirs."""
    scans, refs = s16["scans"], s16["refs"]
    ctx = api.Context(api.default_params(16, batch=4, max_points=max(map(len, scans))))
    try:
        ctx.upload_scan(0, scans[0])
        ctx.extract(0, 1)
        ctx.set_target_from_slot(0)
        for k in (1, 2, 3):
            ctx.upload_scan(k, scans[k % 3])
        ctx.hot_path(1, 3, np.array([0, 0, 0, 1, 0.9, 0.0, 0.0]), vote=True)
        ctx.synchronize()
        _same_labels(ctx, 0, refs[0], "slot 0 after a hot path over slots 1 .. 3")
        for k in (3, 1, 2):
            _same_labels(ctx, k, refs[k % 3], f"slot {k} of the hot path")
        _same_labels(ctx, 0, refs[0], "slot 0 again")
    finally:
        ctx.close()


def test_slot_refilled_by_upload_features_has_no_labels(api, s16):
    """ll_upload_features makes the slot a scan of no points (n = 0): ll_download_labels succeeds and returns nothing, as before."""
    scans, refs = s16["scans"], s16["refs"]
    ctx = api.Context(api.default_params(16, batch=2, max_points=max(map(len, scans))))
    try:
        for k in range(2):
            ctx.upload_scan(k, scans[k])
        ctx.extract(0, 2)
        e = refs[1]
        ctx.upload_features(0, e["sharp"], e["less_sharp"], e["flat"], e["less_flat"])
        assert ctx.scan_info(0).n == 0
        lab = ctx.labels(0)
        assert lab.dtype == np.int8 and len(lab) == 0
        _same_labels(ctx, 1, refs[1], "the neighbour of the refilled slot")
    finally:
        ctx.close()


def test_refused_scan_returns_its_status(api, orc, s16):
    """A ring longer than max_ring_points: the scan is refused (LL_ERR_CAPACITY in the slot's status).  ll_download_labels hands that
    status back, as ll_download_cloud does, and the neighbours' labels are not affected."""
    scans = s16["scans"]
    thin = [scans[0][::2].copy(), scans[2][::2].copy()]                   # ring-major scans: every ring at half its points (<= 1024)
    P = orc.params(16)
    refs = [orc.extract(t, P) for t in thin]
    assert all(r["rc"] == 0 for r in refs) and int((refs[0]["scan_end"] - refs[0]["scan_start"]).max()) + 11 <= 1024
    ctx = api.Context(api.default_params(16, batch=3, max_points=max(map(len, scans)), max_ring_points=1024))
    try:
        ctx.upload_scan(0, thin[0]); ctx.upload_scan(1, scans[1]); ctx.upload_scan(2, thin[1])
        ctx.extract(0, 3)
        assert ctx.scan_info(1).status == -4 and ctx.scan_info(0).status == 0 and ctx.scan_info(2).status == 0
        with pytest.raises(api.LightLoamError) as from_labels:
            ctx.labels(1)
        with pytest.raises(api.LightLoamError) as from_cloud:
            ctx.cloud(1)
        assert from_labels.value.code == -4 and from_cloud.value.code == -4          # LL_ERR_CAPACITY: the slot's status
        _same_labels(ctx, 0, refs[0], "before the refused scan")
        _same_labels(ctx, 2, refs[1], "behind the refused scan")
    finally:
        ctx.close()
