"""The extract kernels (k_organize / the tile-parallel organise path, k_ring_pick, k_ring_features) against the output of the
reference's OWN scanRegistration.cpp -- the binary that oracle/ref.py builds from the reference's source against declared
container doubles and that travels here in oracle/_ref/ -- not against the oracle's restatement.

Bitwise: laserCloud and scanStartInd / scanEndInd, cloudCurvature and cloudLabel on [5, n-5), the sharp / less-sharp / flat
clouds in order (tie rule and its 5 % condition: tests/refcheck.py).  less_flat is compared ring by ring as the VoxelGrid
INPUT: the points of the ring's six segments whose HIP label is <= 0, taken from HIP's laserCloud, equal what the reference
handed to its VoxelGrid (scanRegistration.cpp:361-367).  The filter's OUTPUT (a4: centroids and their order) stays HIP against
the oracle, as in tests/test_gpu_parity.py: the reference binary's VoxelGrid is a pass-through double and pins nothing there.
"""
import numpy as np
import pytest

import refcheck
from conftest import set_org_path

pytestmark = pytest.mark.gpu

VARIANTS = {"default": dict(), "match_any_sort": dict(voxel_sort_ranks=1), "xyz12": dict(input_stride_floats=3)}   # tests/test_gpu_variants.py's switches
N_SCANS = 3


@pytest.fixture(scope="module")
def ref():
    from oracle import ref as r
    refcheck.require_ref(r)
    return r


_want = {}


def _reference(key, ref, orc, make):
    """the reference's output, once per shape / edge group and point size: (rings, scans as given, results)"""
    if key not in _want:
        rings, scans = make()
        _want[key] = (rings, scans, ref.extract(scans, rings, orc.params(rings).minimum_range, variant="f32"))
    return _want[key]


def _hip(ctx, k):
    cloud, ss, se = ctx.cloud(k)
    lab, cv = ctx.labels(k, curvature=True)
    return dict(cloud=cloud, scan_start=ss, scan_end=se, label=lab, curv=cv, **ctx.features(k))


def _run(api, org, rings, scans, **prm):
    set_org_path(org)
    try:
        ctx = api.Context(api.default_params(rings, batch=len(scans), write_curvature=1, max_points=max(map(len, scans)) + 7, **prm))
        for k, s in enumerate(scans):
            ctx.upload_scan(k, s)
        ctx.extract(0, len(scans))
        ctx.synchronize()
    finally:
        set_org_path("tiles")
    return ctx


@pytest.fixture(scope="module", params=[(s, o, v) for s in refcheck.SHAPES for o in ("tiles", "walk") for v in VARIANTS],
                ids=lambda p: "-".join(p))
def case(request, api, orc, synth, ref):
    shape, org, variant = request.param
    xyz12 = variant == "xyz12"

    def make():
        rings, scans = refcheck.shape_scans(shape, synth, N_SCANS)
        return rings, [np.ascontiguousarray(s[:, :3]) for s in scans] if xyz12 else scans

    rings, scans, want = _reference((shape, xyz12), ref, orc, make)
    extra = dict(max_ring_points=4608) if "HDL64E" in shape else {}
    ctx = _run(api, org, rings, scans, **VARIANTS[variant], **extra)
    yield dict(name="-".join(request.param), ctx=ctx, rings=rings, want=want)
    ctx.close()


def test_kernels_equal_reference_binary(case, ref):
    left = total = 0
    for k, r in enumerate(case["want"]):
        assert case["ctx"].scan_info(k).status == 0
        t, p = refcheck.compare_with_reference(_hip(case["ctx"], k), r, case["rings"], ref.ring_of, f"{case['name']} scan {k}")
        left += t; total += p
    print(f"\n{case['name']}: {left} of {total} rings left out of the pick comparison for curvature ties = {100.0 * left / total:.2f} %")
    assert total >= N_SCANS * case["rings"] // 2
    assert left <= refcheck.MAX_LEFT_OUT * total, f"{case['name']}: ties leave out {left} of {total} rings, more than 5 %"


@pytest.mark.parametrize("org", ["tiles", "walk"])
@pytest.mark.parametrize("rings", [16, 32, 64])
def test_kernels_equal_reference_binary_on_edge_scans(rings, org, api, orc, ref):
    """the edge scans of tests/test_ref_scan_registration.py (ring thresholds, wrap / half sweep, NaN / inf, minimum_range, z axis,
    short rings, more than 20 corners, ring-rejected points), one context per ring count and organise path"""
    def make():
        mr, cases = refcheck.edge_groups(orc, rings)
        assert mr == orc.params(rings).minimum_range
        make.names = [(n, p) for n, _, p in cases]
        return rings, [s for _, s, _ in cases]

    key = ("edge", rings)
    if key not in _want:
        _reference(key, ref, orc, make); _want[key + ("names",)] = make.names
    _, scans, want = _want[key]
    ctx = _run(api, org, rings, scans, max_ring_points=8192)
    try:
        for k, ((name, tests_pick), r) in enumerate(zip(_want[key + ("names",)], want)):
            assert ctx.scan_info(k).status == 0, (name, ctx.scan_info(k).status, ctx.scan_info(k).max_ring)
            left, total = refcheck.compare_with_reference(_hip(ctx, k), r, rings, ref.ring_of, f"{rings}-ring {org} edge scan {name}")
            assert not tests_pick or (left == 0 and total > 0), f"{name}: built to be free of curvature ties"
    finally:
        ctx.close()


@pytest.mark.parametrize("org", ["tiles", "walk"])
@pytest.mark.parametrize("name", ["scanreg_s16", "scanreg_s32", "scanreg_s64_azmajor_jitter_nan"])
def test_kernels_reproduce_recorded_reference_output(name, org, api):
    """the committed recordings of the reference binary's output (tests/golden/reference/, see tests/golden/make_golden.py): needs
    no oracle/_ref/, so this part of the pin holds on every machine with a GPU"""
    import os
    from oracle import ref as refmod                              # ring_of / scan_bounds only: no binary is run
    from test_ref_scan_registration import _golden_module, HERE
    mg = _golden_module()
    G = np.load(os.path.join(HERE, "golden", "reference", name + ".npz"))
    rings, scan = mg.reference_input(name)
    r = dict(cloud=G["cloud"], curv=G["curv"], label=G["label"].astype(np.int32), sharp=G["sharp"], less_sharp=G["less_sharp"], flat=G["flat"])
    r["scan_start"], r["scan_end"] = refmod.scan_bounds(r["cloud"], rings)
    r["voxel_inputs"] = [r["cloud"][idx] for idx in np.split(G["voxel_index"], np.cumsum(G["voxel_count"])[:-1])]
    ctx = _run(api, org, rings, [scan])
    try:
        assert ctx.scan_info(0).status == 0
        left, total = refcheck.compare_with_reference(_hip(ctx, 0), r, rings, refmod.ring_of, f"recorded {name} {org}")
        assert left <= refcheck.MAX_LEFT_OUT * total
    finally:
        ctx.close()
