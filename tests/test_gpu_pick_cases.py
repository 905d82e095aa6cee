"""The per-segment feature pick on the device (k_ring_pick6 / 8 / 12 / 22 of ll_pick.hip, read back through k_ring_features and k_labels)
against the independent numpy reference of pickcases.py, at crafted rings: every case goes through Context.upload_scan, extract,
scan_info, cloud, labels(curvature=True) and features and must equal np_pick EXACTLY -- curvature bits over [5, n - 5), labels over
[5, n - 5) and zero outside, the sharp, less-sharp and flat clouds point for point in pick order, the counts of scan_info.  There is no
tolerance and no case is excluded.  The less-flat cloud is compared with the oracle where the thresholds are the defaults (the oracle has
no threshold parameters), so that the net stays closed behind the pick.  test_pick_cases.py shows on the CPU which route of the kernel
each family forces; a failing id names the case, the case's family names the route.

The ways a case is run:
  (a) alone in a context of batch 1, curvature written;
  (b) the default-threshold cases again without the curvature output (the kernel's other code path): same labels and clouds;
  (c) eleven slots in one extract(0, 11) -- a count that is no multiple of the eight slots a block group serves --, ten different cases and
      one scan with nothing beyond the minimum range (refused); every good slot equals its reference, which is what it gave alone;
  (d) extract(3, 5) on that context after slots 3..7 took other cases: they equal their new references, slots 0..2 and 8..10 keep the old;
  (e) stale state: one slot of a max_ring_points = 4608 context takes long feature-rich rings, then short / under 17 points / empty rings
      in the same places, then the first scan again; each time it equals the reference and a fresh context;
  (f) the tier scans at max_ring_points = 2304 are refused with LL_ERR_CAPACITY, as the header documents for a ring longer than that.

On an MI355X every case was equal in all these ways as the kernels stand (40 tests, 2.5 s; test_gpu_assoc_cases.py on the same machine:
71 tests, 8.5 s).  Fourteen scratch mutants of ll_pick.hip that cannot index out of bounds (the list is in DESIGN.md, section 6) each
failed at least one family here.
"""
import numpy as np
import pytest

import pickcases as pc
from conftest import assert_bit_equal

pytestmark = pytest.mark.gpu

LL_ERR_CAPACITY, LL_ERR_EMPTY = -4, -5
BATCH = 11
REFUSED_SLOT = 5


def _key(c, write_curv=1, batch=1):
    return (np.float32(c["curv"]).item(), np.float32(c["gap"]).item(), c["max_ring"], write_curv, batch)


@pytest.fixture(scope="module")
def contexts(api):
    """contexts of 16 rings shared per (thresholds, max_ring_points, write_curvature, batch), large enough for every case"""
    made = {}
    cap = max(len(c["scan"]) for c in pc.cases().values()) + 8

    def get(key):
        if key not in made:
            curv, gap, max_ring, write_curv, batch = key
            made[key] = api.Context(api.default_params(pc.RINGS, batch=batch, max_points=cap, max_ring_points=max_ring, minimum_range=pc.MIN_RANGE,
                                                       curv_threshold=curv, gap_sq_threshold=gap, write_curvature=write_curv))
        return made[key]
    yield get
    for ctx in made.values():
        ctx.close()


_oracle = {}


def _less_flat(orc, name):
    if name not in _oracle:
        _oracle[name] = orc.extract(pc.cases()[name]["scan"], orc.params(pc.RINGS, minimum_range=pc.MIN_RANGE))["less_flat"]
    return _oracle[name]


def _check(ctx, slot, c, ref, what, orc=None, curvature=True):
    """slot `slot` of ctx against np_pick's result for case c"""
    scan, n = c["scan"], len(c["scan"])
    info = ctx.scan_info(slot)
    assert info.status == 0 and info.n == n, (what, info.status, info.n, n)
    cloud, ss, se = ctx.cloud(slot)
    assert_bit_equal(cloud[:, :3], scan[:, :3], f"{what}: the organised cloud is the input")
    assert (ss == c["off"][:-1] + 5).all() and (se == c["off"][1:] - 6).all(), what
    if curvature:
        lab, curv = ctx.labels(slot, curvature=True)
        assert_bit_equal(curv[5:n - 5], ref["curv"][5:n - 5], f"{what}: curvature")
    else:
        lab = ctx.labels(slot)
    lab = lab.astype(np.int32)
    bad = np.flatnonzero(lab[5:n - 5] != ref["label"][5:n - 5]) + 5
    if len(bad):
        i = int(bad[0]); r = int(np.searchsorted(c["off"], i, side="right") - 1)
        seg = [s for s in ref["segs"] if s["sp"] <= i <= s["ep"]]
        raise AssertionError((what, "labels", len(bad), "differ; first at", i, "ring", r, "segment", seg[0]["seg"] if seg else None,
                              "position", i - seg[0]["sp"] if seg else None, "device", int(lab[i]), "numpy", int(ref["label"][i])))
    assert not lab[:5].any() and not lab[n - 5:].any(), (what, "labels outside [5, n - 5)")
    f = ctx.features(slot)
    for kind, cnt in (("sharp", info.n_sharp), ("less_sharp", info.n_less_sharp), ("flat", info.n_flat)):
        idx = ref[kind]
        assert cnt == len(idx) == len(f[kind]), (what, kind, "count", cnt, len(idx))
        assert_bit_equal(f[kind], cloud[idx], f"{what}: {kind} in pick order")
    if orc is not None and pc.is_default(c):
        lf = _less_flat(orc, c["name"])
        assert info.n_less_flat == len(lf), (what, "less_flat count")
        assert_bit_equal(f["less_flat"], lf, f"{what}: less_flat against the oracle")


# ------------------------------------------------------------------------------------------------ (a), (b)
@pytest.mark.parametrize("name", pc.NAMES)
def test_case_alone(contexts, orc, name):
    c = pc.cases()[name]
    ctx = contexts(_key(c))
    ctx.upload_scan(0, c["scan"])
    ctx.extract(0, 1)
    ref = pc.reference(name)
    print(name, "points", len(c["scan"]), "sharp / less sharp / flat", len(ref["sharp"]), len(ref["less_sharp"]), len(ref["flat"]))
    _check(ctx, 0, c, ref, name, orc)


DEFAULT_NAMES = tuple(n for n in pc.NAMES if pc.is_default(pc.cases()[n]))


@pytest.mark.parametrize("name", DEFAULT_NAMES)
def test_case_without_curvature_output(contexts, orc, name):
    c = pc.cases()[name]
    ctx = contexts(_key(c, write_curv=0))
    ctx.upload_scan(0, c["scan"])
    ctx.extract(0, 1)
    _check(ctx, 0, c, pc.reference(name), name + " (write_curvature 0)", orc, curvature=False)


# ------------------------------------------------------------------------------------------------ (c), (d)
SMALL_RING_NAMES = tuple(n for n in DEFAULT_NAMES if pc.cases()[n]["max_ring"] == 2304)


def _nothing_in_range():
    """twenty points inside the minimum range: the registration refuses the scan"""
    az = np.arange(20) * 0.3
    return np.stack([0.001 * np.cos(az), 0.001 * np.sin(az), np.zeros(20), np.zeros(20)], axis=1).astype(np.float32)


def test_eleven_slots_then_five_of_them_again(contexts, orc):
    names = SMALL_RING_NAMES
    assert len(names) >= BATCH - 1 + 4
    c0 = pc.cases()[names[0]]
    ctx = contexts(_key(c0, batch=BATCH))
    first = {}
    it = iter(names)
    for s in range(BATCH):
        if s == REFUSED_SLOT:
            ctx.upload_scan(s, _nothing_in_range())
        else:
            first[s] = next(it)
            ctx.upload_scan(s, pc.cases()[first[s]]["scan"])
    ctx.extract(0, BATCH)
    assert ctx.scan_info(REFUSED_SLOT).status == LL_ERR_EMPTY
    for s, name in first.items():
        _check(ctx, s, pc.cases()[name], pc.reference(name), f"slot {s} of eleven: {name}", orc)
    # (d) slots 3..7 take other cases (one of them the refused slot: it is good now), the others stay
    rest = list(it) + list(names)
    second = dict(first)
    for s in range(3, 8):
        second[s] = next(n for n in rest if n not in (first.get(s), *[second[t] for t in range(3, s)]))
        ctx.upload_scan(s, pc.cases()[second[s]]["scan"])
    assert all(second[s] != first.get(s) for s in range(3, 8))
    ctx.extract(3, 5)
    for s, name in second.items():
        _check(ctx, s, pc.cases()[name], pc.reference(name), f"slot {s} after extract(3, 5): {name}", orc)


# ------------------------------------------------------------------------------------------------ (e)
def _short_in_the_same_places(c):
    """a scan whose rings are short (40 points), under 17 points or empty where c's rings are long"""
    rng = np.random.default_rng(2)
    sizes = np.diff(c["off"])
    rings = []
    for k, n in enumerate(sizes):
        m = (40, 10, 0)[k % 3] if n > 100 else int(n)
        rings.append(None if m == 0 else pc.vlp_ring(k, pc.base_radius(m) * (1.0 + 0.002 * rng.standard_normal(m)) * np.where(rng.random(m) < 0.2, 1.3, 1.0)))
    return pc._case("short-after-" + c["name"], "stale", rings, max_ring=c["max_ring"])


def test_stale_state_after_long_rings(api, contexts, orc):
    a = pc.cases()["tiers-4608"]
    b = _short_in_the_same_places(a)
    ref_a, ref_b = pc.reference(a["name"]), pc.np_pick(b["scan"], b["off"], b["curv"], b["gap"])
    assert len(ref_b["sharp"]) > 0 and len(ref_b["flat"]) > 0
    ctx = contexts(_key(a))
    for step, (c, ref) in enumerate(((a, ref_a), (b, ref_b), (a, ref_a))):
        ctx.upload_scan(0, c["scan"])
        ctx.extract(0, 1)
        _check(ctx, 0, c, ref, f"step {step}: {c['name']}", orc if c is a else None)
        fresh = api.Context(api.default_params(pc.RINGS, batch=1, max_points=len(a["scan"]) + 8, max_ring_points=a["max_ring"],
                                               minimum_range=pc.MIN_RANGE, write_curvature=1))
        fresh.upload_scan(0, c["scan"])
        fresh.extract(0, 1)
        _check(fresh, 0, c, ref, f"step {step} in a fresh context: {c['name']}")
        got, want = ctx.features(0), fresh.features(0)
        for kind in ("sharp", "less_sharp", "flat", "less_flat"):
            assert_bit_equal(got[kind], want[kind], f"step {step}: {kind} against the fresh context")
        fresh.close()


# ------------------------------------------------------------------------------------------------ (f)
@pytest.mark.parametrize("name", ["tiers-4608", "tiers-8192"])
def test_long_rings_are_refused_at_the_common_capacity(contexts, name):
    """include/lightloam_hip.h: LL_ERR_CAPACITY -- "a ring longer than max_ring_points"; the slot gets no features"""
    c = pc.cases()[name]
    ctx = contexts(_key(dict(c, max_ring=2304)))
    ctx.upload_scan(0, c["scan"])
    ctx.extract(0, 1)
    assert ctx.scan_info(0).status == LL_ERR_CAPACITY
