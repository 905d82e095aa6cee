"""The odometry association on the device (ll_associate_block under k_associate, the grid and ring tables of k_build_grid) against the
independent numpy reference of assoccases.py, at crafted targets: every case goes through Context.upload_features, associate,
vote(False), edge_corr and plane_corr and must equal np_associate EXACTLY -- everything is an index, there is no tolerance and no case
is excluded.  test_assoc_cases.py shows on the CPU which route of ll_associate_block each family forces.

Three ways per family:
  (a) the target by set_target (the carry), batch = 1: workgroups of 32 queries, one pass;
  (b) twenty slots associated in one call: workgroups of 256 queries, eight passes, queries dealt by the counting sort; slot k holds a
      case of the family (or the same case under another pose), its target is what slot k - 1 uploaded as less-sharp / less-flat
      clouds; one slot holds no queries and no clouds, so its successor searches an empty target; every slot must also give what it
      gives alone in (a);
  (c) the monotone families and the valid-but-not-monotone one with the target in the previous slot (ll_target's slot branch), two
      slots in one call: the 32-query path on a contiguous slot target.

On an MI355X every case was equal in all three ways as the kernels stand (71 tests, 8 s).  Twelve scratch mutants of ll_associate.h that
cannot index out of bounds (the list is in DESIGN.md, section 6) each failed at least one family here.
"""
import numpy as np
import pytest

import assoccases as ac

pytestmark = pytest.mark.gpu

BATCH = 20
EMPTY_SLOT = 6


@pytest.fixture(scope="module")
def contexts(api):
    """contexts of 64 rings and 4096 points, shared per (batch, nearby_scan, distance limit)"""
    made = {}

    def get(batch, nearby=2.5, dmax=25.0):
        key = (batch, float(nearby), float(dmax))
        if key not in made:
            made[key] = api.Context(api.default_params(64, batch=batch, max_points=ac.MAX_POINTS, nearby_scan=float(nearby), nn_dist_sq_max=float(dmax)))
        return made[key]
    yield get
    for ctx in made.values():
        ctx.close()


def _download(ctx, slot):
    return tuple(x.copy() for x in ctx.edge_corr(slot)), tuple(x.copy() for x in ctx.plane_corr(slot))


def _expect(c, pose, sharp, flat, corner=None, surf=None):
    corner = c["corner"] if corner is None else corner; surf = c["surf"] if surf is None else surf
    return (ac.np_associate(pose, sharp, corner, False, c["nearby"], c["dmax"]), ac.np_associate(pose, flat, surf, True, c["nearby"], c["dmax"]))


def _check(got, want, what):
    for g, w, kind in zip(got, want, ("corner", "plane")):
        for a, b, nm in zip(g, w, ("src", "a", "b", "c")):
            assert len(a) == len(b), (what, kind, nm, len(a), len(b))
            bad = np.flatnonzero(a != b)
            assert len(bad) == 0, (what, kind, nm, "first difference at correspondence", int(bad[0]), "query", int(w[0][bad[0]]), "device", int(a[bad[0]]), "numpy", int(b[bad[0]]))


def _alone(contexts, c, pose, sharp, flat, corner, surf):
    """(a): one slot, the target as the carry"""
    ctx = contexts(1, c["nearby"], c["dmax"])
    ctx.upload_features(0, sharp, ac.EMPTY, flat, ac.EMPTY)
    ctx.set_target(corner, surf)
    ctx.associate(0, 1, pose)
    ctx.vote(0, 1, False)
    return _download(ctx, 0)


@pytest.mark.parametrize("name", ac.NAMES)
def test_one_slot_against_the_carry(contexts, name):
    c = ac.cases()[name]
    got = _alone(contexts, c, c["pose"], c["sharp"], c["flat"], c["corner"], c["surf"])
    ref = ac.reference(name)
    print(name, "correspondences", len(got[0][0]), len(got[1][0]))
    _check(got, (ref[0], ref[1]), name)


def _groups():
    """the cases of a family that can share a context: same nearby_scan and distance limit"""
    out = {}
    for name in ac.NAMES:
        c = ac.cases()[name]
        out.setdefault((c["family"], c["nearby"], c["dmax"]), []).append(name)
    return out


GROUPS = _groups()


@pytest.mark.parametrize("key", list(GROUPS), ids=[f"{k[0]}-{k[1]}-{k[2]}" for k in GROUPS])
def test_twenty_slots_in_one_call(contexts, key):
    names = GROUPS[key]
    ctx = contexts(BATCH, key[1], key[2])
    slots = []
    for s in range(BATCH):
        c = ac.cases()[names[s % len(names)]]
        pose = ac.POSES[(s // len(names)) % len(ac.POSES)]
        if s == EMPTY_SLOT:
            slots.append(dict(c=c, pose=pose, sharp=ac.EMPTY, flat=ac.EMPTY, corner=c["corner"], surf=c["surf"]))
        elif s == EMPTY_SLOT + 1:                           # its target is the empty slot's clouds: nothing
            slots.append(dict(c=c, pose=pose, sharp=ac.to_lidar(pose, c["sharp"]), flat=ac.to_lidar(pose, c["flat"]), corner=ac.EMPTY, surf=ac.EMPTY))
        else:
            slots.append(dict(c=c, pose=pose, sharp=ac.to_lidar(pose, c["sharp"]), flat=ac.to_lidar(pose, c["flat"]), corner=c["corner"], surf=c["surf"]))
    assert np.array_equal(slots[0]["sharp"], slots[0]["c"]["sharp"])                             # the identity pose leaves the crafted queries as they are
    ctx.set_target(slots[0]["corner"], slots[0]["surf"])
    for s, x in enumerate(slots):
        nxt = slots[s + 1] if s + 1 < BATCH else dict(corner=ac.EMPTY, surf=ac.EMPTY)
        ctx.upload_features(s, x["sharp"], nxt["corner"], x["flat"], nxt["surf"])
    ctx.associate(0, BATCH, np.stack([x["pose"] for x in slots]))
    ctx.vote(0, BATCH, False)
    total = [0, 0]
    for s, x in enumerate(slots):
        got = _download(ctx, s)
        what = (key, "slot", s, x["c"]["name"])
        _check(got, _expect(x["c"], x["pose"], x["sharp"], x["flat"], x["corner"], x["surf"]), what)
        _check(got, _alone(contexts, x["c"], x["pose"], x["sharp"], x["flat"], x["corner"], x["surf"]), what + ("against the slot alone",))
        total[0] += len(got[0][0]); total[1] += len(got[1][0])
        if s in (EMPTY_SLOT, EMPTY_SLOT + 1):
            assert len(got[0][0]) == 0 and len(got[1][0]) == 0
    print(key, "correspondences over the twenty slots", total)


SLOT_TARGET_NAMES = tuple(n for n in ac.NAMES if ac.cases()[n]["family"] in ac.MONOTONE_FAMILIES + ("vnm",))


@pytest.mark.parametrize("name", SLOT_TARGET_NAMES)
def test_target_in_the_previous_slot(contexts, name):
    c = ac.cases()[name]
    ctx = contexts(2, c["nearby"], c["dmax"])
    ctx.set_target(ac.EMPTY, ac.EMPTY)
    ctx.upload_features(0, ac.EMPTY, c["corner"], ac.EMPTY, c["surf"])
    ctx.upload_features(1, c["sharp"], ac.EMPTY, c["flat"], ac.EMPTY)
    ctx.associate(0, 2, np.stack([ac.IDENT, c["pose"]]))
    ctx.vote(0, 2, False)
    ref = ac.reference(name)
    _check(_download(ctx, 1), (ref[0], ref[1]), name)
    first = _download(ctx, 0)
    assert len(first[0][0]) == 0 and len(first[1][0]) == 0
