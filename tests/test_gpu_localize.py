"""ll_cubemaps_localize_slots: a read-only frame against a frozen cube map, several readers per map.  The reference is the
single-map API on a private, imported copy of the map: CubeMap.prepare + CubeMap.optimize without update is a localisation
frame (it runs the shift loops on its copy; the batched call must not and cannot, the map is shared).  Pose, ran and the four
clouds are compared bit for bit; the fit record against Map.associate / counts / normal_equations / residual_jacobian at the
final pose, to the 1e-9 relative of test_normal_equations (the sums run in another order)."""
import numpy as np
import pytest

from conftest import assert_bit_equal
from test_gpu_mapping_sequences import CAP, _guesses
from test_gpu_sequences import drives

pytestmark = pytest.mark.gpu

SHAPES = {16: (4, 6), 64: (3, 5)}                 # rings: S sequences, n frames of drive A
FAR = (-431.0, 512.5, 30.0)                       # test_shift_loops_and_negative_coordinates' first offset
REL = 1e-9


class World:
    """map 0 of a CubeMaps built from drive A, its export and layout; copy j of frame k of drive A sits in slot j * n + k, slot
    S * n holds an empty scan (extracted: LL_ERR_EMPTY)"""

    def __init__(self, api, synth, rings):
        self.api, self.synth, self.rings = api, synth, rings
        self.S, self.n = S, n = SHAPES[rings]
        cfgs, scans, _ = drives(synth, rings, 1, n)
        self.cfg, A = cfgs[0], scans[0]
        self.ctx = ctx = api.Context(api.default_params(rings, batch=S * n + 1, max_points=max(map(len, A))))
        for j in range(S):
            for k in range(n):
                ctx.upload_scan(j * n + k, A[k])
        ctx.upload_scan(S * n, np.zeros((0, 4), np.float32))
        ctx.extract(0, S * n + 1)
        self.feats = [ctx.features(k) for k in range(n)]
        c, s, pool = CAP[rings]
        self.many = many = api.CubeMaps(ctx, S, c, s, pool_points=pool)
        for k in range(n):
            many.process_slots(np.tile(self.guess(k), (S, 1)), [k] + [-1] * (S - 1))
        pts, off = many.export([api.MAP_ALL] + [api.MAP_NONE] * (S - 1))
        self.map_pts = pts[off[0]:off[1]].copy()
        self.layout = many.layout(0)
        self.info = many.info(0)
        self.ones = []

    def guess(self, k, offset=(0.0, 0.0, 0.0)):
        return _guesses(self.synth, [self.cfg], k, [offset])[0]

    def private(self):
        """a CubeMap that holds a copy of map 0"""
        c, s, pool = CAP[self.rings]
        one = self.api.CubeMap(self.ctx, c, s, pool_points=pool)
        one.import_map(self.map_pts, self.layout)
        self.ones.append(one)
        return one

    def frame_of(self, q, k):
        """the frame of drive A that sequence q reads on call k: 1: k, 2: n - 1 - k, 3: k + 2"""
        return [None, k, self.n - 1 - k, (k + 2) % self.n][q]

    def call(self, k):
        S, n = self.S, self.n
        frames = [None] + [self.frame_of(q, k) for q in range(1, S)]
        guess = np.array([self.guess(0)] + [self.guess(f) for f in frames[1:]])
        slots = [-1] + [q * n + frames[q] for q in range(1, S)]
        return frames, guess, slots

    def assert_map0_untouched(self):
        api, many = self.api, self.many
        pts, off = many.export([api.MAP_ALL] + [api.MAP_NONE] * (self.S - 1))
        assert many.info(0) == self.info
        lay = many.layout(0)
        for a, b in zip(lay, self.layout):
            assert np.array_equal(a, b)
        assert pts[off[0]:off[1]].tobytes() == self.map_pts.tobytes()

    def close(self):
        for o in self.ones:
            o.close()
        self.many.close(); self.ctx.close()


@pytest.fixture(scope="module")
def worlds(api, synth):
    made = {}

    def get(rings):
        if rings not in made:
            made[rings] = World(api, synth, rings)
        return made[rings]
    yield get
    for w in made.values():
        w.close()


def _one_frame(one, feats, guess):
    one.prepare(guess[4:], feats["less_sharp"], feats["less_flat"])
    return one.optimize(guess)


def _is_zero(rec):
    return (rec.n_edge, rec.n_plane, rec.cost, rec.sq_edge, rec.sq_plane) == (0, 0, 0.0, 0.0, 0.0)


@pytest.mark.parametrize("rings", [16, 64])
def test_equals_the_single_map_calls_and_leaves_the_map_alone(worlds, rings):
    w = worlds(rings)
    S, n, many = w.S, w.n, w.many
    ones = [None] + [w.private() for _ in range(1, S)]
    syncs0, frames0 = many.stats()
    n_ran = 0
    for k in range(n):
        frames, guess, slots = w.call(k)
        poses, ran, fit = many.localize_slots(guess, slots, [0] * S)
        assert_bit_equal(poses[0], guess[0], "a sequence that sits out keeps its pose row")
        assert not ran[0] and _is_zero(fit[0])
        for q in range(1, S):
            p1, r1 = _one_frame(ones[q], w.feats[frames[q]], guess[q])
            assert bool(ran[q]) == r1, (k, q)
            n_ran += r1
            assert_bit_equal(poses[q], p1, f"call {k} sequence {q} pose")
            assert (poses[q] == p1).all(), (k, q)                                   # f64, not only its f32 rounding
            for which in range(4):
                assert_bit_equal(many.cloud(q, which), ones[q].cloud(which), f"call {k} sequence {q} cloud {which}")
    assert n_ran == n * (S - 1)                                                     # every frame lies on the map: all optimised
    w.assert_map0_untouched()
    syncs, frames_now = many.stats()
    assert frames_now == frames0
    # headers, prepare, poses + fit; a filter reads back once when the scans of one type exceed 65 536 points in one call
    big = sum(max(len(f["less_flat"]) for f in w.feats) for _ in range(1, S)) > 65536
    per_call = (syncs - syncs0 - 1) / n                                             # - 1: assert_map0_untouched's export
    print(f"rings {rings}: {per_call} synchronisations per localising call")
    assert syncs - syncs0 - 1 <= (3 + (2 if big else 0)) * n


@pytest.mark.parametrize("rings", [16, 64])
def test_fit_record(worlds, rings):
    w = worlds(rings)
    S, n, many = w.S, w.n, w.many
    ones = [None] + [w.private() for _ in range(1, S)]
    for k in range(n):
        frames, guess, slots = w.call(k)
        poses, ran, fit = many.localize_slots(guess, slots, [0] * S)
        bare, ran_bare, none = many.localize_slots(guess, slots, [0] * S, fit=False)
        assert none is None and (ran == ran_bare).all()
        assert bare.tobytes() == poses.tobytes()
        for q in range(1, S):
            p1, r1 = _one_frame(ones[q], w.feats[frames[q]], guess[q])
            assert r1 and ran[q] and (p1 == poses[q]).all()
            m = ones[q].map()
            m.associate(p1)
            ne, npl = m.counts()
            assert (fit[q].n_edge, fit[q].n_plane) == (ne, npl), (k, q)
            assert ne > 10 and npl > 50
            _, _, cost = m.normal_equations(p1)
            r, _, _ = m.residual_jacobian(p1)
            sq_edge, sq_plane = float(np.sum(r[:3 * ne] ** 2)), float(np.sum(r[3 * ne:] ** 2))
            print(f"rings {rings} call {k} seq {q}: blocks {ne} {npl} cost {fit[q].cost!r} / {cost!r} sq_edge {fit[q].sq_edge!r} / {sq_edge!r} "
                  f"sq_plane {fit[q].sq_plane!r} / {sq_plane!r}")
            assert abs(fit[q].cost - cost) <= REL * abs(cost), (k, q)
            assert abs(fit[q].sq_edge - sq_edge) <= REL * abs(sq_edge), (k, q)
            assert abs(fit[q].sq_plane - sq_plane) <= REL * abs(sq_plane), (k, q)
    # off the map: the gate stays shut, the record is all zero -- also where the array already held one from the call before
    guess = np.tile(w.guess(1, FAR), (S, 1))
    poses, ran, fit = many.localize_slots(guess, [-1, n + 1] + [-1] * (S - 2), [0] * S)
    assert not ran[1] and _is_zero(fit[1])
    w.assert_map0_untouched()


def test_no_shift_same_answer(worlds):
    """the private copy must shift (x by +2, y by -3 cubes) to hold the far guess; no occupied cube (indices 8..12) leaves its
    array, the condition under which the unshifted read equals it"""
    w = worlds(16)
    S, n, many = w.S, w.n, w.many
    occupied = np.argwhere(w.layout[1].reshape(2, 11, 21, 21).sum(axis=0) > 0)      # (k, j, i)
    assert occupied[:, 1:].min() >= 8 and occupied[:, 1:].max() <= 12
    one = w.private()
    slots = [-1, n + 1] + [-1] * (S - 2)
    far = w.guess(1, FAR)
    poses, ran, fit = many.localize_slots(np.tile(far, (S, 1)), slots, [0] * S)
    p1, r1 = _one_frame(one, w.feats[1], far)
    assert not r1 and not ran[1]
    assert (poses[1] == far).all() and (p1 == far).all()
    assert len(many.cloud(1, 0)) == 0 and len(many.cloud(1, 1)) == 0 and len(one.cloud(0)) == 0 and len(one.cloud(1)) == 0
    for which in (2, 3):
        assert_bit_equal(many.cloud(1, which), one.cloud(which), f"far frame stack {which}")
    assert one.info()[0] == (12, 7, 5)
    near = w.guess(1)
    poses, ran, fit = many.localize_slots(np.tile(near, (S, 1)), slots, [0] * S)
    p1, r1 = _one_frame(one, w.feats[1], near)
    assert r1 and ran[1] and (poses[1] == p1).all()
    for which in range(4):
        assert_bit_equal(many.cloud(1, which), one.cloud(which), f"near frame cloud {which}")
    assert one.info()[0] == (12, 7, 5) and many.info(0)[0] == (10, 10, 5)
    w.assert_map0_untouched()


def test_errors_change_nothing(worlds, api):
    w = worlds(16)
    S, n, many = w.S, w.n, w.many
    guess = np.tile(w.guess(1), (S, 1))
    stats0 = many.stats()

    def refused(code, slots, map_of, cms=many, counted=0):
        with pytest.raises(api.LightLoamError) as e:
            cms.localize_slots(guess, slots, map_of)
        assert e.value.code == code, e.value
        assert many.stats() == (stats0[0] + counted, stats0[1])
        return str(e.value)

    idle = [-1] * (S - 2)
    assert "sequence 1" in refused(-2, [-1, n + 1] + idle, [0, S] + [0] * (S - 2))           # LL_ERR_ARG: map_of beyond the maps
    refused(-2, [-1, n + 1] + idle, [0, -1] + [0] * (S - 2))
    assert "slot" in refused(-2, [n + 1, n + 1] + idle, [0] * S)                              # one slot named twice
    refused(-2, [-1, S * n + 1] + idle, [0] * S)                                              # beyond the batch
    assert "sequence 1" in refused(-7, [-1, S * n] + idle, [0] * S, counted=1)                # LL_ERR_STATE: no extracted scan (the header read counts)
    w.assert_map0_untouched()
    # a reader whose scan capacity is too small: LL_ERR_CAPACITY, and its own maps stay empty
    small = api.CubeMaps(w.ctx, 2, 64, 64, pool_points=4096)
    with pytest.raises(api.LightLoamError) as e:
        small.localize_slots(guess[:2], [-1, n + 1], [0, 0])
    assert e.value.code == -4, e.value
    assert small.info(0)[1][:2] == (0, 0) and int(small.export_sizes(api.MAP_ALL)[-1]) == 0
    small.close()
    # and the next legal call gives what it gives without the refused ones
    one = w.private()
    poses, ran, _ = many.localize_slots(guess, [-1, n + 1] + idle, [0] * S)
    p1, r1 = _one_frame(one, w.feats[1], guess[1])
    assert ran[1] and r1 and (poses[1] == p1).all()
    w.assert_map0_untouched()
