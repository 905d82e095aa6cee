"""ll_cubemaps_align: one cube map registered to another on the device.  The expected value never comes from the code under test:
it is the CPU oracle's map_associate / map_normal_equations / map_optimize (and its LidarEdgeFactor / LidarPlaneNormFactor for
the plain sums of squares) on clouds rebuilt from per-cube reads, concatenated per type in LL_MAP_ALL order: cube index ascending,
own order inside a cube.  Poses within 1e-7 per component (the bar of test_gpu_mapping.py), fit sums within REL = 1e-9, block counts
exact.  The maps are fabricated with import_maps and stay at a few thousand points, because the oracle's 5-NN is brute force.

Scenes: surf points on a ground plane and two walls at 0.4 m, corner points on poles and horizontal lines at 0.2 m, a seeded jitter
of 2 cm; no plane passes through the origin of dst's frame (the reference's plane fit n . p = -1 has no solution there).  src is an
independent sampling of the same geometry (another phase, another jitter) taken through the inverse of T_true; T0 is T_true turned
by about a degree around the scene's centre and shifted by a few decimetres.

Synchronisations per call, as lightloam_hip.h and DESIGN.md state them: ONE whenever an op passes the :1822 gate."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_gpu_drives import qmul, qrot
from test_gpu_drives_localize import IDENT, fit_tuple, make_drives, step
from test_gpu_map_merge import ALL, EMPTY, N, check_map, cubes, cubes_of, expected_merge, import_all, make_map, small_ctx, state
from test_gpu_mapping import REL
from test_gpu_mapping_sequences import CAP, _ctx, _guesses
from test_gpu_sequences import drives

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALIGN_SYNCS = 1
POSE_TOL = 1e-7
T_TRUE = np.array([0.0, 0.0, np.sin(np.deg2rad(4.0) / 2), np.cos(np.deg2rad(4.0) / 2), 3.0, -2.0, 0.5])


# ------------------------------------------------------------------ geometry
def _axis_q(axis, deg):
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a)
    h = np.deg2rad(deg) / 2
    return np.r_[a * np.sin(h), np.cos(h)]


def apply(T, p):
    """T(p) in f64 for points [n, 3]"""
    return np.array([qrot(T[:4], v) for v in np.asarray(p, np.float64).reshape(-1, 3)]) + T[4:]


def inverse(T):
    qi = np.r_[-T[:3], T[3]]
    return np.r_[qi, -np.array(qrot(qi, T[4:]))]


def perturbed(T, centre, shift=(0.25, -0.2, 0.1), deg=1.0):
    """T0(p) = R (T(p) - centre) + centre + shift: T turned by `deg` around the scene's centre in dst's frame, then shifted"""
    qd = _axis_q((0.3, -0.2, 0.93), deg)
    c = np.asarray(centre, np.float64)
    return np.r_[qmul(qd, T[:4]), np.array(qrot(qd, T[4:] - c)) + c + np.asarray(shift)]


def pose_error(T, T_ref, centre, half=8.0):
    """the largest distance between T(p) and T_ref(p) over the corners of the scene's box, given in dst's frame"""
    box = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-0.25, 0.25)]) * half + np.asarray(centre)
    p = apply(inverse(T_ref), box)
    return float(np.linalg.norm(apply(T, p) - box, axis=1).max())


def _pts(xyz, rng, w):
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3) + rng.uniform(-0.02, 0.02, size=(len(xyz), 3))
    return np.concatenate([xyz, np.full((len(xyz), 1), float(w))], 1)


def geometry(rng, c, half=8.0, phase=0.0):
    """-> (corner [n, 4], surf [m, 4]) f64 around centre c: the ground at z = c_z - 2, a wall in the plane x = c_x and one in the
    plane y = c_y (both 4 m high, through the centre: they cross the cube faces a centre lies on), five poles and four
    horizontal lines"""
    cx, cy, cz = c
    u = np.arange(-half + phase, half + 1e-9, 0.4)
    h = np.arange(-2.0 + phase, 2.0 + 1e-9, 0.4)
    gx, gy = np.meshgrid(cx + u, cy + u)
    ground = np.stack([gx.ravel(), gy.ravel(), np.full(gx.size, cz - 2.0)], 1)
    wy, wz = np.meshgrid(cy + u, cz + h)
    wall_x = np.stack([np.full(wy.size, cx), wy.ravel(), wz.ravel()], 1)
    wx, wz = np.meshgrid(cx + u, cz + h)
    wall_y = np.stack([wx.ravel(), np.full(wx.size, cy), wz.ravel()], 1)
    z = np.arange(-2.0 + phase / 2, 2.0 + 1e-9, 0.2)
    poles = [np.stack([np.full(len(z), cx + a), np.full(len(z), cy + b), cz + z], 1) for a, b in ((3, 3), (-3, 3), (3, -3), (-3, -3), (0.0, 0.0))]
    v = np.arange(-half + phase / 2, half + 1e-9, 0.2)
    lines = [np.stack([cx + v, np.full(len(v), cy + b), np.full(len(v), cz + 1.0)], 1) for b in (5.0, -5.0)]
    lines += [np.stack([np.full(len(v), cx + a), cy + v, np.full(len(v), cz - 1.0)], 1) for a in (5.0, -5.0)]
    return _pts(np.concatenate(poles + lines), rng, 0), _pts(np.concatenate([ground, wall_x, wall_y]), rng, 1)


def through(T, cloud):
    """a cloud [n, 4] f64 taken through T, as float32"""
    return np.concatenate([apply(T, cloud[:, :3]), cloud[:, 3:]], 1).astype(np.float32)


def pair(seed, centre, cen=(10, 10, 5), T_true=T_TRUE, src_half=8.0, keep=None):
    """-> (dst map, src map, T0): two independent samplings of one geometry; dst in its own frame (keep: a filter on its points),
    src through the inverse of T_true"""
    rng = np.random.default_rng(seed)
    dst = [g.astype(np.float32) for g in geometry(rng, centre)]
    if keep is not None:
        dst = [g[keep(g)] for g in dst]
    src = [through(inverse(T_true), g) for g in geometry(rng, centre, half=src_half, phase=0.13)]
    return make_map(*dst, cen=cen), make_map(*src), perturbed(T_true, centre)


# ------------------------------------------------------------------ the oracle's side
def ordered(pts, cen=(10, 10, 5)):
    """world points of one type -> LL_MAP_ALL order (for checking a scene without a device)"""
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 4)
    return pts[np.argsort(cubes_of(pts, cen), kind="stable")]


def clouds(many, q):
    """[corner, surf] of map q in LL_MAP_ALL order per type, from per-cube reads"""
    have = cubes(many, q)
    out = []
    for w in (0, 1):
        parts = [have[(w, c)] for c in range(N) if (w, c) in have]
        out.append(np.concatenate(parts) if parts else EMPTY)
    return out


def oracle_fit(orc, T, stk, mp):
    """(n_edge, n_plane, cost, sq_edge, sq_plane) of the oracle's blocks at T, and the blocks"""
    q, t = T[:4], T[4:]
    b = orc.map_associate(q, t, stk[0], mp[0], stk[1], mp[1])
    _, _, cost = orc.map_normal_equations(q, t, stk[0], b[0], b[1], b[2], stk[1], b[3], b[4], b[5])
    sq_e = sum(float(np.sum(orc.edge_factor(q, t, stk[0][s, :3], a, bb)[0] ** 2)) for s, a, bb in zip(b[0], b[1], b[2]))
    sq_p = sum(float(orc.plane_norm_factor(q, t, stk[1][s, :3], n, d)[0][0] ** 2) for s, n, d in zip(b[3], b[4], b[5]))
    return (len(b[0]), len(b[3]), cost, sq_e, sq_p), b


def check_fit(rec, want, what):
    got = fit_tuple(rec)
    print(f"{what}: blocks {got[:2]} / {want[:2]} cost {got[2]!r} / {want[2]!r} sq_edge {got[3]!r} / {want[3]!r} sq_plane {got[4]!r} / {want[4]!r}")
    assert got[:2] == want[:2], what
    for g, w, name in zip(got[2:], want[2:], ("cost", "sq_edge", "sq_plane")):
        assert abs(g - w) <= REL * abs(w), (what, name, g, w)


def check_pose(T, q, t, what):
    err = max(np.abs(T[:4] - q).max(), np.abs(T[4:] - t).max())
    print(f"{what}: pose {T.tolist()} oracle {list(q) + list(t)} max diff {err:.3e}")
    assert err < POSE_TOL, (what, err)


def against_oracle(orc, many, dst, src, T0, n_outer, T, ran, rec, what, want_blocks=(100, 500), T_true=None, centre=None):
    """one op's result against orc.map_optimize and, for the record, the oracle's blocks at the returned pose"""
    stk, mp = clouds(many, src), clouds(many, dst)
    at_T0, _ = oracle_fit(orc, T0, stk, mp)
    assert at_T0[0] >= want_blocks[0] and at_T0[1] >= want_blocks[1], (what, at_T0)   # the scene is not empty-handed
    q, t, o_ran = orc.map_optimize(T0[:4], T0[4:], stk[0], mp[0], stk[1], mp[1], n_outer)
    assert o_ran and ran, what
    check_pose(T, q, t, what)
    if T_true is not None and n_outer > 0:
        e0, e1 = pose_error(T0, T_true, centre), pose_error(np.r_[q, t], T_true, centre)
        print(f"{what}: error at the scene {e0:.3f} m at T0, {e1:.3f} m after the oracle's solve")
        assert e1 < e0, (what, e0, e1)
    if rec is not None:
        check_fit(rec, oracle_fit(orc, T, stk, mp)[0], what + " fit")
    return at_T0


def maps_object(api, ctx, maps, pool=1 << 15):
    many = api.CubeMaps(ctx, len(maps), 64, 64, pool_points=pool)
    import_all(many, maps)
    return many


# ------------------------------------------------------------------ cases
def test_blocks_at_the_guess(api, orc):
    """case 1: n_outer = 0 pins the search and the fits without the LM"""
    dst, src, T0 = pair(1, (6.0, -4.0, 1.0))
    ctx = small_ctx(api)
    many = maps_object(api, ctx, [dst, src])
    T, ran, fit = many.align([(0, 1, T0)], n_outer=0)
    assert T.tobytes() == T0.reshape(1, 7).tobytes() and ran.tolist() == [True]
    want, _ = oracle_fit(orc, T0, clouds(many, 1), clouds(many, 0))
    assert want[0] >= 100 and want[1] >= 500, want
    check_fit(fit[0], want, "blocks at T0")
    ms, cnt = many.align_timing()
    assert cnt == (len(src[0]), len(dst[0]), want[0] + want[1]) and all(m >= 0 for m in ms), (ms, cnt)
    many.close(); ctx.close()


@pytest.mark.parametrize("centre", [(25.0, 3.0, 1.0), (3.0, 25.0, 1.0), (3.0, -4.0, 25.0), (25.0, 25.0, 25.0), (-25.0, -75.0, -25.0)],
                         ids=["x-face", "y-face", "z-face", "corner", "negative-corner"])
def test_across_cube_faces(api, orc, centre):
    """case 2: the walls lie in the cube faces through the centre, the poles and the ground cross them: queries have their five
    neighbours in two to eight cubes"""
    dst, src, T0 = pair(2, centre)
    n_cubes = int((dst[1][1][1] > 0).sum())
    assert n_cubes >= 2 ** sum(1 for k in range(3) if (centre[k] + 25.0) % 50.0 == 0.0), n_cubes
    ctx = small_ctx(api)
    many = maps_object(api, ctx, [dst, src])
    T, ran, fit = many.align([(0, 1, T0)], n_outer=2)
    against_oracle(orc, many, 0, 1, T0, 2, T[0], ran[0], fit[0], f"faces {centre}", T_true=T_TRUE, centre=centre)
    T, ran, fit = many.align([(0, 1, T0)], n_outer=0)
    check_fit(fit[0], oracle_fit(orc, T0, clouds(many, 1), clouds(many, 0))[0], f"faces {centre} at T0")
    many.close(); ctx.close()


@pytest.mark.parametrize("side", [0, 20])
def test_edge_cubes_and_queries_outside_the_array(api, orc, side):
    """case 3: dst lies in cube column i = 0 (i = 20) of a map whose centre is shifted so that the array ends at x = -25 (x = 25);
    src is sampled 0.8 m further out, so some of its points land outside the array and must still give the oracle's blocks"""
    sign = -1.0 if side == 0 else 1.0
    centre = (sign * 17.0, 2.0, 1.0)
    inside = (lambda g: g[:, 0] > -24.99) if side == 0 else (lambda g: g[:, 0] < 24.99)
    dst, src, T0 = pair(3, centre, cen=(side, 10, 5), src_half=8.8, keep=inside)
    occupied = np.nonzero(dst[1][1][1])[0]
    assert set((occupied % 21).tolist()) == {side}
    ctx = small_ctx(api)
    many = maps_object(api, ctx, [dst, src])
    stk, mp = clouds(many, 1), clouds(many, 0)
    want, b = oracle_fit(orc, T0, stk, mp)
    outside = 0
    for w, srcs in ((0, b[0]), (1, b[3])):
        tp = orc.point_associate_to_map(T0[:4], T0[4:], stk[w][srcs])
        outside += int((cubes_of(tp, (side, 10, 5)) < 0).sum())
        far = orc.point_associate_to_map(T0[:4], T0[4:], stk[w])[:, 0] * sign
        assert far.max() > 25.5, far.max()
    assert outside >= 5, outside                                                    # blocks whose query lies outside the array
    T, ran, fit = many.align([(0, 1, T0)], n_outer=0)
    check_fit(fit[0], want, f"edge {side} at T0")
    T, ran, fit = many.align([(0, 1, T0)], n_outer=2)
    against_oracle(orc, many, 0, 1, T0, 2, T[0], ran[0], fit[0], f"edge {side}", T_true=T_TRUE, centre=centre)
    many.close(); ctx.close()


def test_src_points_where_dst_is_empty(api, orc):
    """case 4: src patches in a far empty cube, in the empty cube next to dst's and in an empty region of an occupied cube give no
    block; the rest is as without them"""
    centre = (6.0, -4.0, 1.0)
    dst, src, T0 = pair(4, centre)
    rng = np.random.default_rng(40)
    src_c, src_s = ordered(src[0][src[0][:, 3] == 0]), ordered(src[0][src[0][:, 3] == 1])
    extra = []
    for at in ((200.0, 150.0, 0.0), (40.0, -4.0, 1.0), (-20.0, 20.0, -10.0)):
        g = geometry(rng, at, half=2.0)
        extra.append([through(inverse(T_TRUE), x) for x in g])
    with_extra = make_map(np.concatenate([src_c] + [e[0] for e in extra]), np.concatenate([src_s] + [e[1] for e in extra]))
    ctx = small_ctx(api)
    many = maps_object(api, ctx, [dst, with_extra, src])
    stk, mp = clouds(many, 1), clouds(many, 0)
    want, b = oracle_fit(orc, T0, stk, mp)
    plain, _ = oracle_fit(orc, T0, clouds(many, 2), mp)
    assert want[:2] == plain[:2] and sum(len(e[0]) + len(e[1]) for e in extra) > 300   # the patches produced nothing
    T, ran, fit = many.align([(0, 1, T0), (0, 2, T0)], n_outer=0)
    check_fit(fit[0], want, "with patches"); check_fit(fit[1], plain, "without")
    T, ran, fit = many.align([(0, 1, T0)], n_outer=2)
    against_oracle(orc, many, 0, 1, T0, 2, T[0], ran[0], fit[0], "patches", T_true=T_TRUE, centre=centre)
    many.close(); ctx.close()


def lattice_scene():
    """case 5: every coordinate is a multiple of 1/16, so distances tie bit for bit.  surf: a 0.5 m lattice at z = -2 +- 1/16 in a
    chequer pattern, across the cube face x = 25; the queries sit at the cell centres at z = -2: four neighbours tie at the first
    distance, eight at the next, and which of those becomes the fifth changes the plane.  corner: points every 0.25 m along a pole
    with x = 10 +- 1/16 alternating, queries at the midpoints: the fifth neighbour ties between above and below.  Some dst points
    are there twice, bit for bit."""
    ix, iy = np.meshgrid(np.arange(40), np.arange(24))
    surf = np.stack([15.0 + 0.5 * ix.ravel(), -6.0 + 0.5 * iy.ravel(), -2.0 + 0.0625 * np.where((ix + 2 * iy).ravel() % 3 == 0, 1.0, -1.0)], 1)
    k = np.arange(120)
    pole = np.concatenate([np.stack([10.0 + 0.0625 * np.where(k % 2 == 0, 1.0, -1.0), np.full(len(k), y0), -10.0 + 0.25 * k], 1) for y0 in (3.0, 4.5)])
    qs = np.stack([15.25 + 0.5 * ix.ravel(), -5.75 + 0.5 * iy.ravel(), np.full(ix.size, -2.0)], 1)
    qc = np.concatenate([np.stack([np.full(110, 10.0), np.full(110, y0), -9.875 + 0.25 * np.arange(110)], 1) for y0 in (3.0, 4.5)])
    f4 = lambda p, w: np.concatenate([p, np.full((len(p), 1), float(w))], 1).astype(np.float32)
    surf = np.concatenate([surf, surf[37:400:11]]); pole = np.concatenate([pole, pole[5:200:13]])
    return make_map(f4(pole, 0), f4(surf, 1)), make_map(f4(qc, 0), f4(qs, 1))


def test_ties(api, orc):
    dst, src = lattice_scene()
    assert (dst[1][1][1] > 0).sum() >= 2                                            # the lattice crosses a cube face
    ctx = small_ctx(api)
    many = maps_object(api, ctx, [dst, src])
    stk, mp = clouds(many, 1), clouds(many, 0)
    tied = 0
    for w in (0, 1):                                                                # bit-equal fifth and sixth distances, in f32
        d = ((stk[w][:, None, :3] - mp[w][None, :, :3]) ** 2).sum(2, dtype=np.float32)
        d.sort(1)
        tied += int(((d[:, 4] == d[:, 5]) & (d[:, 4] < 1.0)).sum())
        assert len(np.unique(mp[w], axis=0)) < len(mp[w])                           # bit-identical dst points
    assert tied >= 200, tied
    want, _ = oracle_fit(orc, IDENT, stk, mp)
    assert want[0] >= 100 and want[1] >= 500, want
    T, ran, fit = many.align([(0, 1, IDENT)], n_outer=0)
    assert T.tobytes() == IDENT.reshape(1, 7).tobytes()
    check_fit(fit[0], want, "ties")
    many.close(); ctx.close()


def test_sizes_that_are_multiples_of_nothing(api, orc):
    """case 6: stacks of 1, 63, 65 and 257 points; the whole src gives more blocks than one evaluate chunk of 1024 holds, the small
    ones do not fill one"""
    centre = (6.0, -4.0, 1.0)
    dst, src, T0 = pair(6, centre)
    rng = np.random.default_rng(60)
    c_all, s_all = src[0][src[0][:, 3] == 0], src[0][src[0][:, 3] == 1]
    pick = lambda a, n: a[np.sort(rng.choice(len(a), n, replace=False))]
    sizes = [(1, 257), (63, 65), (65, 63), (257, 1)]
    maps = [dst, src] + [make_map(pick(c_all, nc), pick(s_all, ns)) for nc, ns in sizes]
    ctx = small_ctx(api)
    many = maps_object(api, ctx, maps)
    ops = [(0, q, T0) for q in range(1, len(maps))]
    mp = clouds(many, 0)
    T, ran, fit = many.align(ops, n_outer=0)
    wants = [oracle_fit(orc, T0, clouds(many, q), mp)[0] for q in range(1, len(maps))]
    assert wants[0][0] + wants[0][1] > 1024 and all(0 < w[0] + w[1] < 1024 for w in wants[1:]), wants
    for i, w in enumerate(wants):
        check_fit(fit[i], w, f"sizes op {i} at T0")
    T, ran, fit = many.align(ops, n_outer=2)
    for i, (d, s, _) in enumerate(ops):
        stk = clouds(many, s)
        assert i == 0 or (len(stk[0]), len(stk[1])) == sizes[i - 1]
        q, t, o_ran = orc.map_optimize(T0[:4], T0[4:], stk[0], mp[0], stk[1], mp[1], 2)
        assert o_ran and ran[i]
        check_pose(T[i], q, t, f"sizes op {i}")
        check_fit(fit[i], oracle_fit(orc, T[i], stk, mp)[0], f"sizes op {i} fit")
    many.close(); ctx.close()


def mixed(api, ctx):
    """maps 0, 1: two dst; 2: the src they share; 3: a dst whose corner cloud has 10 points (gate shut); 4: another src"""
    c0, c1 = (6.0, -4.0, 1.0), (25.0, 25.0, 25.0)
    d0, s0, T0 = pair(7, c0)
    rng = np.random.default_rng(70)
    d1 = [g.astype(np.float32) for g in geometry(rng, c0, phase=0.07)]
    few = [d1[0][:10], d1[1]]
    d4, s4, T4 = pair(8, c1)
    many = maps_object(api, ctx, [d0, make_map(*d1), s0, make_map(*few), s4, d4])
    ops = [(0, 2, T0), (1, 2, T0), (3, 2, T0), (5, 4, T4), (5, 2, T0)]
    return many, ops


def bits(T, ran, fit):
    return [(T[i].tobytes(), bool(ran[i]), None if fit is None else fit_tuple(fit[i])) for i in range(len(T))]


def test_many_ops_equal_one_op_at_a_time(api, orc):
    """case 7 (and 9, 10): three ops share one src, one op's gate is shut; every op's T, ran and fit are bitwise what it gives alone,
    and a second call gives the same bits; nothing of the object changes; one synchronisation whatever the call holds"""
    ctx = small_ctx(api)
    many, ops = mixed(api, ctx)
    before = state(many)
    sy0, f0 = many.stats()
    T, ran, fit = many.align(ops, n_outer=2)
    assert many.stats() == (sy0 + ALIGN_SYNCS, f0)
    together = bits(T, ran, fit)
    assert ran.tolist() == [True, True, False, True, True]
    assert together[2] == (np.asarray(ops[2][2]).tobytes(), False, (0, 0, 0.0, 0.0, 0.0))   # gate shut: T as given, fit all zero
    assert together[4][2][0] + together[4][2][1] == 0 and together[4][0] == np.asarray(ops[4][2]).tobytes()   # no block: T unchanged
    assert bits(*many.align(ops, n_outer=2)) == together
    for i, op in enumerate(ops):
        sy = many.stats()[0]
        alone = bits(*many.align([op], n_outer=2))
        assert many.stats()[0] - sy == (ALIGN_SYNCS if ran[i] else 0), i
        assert alone[0] == together[i], i
    assert bits(*many.align(ops[::-1], n_outer=2)) == together[::-1]
    for i in (0, 1, 3):
        d, s, T0 = ops[i]
        against_oracle(orc, many, d, s, T0, 2, T[i], ran[i], fit[i], f"op {i}")
    assert state(many) == before and many.stats()[1] == f0
    many.close(); ctx.close()


@pytest.mark.parametrize("n_outer", [2, 4])
def test_outer_iterations_and_no_fit(api, orc, n_outer):
    """case 8"""
    centre = (6.0, -4.0, 1.0)
    dst, src, T0 = pair(9, centre)
    ctx = small_ctx(api)
    many = maps_object(api, ctx, [dst, src])
    T, ran, fit = many.align([(0, 1, T0)], n_outer=n_outer)
    against_oracle(orc, many, 0, 1, T0, n_outer, T[0], ran[0], fit[0], f"n_outer {n_outer}", T_true=T_TRUE, centre=centre)
    T2, ran2, none = many.align([(0, 1, T0)], n_outer=n_outer, fit=False)
    assert none is None and T2.tobytes() == T.tobytes() and ran2.tolist() == ran.tolist()
    opt = api.LmOptions(); many.lib.ll_lm_default_options(C.byref(opt))
    T3, _, _ = many.align([(0, 1, T0)], n_outer=n_outer, opt=opt)
    assert T3.tobytes() == T.tobytes()                                              # NULL means the defaults
    many.close(); ctx.close()


def test_synchronisations(api):
    """case 10: the same number for 1 and 5 ops, with and without the record, for n_outer 0, 2 and 4"""
    ctx = small_ctx(api)
    many, ops = mixed(api, ctx)
    f0 = many.stats()[1]
    for sel in (ops[:1], ops):
        for fit in (True, False):
            for n_outer in (0, 2, 4):
                sy = many.stats()[0]
                many.align(sel, n_outer=n_outer, fit=fit)
                assert many.stats() == (sy + ALIGN_SYNCS, f0), (len(sel), fit, n_outer)
    text = open(os.path.join(ROOT, "include", "lightloam_hip.h")).read()
    assert "whatever n_ops, n_outer, the maps' sizes and fit are: ONE" in text
    many.close(); ctx.close()


def test_refusals(api):
    """case 11"""
    ctx = small_ctx(api)
    many, ops = mixed(api, ctx)
    before = state(many)
    sy = many.stats()
    T0 = ops[0][2]
    for bad, word in (([(0, 2, T0), (1, 1, T0)], "op 1"), ([(0, 6, T0)], "op 0"), ([(0, 2, T0), (1, 2, T0), (-1, 2, T0)], "op 2"), ([(0, -1, T0)], "op 0")):
        with pytest.raises(api.LightLoamError) as e:
            many.align(bad)
        assert e.value.code == -2 and word in str(e.value), (bad, e.value)
    with pytest.raises(api.LightLoamError) as e:
        many.align(ops[:1], n_outer=-1)
    assert e.value.code == -2 and "n_outer" in str(e.value)
    rec = (api.MergeOp * 1)(api.MergeOp(0, 2, (C.c_double * 7)(*T0)))
    out = np.zeros(7)
    lib = many.lib
    assert lib.ll_cubemaps_align(many.h, C.addressof(rec), 1, 2, None, None, None, None) == -2 and "op 0" in lib.ll_cubemaps_last_error(many.h).decode()
    assert lib.ll_cubemaps_align(many.h, C.addressof(rec), -1, 2, None, out.ctypes.data, None, None) == -2
    assert lib.ll_cubemaps_align(many.h, None, 1, 2, None, out.ctypes.data, None, None) == -2
    assert lib.ll_cubemaps_align(None, C.addressof(rec), 1, 2, None, out.ctypes.data, None, None) == -2
    assert lib.ll_cubemaps_align_timing(None, None, None) == -2
    with pytest.raises(api.LightLoamError) as e:
        many.align([ops[1], (0, 2, np.r_[T0[:5], np.nan, T0[6]])])
    assert e.value.code == -7 and "op 1" in str(e.value), e.value
    assert many.stats() == sy and state(many) == before                             # nothing was enqueued, nothing synchronised
    sy = many.stats()                                                               # (state() exports: one synchronisation of its own)
    assert lib.ll_cubemaps_align(many.h, C.addressof(rec), 1, 2, None, out.ctypes.data, None, None) == 0   # NULL ran and fit
    assert lib.ll_cubemaps_align(many.h, None, 0, 2, None, None, None, None) == 0   # no op: nothing to do
    assert many.stats() == (sy[0] + ALIGN_SYNCS, sy[1]) and state(many) == before
    many.close(); ctx.close()


def test_align_then_merge_two_drives(api, orc, synth):
    """case 12: one synthetic 16-ring drive mapped twice, the second time with its world frame shifted by OFFSET; align from a
    perturbed guess, then merge under the result: the merged map is expected_merge's under the same T, bytewise, and the aligned
    T is nearer the known offset than the guess"""
    n, OFFSET = 4, (1.5, -1.0, 0.25)
    cfgs, scans, _ = drives(synth, 16, 1, n)
    cfgs, scans = [cfgs[0]] * 2, [scans[0]] * 2
    ctx = _ctx(api, 16, scans)
    c, s, pool = CAP[16]
    many = api.CubeMaps(ctx, 2, c, s, pool_points=pool)
    for k in range(n):
        many.process_slots(_guesses(synth, cfgs, k, [(0.0, 0.0, 0.0), OFFSET]), [2 * k, 2 * k + 1])
    T_true = np.r_[IDENT[:4], -np.array(OFFSET)]                                    # map 1's world frame into map 0's
    centre = (10.0, 0.0, 0.0)
    T0 = perturbed(T_true, centre, shift=(0.2, -0.15, 0.05), deg=0.5)
    before = state(many)
    T, ran, fit = many.align([(0, 1, T0)], n_outer=3)
    assert ran[0] and fit[0].n_edge > 10 and fit[0].n_plane > 50 and state(many) == before
    e0, e1 = pose_error(T0, T_true, centre, half=20.0), pose_error(T[0], T_true, centre, half=20.0)
    print(f"two drives: {e0:.3f} m at the guess, {e1:.3f} m aligned, fit {fit_tuple(fit[0])}")
    assert e1 < e0, (e0, e1)
    cen, _, valid = many.layout(0)
    want, added, dropped, _ = expected_merge(orc, many, 0, 1, T[0])
    got_added, got_dropped = many.merge([(0, 1, T[0])])
    assert got_added.tolist() == [added] and got_dropped.tolist() == [dropped] and min(added) > 0
    check_map(many, 0, want, cen, valid, "aligned and merged")
    many.close(); ctx.close()


def test_through_drives_between_two_steps(api, synth):
    """case 13: lanes 0 and 1 map two drives and go idle, lane 2 localises against map 0; an align of map 1 to map 0 between two of
    its steps changes nothing: the next step's poses and fit record have the same bits as without the call"""
    n_map, J = 4, 1
    _, scans, pose0 = drives(synth, 16, 2, n_map + 1)
    out = []
    for with_align in (False, True):
        ctx, dr = make_drives(api, scans)
        started, mapped0 = set(), []
        for k in range(n_map):
            _, mapped, _ = step(api, ctx, dr, {0: (0, k), 1: (1, k)}, scans, pose0, started)
            mapped0.append(mapped[0].copy())
        dr.step(np.zeros(3, np.int32))
        start = np.tile(IDENT, (3, 1)); start[2] = mapped0[J]
        dr.set_localize([-1, -1, 0], start)
        started = set()
        step(api, ctx, dr, {2: (0, J)}, scans, pose0, started)
        if with_align:
            s0 = dr.stats()
            T, ran, fit = dr.cubemaps.align([(0, 1, IDENT), (1, 0, IDENT)], n_outer=1)
            assert ran.all() and dr.stats() == s0
            assert dr.cubemaps.align_timing()[1][0] > 0
        odom, mapped, ran = step(api, ctx, dr, {2: (0, J + 1)}, scans, pose0, started)
        out.append((odom[2].tobytes(), mapped[2].tobytes(), bool(ran[2]), fit_tuple(dr.fit()[2]), dr.cubemaps.export(ALL)[0].tobytes()))
        dr.close(); ctx.close()
    assert out[0] == out[1] and out[0][2]


def test_native_host_mirror(tmp_path, api):
    """case 14: lightloam::LaserMappingSequences::align_maps in a native program on the same two maps: the same bits as CubeMaps.align"""
    from lightloam_amd import build
    dst, src, T0 = pair(14, (6.0, -4.0, 1.0))
    ctx = small_ctx(api)
    many = maps_object(api, ctx, [dst, src])
    T, ran, fit = many.align([(0, 1, T0)], n_outer=2)
    many.close(); ctx.close()
    for q, m in enumerate((dst, src)):
        m[0].astype("<f4").tofile(tmp_path / f"map{q}.bin")
        np.r_[m[1][0], m[1][1].ravel()].astype("<i4").tofile(tmp_path / f"layout{q}.bin")
    np.asarray(T0, "<f8").tofile(tmp_path / "guess.bin")
    lib_dir = os.path.dirname(build.lib_path())
    exe = str(tmp_path / "align_host")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "native", "align_host.cpp"), "-o", exe,
                           "-L", lib_dir, "-llightloam_hip", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"])
    res = subprocess.run(["timeout", "-k", "10", "120", exe, str(tmp_path)], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    got = np.fromfile(tmp_path / "result.bin", "<f8")
    assert got[:7].tobytes() == T[0].tobytes() and got[7] == 1.0 == float(ran[0])
    assert tuple(got[8:13]) == tuple(float(x) for x in fit_tuple(fit[0]))
