"""The three ways the library solves laserMapping's scan-to-map problem give the same pose, bit for bit, on the same residual
blocks from the same start pose:
  (a) Map.solve             k_map_lm_solve: LL_NEQ_NB = 16 workgroups x 256 threads, one launch per ceres::Solve;
  (b) the stepwise calls    set_pose, evaluate (k_map_normal_eq), lm_begin, 4 x (lm_propose, evaluate, lm_accept), pose;
  (c) a CubeMaps frame      k_cms_lm: one workgroup that walks the 16 workgroups' shares as 16 passes.
All three take a block's sums, the reduction tree and the order of the partial sums from ll_map_neq.h.

The scene is fabricated: lattice-sampled planes and lines (no recorded data).  One CubeMaps sequence takes the map as its first
frame (an empty map optimises nothing and stores the frame) and the scan as its second; its search clouds and stacks of that frame
are read back and given to a Map, so that (a) and (b) associate exactly what (c) did.  The sizes are chosen for the partition: a
thread of workgroup b takes blocks 256 b + tid, + 4096, ...
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LINE_RES, PLANE_RES = 0.2, 0.4
T_TRUE = np.array([0.0, 0.0, np.sin(np.deg2rad(2.0) / 2), np.cos(np.deg2rad(2.0) / 2), 0.30, -0.20, 0.10])


def _rot(q, v):
    u, w = q[:3], q[3]
    uv = 2.0 * np.cross(u, v)
    return v + w * uv + np.cross(u, uv)


def _apply(T, p):
    return _rot(T[:4], p) + T[4:]


def _inverse(T):
    qi = np.array([-T[0], -T[1], -T[2], T[3]])
    return np.concatenate([qi, -_rot(qi, T[4:][None, :])[0]])


def _scene(rng, half, phase, r):
    """-> (corner [n, 4], surf [m, 4]) f64: the ground, two walls 4 m high, two poles and two horizontal lines (r from the walls) inside a square
    of side 2 * half.  The constant coordinate of every plane and line sits well inside a voxel of either leaf size, and so do the
    lattice points (0.4 m apart on planes, 0.2 m on lines, +- 0.02 m of noise): one stack point per lattice point, give or take"""
    u = np.arange(-half, half + 1e-9, 0.4) + phase
    h = np.arange(-1.6, 2.0 + 1e-9, 0.4) + phase
    gx, gy = np.meshgrid(u, u)
    ground = np.stack([gx.ravel(), gy.ravel(), np.full(gx.size, -1.87)], 1)
    wy, wz = np.meshgrid(u, h)
    wall_x = np.stack([np.full(wy.size, 0.13), wy.ravel(), wz.ravel()], 1)
    wall_y = np.stack([wy.ravel(), np.full(wy.size, -0.27), wz.ravel()], 1)
    z = np.arange(-1.6, 2.0 + 1e-9, 0.2) + phase / 2
    v = np.arange(-half, half + 1e-9, 0.2) + phase / 2
    poles = [np.stack([np.full(len(z), a), np.full(len(z), b), z], 1) for a, b in ((r, r), (-r, r))]
    lines = [np.stack([v, np.full(len(v), -r), np.full(len(v), 1.09)], 1), np.stack([np.full(len(v), -r - 0.3), v, np.full(len(v), 0.51)], 1)]

    def pts(xyz, w):
        xyz = np.concatenate(xyz) + rng.uniform(-0.02, 0.02, size=(sum(map(len, xyz)), 3))
        return np.concatenate([xyz, np.full((len(xyz), 1), float(w))], 1)
    return pts(poles + lines, 0), pts([ground, wall_x, wall_y], 1)


def _stepwise(m, pose, n_it=4):
    m.set_pose(pose)
    m.lm_begin(m.evaluate())
    for _ in range(n_it):
        m.lm_propose()
        m.lm_accept(m.evaluate())
    return m.pose()


def _same(a, b):
    return np.ascontiguousarray(a, np.float64).view(np.uint64).tolist() == np.ascontiguousarray(b, np.float64).view(np.uint64).tolist()


# scan half-width -> the ranges the edge and the plane blocks have to fall into
#   1.2:  both below 256: every partial sum but the first is zero
#   5.6:  planes in 257 .. 4095: several workgroups' shares, nobody takes a second block
#   13.2: planes in 4097 .. 8191: the first threads take a second block
@pytest.mark.parametrize("half,edges,planes", [(1.2, (1, 255), (1, 255)), (5.6, (1, 4095), (257, 4095)), (13.2, (257, 4095), (4097, 8191))])
def test_solve_stepwise_and_cubemaps_frame_agree(api, half, edges, planes):
    rng = np.random.default_rng(int(half * 10))
    r = 0.5 * half + 0.07
    map_c, map_s = [g.astype(np.float32) for g in _scene(rng, half + 2.0, 0.0, r)]
    Ti = _inverse(T_TRUE)
    scan_c, scan_s = [np.concatenate([_apply(Ti, g[:, :3]), g[:, 3:]], 1).astype(np.float32) for g in _scene(rng, half, 0.13, r)]
    pose0 = T_TRUE.copy()
    pose0[4:] += (0.10, -0.08, 0.05)
    cap_c, cap_s = len(map_c) + 64, len(map_s) + 64
    ctx = api.Context(api.default_params(16, batch=1, max_points=4096))
    many = api.CubeMaps(ctx, 1, cap_c, cap_s, pool_points=1 << 16, line_res=LINE_RES, plane_res=PLANE_RES)
    ident = np.array([[0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]])
    _, ran = many.process(ident, [map_c], [map_s])
    assert not ran[0]                                             # the empty map: the frame is stored, nothing is solved
    pose_c, ran = many.process(pose0[None, :], [scan_c], [scan_s])
    assert ran[0]
    cl = [many.cloud(0, w) for w in range(4)]                     # the search clouds and the stacks k_cms_lm's blocks came from
    m = api.Map(ctx, len(cl[0]), len(cl[1]), len(cl[2]), len(cl[3]))
    m.set_map(cl[0], cl[1])
    m.set_scan(cl[2], cl[3])
    p = pose0
    for outer in range(2):                                        # the frame's two rounds of (associate, solve), laserMapping.cpp:1832
        m.associate(p)
        ne, npl = m.counts()
        print(f"half {half} outer {outer}: {ne} edge blocks, {npl} plane blocks")
        assert edges[0] <= ne <= edges[1] and planes[0] <= npl <= planes[1], (ne, npl)
        a = m.solve(p)
        b = _stepwise(m, p)
        assert not np.isnan(a).any()
        assert _same(a, b), (outer, a, b)                         # (a) == (b)
        p = a
    assert _same(p, pose_c[0]), (p, pose_c[0])                    # (a) == (c)
    assert np.abs(p[4:] - T_TRUE[4:]).max() < np.abs(pose0[4:] - T_TRUE[4:]).max()   # and it is a solve: nearer the true pose than the guess
    m.close(); many.close(); ctx.close()
