"""An independent numpy restatement of ll_bev (include/lightloam_hip.h) and the inputs of its tests.

np_side takes the listed frames of a side into the anchor's frame (np_to_world / np_to_frame of tests/viscases.py: float64 with the
header's operation order, each coordinate rounded to float once).  np_grid, np_query, np_volume, np_peak and np_result restate the
definition operation by operation in float32 numpy -- the volume by brute force, one gather per hypothesis -- with the cosine and sine
from math.cos / math.sin (the libm the library's host code calls; numpy's vectorised ones may differ in the last bit).  np_guess is
ll_bev_guess.  No expected value of any test comes from the library.  tests/test_bev_cases.py checks, without a GPU, the restatement
against hand-computed cases and what the default parameters do on the yard scene.
"""
import functools
import math

import numpy as np

from viscases import np_to_frame, np_to_world, pts4, quat

F = np.float32
DEFAULTS = dict(cell=0.5, half=128, shift_half=16, z_min=-1.0, z_layer=1.0, excl_yaw=1, excl_shift=2, max_ops=64, max_yaws=16, max_points=1 << 21)
SMALL = dict(half=16, shift_half=4, cell=0.5)
IDENTITY = np.array([0, 0, 0, 1, 0, 0, 0], np.float64)
EMPTY = pts4(np.zeros((0, 3)))


def cfg(**kw):
    """the parameters as the library holds them (floats) and the derived constants inv, invz"""
    c = dict(DEFAULTS); c.update(kw)
    for k in ("cell", "z_min", "z_layer"):
        c[k] = F(c[k])
    c["inv"] = F(1.0 / np.float64(c["cell"]))
    c["invz"] = F(1.0 / np.float64(c["z_layer"]))
    return c


def lib_params(c):
    """the keyword arguments of Context.bev for cfg c"""
    return {k: (float(c[k]) if k in ("cell", "z_min", "z_layer") else int(c[k])) for k in DEFAULTS}


# ---------------------------------------------------------------------------------------------- the restatement
def np_side(frames, poses):
    """frames: a list of (corner (n, 4), surf (m, 4)) float32, the first is the anchor; poses [n_frames][7] -> (N, 3) float32 in the
    anchor's frame: the frames in list order, per frame the corner cloud and then the surf cloud"""
    poses = np.asarray(poses, np.float64).reshape(-1, 7)
    out = [np.zeros((0, 3), F)]
    for (co, su), P in zip(frames, poses):
        for cloud in (co, su):
            p = np.asarray(cloud, F).reshape(-1, 4)[:, :3]
            if len(p):
                out.append(np_to_frame(poses[0], np_to_world(P, p)))
    return np.concatenate(out)


def np_layer(l, c):
    """(N, 3) float32 -> (N,) int: the layer 0 .. 7, -1: dropped (a non-finite coordinate) or no layer; tests on the floats"""
    l = np.asarray(l, F).reshape(-1, 3)
    with np.errstate(all="ignore"):
        fl = np.floor((l[:, 2] - c["z_min"]) * c["invz"])
        ok = np.isfinite(l).all(axis=1) & (fl >= 0) & (fl <= 7)
    return np.where(ok, fl, F(-1)).astype(np.int64)


def np_cell(x, y, c):
    """float32 x, y -> (ix, iy int64 (0 where outside), inside bool): floorf(x * inv), tested on the floats"""
    h = c["half"]
    with np.errstate(all="ignore"):
        fx = np.floor(x * c["inv"]); fy = np.floor(y * c["inv"])
        inside = (fx >= -h) & (fx <= h - 1) & (fy >= -h) & (fy <= h - 1)
    return np.where(inside, fx, F(0)).astype(np.int64), np.where(inside, fy, F(0)).astype(np.int64), inside


def np_grid(l, c):
    """the target grid [2 half][2 half] uint8 of the side's points l"""
    h = c["half"]
    l = np.asarray(l, F).reshape(-1, 3)
    lay = np_layer(l, c)
    ix, iy, inside = np_cell(l[:, 0], l[:, 1], c)
    ok = inside & (lay >= 0)
    g = np.zeros((2 * h, 2 * h), np.uint8)
    np.bitwise_or.at(g, (iy[ok] + h, ix[ok] + h), (1 << lay[ok]).astype(np.uint8))
    return g


def np_yaws(yaw0, yaw_step, n_yaws):
    return [float(yaw0) + float(j) * float(yaw_step) for j in range(n_yaws)]


def np_volume(grid, l, yaws, c):
    """scores [n_yaws][2 sh][2 sh] int32 of the query side's points l against the target grid, and n_query"""
    h, sh = c["half"], c["shift_half"]
    l = np.asarray(l, F).reshape(-1, 3)
    lay = np_layer(l, c)
    x, y = l[lay >= 0, 0], l[lay >= 0, 1]; lay = lay[lay >= 0]
    pad = np.zeros((2 * h + 2 * sh, 2 * h + 2 * sh), np.uint8)              # a cell outside the grid is empty
    pad[sh:sh + 2 * h, sh:sh + 2 * h] = grid
    vol = np.zeros((len(yaws), 2 * sh, 2 * sh), np.int32)
    for j, yaw in enumerate(yaws):
        cs, sn = F(math.cos(yaw)), F(math.sin(yaw))
        with np.errstate(all="ignore"):
            xr = cs * x - sn * y; yr = sn * x + cs * y                       # float32: every product and sum rounded
        ix, iy, inside = np_cell(xr, yr, c)
        ix, iy, bit = ix[inside] + h + sh, iy[inside] + h + sh, lay[inside]
        for a, sy in enumerate(range(-sh, sh)):
            for b, sx in enumerate(range(-sh, sh)):
                vol[j, a, b] = np.count_nonzero((pad[iy + sy, ix + sx] >> bit) & 1)
    return vol, int(len(lay))


def np_peak(vol, c):
    """(score, second, iyaw, sx, sy): the largest score, ties to the lowest flat index; second: the largest outside the window, -1: none"""
    sh = c["shift_half"]
    j, a, b = np.unravel_index(int(np.argmax(vol)), vol.shape)            # argmax returns the first of equal maxima
    jj, aa, bb = np.meshgrid(np.arange(vol.shape[0]), np.arange(vol.shape[1]), np.arange(vol.shape[2]), indexing="ij")
    out = (np.abs(jj - j) > c["excl_yaw"]) | (np.abs(bb - b) > c["excl_shift"]) | (np.abs(aa - a) > c["excl_shift"])
    second = int(vol[out].max()) if out.any() else -1
    return int(vol[j, a, b]), second, int(j), int(b) - sh, int(a) - sh


def np_result(vol, n_query, yaws, c):
    score, second, j, sx, sy = np_peak(vol, c)
    yaw = yaws[j]
    D = np.array([0.0, 0.0, math.sin(yaw / 2.0), math.cos(yaw / 2.0), float(sx) * float(c["cell"]), float(sy) * float(c["cell"]), 0.0])
    return dict(score=score, second=second, iyaw=j, sx=sx, sy=sy, n_query=n_query, yaw=yaw, D=D)


def np_match(case, c):
    """a case (below) -> (grid, volume, result)"""
    frames, poses = case["frames"], case["poses"]
    side = lambda ids, given: np_side([frames[i] for i in ids], given if given is not None else [poses[i] for i in ids])   # noqa: E731
    grid = np_grid(side(case["target"], case["target_poses"]), c)
    yaws = np_yaws(case["yaw0"], case["yaw_step"], case["n_yaws"])
    vol, nq = np_volume(grid, side(case["query"], case["query_poses"]), yaws, c)
    return grid, vol, np_result(vol, nq, yaws, c)


def _rot(q, v):
    ux, uy, uz, w = q
    uvx = uy * v[2] - uz * v[1]; uvy = uz * v[0] - ux * v[2]; uvz = ux * v[1] - uy * v[0]
    uvx = uvx + uvx; uvy = uvy + uvy; uvz = uvz + uvz
    return np.array([(v[0] + w * uvx) + (uy * uvz - uz * uvy), (v[1] + w * uvy) + (uz * uvx - ux * uvz), (v[2] + w * uvz) + (ux * uvy - uy * uvx)])


def np_compose(A, B):
    """A o B = (q_A x q_B, R(q_A) t_B + t_A) in float64, the operations in the header's order"""
    ax, ay, az, aw = (float(v) for v in A[:4]); bx, by, bz, bw = (float(v) for v in B[:4])
    q = [aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw,
         aw * bw - ax * bx - ay * by - az * bz]
    return np.concatenate([q, _rot([float(v) for v in A[:4]], [float(v) for v in B[4:]]) + np.asarray(A[4:], np.float64)])


def np_inverse(P):
    P = np.asarray(P, np.float64)
    q = np.array([-P[0], -P[1], -P[2], P[3]])
    return np.concatenate([q, -_rot([float(v) for v in q], [float(v) for v in P[4:]])])


def np_guess(Pc, D, Pq):
    """T0 = P_c o (D o P_q^-1)"""
    return np_compose(np.asarray(Pc, np.float64), np_compose(np.asarray(D, np.float64), np_inverse(Pq)))


def pose_matrix(P):
    """the 4 x 4 matrix of a pose with a unit quaternion, by the textbook formula (an independent check of np_guess)"""
    x, y, z, w = (float(v) for v in P[:4])
    M = np.eye(4)
    M[:3, :3] = [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                 [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                 [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]
    M[:3, 3] = P[4:]
    return M


# ---------------------------------------------------------------------------------------------- crafted inputs
def case(name, frames, target, query, yaw0=0.0, yaw_step=math.radians(1.0), n_yaws=1, poses=None, target_poses=None, query_poses=None):
    """frames: the store's content, a list of (corner, surf); target / query: ids into it"""
    poses = np.tile(IDENTITY, (len(frames), 1)) if poses is None else np.asarray(poses, np.float64).reshape(len(frames), 7)
    return dict(name=name, frames=frames, poses=poses, target=list(target), query=list(query), target_poses=target_poses, query_poses=query_poses,
                yaw0=float(yaw0), yaw_step=float(yaw_step), n_yaws=int(n_yaws))


def split(xyz):
    """(n, 3) -> a frame (corner, surf): every third point is a corner point"""
    p = pts4(xyz)
    k = np.arange(len(p)) % 3 == 0
    return p[k], p[~k]


def _ulps(v):
    v = F(v)
    return [np.nextafter(v, F(-np.inf)), v, np.nextafter(v, F(np.inf))]


def random_points(rng, n, c, spread=0.9, z=(-2.0, 8.0)):
    """n points over `spread` of the square and a z range that leaves some points below layer 0 and above layer 7"""
    r = spread * c["half"] * float(c["cell"])
    return np.stack([rng.uniform(-r, r, n), rng.uniform(-r, r, n), rng.uniform(float(c["z_min"]) + z[0], float(c["z_min"]) + z[1], n)], axis=1)


def crafted_cases(c):
    """name -> case, for a cfg with the SMALL parameters (half 16, shift_half 4, cell 0.5): the square is -8 .. 8 m"""
    cell, zmin, zl, h, sh = float(c["cell"]), float(c["z_min"]), float(c["z_layer"]), c["half"], c["shift_half"]
    rng = np.random.default_rng(20261020)
    out = []
    # coordinates at k * cell and one ulp either side, z at z_min + k * z_layer and one ulp either side; the query is the target
    # moved by less than a cell, so that its own edges are others
    edge = []
    for k in (-3, -1, 0, 1, 2, 5):
        for v in _ulps(k * cell):
            edge += [[v, 0.7, zmin + 1.5], [-1.3, v, zmin + 2.5]]
    for k in (0, 1, 4, 7, 8):
        for v in _ulps(zmin + k * zl):
            edge.append([2.2 + 0.5 * k, -3.1, v])
    edge = np.array(edge, np.float64)
    out.append(case("cell_edges", [split(edge), split(edge[::-1] + [0.25, 0.25, 0.0])], [0], [1], n_yaws=3, yaw0=math.radians(-1.0)))
    out.append(case("cell_edges_same", [split(edge)], [0], [0]))
    # the outermost cells of the square and the first ones outside it, both sides: extreme shifts read the zero border
    lim = h * cell
    ring = []
    for v in (-lim - 0.01, -lim, -lim + 0.01, lim - cell, lim - 0.01, lim, lim + 0.3):
        for u in (-lim, -2.6, 0.1, lim - 0.2):
            ring += [[v, u, zmin + 0.5], [u, v, zmin + 3.5]]
    ring = np.array(ring)
    out.append(case("square_edges", [split(ring), split(ring[::2])], [0], [1], n_yaws=2, yaw0=0.0, yaw_step=math.radians(90.0)))
    # layers -1 and 8 are dropped, 0 and 7 are kept
    lay = np.array([[1.1, 1.1, zmin - 0.5], [1.1, 1.1, zmin + 0.5], [1.1, 1.1, zmin + 7.5], [1.1, 1.1, zmin + 8.5], [-2.1, 0.3, zmin - 0.01], [-2.1, 0.3, zmin + 8.0]])
    out.append(case("layer_limits", [(pts4(lay[:3]), pts4(lay[3:]))], [0], [0]))
    # NaN, +-inf and 1e30 in every coordinate, on both sides, among plain points
    bad = [[np.nan, 1, 0], [1, np.nan, 0], [1, 1, np.nan], [np.inf, 1, 0], [1, -np.inf, 0], [1, 1, np.inf], [-np.inf, np.inf, 0], [1e30, 1, 0], [1, -1e30, 0],
           [1, 1, 1e30], [1e30, 1e30, 1e30], [3e38, 3e38, 0.5], [np.nan, np.nan, np.nan]]
    plain = random_points(rng, 40, c)
    mix = np.concatenate([plain[:20], np.array(bad, np.float64), plain[20:]])
    out.append(case("bad_values", [split(mix), split(mix[::-1])], [0], [1], n_yaws=2, yaw0=math.radians(45.0), yaw_step=math.radians(45.0)))
    # empty and tiny sides
    some = split(random_points(rng, 50, c))
    out.append(case("empty_query", [some, (EMPTY, EMPTY)], [0], [1], n_yaws=2))
    out.append(case("empty_target", [(EMPTY, EMPTY), some], [0], [1], n_yaws=2))
    out.append(case("no_layer_at_all", [split(random_points(rng, 30, c, z=(-3.0, -0.1))), some], [0], [1]))
    k = int(np.flatnonzero((np_layer(some[1][:, :3], c) >= 0) & (np.abs(some[1][:, :2]) < 5.0).all(axis=1))[0])      # a target point with a layer
    out.append(case("one_point_query", [some, (EMPTY, pts4(some[1][k:k + 1, :3] + [0.5, -1.0, 0.0]))], [0], [1], n_yaws=3, yaw0=math.radians(-1.0)))
    # the staging chunk and its neighbours
    tgt = split(random_points(rng, 900, c))
    for n in (1023, 1024, 1025, 2049):
        q = random_points(rng, n, c, spread=1.05)
        out.append(case(f"chunk_{n}", [tgt, (pts4(q[:n // 2]), pts4(q[n // 2:]))], [0], [1], n_yaws=2, yaw0=math.radians(30.0), yaw_step=math.radians(-60.0)))
    # the limits of the search
    out.append(case("max_yaws", [tgt, split(random_points(rng, 300, c))], [0], [1], n_yaws=c["max_yaws"], yaw0=-math.pi, yaw_step=2.0 * math.pi / c["max_yaws"]))
    # two equal peaks: one query point, two target cells that two different shifts reach; and a volume of zeros
    one = np.array([[0.3, 0.3, zmin + 2.5]])
    two = np.array([[0.3 + 2 * cell, 0.3 - cell, zmin + 2.5], [0.3 - 3 * cell, 0.3 + 2 * cell, zmin + 2.5]])
    out.append(case("tie_two_peaks", [(pts4(two), EMPTY), (EMPTY, pts4(one))], [0], [1], n_yaws=2, yaw0=0.0, yaw_step=0.0))
    out.append(case("tie_all_zero", [(pts4(two + [0, 0, 3.0]), EMPTY), (EMPTY, pts4(one))], [0], [1], n_yaws=2))
    # the peak at a corner of the volume: the last yaw, the largest shifts
    far = np.array([[0.3 + (sh - 1) * cell, 0.3 + (sh - 1) * cell, zmin + 2.5]])
    out.append(case("peak_at_corner", [(pts4(far), EMPTY), (EMPTY, pts4(one))], [0], [1], n_yaws=1))
    near = np.array([[0.3 - sh * cell, 0.3 - sh * cell, zmin + 2.5], [0.3 + cell, 0.3, zmin + 2.5], [0.3 - sh * cell, 0.3 - sh * cell, zmin + 3.5]])
    q2 = np.array([[0.3, 0.3, zmin + 2.5], [0.3, 0.3, zmin + 3.5]])
    out.append(case("peak_at_first_corner", [(pts4(near), EMPTY), (EMPTY, pts4(q2))], [0], [1], n_yaws=1))
    # one target cell, one query point, a yaw of 90 degrees: the signs of c, s, sx, sy (hand-computed in tests/test_bev_cases.py)
    out.append(case("one_hot_90", [(pts4([[0.7, 3.3, zmin + 1.5]]), EMPTY), (pts4([[2.2, 0.3, zmin + 1.5]]), EMPTY)], [0], [1], yaw0=math.pi / 2.0))
    # sides of several frames under non-trivial poses, a repeated id, given and stored poses
    fr = [split(random_points(rng, 200 + 37 * k, c, spread=0.5)) for k in range(5)]
    ps = np.array([np.concatenate([quat(rng.uniform(-3, 3), rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1)), rng.uniform(-2.5, 2.5, 3) * [1, 1, 0.1]]) for _ in range(5)])
    out.append(case("multi_frame_stored", fr, [0, 1, 2, 1], [3, 4, 0], poses=ps, n_yaws=5, yaw0=math.radians(10.0), yaw_step=math.radians(-4.0)))
    given_t = ps[[2, 0, 4]] * 1.0; given_t[:, 4:] += 0.4
    given_q = ps[[1, 1, 3]] * 1.0; given_q[1, 4:] -= 1.1
    out.append(case("multi_frame_given", fr, [2, 0, 4], [1, 1, 3], poses=np.tile(IDENTITY * 3.0, (5, 1)), target_poses=given_t, query_poses=given_q, n_yaws=4,
                    yaw0=math.radians(-100.0), yaw_step=math.radians(3.0)))
    return {k["name"]: k for k in out}


def shift_limit_cases():
    """(cfg, case) for shift_half 1 and 16, each with a half that fits LDS and differs from the crafted cases'"""
    out = []
    for sh, half, seed in ((1, 8, 1), (16, 24, 2)):
        c = cfg(half=half, shift_half=sh, cell=0.5, max_ops=4, max_yaws=4)
        rng = np.random.default_rng(seed)
        t = random_points(rng, 600, c, spread=1.1); q = t[::2] + [1.5 * min(sh, 6), -0.5 * min(sh, 6), 0.0]
        out.append((c, case(f"shift_half_{sh}", [split(t), split(q)], [0], [1], n_yaws=3, yaw0=math.radians(-2.0), yaw_step=math.radians(2.0))))
    return out


def window_case():
    """a window that covers the whole volume: second = -1"""
    c = cfg(excl_yaw=2, excl_shift=7, **SMALL)
    rng = np.random.default_rng(5)
    t = random_points(rng, 200, c)
    return c, case("window_covers_all", [split(t), split(t + [0.5, 0.5, 0.0])], [0], [1], n_yaws=3, yaw0=math.radians(-1.0))


# ---------------------------------------------------------------------------------------------- the yard scene
YARD = dict(seed=11, n_boxes=14, extent=50.0, clear=9.0, sensor_z=1.8, rings=64, el_lo=-24.8, el_hi=2.0, az_step=0.5, leaf=0.4, max_range=100.0)
DISPLACEMENTS = [(3.2, -2.1, 184.0), (-6.3, 5.4, -3.0), (1.0, 7.6, 92.0)]       # dx, dy in metres, yaw in degrees: p_target = Rz(yaw) p_query + (dx, dy)


def _yard_boxes(Y):
    rng = np.random.default_rng(Y["seed"])
    boxes = []
    for _ in range(Y["n_boxes"]):
        cen = rng.uniform(-Y["extent"], Y["extent"], 2); size = rng.uniform(3, 12, 2); height = rng.uniform(1.5, 9)
        if np.all(np.abs(cen) < Y["clear"]):
            cen += 15                                                   # nothing stands where the sensors drive
        boxes.append((np.array([cen[0] - size[0] / 2, cen[1] - size[1] / 2, 0.0]), np.array([cen[0] + size[0] / 2, cen[1] + size[1] / 2, height])))
    return boxes


def _voxel(p, leaf):
    key = np.floor(p / leaf).astype(np.int64)
    _, first, inv = np.unique(key, axis=0, return_index=True, return_inverse=True)
    inv = inv.reshape(-1)
    s = np.zeros((len(first), 3)); np.add.at(s, inv, p)
    return (s / np.bincount(inv)[:, None])[np.argsort(first)]


def yard_scan(boxes, x, y, yaw, Y):
    """the scan of a sensor at (x, y, sensor_z) with heading yaw, in the sensor frame, one centroid per leaf-sized voxel"""
    el = np.radians(np.linspace(Y["el_lo"], Y["el_hi"], Y["rings"])); az = np.radians(np.arange(0.0, 360.0, Y["az_step"]))
    E, A = np.meshgrid(el, az, indexing="ij")
    d0 = np.stack([np.cos(E) * np.cos(A), np.cos(E) * np.sin(A), np.sin(E)], axis=-1).reshape(-1, 3)
    cs, sn = math.cos(yaw), math.sin(yaw)
    d = d0 @ np.array([[cs, -sn, 0], [sn, cs, 0], [0, 0, 1.0]]).T
    o = np.array([x, y, Y["sensor_z"]])
    with np.errstate(all="ignore"):
        t = np.where(d[:, 2] < 0, -o[2] / d[:, 2], np.inf)             # the ground plane
        for lo, hi in boxes:
            t0 = (lo - o) / d; t1 = (hi - o) / d
            tn = np.minimum(t0, t1).max(axis=1); tf = np.maximum(t0, t1).min(axis=1)
            hit = (tn <= tf) & (tn > 1e-6) & (tn < t)
            t = np.where(hit, tn, t)
    ok = np.isfinite(t) & (t < Y["max_range"])
    return _voxel(t[ok, None] * d0[ok], Y["leaf"])


@functools.lru_cache(maxsize=None)
def yard_scene(seed=YARD["seed"]):
    """-> (frames, poses): frame 0 is the target scan at the origin, frame 1 + k the query scan displaced by DISPLACEMENTS[k]; the
    poses are the sensors' in the yard.  A ground plane and 14 boxes of 1.5 .. 9 m height, 64 rings over -24.8 .. 2 degrees at 0.5
    degree azimuth, one centroid per 0.4 m voxel; every fifth point goes to the corner cloud"""
    Y = dict(YARD, seed=seed)
    boxes = _yard_boxes(Y)
    frames, poses = [], []
    for dx, dy, deg in [(0.0, 0.0, 0.0)] + DISPLACEMENTS:
        p = pts4(yard_scan(boxes, dx, dy, math.radians(deg), Y))
        k = np.arange(len(p)) % 5 == 0
        frames.append((p[k], p[~k]))
        poses.append(np.concatenate([quat(math.radians(deg), 0.0, 0.0), [dx, dy, Y["sensor_z"]]]))
    return frames, np.array(poses)


def yard_case(k, seed=YARD["seed"]):
    """displacement k as a case: yaw0 is the displacement rounded to the 6 degree sector minus 6 degrees, 13 yaws at 1 degree.  Both
    sides go in under the identity: a place match knows no pose of the query in the target's map"""
    frames, _ = yard_scene(seed)
    sector = math.radians(6.0)
    yaw0 = round(math.radians(DISPLACEMENTS[k][2]) / sector) * sector - sector
    return case(f"yard_{k}", list(frames), [0], [1 + k], yaw0=yaw0, yaw_step=math.radians(1.0), n_yaws=13)


@functools.lru_cache(maxsize=None)
def yard_reference(k, z_min=DEFAULTS["z_min"], seed=YARD["seed"]):
    """(grid, volume, result) of yard_case(k) by the restatement at the default parameters (z_min replaced): computed once per process"""
    return np_match(yard_case(k, seed), cfg(z_min=z_min))


def yard_found(res, k, c):
    """is displacement k recovered within one cell and one yaw step (1 degree)?"""
    dx, dy, deg = DISPLACEMENTS[k]
    dyaw = (res["yaw"] - math.radians(deg) + math.pi) % (2.0 * math.pi) - math.pi
    cell = float(c["cell"])
    return abs(res["D"][4] - dx) <= cell and abs(res["D"][5] - dy) <= cell and abs(dyaw) <= math.radians(1.0) + 1e-12
