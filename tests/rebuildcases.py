"""What ll_cubemaps_insert_keyframes has to produce, restated in numpy from the CPU oracle's pointAssociateToMap, the cube arithmetic
of laserMapping.cpp:2108-2125 and the oracle's VoxelGrid -- nothing here comes from the library under test -- and the crafted scenes
of tests/test_gpu_keyframes.py.  A keyframe is (corner cloud, surf cloud, pose_w7): clouds (n, 4) float32 in the sensor frame."""
import numpy as np

W, H, D = 21, 21, 11
N = W * H * D
LEAF = (0.4, 0.8)
EMPTY = np.zeros((0, 4), np.float32)
IDENT = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])


def yaw_pose(deg, t):
    a = np.deg2rad(deg) / 2
    return np.array([0.0, 0.0, np.sin(a), np.cos(a), t[0], t[1], t[2]])


def cubes_of(pts, cen):
    """:2108-2125 for float32 points: the cube index per point, -1 outside the array"""
    idx = []
    for k in range(3):
        v = pts[:, k].astype(np.float64) + 25.0
        c = np.trunc(v / 50.0).astype(np.int64) + int(cen[k])
        c[v < 0] -= 1
        idx.append(c)
    i, j, k = idx
    inside = (i >= 0) & (i < W) & (j >= 0) & (j < H) & (k >= 0) & (k < D)
    return np.where(inside, i + W * j + W * H * k, -1)


def box(rng, n, lo, hi, intensity=0.0):
    p = rng.uniform(lo, hi, size=(n, 3)).astype(np.float32)
    return np.concatenate([p, np.full((n, 1), intensity, np.float32) + rng.integers(0, 64, (n, 1)).astype(np.float32)], 1)


def expected_insert(orc, cubes_of_dst, cen, frames, poses, pre=None):
    """cubes_of_dst: {(w, cube): cloud} of dst before the call ({} for a reset map); frames: the listed keyframes in list order
    (a repeated id is listed twice), poses [n, 7] -> ({(w, cube): cloud} after, added [2], dropped [2]).  Per type the listed frames'
    clouds back to back, each under its own pose; every cube that receives a point = old cloud + new points in that order through
    VoxelGrid once.  pre (a dict, optional) receives the filter input sizes per touched cube"""
    want = dict(cubes_of_dst)
    added, dropped = [0, 0], [0, 0]
    for w in (0, 1):
        parts = [orc.point_associate_to_map(np.asarray(P[:4], np.float64), np.asarray(P[4:], np.float64), f[w]) for f, P in zip(frames, poses) if len(f[w])]
        if not parts:
            continue
        tp = np.concatenate(parts)
        c = cubes_of(tp, cen)
        dropped[w] = int((c < 0).sum()); added[w] = int((c >= 0).sum())
        for cube in np.unique(c[c >= 0]):
            cloud = np.concatenate([want.get((w, int(cube)), EMPTY), tp[c == cube]])
            want[(w, int(cube))] = orc.voxel_grid(cloud, LEAF[w])
            if pre is not None:
                pre[(w, int(cube))] = len(cloud)
    return want, added, dropped


# ---------------------------------------------------------------- crafted scenes (seeded; sensor-frame clouds around the origin)
def frame(rng, n_corner, n_surf, half=(20.0, 20.0, 4.0), centre=(0.0, 0.0, 0.0)):
    lo, hi = np.array(centre) - np.array(half), np.array(centre) + np.array(half)
    return (box(rng, n_corner, lo, hi, 0.0) if n_corner else EMPTY, box(rng, n_surf, lo, hi, 1.0) if n_surf else EMPTY)


def general_scene(seed):
    """5 frames with distinct yaw + translation poses whose clouds (+-24 m boxes) straddle cube faces after the transform (the poses
    put them near x = 25, y = -25); dst: points in 4 cubes, two of them where the frames land"""
    rng = np.random.default_rng(seed)
    poses = [yaw_pose(10.0 + 17.0 * k, (20.0 + 3.0 * k, -22.0 + 2.5 * k, 0.5 * k)) for k in range(5)]
    frames = [frame(rng, 500 + 130 * k, 900 + 210 * k, half=(24.0, 24.0, 5.0)) for k in range(5)]
    dcentres = [(0.0, 0.0, 0.0), (50.0, -50.0, 0.0), (-400.0, 300.0, 20.0), (150.0, 420.0, -30.0)]
    dst = [np.concatenate([box(rng, 600 + 100 * k, np.array(c) - 15.0, np.array(c) + 15.0, w) for k, c in enumerate(dcentres)]) for w in (0, 1)]
    return frames, poses, dst


def moved_centre_scene(seed):
    """centre (3, 17, 5): cube index 20 ends at x = (21 - 3) * 50 - 25 = 875.  Frame 0 lies across that edge (drops), frame 1 across
    x + 25 = 0 with y and z negative, frame 2 wholly outside"""
    rng = np.random.default_rng(seed)
    frames = [frame(rng, 1500, 1500, half=(40.0, 25.0, 20.0)), frame(rng, 500, 700, half=(15.0, 25.0, 20.0)), frame(rng, 90, 10)]
    poses = [yaw_pose(0.6, (870.0, -275.0, -40.0)), yaw_pose(-3.0, (-25.0, -275.0, -40.0)), yaw_pose(0.0, (2000.0, 0.0, 0.0))]
    return frames, poses, (3, 17, 5)


SIZES = [(0, 5), (7, 0), (0, 0), (1, 1), (63, 64), (65, 63), (1023, 1025), (1024, 1024), (1025, 1023), (2047, 2049), (2049, 2047)]


def sizes_scene(seed):
    """one frame per entry of SIZES (corner, surf points: 0 for one type and for both, 1, around the wave, the tile and the chunk),
    each in a cube of its own along x"""
    rng = np.random.default_rng(seed)
    frames = [frame(rng, c, s) for c, s in SIZES]
    poses = [yaw_pose(5.0 * k, (-250.0 + 50.0 * k, 100.0, 0.0)) for k in range(len(SIZES))]
    return frames, poses


def chunk_scene(seed):
    """three frames of 700 points per type: the first 2048-point chunk of the counting sort spans two frame boundaries; the poses are
    100 m apart so that a wrong pose for a tile shows in the cube"""
    rng = np.random.default_rng(seed)
    frames = [frame(rng, 700, 700) for _ in range(3)]
    poses = [yaw_pose(20.0 * k, (100.0 * k, -30.0, 1.0)) for k in range(3)]
    return frames, poses


def one_cube_scene(seed):
    """four frames (+-4 m) that all land inside cube (10, 10, 5)"""
    rng = np.random.default_rng(seed)
    frames = [frame(rng, 300 + 50 * k, 400 + 50 * k, half=(4.0, 4.0, 2.0)) for k in range(4)]
    poses = [yaw_pose(30.0 * k, (2.0 * k - 3.0, 1.5 * k, 0.2 * k)) for k in range(4)]
    return frames, poses


def spread_scene(seed):
    """one frame of +-70 m x +-70 m x +-30 m around a cube corner: 3 x 3 x 2 = 18 cubes and more"""
    rng = np.random.default_rng(seed)
    return [frame(rng, 3000, 3000, half=(70.0, 70.0, 30.0))], [yaw_pose(33.0, (25.0, 25.0, 25.0))]
