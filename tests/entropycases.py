"""An independent numpy restatement of ll_entropy (include/lightloam_hip.h) and the inputs of its tests.

np_cloud is the op's cloud (viscases.np_to_world per frame, corner before surf).  np_outside is the header's cell test in float32.
np_moments is BRUTE FORCE: every point of the op against every other one with the float32 membership test operation by operation,
float64 moments of the float32 differences, numpy.linalg.eigvalsh.  There is no grid in it; the one economy is that the points are
walked in the order of their x coordinate and a block of queries is compared with the points whose x lies within 1.01 radius of the
block (a pair farther apart in x alone cannot pass the test), all of them.  np_rec sums with math.fsum.  bounds() is the error bound
of tests/test_gpu_entropy.py, derived there.  No expected value of any test comes from the library.
"""
import functools
import math

import numpy as np

import viscases as vc

F = np.float32
U = 2.0 ** -53
HALF = 65536
LOG_2PIE3 = 3.0 * (1.0 + math.log(2.0 * math.pi))
DEFAULTS = dict(radius=0.5, min_neighbours=6, lambda_floor=1e-6)
CHUNK = 256                                    # EN_CHUNK of ll_entropy.hip: float4 candidates per LDS staging chunk
IDENTITY = vc.IDENTITY


def cfg(**kw):
    """the parameters as the library holds them and the derived constants cell and r2, all float32"""
    c = dict(DEFAULTS); c.update(kw)
    c["radius"] = F(c["radius"]); c["lambda_floor"] = F(c["lambda_floor"]); c["min_neighbours"] = int(c["min_neighbours"])
    c["cell"] = c["radius"] * F(1.03125)
    c["r2"] = c["radius"] * c["radius"]
    return c


def lib_params(c):
    return dict(radius=float(c["radius"]), min_neighbours=c["min_neighbours"], lambda_floor=float(c["lambda_floor"]))


def np_cloud(frames, poses):
    """-> (w (n, 3) float32 world points in list order, sizes [(n_corner, n_surf)] per frame)"""
    poses = np.asarray(poses, np.float64).reshape(-1, 7)
    parts, sizes = [], []
    for (co, su), P in zip(frames, poses):
        co = np.asarray(co, F).reshape(-1, 4); su = np.asarray(su, F).reshape(-1, 4)
        parts += [vc.np_to_world(P, co), vc.np_to_world(P, su)]
        sizes.append((len(co), len(su)))
    return (np.concatenate(parts) if parts else np.zeros((0, 3), F)).astype(F).reshape(-1, 3), sizes


def np_outside(w, c):
    """(n,) bool: a coordinate is not finite, or its cell floorf(w / cell) is not in -65536 .. 65535"""
    with np.errstate(all="ignore"):
        f = np.floor(np.asarray(w, F) / c["cell"])                    # float32 quotient, correctly rounded
        ok = (f >= F(-HALF)) & (f < F(HALF))                          # a NaN fails
    return ~ok.all(axis=1)


def np_moments(w, c, block=256):
    """w (n, 3) float32, one op -> dict: nn (n,) int64 (0: outside), lam (n, 3) float64 eigenvalues ascending (NaN where nn == 0)"""
    w = np.asarray(w, F).reshape(-1, 3)
    n = len(w)
    nn = np.zeros(n, np.int64); lam = np.full((n, 3), np.nan)
    inside = np.nonzero(~np_outside(w, c))[0]
    if len(inside) == 0:
        return dict(nn=nn, lam=lam)
    order = inside[np.argsort(w[inside, 0], kind="stable")]
    P = w[order]
    px = P[:, 0].astype(np.float64)
    reach = 1.01 * float(c["radius"]) + 1e-30
    r2 = c["r2"]
    for b0 in range(0, len(P), block):
        Q = P[b0:b0 + block]
        lo = np.searchsorted(px, float(Q[0, 0]) - reach, "left"); hi = np.searchsorted(px, float(Q[-1, 0]) + reach, "right")
        C = P[lo:hi]
        d = C[None, :, :] - Q[:, None, :]                              # float32: d = p - q, rounded
        dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
        d2 = (dx * dx + dy * dy) + dz * dz                             # float32, every product and sum rounded
        m = d2 <= r2
        cnt = m.sum(axis=1)
        D = [np.where(m, d[..., k], F(0)).astype(np.float64) for k in range(3)]
        S1 = np.stack([D[k].sum(axis=1) for k in range(3)], axis=1)
        S2 = np.empty((len(Q), 3, 3))
        for i in range(3):
            for j in range(i, 3):
                S2[:, i, j] = S2[:, j, i] = (D[i] * D[j]).sum(axis=1)
        mean = S1 / cnt[:, None]
        Sigma = S2 / cnt[:, None, None] - mean[:, :, None] * mean[:, None, :]
        nn[order[b0:b0 + block]] = cnt
        lam[order[b0:b0 + block]] = np.linalg.eigvalsh(Sigma)
    return dict(nn=nn, lam=lam)


def np_values(mom, c):
    """-> (h float64, pv float64, nn int64): the values before the float32 store; NaN where the point is sparse or outside"""
    nn, lam = mom["nn"], mom["lam"]
    valid = nn >= c["min_neighbours"]
    with np.errstate(all="ignore"):
        fl = np.float64(c["lambda_floor"])
        h = 0.5 * (LOG_2PIE3 + np.log(np.maximum(lam, fl)).sum(axis=1))
        pv = np.maximum(lam[:, 0], 0.0)
    return np.where(valid, h, np.nan), np.where(valid, pv, np.nan), nn


def bounds(nn, c):
    """(bound on pv, bound on h) before the float32 store, per point: with u = 2^-53 every entry of Sigma carries at most
    4 (n + 8) u radius^2, an eigenvalue moves by at most three times that (Weyl) plus 64 u radius^2 for the Jacobi; h by at most 1.5
    times the eigenvalue bound over lambda_floor"""
    r2 = float(c["radius"]) ** 2
    e = 3.0 * 4.0 * (np.asarray(nn, np.float64) + 8.0) * U * r2 + 64.0 * U * r2
    return e, 1.5 * e / float(c["lambda_floor"])


def half_ulp32(v):
    return 0.5 * np.spacing(np.abs(np.asarray(v, np.float64)).astype(F)).astype(np.float64)


def np_rec(h32, pv32, nn, c):
    """the record of an op from stored values (float32 h and pv, unsaturated nn): counts, fsum sums, means"""
    nn = np.asarray(nn, np.int64)
    valid = nn >= c["min_neighbours"]
    sum_h = math.fsum(np.asarray(h32, np.float64)[valid]); sum_pv = math.fsum(np.asarray(pv32, np.float64)[valid])
    nv = int(valid.sum())
    return dict(n_points=len(nn), n_valid=nv, n_sparse=int(((nn > 0) & ~valid).sum()), n_outside=int((nn == 0).sum()), n_pairs=int(nn.sum()),
                sum_h=sum_h, sum_pv=sum_pv, mme=sum_h / nv if nv else 0.0, mpv=sum_pv / nv if nv else 0.0)


def np_op(frames, poses, c):
    """one op -> dict: h, pv (float32 as stored), nn, lam, sizes, rec (np_rec of those)"""
    w, sizes = np_cloud(frames, poses)
    mom = np_moments(w, c)
    h, pv, nn = np_values(mom, c)
    h32, pv32 = h.astype(F), pv.astype(F)
    return dict(w=w, h=h32, pv=pv32, h64=h, pv64=pv, nn=nn, lam=mom["lam"], sizes=sizes, rec=np_rec(h32, pv32, nn, c))


# ---------------------------------------------------------------------------------------------- crafted inputs
pts4 = vc.pts4


def one_frame(xyz):
    """a frame whose points go one in five to the corner cloud"""
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    corner = np.arange(len(xyz)) % 5 == 0
    return (pts4(xyz[corner]), pts4(xyz[~corner]))


def random_box(rng, n, side):
    return rng.uniform(-side / 2, side / 2, (n, 3))


def plane_cloud(rng, n, sigma, side=2.0):
    """a plane z = 0 of side x side metres with Gaussian thickness sigma"""
    p = rng.uniform(-side / 2, side / 2, (n, 3)); p[:, 2] = rng.normal(0.0, sigma, n)
    return p


def ball_cloud(rng, n, radius):
    v = rng.normal(size=(n, 3)); v /= np.linalg.norm(v, axis=1)[:, None]
    return v * (radius * rng.uniform(0, 1, n) ** (1 / 3))[:, None]


def ulp_steps(x, ks):
    """float32 x moved by k float32 steps, for k in ks"""
    b = int(F(x).view(np.int32))
    return [np.int32(b + k).view(F) for k in ks]


def edge_pairs(c):
    """a query at the origin and points at distance radius and a few float32 steps either side of it, along an axis and along the
    diagonal; 30 m away the same with the query at (30, 0, 0), where p - q rounds"""
    r = c["radius"]
    out = [[0, 0, 0]]
    out += [[d, 0, 0] for d in ulp_steps(r, (-1, 0, 1))] + [[0, -d, 0] for d in ulp_steps(r, (-1, 0, 1))] + [[0, 0, d] for d in ulp_steps(r, (-2, 0, 2))]
    a = F(float(r) / math.sqrt(3.0))
    out += [[-s, s, s] for s in ulp_steps(a, range(-4, 5))]
    far = [[30, 0, 0]] + [[F(30) + d, 0, 0] for d in ulp_steps(r, (-3, 0, 3))] + [[30, F(0) - d, 0] for d in ulp_steps(r, (-1, 0, 1))]
    return np.array(out + far, np.float64)


def face_points(c, ks=(-1, 0, 1, 2)):
    """points on cell faces and cell corners: per axis the coordinates k cell, one float32 step below and above it, and +-0.49 radius
    and +-0.98 radius away from it; every combination for the corner (k, k, k) -- 343 points a corner"""
    out = []
    for k in ks:
        base = F(k) * c["cell"]
        steps = [base - F(0.98) * c["radius"], base - F(0.49) * c["radius"]] + ulp_steps(base, (-1, 0, 1)) if k else \
                [-F(0.98) * c["radius"], -F(0.49) * c["radius"], F(-1e-45), F(0.0), F(1e-45)]
        steps = list(steps) + [base + F(0.49) * c["radius"], base + F(0.98) * c["radius"]]
        g = np.array(steps, np.float64)
        X, Y, Z = np.meshgrid(g, g, g, indexing="ij")
        out.append(np.stack([X.ravel(), Y.ravel(), Z.ravel()], axis=1))
    return np.concatenate(out)


def cell_clusters(c, sizes=(1, 63, 64, 65, 300), seed=5):
    """clusters of the given sizes, each inside its own cell (a 0.2 cell cube about the centre of cell (4 j, 7, -3)), four cells apart"""
    rng = np.random.default_rng(seed)
    cell = float(c["cell"])
    out = []
    for j, m in enumerate(sizes):
        centre = (np.array([4 * j, 7, -3]) + 0.5) * cell
        out.append(centre + rng.uniform(-0.1, 0.1, (m, 3)) * cell)
    return np.concatenate(out), list(sizes)


def range_edge(c):
    """points about the upper end of the key range on x (the first coordinate without a cell is 65536 cell): inside and outside, within
    a radius of each other; and the same at the lower end on z"""
    edge = float(F(HALF) * c["cell"])
    r = float(c["radius"])
    xs = [edge - 0.9 * r, edge - 0.5 * r, edge - 0.1 * r, edge - 0.01, edge + 0.01, edge + 0.2 * r]
    hi = [[x, y, 1.0] for x in xs for y in (0.0, 0.2 * r, -0.3 * r)]
    lo = [[3.0, y, -edge + dz] for dz in (-0.2 * r, -0.01, 0.01, 0.3 * r, 0.6 * r) for y in (0.0, 0.25 * r)]
    return np.array(hi + lo, np.float64)


BAD_POINTS = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [1e30, 0, 0], [0.1, -1e30, 0.1], [np.nan, np.nan, np.nan]], np.float64)


def min_edge_clusters(c, seed=9):
    """two isolated clusters: min_neighbours - 1 points (sparse) and min_neighbours points (valid), each within 0.2 radius"""
    rng = np.random.default_rng(seed)
    m = c["min_neighbours"]; r = float(c["radius"])
    a = np.array([50.0, 50.0, 5.0]) + rng.uniform(-0.1, 0.1, (m - 1, 3)) * r
    b = np.array([60.0, 50.0, 5.0]) + rng.uniform(-0.1, 0.1, (m, 3)) * r
    return np.concatenate([a, b])


def flat_and_line(n=40):
    """an exactly planar patch (z = 2 for every point, a grid of 0.05 m) and an exactly collinear run along y (x = 9, z = -1)"""
    g = np.arange(7) * 0.0625
    X, Y = np.meshgrid(g, g, indexing="ij")
    flat = np.stack([X.ravel(), Y.ravel(), np.full(X.size, 2.0)], axis=1)
    line = np.stack([np.full(n, 9.0), np.arange(n) * 0.03125, np.full(n, -1.0)], axis=1)
    return flat, line


def shift_pose(t):
    return np.concatenate([[0.0, 0.0, 0.0, 1.0], np.asarray(t, np.float64)])


# ---------------------------------------------------------------------------------------------- the street scene under drift
DRIFTS = (0.0, 0.5, 1.0)


def drift_poses(poses, d):
    """frame k gets a yaw of 0.4 k d degrees, 0.04 k d m sideways and 0.02 k d m upward"""
    out = []
    for k, P in enumerate(np.asarray(poses, np.float64)):
        q = vc.quat(np.radians(0.4 * k * d), 0.0, 0.0)
        out.append(np.concatenate([q, P[4:] + np.array([0.0, 0.04 * k * d, 0.02 * k * d])]))
    return np.array(out)


@functools.lru_cache(maxsize=None)
def street():
    """-> (frames, [poses under drift d for d in DRIFTS], [np_op of each]): computed once per process, never changed"""
    frames, poses, _ = vc.street_scene()
    c = cfg()
    P = [drift_poses(poses, d) for d in DRIFTS]
    return frames, P, [np_op(frames, p, c) for p in P]
