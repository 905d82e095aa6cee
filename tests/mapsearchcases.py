"""Crafted inputs for the MAPPING stage's five-nearest search and its line / plane fits, and an independent reference of both.

A plain helper module (not a conftest): test_map_search_cases.py checks the reference and the generators on the CPU,
test_gpu_map_search.py runs the same cases through Map.knn_partial, Map.associate and Map.associate_merged (ll_map_search.h under
k_map_knn, k_map_knn_partial and k_map_fit_merged).

The reference restates laserMapping.cpp:125-134 and :1822-2035, not oracle/ll_oracle.c:
  np_to_world     pointAssociateToMap in f64 in Eigen's operation order, stored as f32 (explicit numpy steps: nothing is contracted)
  np_search5      brute force over ALL map points, FLANN L2_Simple in f32 -- ((dx*dx + dy*dy) + dz*dz), every step f32 --, the five
                  smallest by (distance, index), or by (distance, gid[index]) for a tile shard
  np_fit_edge     f64 mean and covariance, numpy.linalg.eigh (LAPACK, not the cyclic Jacobi of the device and the oracle), line iff
                  w[2] > 3 * w[1]
  np_fit_plane    numpy.linalg.lstsq (SVD, not the pivoted Householder QR of the device and the oracle), valid iff all five points
                  are within 0.2 of the plane
  np_merge5       the five best by (distance, id) of the union of several parts' candidate lists
A block exists iff five neighbours exist, the fifth f32 distance is < 1.0f, and the fit says yes.

Decision bands.  The search and the 1 m gate are pure f32: indices and distances are exact, there is no band.  A fit whose margin
-- |w2 - 3 w1| / w2 for the line, min | |n.p + nd| - 0.2 | in metres for the plane -- is below MARGIN_MIN = 1e-9 could not be told
apart honestly; the generators are built so that NO case lands there (the CPU test asserts it), so the GPU test excludes nothing.
Where the covariance is exactly zero (five identical points: every centred coordinate is an exact 0.0) all eigenvalues are exact
zeros in any algorithm, the decision 0 > 3 * 0 is exact, and the margin is reported as infinite.

Untested on purpose: non-finite coordinates.  Every coordinate of every case is finite, and nothing here may be changed to send
NaN or Inf map or stack points to the device: ll_map_bbox_to_grid turns an infinite bounding box into undefined grid dimensions
on the host.  Exactly rank-deficient plane sets other than "all z == 0" (where the pivoted basic solution and the minimum-norm
solution coincide) are left out too: there numpy's minimum-norm answer is not Eigen's basic solution and no independent reference
exists.

`wrong` (a set of names) turns the reference into a deliberately wrong one -- only to show that the cases can see such an error:
  "tie_high" ties go to the HIGHEST index, "gate_le" d5 <= 1, "ratio_ge" w2 >= 3 w1, "residual_lt" all |r| < 0.2,
  "residual_no_abs" all r <= 0.2 (the fabs forgotten), "dist_f64" the distance summed in f64.
"""
import numpy as np

F32 = np.float32
INT_MAX = 2 ** 31 - 1
MARGIN_MIN = 1e-9
CELL = F32(1.01)                                        # ll_map_bbox_to_grid's first cell size
MAX_CELLS = 1 << 23                                     # ll_map_create's max_cells
KNNB = 64                                               # LL_KNNB
CMPB = 256                                              # LL_CMPB
IDENT = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])


def f4(xyz):
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    out = np.zeros((len(xyz), 4), np.float32)
    out[:, :3] = xyz.astype(np.float32)
    return out


EMPTY = np.zeros((0, 4), np.float32)


# ------------------------------------------------------------------------------------------------ the reference
def np_to_world(pose7, pts):
    """:125-134: q_w_curr * p + t_w_curr (Eigen _transformVector: uv = u x v; uv += uv; ((v + w*uv) + u x uv) + t) -> f32 (n, 3)"""
    p = np.asarray(pose7, np.float64)
    ux, uy, uz, w = p[0], p[1], p[2], p[3]
    v = np.ascontiguousarray(pts, np.float32).reshape(-1, 4)[:, :3].astype(np.float64)
    vx, vy, vz = v[:, 0], v[:, 1], v[:, 2]
    uvx = uy * vz - uz * vy; uvy = uz * vx - ux * vz; uvz = ux * vy - uy * vx
    uvx = uvx + uvx; uvy = uvy + uvy; uvz = uvz + uvz
    x = ((vx + w * uvx) + (uy * uvz - uz * uvy)) + p[4]
    y = ((vy + w * uvy) + (uz * uvx - ux * uvz)) + p[5]
    z = ((vz + w * uvz) + (ux * uvy - uy * uvx)) + p[6]
    return np.stack([x, y, z], axis=1).astype(np.float32)


def sq_dist(s, cloud, f64=False):
    """FLANN L2_Simple of every (query, map point) pair: ((dx*dx + dy*dy) + dz*dz), a = query, b = data, in f32 (or, wrongly, f64)"""
    t = np.float64 if f64 else np.float32
    s = np.ascontiguousarray(s, np.float32).astype(t); m = np.ascontiguousarray(cloud, np.float32)[:, :3].astype(t)
    d = s[:, None, 0] - m[None, :, 0]; out = d * d
    d = s[:, None, 1] - m[None, :, 1]; out = out + d * d
    d = s[:, None, 2] - m[None, :, 2]; out = out + d * d
    assert out.dtype == t
    return out


def np_search5(s, cloud, gid=None, wrong=()):
    """s (n, 3) f32 world-frame queries -> (pos int64 [n, 5], d [n, 5], nb [n]): the positions in `cloud` of the five nearest in
    ascending (distance, index) -- index = position, or gid[position] --, -1 / inf where the cloud has fewer than five points"""
    s = np.ascontiguousarray(s, np.float32).reshape(-1, 3)
    n, m = len(s), len(cloud)
    pos = np.full((n, 5), -1, np.int64); dd = np.full((n, 5), np.inf, np.float64 if "dist_f64" in wrong else np.float32)
    k = min(5, m)
    if n and m:
        d = sq_dist(s, cloud, "dist_f64" in wrong)
        key = np.arange(m, dtype=np.int64) if gid is None else np.asarray(gid, np.int64)
        if "tie_high" in wrong:
            key = -key
        order = np.lexsort((np.broadcast_to(key, (n, m)), d), axis=1)[:, :k]
        pos[:, :k] = order
        dd[:, :k] = np.take_along_axis(d, order, axis=1)
    return pos, dd, np.full(n, k, np.int64)


def np_fit_edge(P5, wrong=()):
    """:1886-1921 -> (line?, margin, a, b)"""
    P = np.asarray(P5, np.float64)
    c = np.zeros(3)
    for j in range(5):
        c = c + P[j]
    c = c / 5.0
    cov = np.zeros((3, 3))
    for j in range(5):
        z = P[j] - c
        cov = cov + np.outer(z, z)
    w, V = np.linalg.eigh(cov)
    ok = bool(w[2] >= 3 * w[1]) if "ratio_ge" in wrong else bool(w[2] > 3 * w[1])
    margin = np.inf if not cov.any() else float(abs(w[2] - 3 * w[1]) / w[2])
    return ok, margin, 0.1 * V[:, 2] + c, -0.1 * V[:, 2] + c


def np_fit_plane(P5, wrong=()):
    """:1954-2000 -> (valid?, margin in metres, unit normal, negative_OA_dot_norm, rank of the 5 x 3 system)"""
    P = np.asarray(P5, np.float64)
    x, _, rank, _ = np.linalg.lstsq(P, -np.ones(5), rcond=None)
    ln = np.sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2])
    nd = 1 / ln
    n = x / ln
    r = ((n[0] * P[:, 0] + n[1] * P[:, 1]) + n[2] * P[:, 2]) + nd
    if "residual_lt" in wrong:
        ok = bool((np.abs(r) < 0.2).all())
    elif "residual_no_abs" in wrong:
        ok = bool((r <= 0.2).all())
    else:
        ok = bool((np.abs(r) <= 0.2).all())
    return ok, float(np.abs(np.abs(r) - 0.2).min()), n, nd, int(rank)


def _gate(d5, wrong):
    """the fifth distance against 1: an f32 comparison (:1884, :1952)"""
    return d5 <= 1.0 if "gate_le" in wrong else d5 < 1.0


def _fit_all(pts5, nb, d5, wrong):
    """pts5 (2 types, each [n, 5, 3] f32 in neighbour order), nb, d5 per type -> the blocks and the extras"""
    e_src, e_a, e_b, p_src, p_n, p_d = [], [], [], [], [], []
    ok = [np.zeros(len(nb[0]), bool), np.zeros(len(nb[1]), bool)]; min_rank = 3
    margins = [np.full(len(nb[0]), np.inf), np.full(len(nb[1]), np.inf)]                   # per stack point; inf where nothing was fitted
    for i in np.flatnonzero((nb[0] == 5) & _gate(d5[0], wrong)):
        yes, mg, a, b = np_fit_edge(pts5[0][i], wrong)
        margins[0][i] = mg
        if yes:
            ok[0][i] = True; e_src.append(i); e_a.append(a); e_b.append(b)
    for i in np.flatnonzero((nb[1] == 5) & _gate(d5[1], wrong)):
        yes, mg, n, nd, rank = np_fit_plane(pts5[1][i], wrong)
        margins[1][i] = mg; min_rank = min(min_rank, rank)
        if yes:
            ok[1][i] = True; p_src.append(i); p_n.append(n); p_d.append(nd)
    extra = dict(margin_edge=float(margins[0].min(initial=np.inf)), margin_plane=float(margins[1].min(initial=np.inf)),
                 margins_corner=margins[0], margins_surf=margins[1], ok_corner=ok[0], ok_surf=ok[1], min_rank=min_rank)
    return (np.array(e_src, np.int32), np.array(e_a, np.float64).reshape(-1, 3), np.array(e_b, np.float64).reshape(-1, 3),
            np.array(p_src, np.int32), np.array(p_n, np.float64).reshape(-1, 3), np.array(p_d, np.float64), extra)


def np_map_associate(pose7, corner_stack, corner_map, surf_stack, surf_map, gid_c=None, gid_s=None, wrong=()):
    """one association pass (:1877-2047) -> orc.map_associate's (e_src, e_a, e_b, p_src, p_n, p_d) in stack order, and a dict with
    the smallest fit margin per cloud type (margin_edge, margin_plane), the per-stack-point flags (ok_corner, ok_surf), the
    neighbours (pos_*, d_*) and the smallest rank seen in a plane system (min_rank)"""
    pts5, nbs, d5s, found = [], [], [], {}
    for tag, stack, cloud, gid in (("corner", corner_stack, corner_map, gid_c), ("surf", surf_stack, surf_map, gid_s)):
        cloud = np.ascontiguousarray(cloud, np.float32).reshape(-1, 4)
        pos, d, nb = np_search5(np_to_world(pose7, stack), cloud, gid, wrong)
        found["pos_" + tag] = pos; found["d_" + tag] = d
        pts5.append(cloud[np.maximum(pos, 0), :3] if len(cloud) else np.zeros((len(pos), 5, 3), np.float32))
        nbs.append(nb); d5s.append(d[:, 4])
    out = _fit_all(pts5, nbs, d5s, wrong)
    out[6].update(found)
    return out


def np_merge5(nn, ids):
    """nn [parts, n, 5, 4] f32 (x, y, z, d), ids [parts, n, 5] (INT_MAX = padding) -> (pts [n, 5, 3] f32, d [n, 5] f32, id [n, 5], nb [n]):
    per stack point the five best of all parts by (distance, id)"""
    nn = np.ascontiguousarray(nn, np.float32); ids = np.ascontiguousarray(ids, np.int32)
    parts, n = ids.shape[:2]
    a = np.moveaxis(nn, 0, 1).reshape(n, parts * 5, 4); b = np.moveaxis(ids, 0, 1).reshape(n, parts * 5).astype(np.int64)
    d = np.where(b == INT_MAX, F32(np.inf), a[:, :, 3])
    order = np.lexsort((b, d), axis=1)[:, :5]
    nb = np.minimum(5, (b != INT_MAX).sum(axis=1))
    pts = np.take_along_axis(a[:, :, :3], order[:, :, None], axis=1)
    return pts, np.take_along_axis(d, order, axis=1), np.take_along_axis(b, order, axis=1), nb


def np_merge_associate(cn, ci, sn, si, wrong=()):
    """Map.associate_merged: np_merge5 per cloud type, the gate, the fits -> as np_map_associate"""
    pts5, nbs, d5s = [], [], []
    for nn, ids in ((cn, ci), (sn, si)):
        pts, d, _, nb = np_merge5(nn, ids)
        pts5.append(pts); nbs.append(nb); d5s.append(d[:, 4])
    return _fit_all(pts5, nbs, d5s, wrong)


# ------------------------------------------------------------------------------------------------ small tools
def rotation(rng):
    q = rng.standard_normal(4); q /= np.linalg.norm(q)
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def small_pose():
    """a small rotation plus a translation"""
    q = np.array([0.01, -0.02, 0.015, 1.0]); q /= np.linalg.norm(q)
    return np.concatenate([q, [0.3, -0.2, 0.05]])


def to_lidar(pose7, world):
    """stack points whose pointAssociateToMap lands near `world` (f64 inverse, rounded to f32 by f4)"""
    x, y, z, w = pose7[:4]
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    return (np.asarray(world, np.float64) - pose7[4:]) @ R


def grid_dims(cloud, cell=CELL):
    """ll_map_bbox_to_grid's dimensions for one cell size (f32 arithmetic)"""
    c = np.ascontiguousarray(cloud, np.float32)[:, :3]
    mn, mx = c.min(axis=0), c.max(axis=0)
    return (np.floor((mx - mn) / F32(cell)).astype(np.int64) + 1), mn


def cell_of(cloud, pts, cell=CELL):
    dims, mn = grid_dims(cloud, cell)
    c = np.floor((np.ascontiguousarray(pts, np.float32)[:, :3] - mn) / F32(cell)).astype(np.int64)
    return np.clip(c, 0, dims - 1)


def case(family, pose, cs, cm, ss, sm, gid_c=None, gid_s=None):
    return dict(family=family, pose=np.asarray(pose, np.float64), cs=f4(np.asarray(cs)[:, :3]) if len(cs) else EMPTY,
                cm=f4(np.asarray(cm)[:, :3]) if len(cm) else EMPTY, ss=f4(np.asarray(ss)[:, :3]) if len(ss) else EMPTY,
                sm=f4(np.asarray(sm)[:, :3]) if len(sm) else EMPTY, gid_c=gid_c, gid_s=gid_s)


# ------------------------------------------------------------------------------------------------ search families
LATTICE_ORG = np.array([10.0, 5.0, 2.0])                 # away from the origin: no lattice plane of a five-set passes through it
LATTICE_DIM = (12, 10, 8)


def lattice():
    i, j, k = np.meshgrid(*[np.arange(n) for n in LATTICE_DIM], indexing="ij")
    return LATTICE_ORG + 0.25 * np.stack([i.ravel(), j.ravel(), k.ravel()], axis=1)


def tie_cases():
    """map and queries on a 0.25 m lattice (queries on lattice points, edge mid-points, face and cube centres: 1, 2, 4 or 8 nearest
    points exactly tied): identity pose, a small pose, and identity with a random permutation as gids"""
    rng = np.random.default_rng(41)
    m = lattice(); rng.shuffle(m)                           # position in the cloud is unrelated to position in space
    hi = np.array(LATTICE_DIM) * 2 - 1
    q = LATTICE_ORG + 0.125 * np.stack([rng.integers(0, hi[a], 800) for a in range(3)], axis=1)
    p = small_pose()
    gid_c = rng.permutation(len(m)).astype(np.int32); gid_s = rng.permutation(len(m)).astype(np.int32)

    def clear_of_the_band(pose, gc, gs):
        # lattice five-sets can have an eigenvalue ratio of exactly 3 (or a residual of exactly 0.2): such queries are left out,
        # decided on the reference alone, and 320 of the rest are kept per cloud type
        c = case("ties", pose, to_lidar(pose, q[:400]), m, to_lidar(pose, q[400:]), m, gc, gs)
        x = np_map_associate(c["pose"], c["cs"], c["cm"], c["ss"], c["sm"], gc, gs)[6]
        y = np_map_associate(c["pose"], c["cs"], c["cm"], c["ss"], c["sm"])[6]              # Map.associate orders by position whatever the gids
        c["cs"] = c["cs"][np.minimum(x["margins_corner"], y["margins_corner"]) > 1e-6][:320]
        c["ss"] = c["ss"][np.minimum(x["margins_surf"], y["margins_surf"]) > 1e-6][:320]
        assert len(c["cs"]) == 320 and len(c["ss"]) == 320
        return c
    return {"ties-identity": clear_of_the_band(IDENT, None, None), "ties-pose": clear_of_the_band(p, None, None),
            "ties-gid": clear_of_the_band(IDENT, gid_c, gid_s)}


def _blob(rng, n, centre, extent):
    return np.asarray(centre, np.float64) + rng.uniform(-0.5, 0.5, (n, 3)) * extent


def _around(rng, n, cloud, spread=0.4):
    """n queries near randomly chosen points of the cloud"""
    c = np.asarray(cloud, np.float64)[:, :3]
    return c[rng.integers(0, len(c), n)] + rng.uniform(-spread, spread, (n, 3))


def grid_cases():
    rng = np.random.default_rng(42)
    out = {}
    m = _blob(rng, 200, [10.4, 5.4, 2.4], 0.9)                                           # extent < 1 m: one cell
    out["grid-one-cell"] = case("grid", IDENT, _around(rng, 90, m), m, _around(rng, 90, m), m)
    for ax, name in enumerate(("x", "y", "z")):                                          # all of one coordinate equal: dim == 1 there
        m = _blob(rng, 900, [12.0, 7.0, 4.0], 5.0); m[:, ax] = (3.5, 2.5, 2.0)[ax]
        q = _around(rng, 120, m, 0.3)
        out[f"grid-flat-{name}"] = case("grid", IDENT, q[:60], m, q[60:], m)
    m = _blob(rng, 1600, [30.0, 5.45, 2.45], [40.3, 0.9, 0.9])                           # 1 cell thick, 40 cells long
    out["grid-thin-long"] = case("grid", IDENT, _around(rng, 100, m, 0.3), m, _around(rng, 100, m, 0.3), m)
    far = np.array([[6.0, 2.0, 1.0], [14.0, 9.0, 4.0]])                                  # two lone points stretch the box: empty cells
    for n in (300, 301):                                                                 # even and odd row length in the two-per-round loop
        m = np.concatenate([_blob(rng, n, [10.5, 5.5, 2.5], 0.45), far])
        q = np.concatenate([_around(rng, 70, m[:n], 0.5), _around(rng, 10, far, 0.3)])
        out[f"grid-dense-{n}"] = case("grid", IDENT, q[:40], m, q[40:], m)
    a = _blob(rng, 400, [1.0, 1.0, 1.0], 1.6); b = _blob(rng, 400, [401.0, 351.0, 121.0], 1.6)
    m = np.concatenate([a, b]); rng.shuffle(m)
    out["grid-two-clusters"] = case("grid", IDENT, _around(rng, 80, m, 0.3), m, _around(rng, 80, m, 0.3), m)
    return out


def mapsize_cases():
    """maps of 0, 1, 4, 5 and 6 points: fewer than five neighbours, exactly five, one spare"""
    rng = np.random.default_rng(43)
    out = {}
    for n in (0, 1, 4, 5, 6):
        line = np.array([10.0, 5.0, 2.0]) + np.outer(rng.uniform(-0.4, 0.4, n), [1.0, 0.2, 0.1]) + rng.normal(0, 0.004, (n, 3))
        plane = np.array([10.0, 5.0, 2.0]) + rng.uniform(-0.3, 0.3, (n, 3)) * [1.0, 1.0, 0.01]
        qc = np.array([10.0, 5.0, 2.0]) + rng.uniform(-0.2, 0.2, (7, 3)); qs = np.array([10.0, 5.0, 2.0]) + rng.uniform(-0.2, 0.2, (7, 3))
        out[f"mapsize-{n}"] = case("mapsize", IDENT, qc, line, qs, plane)
    return out


def _box_map(rng):
    return np.array([10.0, 5.0, 2.0]) + rng.uniform(0, 1, (2400, 3)) * [6.0, 5.0, 3.0]


def box_cases():
    rng = np.random.default_rng(44)
    m = f4(_box_map(rng))[:, :3]
    mn, mx = m.min(axis=0), m.max(axis=0)
    out = {}
    q = []
    for ax in range(3):                                                                  # outside each of the six faces by 0.5 m and 3 m
        for side, edge in ((-1, mn), (1, mx)):
            for by in (0.5, 3.0):
                near =np.argsort(np.abs(m[:, ax] - edge[ax]))[:12]                      # beside map points that lie close to that face
                p = m[near].astype(np.float64) + rng.uniform(-0.1, 0.1, (12, 3))
                p[:, ax] = edge[ax] + side * by
                q.append(p)
    q = np.concatenate(q); rng.shuffle(q)
    out["box-outside"] = case("box", IDENT, q[:72], m, q[72:], m)
    corners = np.array([[(mn, mx)[b][a] for a, b in enumerate(bits)] for bits in np.ndindex(2, 2, 2)], np.float64)
    out["box-corners"] = case("box", IDENT, corners, m, corners[::-1], m)
    q = []
    for ax in range(3):                                                                  # org + k * cell -/+ 1 ulp, f32 arithmetic as on the device
        for k in range(1, int(grid_dims(m)[0][ax])):
            edge = F32(mn[ax] + F32(F32(k) * CELL))
            for v in (np.nextafter(edge, F32(-np.inf)), edge, np.nextafter(edge, F32(np.inf))):
                p = m[rng.integers(0, len(m), 4)].astype(np.float64) + rng.uniform(-0.2, 0.2, (4, 3))
                p[:, ax] = v
                q.append(p)
    q = np.concatenate(q); rng.shuffle(q)
    h = len(q) // 2
    out["box-cell-boundary"] = case("box", IDENT, q[:h], m, q[h:], m)
    return out


ULP_BELOW_ONE = float(np.nextafter(F32(1), F32(0)))      # 1 - 2^-24
ULP_ABOVE_ONE = float(np.nextafter(F32(1), F32(2)))      # 1 + 2^-23
GATE_R = (ULP_BELOW_ONE, 1.0, ULP_ABOVE_ONE)


def _gate_layout(anchor, pairs):
    """canonical coordinates (u = the gate's axis, v, w): one cluster per (query u, sign, r) at v = 4 * cluster, w = 4: the query, four
    close neighbours on the side of the fifth, the fifth at u + sign * r -- every value and every difference exact in f32.  The
    corner clusters are collinear (a line), the surf clusters lie in the plane w = 4 (not through the origin).  A lone anchor point
    fixes the grid's origin along u.  -> (queries_c, map_c, queries_s, map_s, expect) with expect[cluster] = the f32 distance < 1"""
    qc, mc, qs, ms, expect = [], [anchor], [], [anchor], []
    k = 0
    for u, sign in pairs:
        for r in GATE_R:
            v = 4.0 * k; k += 1
            fifth = u + sign * r
            assert float(F32(fifth)) == fifth and float(F32(F32(u) - F32(fifth))) == -sign * r
            qc.append([u, v, 4.0]); qs.append([u, v, 4.0])
            mc += [[u + sign * s, v, 4.0] for s in (0.0, 0.0625, 0.125, 0.1875)] + [[fifth, v, 4.0]]
            ms += [[u + sign * s, v + t, 4.0] for s in (0.0, 0.0625) for t in (-0.125, 0.125)] + [[fifth, v, 4.0]]
            expect.append(r < 1.0)
    return np.array(qc), np.array(mc), np.array(qs), np.array(ms), np.array(expect)


def _rounding_points(rng):
    """offsets (on a 2^-20 lattice, so that the sum with a query below 8 is exact) whose f32 distance and exact distance fall on
    different sides of 1: [f32 == 1.0 and exact < 1, f32 < 1.0 and exact >= 1]"""
    found = {}
    for _ in range(50):
        if len(found) == 2:
            break
        v = rng.standard_normal((20000, 3)); v /= np.linalg.norm(v, axis=1)[:, None]
        v = np.round(v * 2 ** 20) / 2 ** 20
        d32 = sq_dist(np.zeros((1, 3), np.float32), f4(v))[0]; d64 = (v * v).sum(axis=1)
        for key, hit in (("round_up", (d32 == F32(1)) & (d64 < 1.0)), ("round_down", (d32 < F32(1)) & (d64 >= 1.0))):
            if key not in found and hit.any():
                found[key] = v[np.flatnonzero(hit)[0]]
    return found["round_up"], found["round_down"]


def gate_cases():
    """the 1 m gate, per axis: `same` -- the fifth in the query's cell (cells [-0.505, 0.505)), `adjacent` -- in the next cell in
    either direction (cells [-0.9, 0.11), [0.11, 1.12)); `rounding` -- corner clusters whose fifth is off-axis so that the f32 sum
    and the exact sum disagree about < 1"""
    out = {}
    layouts = {"same": (-0.505, ((-0.5, 1.0), (0.5, -1.0))), "adjacent": (-0.9, ((-0.25, 1.0), (0.25, -1.0)))}
    for ax, name in enumerate(("x", "y", "z")):
        perm = [(0, 1, 2), (2, 0, 1), (1, 2, 0)][ax]                                     # canonical (u, v, w) -> the axis under test gets u
        for kind, (org, pairs) in layouts.items():
            qc, mc, qs, ms, expect = _gate_layout([org, -8.0, 4.0], pairs)
            c = case("gate", IDENT, qc[:, perm], mc[:, perm], qs[:, perm], ms[:, perm])
            c["expect"] = expect; c["axis"] = ax; c["kind"] = kind
            out[f"gate-{name}-{kind}"] = c
    up, down = _rounding_points(np.random.default_rng(45))
    qc, mc, expect = [], [], []
    for k, (off, exp) in enumerate(((up, False), (down, True))):
        base = np.array([0.25, 4.0 * k, 4.0])
        qc.append(base); expect.append(exp)
        mc += [base + off * s for s in (0.0, 0.0625, 0.125, 0.1875)] + [base + off]
    c = case("gate", IDENT, np.array(qc), np.array(mc), EMPTY, EMPTY)
    c["expect"] = np.array(expect); c["kind"] = "rounding"
    out["gate-rounding"] = c
    return out


STACK_SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 1025)     # around LL_KNNB = 64 and LL_CMPB = 256


def _runs(rng, n):
    """valid / invalid flags in irregular runs of 1..7"""
    flags = np.zeros(n, bool); at = 0; v = bool(rng.integers(0, 2))
    while at < n:
        ln = int(rng.integers(1, 8)); flags[at:at + ln] = v; at += ln; v = not v
    return flags


def stack_cases():
    """corner stack of STACK_SIZES[k] points beside a surf stack of STACK_SIZES[-1 - k]: every size for both types, and one type
    empty while the other is not.  Valid points sit on the map's lines / plane, invalid ones 5 m above it."""
    rng = np.random.default_rng(46)
    lines = np.concatenate([np.stack([10.0 + 0.1 * np.arange(60), np.full(60, 5.0 + 1.5 * k), np.full(60, 2.0)], axis=1) for k in range(8)])
    lines = lines + rng.normal(0, 0.004, lines.shape)
    i, j = np.meshgrid(np.arange(40), np.arange(40), indexing="ij")
    plane = np.stack([10.0 + 0.2 * i.ravel(), 5.0 + 0.2 * j.ravel(), np.full(1600, 3.0)], axis=1) + rng.normal(0, 0.01, (1600, 3))
    out = {}
    for k, nc in enumerate(STACK_SIZES):
        ns = STACK_SIZES[-1 - k]
        qc = lines[rng.integers(0, len(lines), nc)] + rng.normal(0, 0.03, (nc, 3))
        qs = plane[rng.integers(0, len(plane), ns)] + rng.normal(0, 0.03, (ns, 3))
        qc[~_runs(rng, nc), 2] += 5.0; qs[~_runs(rng, ns), 2] += 5.0
        out[f"stack-{nc}-{ns}"] = case("stack", small_pose(), to_lidar(small_pose(), qc), lines, to_lidar(small_pose(), qs), plane)
    return out


# ------------------------------------------------------------------------------------------------ fit families
DELTAS = (-1e-2, -1e-4, -1e-6, 1e-6, 1e-4, 1e-2)
PLACEMENTS = (0.0, 50.0, 1000.0)                          # |c| of a five-point set: at the origin un-rotated, rotated and moved


def _centres(rng, n, radius):
    """n set centres: `radius` from the origin, on a 4 m grid there (each set in a cell of its own, far from the others)"""
    d = np.array([0.6, -0.64, 0.48])
    side = int(np.ceil(np.sqrt(n)))
    g = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), axis=-1).reshape(-1, 2)[:n]
    return radius * d + np.concatenate([4.0 * g, np.zeros((n, 1))], axis=1)


def ratio_ladder(rng, radius, per_delta):
    """(+-a, 0, 0), (0, +-b, 0), (0, 0, 0) with a = b * sqrt(3 (1 + delta)): the exact eigenvalue ratio is a^2 / b^2 = 3 (1 + delta).
    radius 0: every set at the origin, un-rotated; otherwise rotated at random and moved to a centre of its own"""
    n = per_delta * len(DELTAS)
    cen = _centres(rng, n, radius) if radius else np.zeros((n, 3))
    sets = np.zeros((n, 5, 3))
    for i in range(n):
        b = rng.uniform(0.2, 0.45); a = b * np.sqrt(3 * (1 + DELTAS[i % len(DELTAS)]))
        p = np.array([[0, 0, 0], [a, 0, 0], [-a, 0, 0], [0, b, 0], [0, -b, 0.0]])
        while True:                                                                      # the rounded set decides; none may land in the band
            R = rotation(rng) if radius else np.eye(3)
            sets[i] = (p @ R.T + cen[i]).astype(np.float32)
            if np_fit_edge(sets[i])[1] > 1e-8:
                break
            p = p * (1 + 1e-3)
    return sets.astype(np.float32), cen


def eigen_degenerate(rng, radius, n_each):
    """exact lines (a block), isotropic blobs, two equal largest eigenvalues, five identical points (no block)"""
    n = 4 * n_each
    cen = _centres(rng, n, radius)
    sets = np.zeros((n, 5, 3), np.float32)
    for i in range(n):
        kind = i % 4
        c = np.round(cen[i] * 8) / 8                                                     # exactly representable centres and offsets
        if kind == 0:
            direction = np.array([[1, 0, 0], [0, 1, 0], [1, 1, 0], [1, -2, 1.0]])[(i // 4) % 4]
            sets[i] = c + np.outer(np.array([0, 1, -1, 2, -2]) * 0.0625, direction)      # an exact line: w1 = w0 = 0
        elif kind == 1:
            ang = 2 * np.pi * np.arange(3) / 3                                           # a triangular bipyramid: eigenvalues 0.135, 0.135, 0.125
            blob = np.concatenate([0.3 * np.stack([np.cos(ang), np.sin(ang), 0 * ang], axis=1), [[0, 0, 0.25], [0, 0, -0.25]]])
            sets[i] = c + blob @ rotation(rng).T + rng.uniform(-0.02, 0.02, (5, 3))
        elif kind == 2:
            s = 0.25
            sets[i] = c + np.array([[0, 0, 0], [s, 0, 0], [-s, 0, 0], [0, s, 0], [0, -s, 0]])   # w2 == w1 exactly
        else:
            sets[i] = np.tile(c, (5, 1))                                                 # zero covariance
    return sets, cen


def plane_sets(rng, offsets, per_offset, in_plane=0.35):
    """five points around the foot of a plane at distance |d| from the origin: random and axis-aligned normals, out-of-plane noise
    0 .. 0.05 m -> (sets, centres)"""
    sets, cen = [], []
    for d in offsets:
        for i in range(per_offset):
            if i % 4 == 0:
                n = np.zeros(3); n[(i // 4) % 3] = 1.0 if (i // 12) % 2 == 0 else -1.0
            else:
                n = rng.standard_normal(3); n /= np.linalg.norm(n)
            u = np.cross(n, [0.3, 0.5, 0.8]); u /= np.linalg.norm(u); v = np.cross(n, u)
            st = rng.uniform(-in_plane, in_plane, (5, 2))
            noise = rng.uniform(0, 0.05) * rng.uniform(-1, 1, 5) * (i % 3 != 0)          # every third set is exactly planar before rounding
            sets.append(d * n + st[:, :1] * u + st[:, 1:] * v + noise[:, None] * n); cen.append(d * n)
    return np.array(sets).astype(np.float32), np.array(cen)


def _max_residual(P):
    x = np.linalg.lstsq(P, -np.ones(5), rcond=None)[0]
    ln = np.linalg.norm(x)
    return float(np.abs(P @ (x / ln) + 1 / ln).max())


def residual_ladder(rng, per_delta):
    """four points on a plane and the fifth lifted by h (to either side), h bisected in f64 on the reference so that the largest
    residual is 0.2 (1 + delta)"""
    sets, cen = [], []
    for i in range(per_delta * len(DELTAS)):
        want = 0.2 * (1 + DELTAS[i % len(DELTAS)])
        d = rng.uniform(2.0, 12.0)
        n = rng.standard_normal(3); n /= np.linalg.norm(n)
        u = np.cross(n, [0.3, 0.5, 0.8]); u /= np.linalg.norm(u); v = np.cross(n, u)
        st = np.array([[0.3, 0.3], [-0.3, 0.3], [-0.3, -0.3], [0.3, -0.3], [0.0, 0.0]]) + rng.uniform(-0.08, 0.08, (5, 2))
        base = d * n + st[:, :1] * u + st[:, 1:] * v
        sign = 1.0 if (i // len(DELTAS)) % 2 == 0 else -1.0

        def lifted(h):
            p = base.copy(); p[4] += sign * h * n
            return p
        lo, hi = 0.0, 0.6
        assert _max_residual(lifted(hi)) > want
        for _ in range(80):
            mid = 0.5 * (lo + hi)
            if _max_residual(lifted(mid)) < want:
                lo = mid
            else:
                hi = mid
        got = lifted(hi).astype(np.float32)
        k = 0
        while np_fit_plane(got)[1] <= 1e-8:                                              # the rounded set decides; none may land in the band
            k += 1; got = lifted(hi * (1 + k * 1e-7)).astype(np.float32)
        sets.append(got); cen.append(d * n)
    return np.array(sets), np.array(cen)


def plane_degenerate(rng, n):
    """all z exactly 0: an exact zero column, rank 2 -- the pivoted basic solution and the minimum-norm solution coincide"""
    sets = np.zeros((n, 5, 3), np.float32)
    for i in range(n):
        c = rng.uniform(2.0, 9.0, 2) * rng.choice([-1.0, 1.0], 2)
        sets[i, :, :2] = c + rng.uniform(-0.4, 0.4, (5, 2)) * ([1.0, 0.05] if i % 2 else [1.0, 1.0])
    return sets, None


def merged_from_sets(sets):
    """each five-point set as one part's candidates of one stack point: distances 0.1 .. 0.5 (all below 1), ids 5 i + j"""
    n = len(sets)
    nn = np.zeros((1, n, 5, 4), np.float32); nn[0, :, :, :3] = sets
    nn[0, :, :, 3] = np.array([0.1, 0.2, 0.3, 0.4, 0.5], np.float32)
    ids = (5 * np.arange(n)[:, None] + np.arange(5)[None, :]).astype(np.int32)[None]
    return nn, ids


def merged_case(family, corner_sets, surf_sets):
    z = np.zeros((0, 5, 3), np.float32)
    cn, ci = merged_from_sets(corner_sets if corner_sets is not None else z)
    sn, si = merged_from_sets(surf_sets if surf_sets is not None else z)
    return dict(family=family, cn=cn, ci=ci, sn=sn, si=si)


def placed_case(family, corner_sets, corner_cen, surf_sets, surf_cen):
    """the sets as a map, one query per set at its centre (identity pose: the world point is the stack point)"""
    e = np.zeros((0, 3))
    return case(family, IDENT, corner_cen if corner_sets is not None else e, corner_sets.reshape(-1, 3) if corner_sets is not None else e,
                surf_cen if surf_sets is not None else e, surf_sets.reshape(-1, 3) if surf_sets is not None else e)


PLANE_OFFSETS = (0.05, 1.0, 10.0, 100.0, 1000.0)


def fit_cases():
    """-> (merged cases: name -> dict(cn, ci, sn, si), placed cases: name -> case)"""
    rng = np.random.default_rng(47)
    merged, placed = {}, {}
    for radius in PLACEMENTS:
        sets, cen = ratio_ladder(rng, radius, 60)
        merged[f"fit-ratio-{int(radius)}"] = merged_case("ratio", sets, None)
        if radius:
            placed[f"fit-ratio-map-{int(radius)}"] = placed_case("ratio", sets[:96], cen[:96], None, None)
    sets, cen = eigen_degenerate(rng, 50.0, 24)
    merged["fit-eigen-degenerate"] = merged_case("eigen-degenerate", sets, None)
    placed["fit-eigen-degenerate-map"] = placed_case("eigen-degenerate", sets, np.round(cen * 8) / 8, None, None)
    sets, cen = plane_sets(rng, PLANE_OFFSETS, 200)
    merged["fit-plane"] = merged_case("plane", None, sets)
    near, ncen = plane_sets(rng, (10.0, 100.0), 40, in_plane=0.25)
    placed["fit-plane-map"] = placed_case("plane", None, None, near, ncen)
    sets, cen = residual_ladder(rng, 80)
    merged["fit-residual"] = merged_case("residual", None, sets)
    placed["fit-residual-map"] = placed_case("residual", None, None, sets[:120], sets[:120, :4].mean(axis=1, dtype=np.float64))
    sets, _ = plane_degenerate(rng, 60)
    merged["fit-plane-z0"] = merged_case("plane-degenerate", None, sets)
    return merged, placed


def merge_cases():
    """the candidate merge itself: name -> dict(cn, ci, sn, si), three parts"""
    rng = np.random.default_rng(48)
    n = 70
    pad_pt = np.array([0, 0, 0, np.inf], np.float32)

    def build(fill, surf):
        nn = np.tile(pad_pt, (3, n, 5, 1)); ids = np.full((3, n, 5), INT_MAX, np.int32)
        for i in range(n):
            base = np.array([10.0, 5.0, 2.0]) + 4.0 * np.array([i % 8, i // 8, 0])
            for part, cand in enumerate(fill(i)):                                        # cand: [(distance, id)], ascending by (distance, id)
                for j, (d, gid) in enumerate(sorted(cand)[:5]):
                    g = np.random.default_rng(gid)                                       # a candidate's point is a function of its id
                    off = g.uniform(-0.4, 0.4, 3) * [1.0, 1.0, 0.02] if surf else g.uniform(-0.4, 0.4) * np.array([1.0, 0.3, 0.1]) + g.normal(0, 0.01, 3)
                    nn[part, i, j, :3] = (base + off).astype(np.float32)
                    nn[part, i, j, 3] = F32(d); ids[part, i, j] = gid
        return nn, ids

    q = lambda k: float(F32(0.0625 * k))                                                 # distances on a coarse lattice: many exact ties

    def equal_across_parts(i):                                                            # equal distances under different ids across parts
        ids3 = rng.permutation(15) + 100 * i
        return [[(q(1 + (j // 2)), int(ids3[5 * part + j])) for j in range(5)] for part in range(3)]

    def short_parts(i):                                                                   # two candidates then padding, a part with none
        ids3 = rng.permutation(9) + 100 * i
        return [[(q(rng.integers(1, 6)), int(ids3[j])) for j in range(2)], [], [(q(rng.integers(1, 6)), int(ids3[2 + j])) for j in range(1 + i % 5)]]

    def all_empty(i):
        return [[], [], []]

    def more_than_five(i):                                                                # 15 candidates below 1: only the best five count
        ids3 = rng.permutation(15) + 100 * i
        return [[(float(F32(rng.uniform(0.05, 0.95))), int(ids3[5 * part + j])) for j in range(5)] for part in range(3)]

    def around_the_gate(i):                                                               # the merged fifth at 1 - ulp, 1, 1 + ulp
        ids3 = rng.permutation(15) + 100 * i
        fifth = GATE_R[i % 3]
        c = [[(q(1), int(ids3[0])), (q(2), int(ids3[1]))], [(q(3), int(ids3[5])), (fifth, int(ids3[6])), (2.0, int(ids3[7]))], [(q(4), int(ids3[10])), (1.5, int(ids3[11]))]]
        return c

    out = {}
    for name, fill in (("merge-equal-distances", equal_across_parts), ("merge-short-parts", short_parts), ("merge-all-empty", all_empty),
                       ("merge-more-than-five", more_than_five), ("merge-gate", around_the_gate)):
        cn, ci = build(fill, False); sn, si = build(fill, True)
        out[name] = dict(family="merge", cn=cn, ci=ci, sn=sn, si=si)
    return out


# ------------------------------------------------------------------------------------------------ the registry
TIE_NAMES = ("ties-identity", "ties-pose", "ties-gid")
GRID_NAMES = ("grid-one-cell", "grid-flat-x", "grid-flat-y", "grid-flat-z", "grid-thin-long", "grid-dense-300", "grid-dense-301", "grid-two-clusters")
MAPSIZE_NAMES = tuple(f"mapsize-{n}" for n in (0, 1, 4, 5, 6))
BOX_NAMES = ("box-outside", "box-corners", "box-cell-boundary")
GATE_NAMES = tuple(f"gate-{a}-{k}" for a in "xyz" for k in ("same", "adjacent")) + ("gate-rounding",)
STACK_NAMES = tuple(f"stack-{n}-{STACK_SIZES[-1 - k]}" for k, n in enumerate(STACK_SIZES))
SEARCH_NAMES = TIE_NAMES + GRID_NAMES + MAPSIZE_NAMES + BOX_NAMES + GATE_NAMES + STACK_NAMES
PLACED_NAMES = ("fit-ratio-map-50", "fit-ratio-map-1000", "fit-eigen-degenerate-map", "fit-plane-map", "fit-residual-map")
MAP_NAMES = SEARCH_NAMES + PLACED_NAMES                  # cases with maps and stacks: knn_partial, associate
FIT_NAMES = ("fit-ratio-0", "fit-ratio-50", "fit-ratio-1000", "fit-eigen-degenerate", "fit-plane", "fit-residual", "fit-plane-z0")
MERGE_NAMES = ("merge-equal-distances", "merge-short-parts", "merge-all-empty", "merge-more-than-five", "merge-gate")
MERGED_NAMES = FIT_NAMES + MERGE_NAMES                   # cases of candidate lists: associate_merged          (for parametrize: builds nothing)

_MAP = None
_MERGED = None
_REF = {}


def _build():
    global _MAP, _MERGED
    if _MAP is None:
        c = {}
        for f in (tie_cases, grid_cases, mapsize_cases, box_cases, gate_cases, stack_cases):
            c.update(f())
        merged, placed = fit_cases()
        c.update(placed); merged.update(merge_cases())
        assert tuple(c) == MAP_NAMES and tuple(merged) == MERGED_NAMES, (tuple(c), tuple(merged))
        for v in c.values():
            for k in ("cs", "cm", "ss", "sm"):
                assert np.isfinite(v[k]).all()
        for v in merged.values():
            for nn, ids in ((v["cn"], v["ci"]), (v["sn"], v["si"])):
                assert np.isfinite(nn[ids != INT_MAX]).all() and np.isfinite(nn[..., :3]).all()
        _MAP, _MERGED = c, merged


def map_cases():
    """name -> dict(family, pose, cs, cm, ss, sm, gid_c, gid_s): every family with maps and stacks, built once on first use"""
    _build()
    return _MAP


def merged_cases():
    """name -> dict(family, cn, ci, sn, si): every family of candidate lists"""
    _build()
    return _MERGED


def reference(name):
    """np_map_associate (ties by gid where the case has gids) / np_merge_associate of a case, computed once and shared"""
    if name not in _REF:
        if name in MAP_NAMES:
            c = map_cases()[name]
            _REF[name] = np_map_associate(c["pose"], c["cs"], c["cm"], c["ss"], c["sm"], c["gid_c"], c["gid_s"])
        else:
            c = merged_cases()[name]
            _REF[name] = np_merge_associate(c["cn"], c["ci"], c["sn"], c["si"])
    return _REF[name]


def reference_by_position(name):
    """a map case's blocks with ties by POSITION whatever its gids: what Map.associate (which never reads the gids) computes"""
    c = map_cases()[name]
    if c["gid_c"] is None:
        return reference(name)
    key = name + "/position"
    if key not in _REF:
        _REF[key] = np_map_associate(c["pose"], c["cs"], c["cm"], c["ss"], c["sm"])
    return _REF[key]


def block_differences(got, ref, rel):
    """the blocks `got` (e_src, e_a, e_b, p_src, p_n, p_d) against `ref`: the source lists exactly, the values within
    rel * max(1, |value|) per value with (a, b) possibly swapped (the eigenvector's sign is a convention)
    -> (list of complaints, largest |difference| over a / b, over n, over d)"""
    bad = []
    worst = [0.0, 0.0, 0.0]
    for k in (0, 3):
        if not np.array_equal(np.asarray(got[k]), np.asarray(ref[k])):
            g, r = np.asarray(got[k]), np.asarray(ref[k])
            bad.append(f"{'edge' if k == 0 else 'plane'} sources differ: {len(g)} vs {len(r)} blocks, only in got {np.setdiff1d(g, r)[:6]}, only in ref {np.setdiff1d(r, g)[:6]}")
    if bad:
        return bad, worst

    def off(x, y):
        return np.abs(x - y) / np.maximum(1.0, np.abs(y))
    a, b, ra, rb = (np.asarray(v, np.float64) for v in (got[1], got[2], ref[1], ref[2]))
    if len(a):
        same = np.maximum(off(a, ra), off(b, rb)).max(axis=1); swap = np.maximum(off(a, rb), off(b, ra)).max(axis=1)
        worst[0] = float(np.where(same <= swap, np.maximum(np.abs(a - ra), np.abs(b - rb)).max(axis=1), np.maximum(np.abs(a - rb), np.abs(b - ra)).max(axis=1)).max())
        if np.minimum(same, swap).max() > rel:
            bad.append(f"line points off by {np.minimum(same, swap).max():.3e} relative at block {int(np.minimum(same, swap).argmax())}")
    n, d, rn, rd = (np.asarray(v, np.float64) for v in (got[4], got[5], ref[4], ref[5]))
    if len(n):
        worst[1] = float(np.abs(n - rn).max()); worst[2] = float(np.abs(d - rd).max())
        if off(n, rn).max() > rel:
            bad.append(f"plane normals off by {off(n, rn).max():.3e} at block {int(off(n, rn).max(axis=1).argmax())}")
        if off(d, rd).max() > rel:
            bad.append(f"negative_OA_dot_norm off by {off(d, rd).max():.3e} relative at block {int(off(d, rd).argmax())}")
    return bad, worst
