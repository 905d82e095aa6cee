"""Crafted inputs for the ODOMETRY association (ll_associate_block under k_associate, its grid and ring tables from k_build_grid), and
an independent reference of it.

A plain helper module (not a conftest): test_assoc_cases.py checks the reference and the generators on the CPU,
test_gpu_assoc_cases.py runs the same cases through Context.upload_features / set_target / associate / vote(False) / edge_corr /
plane_corr.  Everything compared is an index: there is no tolerance anywhere.

The reference restates laserOdometry.cpp:77-95, :491-556 and :653-723, not oracle/ll_oracle.c:
  np_to_start      TransformToStart without distortion: q * p + t in f64 in Eigen's operation order (as mapsearchcases.np_to_world
                   writes it), stored as f32
  np_nearest       brute force over ALL target points, FLANN L2_Simple in f32 -- ((dx*dx + dy*dy) + dz*dz), a = query --, the winner by
                   (distance, index), accepted only if d < dmax
  np_walk_corner,  the two sequential loops over INDICES: ring = int(intensity), the break compared in f64, a running minimum under
  np_walk_plane    strict '<', the walk's own f32 expression (p.x - s.x) * (p.x - s.x) + ...; written as a lexicographic minimum of
                   (distance, visiting order) per query
  np_walk_corner_loop, np_walk_plane_loop   the same two walks as plain Python loops, statement by statement
  np_associate     the compacted correspondences (src, a, b[, c]) in query order

What decides a query's ROUTE through ll_associate_block is restated too, from the reference's own values only: the grid cell
(cell_of), the ring the query's elevation predicts (pred_ring: the sensor model's formula; queries whose route is asserted keep 5 % of
a bin away from a bin edge, so the last bit of atan does not matter), the table flags of k_build_grid's comment (table_flags) and
"window inside the 14-ring table, at most 8 values, no ring with two places at its minimal distance" (routes).

`wrong` (a set of names) turns the reference into a deliberately wrong one -- only to show that the cases can see such an error:
  "nn_tie_high"     nearest ties go to the HIGHEST index          "down_tie_low"    down-walk ties go to the LOWEST index
  "down_before_up"  an up / down tie goes to the down-walk        "limit_le"        d <= dmax for the neighbour and the partners
  "plane_same_eq"   plane point b requires rj == rc both ways     "dist_f64"        distances are summed in f64
  "nearby_floor"    the window is [floor(rc - nearby), floor(rc + nearby)]: floor on BOTH bounds, one ring too far down when nearby is
                    no integer.  (Read as rc +- floor(nearby) the mistake cannot be seen at all: ring ids are integers, and for an
                    integer rj,  rj > rc + nearby  <=>  rj > rc + floor(nearby)  and  rj < rc - nearby  <=>  rj < rc - floor(nearby);
                    test_assoc_cases.py states that.)
  "break_inclusive" the point at which a walk breaks still counts as a candidate

Second-round entries.  The sweep beyond Chebyshev ring 2 has 2 * rmax + 6 entries, rmax = ceil(sqrt(dmax)) + 1, fetched 18 at a time: 18
at dmax = 25 (one round), 20 at dmax = 36.  Entries 18 and 19 are the rows cy -+ rmax, which lie more than sqrt(dmax) away: they can
hold decoys only, never an acceptable point.  The case far-round2 runs at dmax = 36 and puts target points there.

Untested on purpose: non-finite coordinates (ll_cell_coord of a NaN is an undefined conversion; nothing here may be changed to send
one to the device), DISTORTION 1, and the ring-strided extracted less-flat target.
"""
import functools

import numpy as np

F32 = np.float32
R = 64
LOWER, UPPER = F32(-24.9), F32(2.0)                     # ll_default_params(64)
FACTOR = F32(R - 1) / (UPPER - LOWER)                   # scanRegistration.cpp:441 in f32
GRID_G, GRID_ORG = 128, F32(64.0)                       # LL_GRID_G cells of 1 m, origin -64 m
TAB = 160                                               # LL_TAB: ring ids the tables hold
ATAB_W, ATAB_BACK = 14, 7                               # LL_ATAB_W, LL_ATAB_BACK
ROWS_BELOW = 64                                         # LL_ASSOC_PLANE_ROWS_BELOW
CAP_SHARP, CAP_FLAT, CAP_LSHARP, MAX_POINTS = 768, 1536, 7680, 4096
IDENT = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])
EMPTY = np.zeros((0, 4), np.float32)
NEARBY_VALUES = (0.5, 1.0, 2.5, 3.5, 4.0)
SIZES = (1, 31, 32, 33, 255, 256, 257)
WRONG = ("nn_tie_high", "down_tie_low", "down_before_up", "limit_le", "nearby_floor", "plane_same_eq", "dist_f64", "break_inclusive")


# ------------------------------------------------------------------------------------------------ the reference
def np_to_start(pose7, pts):
    """:77-95 with s = 1: q_last_curr * p + t_last_curr (Eigen _transformVector: uv = u x v; uv += uv; ((v + w*uv) + u x uv) + t) -> f32 (n, 3)"""
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


def _xyz(cloud, wrong):
    t = np.float64 if "dist_f64" in wrong else np.float32
    return np.ascontiguousarray(cloud, np.float32).reshape(-1, 4)[:, :3].astype(t), t


def nn_dist(sel, target, wrong=()):
    """FLANN L2_Simple of every (query, target point) pair: ((dx*dx + dy*dy) + dz*dz), a = query, b = data, every step f32 -> [n, m]"""
    m, t = _xyz(target, wrong)
    s = np.ascontiguousarray(sel, np.float32).reshape(-1, 3).astype(t)
    d = s[:, None, 0] - m[None, :, 0]; out = d * d
    d = s[:, None, 1] - m[None, :, 1]; out = out + d * d
    d = s[:, None, 2] - m[None, :, 2]; out = out + d * d
    assert out.dtype == t
    return out


def walk_dist(s, target, wrong=()):
    """:514-519: (p.x - s.x) * (p.x - s.x) + (p.y - s.y) * (p.y - s.y) + (p.z - s.z) * (p.z - s.z) of one query against every target point"""
    m, t = _xyz(target, wrong)
    s = np.asarray(s, np.float32).astype(t)
    out = ((m[:, 0] - s[0]) * (m[:, 0] - s[0]) + (m[:, 1] - s[1]) * (m[:, 1] - s[1])) + (m[:, 2] - s[2]) * (m[:, 2] - s[2])
    assert out.dtype == t
    return out


def rings_of(target):
    """int(intensity): truncation towards zero"""
    return np.trunc(np.ascontiguousarray(target, np.float32).reshape(-1, 4)[:, 3].astype(np.float64)).astype(np.int64)


def np_nearest(sel, target, dmax=25, wrong=()):
    """-> (index of the nearest target point per query, -1 where none is closer than dmax; its distance)"""
    sel = np.ascontiguousarray(sel, np.float32).reshape(-1, 3)
    n, m = len(sel), len(target)
    idx = np.full(n, -1, np.int64); dd = np.full(n, np.inf)
    if n and m:
        d = nn_dist(sel, target, wrong)
        key = np.arange(m, dtype=np.int64)
        best = np.lexsort((np.broadcast_to(-key if "nn_tie_high" in wrong else key, (n, m)), d), axis=1)[:, 0]
        dd = d[np.arange(n), best]
        ok = dd <= F32(dmax) if "limit_le" in wrong else dd < F32(dmax)
        idx = np.where(ok, best, -1)
    return idx, dd


def _bounds(rc, nearby, wrong):
    """the two f64 values the breaks compare int(intensity) with (:511, :537)"""
    up, down = float(rc) + float(nearby), float(rc) - float(nearby)
    return (np.floor(up), np.floor(down)) if "nearby_floor" in wrong else (up, down)


def _takes(d, cur_d, cur_j, cur_down, now_down, wrong):
    """`if (pointSqDis < minPointSqDis)`, and what the wrong variants add to it"""
    if d < cur_d:
        return True
    if d == cur_d:
        if cur_j < 0:
            return "limit_le" in wrong
        if now_down:
            return ("down_tie_low" in wrong) if cur_down else ("down_before_up" in wrong)
    return False


def np_walk_corner_loop(s, target, c, nearby=2.5, dmax=25, wrong=()):
    """:500-553, statement by statement -> minPointInd2"""
    ring = rings_of(target); d = walk_dist(s, target, wrong)
    rc = int(ring[c]); up, down = _bounds(rc, nearby, wrong)
    m2, j2, f2 = float(dmax), -1, False
    for j in range(c + 1, len(ring)):
        if ring[j] <= rc:
            continue
        stop = float(ring[j]) > up
        if stop and "break_inclusive" not in wrong:
            break
        if _takes(float(d[j]), m2, j2, f2, False, wrong):
            m2, j2, f2 = float(d[j]), j, False
        if stop:
            break
    for j in range(c - 1, -1, -1):
        if ring[j] >= rc:
            continue
        stop = float(ring[j]) < down
        if stop and "break_inclusive" not in wrong:
            break
        if _takes(float(d[j]), m2, j2, f2, True, wrong):
            m2, j2, f2 = float(d[j]), j, True
        if stop:
            break
    return j2


def np_walk_plane_loop(s, target, c, nearby=2.5, dmax=25, wrong=()):
    """:664-721, statement by statement -> (minPointInd2, minPointInd3)"""
    ring = rings_of(target); d = walk_dist(s, target, wrong)
    rc = int(ring[c]); up, down = _bounds(rc, nearby, wrong)
    eq = "plane_same_eq" in wrong
    m2, j2, f2, m3, j3, f3 = float(dmax), -1, False, float(dmax), -1, False
    for j in range(c + 1, len(ring)):
        stop = float(ring[j]) > up
        if stop and "break_inclusive" not in wrong:
            break
        dj = float(d[j])
        same = ring[j] == rc if eq else ring[j] <= rc
        if same and _takes(dj, m2, j2, f2, False, wrong):
            m2, j2, f2 = dj, j, False
        elif not same and _takes(dj, m3, j3, f3, False, wrong):
            m3, j3, f3 = dj, j, False
        if stop:
            break
    for j in range(c - 1, -1, -1):
        stop = float(ring[j]) < down
        if stop and "break_inclusive" not in wrong:
            break
        dj = float(d[j])
        same = ring[j] == rc if eq else ring[j] >= rc
        if same and _takes(dj, m2, j2, f2, True, wrong):
            m2, j2, f2 = dj, j, True
        elif not same and _takes(dj, m3, j3, f3, True, wrong):
            m3, j3, f3 = dj, j, True
        if stop:
            break
    return j2, j3


def _window(ring, c, nearby, wrong):
    """what the two loops visit before they break: (visited by the up-walk, visited by the down-walk, first index the up-walk breaks at
    or m, last index the down-walk breaks at or -1)"""
    m = len(ring); j = np.arange(m)
    up, down = _bounds(int(ring[c]), nearby, wrong)
    brk = np.flatnonzero((j > c) & (ring.astype(np.float64) > up))
    stop_up = int(brk[0]) if len(brk) else m
    brk = np.flatnonzero((j < c) & (ring.astype(np.float64) < down))
    stop_dn = int(brk[-1]) if len(brk) else -1
    if "break_inclusive" in wrong:
        return (j > c) & (j <= stop_up), (j < c) & (j >= stop_dn), stop_up, stop_dn
    return (j > c) & (j < stop_up), (j < c) & (j > stop_dn), stop_up, stop_dn


def _lexmin(d, cand, c, dmax, wrong):
    """the running minimum under strict '<' over the visiting order = the lexicographic minimum of (distance, visiting order)"""
    m = len(d); j = np.arange(m)
    cand = cand & ((d <= F32(dmax)) if "limit_le" in wrong else (d < F32(dmax)))
    if not cand.any():
        return -1
    o_up = j - c - 1
    o_dn = (m + j) if "down_tie_low" in wrong else (m + (c - 1 - j))
    if "down_before_up" in wrong:
        o_up, o_dn = o_up + 2 * m, o_dn - m
    order = np.where(j > c, o_up, o_dn)
    at = np.flatnonzero(cand)
    return int(at[np.lexsort((order[at], d[at]))[0]])


def np_walk_corner(s, target, c, nearby=2.5, dmax=25, wrong=()):
    ring = rings_of(target); d = walk_dist(s, target, wrong)
    in_up, in_dn, _, _ = _window(ring, c, nearby, wrong)
    return _lexmin(d, (in_up & (ring > ring[c])) | (in_dn & (ring < ring[c])), c, dmax, wrong)


def np_walk_plane(s, target, c, nearby=2.5, dmax=25, wrong=()):
    ring = rings_of(target); d = walk_dist(s, target, wrong)
    in_up, in_dn, _, _ = _window(ring, c, nearby, wrong)
    if "plane_same_eq" in wrong:
        same = (in_up | in_dn) & (ring == ring[c])
    else:
        same = (in_up & (ring <= ring[c])) | (in_dn & (ring >= ring[c]))
    return _lexmin(d, same, c, dmax, wrong), _lexmin(d, (in_up | in_dn) & ~same, c, dmax, wrong)


def np_associate(pose7, queries, target, plane, nearby=2.5, dmax=25, wrong=(), loop=False, detail=False):
    """one association pass -> (src, a, b) or (src, a, b, c): the compacted correspondences in query order (int32), and with
    detail=True a dict of the per-query values before compaction (sel, nn, d_nn, b, c; -1 where there is none)"""
    target = np.ascontiguousarray(target, np.float32).reshape(-1, 4)
    sel = np_to_start(pose7, queries)
    nn, d_nn = np_nearest(sel, target, dmax, wrong)
    n = len(sel)
    b = np.full(n, -1, np.int64); c3 = np.full(n, -1, np.int64)
    for i in np.flatnonzero(nn >= 0):
        if plane:
            b[i], c3[i] = (np_walk_plane_loop if loop else np_walk_plane)(sel[i], target, int(nn[i]), nearby, dmax, wrong)
        else:
            b[i] = (np_walk_corner_loop if loop else np_walk_corner)(sel[i], target, int(nn[i]), nearby, dmax, wrong)
    ok = (nn >= 0) & (b >= 0) & ((c3 >= 0) if plane else True)
    src = np.flatnonzero(ok)
    out = (src.astype(np.int32), nn[src].astype(np.int32), b[src].astype(np.int32)) + ((c3[src].astype(np.int32),) if plane else ())
    return out + (dict(sel=sel, nn=nn, d_nn=d_nn, b=b, c=c3, ok=ok),) if detail else out


def same_result(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------ the routes, restated
def cell_of(v):
    """ll_cell_coord: floor((v + 64) * 1) in f32, saturated into 0 .. 127"""
    return np.clip(np.floor((np.asarray(v, np.float32) + GRID_ORG) * F32(1.0)), 0, GRID_G - 1).astype(np.int64)


def cell_counts(target):
    t = np.ascontiguousarray(target, np.float32).reshape(-1, 4)
    return np.bincount(cell_of(t[:, 1]) * GRID_G + cell_of(t[:, 0]), minlength=GRID_G * GRID_G).reshape(GRID_G, GRID_G)     # [cy, cx]


def ring_position(t):
    """scanRegistration.cpp:139-162 for 64 rings as a function of t = z / sqrt(x*x + y*y): (angle - lower_bound) * factor + 0.5 before
    the truncation (f32 atan, f32 product, f64 division, f32 store, f32 bin arithmetic)"""
    ang = (np.arctan(np.asarray(t, np.float32)).astype(np.float32) * F32(180.0)).astype(np.float64) / np.pi
    return ((ang.astype(np.float32) - LOWER) * FACTOR).astype(np.float64) + 0.5


def pred_ring(sel):
    """-> (the ring the table of a query is centred on: the sensor model's ring of its elevation, clamped into 0 .. 250; how far, in
    bins, the elevation is from the nearest bin edge)"""
    s = np.ascontiguousarray(sel, np.float32).reshape(-1, 3)
    with np.errstate(divide="ignore", invalid="ignore"):
        u = ring_position(s[:, 2] / np.sqrt(s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]))
    pred = np.clip(np.trunc(u), 0, 250).astype(np.int64)
    return pred, np.minimum(u - np.floor(u), np.ceil(u) - u)


def ring_hi(rc, nearby):
    return np.floor(np.asarray(rc, np.float64) + nearby).astype(np.int64)


def ring_lo(rc, nearby):
    return np.ceil(np.asarray(rc, np.float64) - nearby).astype(np.int64)


def table_flags(target, nearby):
    """k_build_grid's flags.  Bit 0, the tables bound the walks of EVERY start point: every ring id lies in 0 .. 159, no point lies
    before a point whose up-window it exceeds and none after a point whose down-window it undercuts.  Bit 1: bit 0, and the ring ids
    never decrease along the cloud."""
    ring = rings_of(target)
    if len(ring) == 0:
        return 3
    before = np.concatenate([[-(1 << 40)], np.maximum.accumulate(ring)[:-1]])          # the largest ring id in front of each point
    after = np.concatenate([np.minimum.accumulate(ring[::-1])[::-1][1:], [1 << 40]])   # the smallest behind it
    ok = bool(((ring >= 0) & (ring < TAB)).all()) and not (before > ring_hi(ring, nearby)).any() and not (after < ring_lo(ring, nearby)).any()
    return (1 if ok else 0) | (2 if ok and (np.diff(ring) >= 0).all() else 0)


def routes(case, plane):
    """per query of one cloud type, from the reference's values only: pred, margin, rc, inside (the window [lo, hi] lies inside the
    table around pred and holds at most 8 values), tie (a ring of the window holds two or more places, the neighbour left out, at
    its minimal distance < dmax), own (points in the query's own cell), plus the target's table flags"""
    q, tgt = (case["flat"], case["surf"]) if plane else (case["sharp"], case["corner"])
    x = reference(case["name"])[3 if plane else 2]
    sel, nn = x["sel"], x["nn"]
    n = len(sel)
    pred, margin = pred_ring(sel)
    ring = rings_of(tgt)
    rc = np.where(nn >= 0, ring[np.maximum(nn, 0)] if len(ring) else 0, -1)
    lo, hi = ring_lo(rc, case["nearby"]), ring_hi(rc, case["nearby"])
    rq0 = pred - ATAB_BACK
    inside = (nn >= 0) & (lo >= rq0) & (hi < rq0 + ATAB_W) & (hi - lo < 8)
    tie = np.zeros(n, bool)
    for i in np.flatnonzero(nn >= 0):
        d = walk_dist(sel[i], tgt)
        d = np.where((np.arange(len(d)) != nn[i]) & (d < F32(case["dmax"])), d, np.inf)
        for v in range(int(lo[i]), int(hi[i]) + 1):
            dv = d[ring == v]
            if len(dv) and np.isfinite(dv.min()) and (dv == dv.min()).sum() >= 2:
                tie[i] = True
    cnt = cell_counts(tgt)
    own = cnt[cell_of(sel[:, 1]), cell_of(sel[:, 0])] if n else np.zeros(0, np.int64)
    return dict(pred=pred, margin=margin, rc=rc, inside=inside, tie=tie, own=own, flags=table_flags(tgt, case["nearby"]), nn=nn, b=x["b"], c=x["c"],
                sel=sel, ok=x["ok"], ring=ring)


# ------------------------------------------------------------------------------------------------ small tools
def small_pose():
    q = np.array([0.01, -0.02, 0.015, 1.0]); q /= np.linalg.norm(q)
    return np.concatenate([q, [0.3, -0.2, 0.05]])


def yaw_pose():
    q = np.array([0.0, 0.0, np.sin(0.35), np.cos(0.35)])
    return np.concatenate([q, [-1.5, 2.0, 0.1]])


POSES = (IDENT, small_pose(), yaw_pose())


def to_lidar(pose7, queries):
    """queries whose TransformToStart lands near the given ones (f64 inverse, rounded to f32): the same case under another pose"""
    x, y, z, w = pose7[:4]
    Rm = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                   [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                   [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    out = np.array(queries, np.float32).reshape(-1, 4)
    out[:, :3] = ((out[:, :3].astype(np.float64) - pose7[4:]) @ Rm).astype(np.float32)
    return out


def q16(v):
    """onto the 2^-4 lattice: sums and squares of such small values are exact in f32"""
    return np.round(np.asarray(v, np.float64) * 16.0) / 16.0


def z_of(rho, ring):
    """height, on the 2^-4 lattice, at which a point at horizontal range rho falls into the middle of `ring`'s elevation bin"""
    return float(q16(rho * np.tan(np.deg2rad(float(LOWER) + ring / float(FACTOR)))))


def sites(pitch=7.0, rho_min=20.0):
    """cell centres, `pitch` metres apart, at least rho_min from the sensor: clusters built around them cannot see each other's points"""
    v = np.arange(-59.5, 60.0, pitch)
    out = [(float(x), float(y)) for y in v for x in v if np.hypot(x, y) >= rho_min]
    return [out[k] for k in np.random.default_rng(7).permutation(len(out))]       # consecutive clusters far apart in space


class Scene:
    """queries and target points of ONE cloud type, cluster by cluster.  A cluster is a query on the sensor model's ring `pred` and
    target points at offsets from it, labelled with ring ids of the caller's choice; finish() orders the target by (ring id + e),
    stably: e = 0 everywhere gives a monotone cloud, clusters keep their insertion order inside a ring."""

    def __init__(self):
        self.q, self.t, self.key = [], [], []

    def query(self, xy, pred, off=(0.0, 0.0, 0.0)):
        z = z_of(np.hypot(xy[0] + off[0], xy[1] + off[1]), pred)
        p = np.array([xy[0] + off[0], xy[1] + off[1], z + off[2]])
        self.q.append([p[0], p[1], p[2], pred + 0.5])
        return p

    def point(self, p, off, ring, e=0.0):
        if ring < 0:
            return
        k = len(self.t)
        self.t.append([p[0] + off[0], p[1] + off[1], p[2] + off[2], ring + 0.25 * (k % 3)])   # int(intensity) drops the fraction
        self.key.append(ring + e)

    def finish(self, order=None):
        q = np.array(self.q, np.float32).reshape(-1, 4); t = np.array(self.t, np.float32).reshape(-1, 4)
        if order is None:
            order = np.argsort(np.array(self.key), kind="stable")
        return q, np.ascontiguousarray(t[order])


def case(family, name, sharp, corner, flat, surf, pose=IDENT, nearby=2.5, dmax=25.0, **kw):
    c = dict(family=family, name=name, pose=np.asarray(pose, np.float64), nearby=float(nearby), dmax=float(dmax),
             sharp=np.ascontiguousarray(sharp, np.float32).reshape(-1, 4), corner=np.ascontiguousarray(corner, np.float32).reshape(-1, 4),
             flat=np.ascontiguousarray(flat, np.float32).reshape(-1, 4), surf=np.ascontiguousarray(surf, np.float32).reshape(-1, 4))
    assert len(c["sharp"]) <= CAP_SHARP and len(c["flat"]) <= CAP_FLAT and len(c["corner"]) <= CAP_LSHARP and len(c["surf"]) <= MAX_POINTS, name
    c.update(kw)
    return c


# ------------------------------------------------------------------------------------------------ monotone families on the sensor model
PARTNERS = ((1,), (-1,), (2,), (-2,), (1, -1), (2, -2, 1), (), (3, -3), (-2, 2), (1, 2), (4,), (-4,), (3,), (-3, 4))
ABSENT = 7                                              # ring ids = 3 (mod 7) hold no partner: some rings are absent from the target


def model_scene(plane, n, seed, delta=lambda i, pred: 0, preds=None, label=None, partners=PARTNERS):
    """n clusters on the sensor model: the neighbour 1/16 m beside the query on ring rc = pred + delta, partners on rc + k at the heights
    of their own bins, a nearer decoy on a ring outside every window, for a plane query one more point on rc (not always)"""
    rng = np.random.default_rng(seed)
    S = Scene(); st = sites()
    for i in range(n):
        xy = st[i % len(st)]
        rho = np.hypot(*xy)
        pred = int(preds[i % len(preds)]) if preds is not None else int(8 + (i * 11) % 48)
        d = delta(i, pred)
        rc = pred + d if label is None else label(pred)
        if label is None and d == 0 and rc % ABSENT == 3:
            pred += 1; rc += 1
        p = S.query(xy, pred, (0.0625 * int(rng.integers(-3, 4)), 0.0625 * int(rng.integers(-3, 4)), 0.0))
        zq = p[2]
        S.point(p, (0.0625, 0.0, 0.0), rc)
        ks = partners[i % len(partners)]
        for a, k in enumerate(ks):
            if label is None and (rc + k) % ABSENT == 3:
                continue
            S.point(p, (0.125 * abs(k) + 0.0625 * a, 0.25, z_of(rho, pred + k) - zq), rc + k)
        if i % 3 == 0 and label is None:
            S.point(p, (0.125, 0.0, 0.0625), rc + 6)                                # nearer than every partner, in no window: no candidate
        if plane and i % 5 != 4:
            S.point(p, (-0.1875, 0.125 * (1 + i % 2), 0.0), rc)
    return S.finish()


def _model_case(family, name, n_c, n_p, seed, nearby=2.5, **kw):
    sharp, corner = model_scene(False, n_c, seed, **kw)
    flat, surf = model_scene(True, n_p, seed + 1, **kw)
    return case(family, name, sharp, corner, flat, surf, nearby=nearby)


EDGE_DELTAS = (-6, -5, 4, 5)


def _edge_delta(i, pred):
    return EDGE_DELTAS[i % 4]


def _low(i, pred):                                      # rc in {0, 1, 2} under pred <= 5: the table's first ring pred - 7 is negative
    return (i % 3) - pred


def _high(i, pred):                                     # rc and pred near the last ring, rc past it too
    return (-6, -5, 0, 4, 5, 6)[i % 6]


def model_cases():
    out = {"inside": _model_case("inside", "inside", 224, 224, 100)}
    out["edges-delta"] = _model_case("edges", "edges-delta", 160, 160, 110, delta=_edge_delta, preds=np.arange(10, 54))
    out["edges-low"] = _model_case("edges", "edges-low", 96, 96, 112, delta=_low, preds=(0, 1, 2, 3, 4, 5))
    out["edges-high"] = _model_case("edges", "edges-high", 96, 96, 114, delta=_high, preds=(60, 61, 62, 63))
    out["bypass"] = _model_case("bypass", "bypass", 128, 128, 120, label=lambda pred: 103 + pred % 4, partners=PARTNERS[:10])
    for nb in NEARBY_VALUES:
        out[f"nearby-{nb}"] = _model_case("nearby", f"nearby-{nb}", 140, 140, 130, nearby=nb)
    for n in SIZES:
        out[f"size-{n}"] = _model_case("sizes", f"size-{n}", n, n, 140 + n)
    return out


# ------------------------------------------------------------------------------------------------ ties
D = 0.25                                                # tied candidates sit 1/4 m from the query: d = 0.0625 exactly
MIRROR = (((D, 0, 0), (-D, 0, 0)), ((0, D, 0), (0, -D, 0)), ((0, 0, D), (0, 0, -D)))
TIE_KINDS = 16


def tie_cluster(S, plane, xy, pred, kind, e=lambda ring_off, k: 0.0):
    """one tied cluster around a query at a cell centre; every point lies in the query's own cell"""
    p = S.query(xy, pred)
    rc = pred
    nb = (0.0625, 0.0625, 0.0)
    plain_b = lambda: S.point(p, (-0.125, 0.0625, 0.0), rc, e(0, 9)) if plane else None
    plain_p = lambda: S.point(p, (0.1875, -0.125, 0.0625), rc + 1, e(1, 9))
    if kind < 3:                                        # mirror pair on rc + 1: the up-walk keeps the lower index
        S.point(p, nb, rc, e(0, 0)); [S.point(p, o, rc + 1, e(1, k)) for k, o in enumerate(MIRROR[kind])]; plain_b()
    elif kind < 6:                                      # mirror pair on rc - 1: the down-walk keeps the HIGHER index
        S.point(p, nb, rc, e(0, 0)); [S.point(p, o, rc - 1, e(-1, k)) for k, o in enumerate(MIRROR[kind - 3])]; plain_b()
    elif kind < 9:                                      # mirror pair on rc: both behind the neighbour, both in front of it, one on each side
        a, b = MIRROR[kind - 6]
        if kind == 6:
            S.point(p, nb, rc, e(0, 0)); S.point(p, a, rc, e(0, 1)); S.point(p, b, rc, e(0, 2))
        elif kind == 7:
            S.point(p, a, rc, e(0, 1)); S.point(p, b, rc, e(0, 2)); S.point(p, nb, rc, e(0, 0))
        else:
            S.point(p, a, rc, e(0, 1)); S.point(p, nb, rc, e(0, 0)); S.point(p, b, rc, e(0, 2))
        plain_p()
    elif kind == 9:                                     # one on rc + 1 and one on rc - 1 at the same distance: the up-walk's
        S.point(p, nb, rc, e(0, 0)); S.point(p, (-D, 0, 0), rc + 1, e(1, 0)); S.point(p, (D, 0, 0), rc - 1, e(-1, 0)); plain_b()
    elif kind == 10:                                    # ... and at two rings' distance
        S.point(p, nb, rc, e(0, 0)); S.point(p, (0, D, 0), rc - 2, e(-2, 0)); S.point(p, (0, -D, 0), rc + 2, e(2, 0)); plain_b()
    elif kind == 11:                                    # the neighbour has a bit-identical twin: b of a plane query, never a corner's partner
        S.point(p, nb, rc, e(0, 0)); S.point(p, nb, rc, e(0, 1)); plain_p()
    elif kind == 12:                                    # three equal candidates on rc + 1: three lanes' shares of the cell range
        S.point(p, nb, rc, e(0, 0)); [S.point(p, o, rc + 1, e(1, k)) for k, o in enumerate(((D, 0, 0), (0, -D, 0), (0, 0, D)))]; plain_b()
    elif kind == 13:                                    # three on rc - 1
        S.point(p, nb, rc, e(0, 0)); [S.point(p, o, rc - 1, e(-1, k)) for k, o in enumerate(((0, 0, -D), (-D, 0, 0), (0, D, 0)))]; plain_b()
    elif kind == 14:                                    # a tied pair BEHIND the ring's minimum: the table may be used
        S.point(p, nb, rc, e(0, 0)); S.point(p, (0.125, 0, 0), rc + 1, e(1, 0)); [S.point(p, o, rc + 1, e(1, 1 + k)) for k, o in enumerate(MIRROR[0])]; plain_b()
    else:                                               # pairs on rc + 1 and on rc - 1, all four at one distance
        S.point(p, nb, rc, e(0, 0)); [S.point(p, o, rc + 1, e(1, k)) for k, o in enumerate(MIRROR[1])]
        [S.point(p, o, rc - 1, e(-1, k)) for k, o in enumerate(MIRROR[0])]; plain_b()


def tie_scene(plane, n, e=None, S=None):
    S = Scene() if S is None else S; st = sites()
    for i in range(n):
        xy = st[i % len(st)]
        tie_cluster(S, plane, xy, int(6 + (i * 5) % 52), i % TIE_KINDS, *(() if e is None else (e(i),)))
    return S


def rounding_scene(plane, n, seed):
    """two candidates on rc + 1 whose f32 distances are bit-equal (0.0625) while the exact ones differ: one on the lattice, one found by
    search off it, exactly nearer; the off-lattice one has the higher index (f32: the tie goes to the lattice point) or the lower one"""
    rng = np.random.default_rng(seed)
    S = Scene(); st = sites()
    for i in range(n):
        p = S.query(st[i % len(st)], int(6 + (i * 5) % 52))
        rc = int(6 + (i * 5) % 52)
        while True:
            u = rng.standard_normal((4096, 3)); u = (p + D * u / np.linalg.norm(u, axis=1, keepdims=True)).astype(np.float32)
            d32 = walk_dist(p.astype(np.float32), np.concatenate([u, u[:, :1]], axis=1))
            d64 = walk_dist(p.astype(np.float32), np.concatenate([u, u[:, :1]], axis=1), wrong=("dist_f64",))
            hit = np.flatnonzero((d32 == F32(D * D)) & (d64 < D * D))
            if len(hit):
                break
        o = tuple(u[hit[0]].astype(np.float64) - p)
        S.point(p, (0.0625, 0.0625, 0.0), rc)
        if plane:
            S.point(p, (-0.125, 0.0625, 0.0), rc)
        [S.point(p, off, rc + 1) for off in (((D, 0, 0), o) if i % 2 == 0 else (o, (D, 0, 0)))]
    return S.finish()


def tie_cases():
    a = tie_scene(False, 256).finish(); b = tie_scene(True, 256).finish()
    c = rounding_scene(False, 24, 150); d = rounding_scene(True, 24, 151)
    return {"ties": case("ties", "ties", a[0], a[1], b[0], b[1]), "ties-rounding": case("ties", "ties-rounding", c[0], c[1], d[0], d[1])}


# ------------------------------------------------------------------------------------------------ displaced minima
def displaced_scene(plane, n, seed):
    """cells of 9 .. 40 points around a query: the nearest neighbour carries the cluster's lowest ring id (the first of its cell in index
    order) or its highest (the last), points of the cell to the left are met before it in the own row, and the second-nearest point
    overall is the partner on the next ring"""
    rng = np.random.default_rng(seed)
    S = Scene(); st = sites()
    for i in range(n):
        xy = st[i % len(st)]
        first = i % 2 == 0
        pred = int(8 + (i * 7) % 48)
        rc = pred - 2 if first else pred + 2
        p = S.query(xy, pred, tuple(rng.uniform(-0.2, 0.2, 2)) + (0.0,))
        ctr = np.array([xy[0], xy[1], p[2]])
        u = rng.standard_normal(3); u /= np.linalg.norm(u)
        if first:
            S.point(p, tuple(0.03 * u), rc)             # the nearest, inside the own cell (the query is at most 0.2 m from its centre)
        n_own = int(rng.integers(8, 38))
        for k in range(n_own):                          # the own cell, all farther than 0.2 m from the query
            while True:
                o = ctr + rng.uniform(-0.49, 0.49, 3)
                if np.linalg.norm(o - p) > 0.2:
                    break
            S.point(o, (0, 0, 0), rc + (int(rng.integers(0, 5)) if first else -int(rng.integers(0, 5))))
        for side in (-1.0, 1.0):                        # the cells to the left and to the right
            for k in range(int(rng.integers(3, 9))):
                o = ctr + np.array([side, 0, 0]) + rng.uniform(-0.49, 0.49, 3)
                S.point(o, (0, 0, 0), rc + (int(rng.integers(0, 5)) if first else -int(rng.integers(0, 5))))
        if not first:
            S.point(p, tuple(0.03 * u), rc)
        v = rng.standard_normal(3); v /= np.linalg.norm(v)
        S.point(p, tuple(0.07 * v), rc + (1 if first else -1))      # the second-nearest overall: the partner
    return S.finish()


def displaced_cases():
    a = displaced_scene(False, 120, 200); b = displaced_scene(True, 90, 201)
    return {"displaced": case("displaced", "displaced", a[0], a[1], b[0], b[1])}


# ------------------------------------------------------------------------------------------------ valid tables that are not monotone
def vnm_scene(plane, n, seed):
    """clusters ordered by ring id + e, e in {0, 1.2}: the ring ids run locally backwards (.. r, r + 1, r, r + 1, r + 2, r + 1 ..), never more
    than one ring ahead of or behind their position: inside every window of nearby = 2.5"""
    rng = np.random.default_rng(seed)
    S = Scene(); st = sites()
    for i in range(n):
        xy = st[i % len(st)]
        pred = int(6 + (i * 5) % 52)
        kind = i % (TIE_KINDS + 4)
        if kind < TIE_KINDS:
            tie_cluster(S, plane, xy, pred, kind, lambda ring_off, k: 1.2 * int(rng.integers(0, 2)))
            continue
        p = S.query(xy, pred)
        rc = pred
        if kind == TIE_KINDS:                           # the only other point of the up-walk lies one ring BELOW: b of a plane query (rj <= rc), nothing for a corner
            S.point(p, (0.0625, 0, 0), rc, 0.0); S.point(p, (0, 0.1875, 0), rc - 1, 1.2); S.point(p, (0.25, 0.125, 0), rc + 1, 1.2)
        elif kind == TIE_KINDS + 1:                     # the only other point of the down-walk lies one ring ABOVE (rj >= rc)
            S.point(p, (0.0625, 0, 0), rc, 1.2); S.point(p, (0, 0.1875, 0), rc + 1, 0.0); S.point(p, (0.25, 0.125, 0), rc - 1, 0.0)
        elif kind == TIE_KINDS + 2:                     # a wrong-side point nearer than the right-side one of ring rc
            S.point(p, (0.0625, 0, 0), rc, 0.0); S.point(p, (0, 0.125, 0), rc - 1, 1.2); S.point(p, (0, -0.25, 0), rc, 0.0); S.point(p, (0.25, 0.125, 0), rc + 1, 0.0)
        else:                                           # a corner's partner of a lower ring behind the neighbour: the up-walk skips it, the down-walk never meets it
            S.point(p, (0.0625, 0, 0), rc, 0.0); S.point(p, (0, 0.125, 0), rc - 1, 1.2); S.point(p, (0.25, 0.25, 0), rc + 2, 0.0)
            if plane:
                S.point(p, (0, -0.25, 0), rc + 1, 0.0)
    return S.finish()


def vnm_cases():
    a = vnm_scene(False, 240, 300); b = vnm_scene(True, 240, 301)
    return {"vnm": case("vnm", "vnm", a[0], a[1], b[0], b[1])}


# ------------------------------------------------------------------------------------------------ invalid tables
def break_lanes(sel, target, nearby=2.5):
    """on which lane of its 64-index steps every up-walk and every down-walk of the sequential fallback breaks"""
    ring = rings_of(target); ups, downs = [], []
    for c in np_nearest(sel, target)[0]:
        if c >= 0:
            _, _, su, sd = _window(ring, int(c), nearby, ())
            ups += [(su - int(c) - 1) % 64] if su < len(ring) else []
            downs += [(int(c) - 1 - sd) % 64] if sd >= 0 else []
    return ups, downs


def _strew(t, rng, n, ahead):
    """n lone points far outside (90 m and beyond), labelled like their surroundings (ahead = 0: the cloud stays monotone) or 5 .. 9 rings ahead"""
    for at in sorted(rng.choice(np.arange(10, len(t) - 10), n, replace=False).tolist(), reverse=True):
        lab = float(rings_of(t[at:at + 1])[0] + (int(rng.integers(5, 10)) if ahead else 0))
        t = np.concatenate([t[:at], np.array([[90.0 + at % 7, 90.0, 0.0, lab]], np.float32), t[at:]])
    return t


BOUNDARY_UP, BOUNDARY_DOWN = (10, 20, 30, 40), (16, 26, 36, 46)


def invalid_scene(plane, ahead):
    """240 tie clusters, and clusters whose walk breaks AT a point that would otherwise be the partner (the break is tested before the
    distance: no correspondence).  Boundary clusters: the only other-ring point lies three rings away and is the first of its ring in
    index order (added before everything else) or the last (added after everything else).  With `ahead`, clusters on the rings 61 .. 63
    whose nearest other point is labelled five rings ahead (behind) of where it stands, between the neighbour and the true partner."""
    S = Scene(); st = sites()
    spot = iter(st[::-1])
    def lone(pred, k, e=0.0, partner=None):
        p = S.query(next(spot), pred)
        S.point(p, (0.0625, 0.0625, 0.0), pred)
        if plane:
            S.point(p, (-0.125, 0.0625, 0.0), pred)
        S.point(p, (0.0, 0.1875, 0.0625), pred + k, e)
        if partner is not None:
            S.point(p, (0.25, -0.125, 0.0), pred + partner)
    for pred in BOUNDARY_UP:
        lone(pred, 3)
    tie_scene(plane, 240, S=S)
    if ahead:
        for k in range(4):
            lone(61, 5, -4.5, 1); lone(62, 5, -4.5, 1); lone(63, -5, 4.5, -1)
    for pred in BOUNDARY_DOWN:
        lone(pred, -3)
    return S.finish()


def invalid_cases():
    """tables that do NOT bound the walks: (i) one ring id of 200, outside the tables; (ii) ring ids that run ahead of their position by
    more than nearby: the clusters of invalid_scene, and lone points labelled + 5 .. + 9 strewn into the cloud, at which up-walks break
    early.  Lone far points also shift the places at which the walks break: the first strewing (by seed) under which up-walks and
    down-walks break on the first lane of a 64-index step, on its last lane and in between is kept."""
    out = {}
    for name in ("invalid-ring200", "invalid-ahead"):
        clouds = []
        for plane in (False, True):
            q, t0 = invalid_scene(plane, name == "invalid-ahead")
            for seed in range(400, 500):
                rng = np.random.default_rng(seed)
                t = t0
                if name == "invalid-ring200":
                    at = len(t) // 2
                    t = np.concatenate([t[:at], np.array([[90.0, 97.0, 0.0, 200.0]], np.float32), t[at:]])
                else:
                    t = _strew(t, rng, 24, True)
                ups, downs = break_lanes(q[:, :3], t)
                if all(l.count(0) and l.count(63) and len(set(l)) >= 32 for l in (ups, downs)):
                    break
                t0 = _strew(t0, rng, 3, False)
            clouds += [q, t]
        out[name] = case("invalid", name, *clouds)
    return out


# ------------------------------------------------------------------------------------------------ far partners
FAR_CLASSES = ("left", "right", "above", "below")


def far_offsets(cls, k):
    s = (k % 5) - 2.0
    return {"left": (-4.5, s, 0.0), "right": (4.5, s, 0.0), "above": (s, 4.25, 0.0), "below": (s, -4.25, 0.0)}[cls]


def far_scene(plane, n, dmax):
    """the neighbour 0.1 m away, the only partner 4 .. 4.99 m away in one class of annulus entry.  kinds: 0-3 the four classes, 4 a
    partner at exactly d^2 = 25 (3-4-0) beside one just inside, 5 the one at exactly 25 alone (no correspondence), 6 a class with a
    nearer decoy on a ring outside the window, 7 a NEIGHBOUR at exactly 25 and nothing nearer.  At dmax = 36 the partner is 5.25 m away and target points lie in the rows cy -+ 7 too."""
    S = Scene(); st = sites(14.0, 20.0)
    for i in range(n):
        xy = st[i % len(st)]
        pred = int(8 + (i * 7) % 48); rc = pred
        p = S.query(xy, pred)
        kind = i % 8
        if kind == 7 and dmax == 25:                    # the only near point at exactly d^2 = 25: no neighbour at all
            S.point(p, (-3.0, 4.0, 0.0), rc); S.point(p, (-3.0, 4.0, 0.25), rc + 1)
            continue
        S.point(p, (0.0625, 0.0625, 0.0625), rc)
        if plane:
            S.point(p, (-0.125, 0.0, 0.0625), rc)
        up = 1 if (i // 8) % 2 == 0 else -1
        if dmax > 25:
            S.point(p, ((i % 5) - 2.0, 5.25 * up, 0.0), rc + up)                   # inside: 27.6 .. 31.6 < 36
            S.point(p, ((i % 3) - 1.0, 6.75, 0.0), rc + 1); S.point(p, ((i % 3) - 1.0, -6.75, 0.0), rc - 1)     # rows cy +- 7: beyond 6 m
            continue
        if kind < 4:
            S.point(p, far_offsets(FAR_CLASSES[kind], i // 8), rc + up)
        elif kind == 4:
            S.point(p, (3.0, 4.0, 0.0), rc + up); S.point(p, (3.0, 3.9375, 0.0), rc + 2 * up)
        elif kind == 5:
            S.point(p, (-4.0, 3.0, 0.0), rc + up)
        else:
            S.point(p, far_offsets(FAR_CLASSES[(i // 8) % 4], i // 8 + 1), rc + up); S.point(p, (2.0, 0.0, 0.0), rc + 5)
    return S.finish()


def far_cases():
    out = {}
    for name, dmax in (("far", 25.0), ("far-round2", 36.0)):
        a = far_scene(False, 64, dmax); b = far_scene(True, 64, dmax)
        out[name] = case("far", name, a[0], a[1], b[0], b[1], dmax=dmax)
    return out


# ------------------------------------------------------------------------------------------------ dense and sparse near cells
DENSE_COUNTS = (63, 64, 200)


def dense_cases():
    """plane queries whose own cell holds 63 (three rows), 64 and 200 points (five entries), dealt in turn so that one wave holds both
    layouts.  The cell's points fill one side of it; queries near the other side have their nearest neighbour just across the border, in
    the cell to the left or to the right: entries 3 and 4 of the five-entry layout."""
    rng = np.random.default_rng(500)
    S = Scene(); st = sites(14.0, 24.0)
    cells = []
    for ci, cnt in enumerate(DENSE_COUNTS * 2):
        xy = st[ci]
        pred = 20 + 3 * ci
        left = ci < 3                                   # the points fill the right part of the cell, queries come from the left -- or mirrored
        zc = z_of(np.hypot(*xy), pred)
        for k in range(cnt):
            o = np.array([xy[0] + (1 if left else -1) * rng.uniform(-0.15, 0.45), xy[1] + rng.uniform(-0.45, 0.45), zc + rng.uniform(-0.3, 0.3)])
            S.point(o, (0, 0, 0), pred + int(rng.integers(-2, 3)))
        cells.append((xy, pred, left))
    for k in range(14):
        for xy, pred, left in cells:
            sgn = -1.0 if left else 1.0
            if k % 2 == 0:                              # 5 cm inside the border, the nearest 4 cm beyond it
                p = S.query(xy, pred, (sgn * 0.45, 0.05 * (k - 7), 0.0))
                S.point(p, (sgn * 0.09, 0.0, 0.0), pred)
            else:
                p = S.query(xy, pred, (-sgn * rng.uniform(0.0, 0.3), rng.uniform(-0.3, 0.3), 0.0))
    flat, surf = S.finish()
    sharp, corner = model_scene(False, 40, 501)
    return {"dense": case("dense", "dense", sharp, corner, flat, surf)}


def deal_octets(own, qpb):
    """the counting sort of ll_associate_block: per block of qpb queries, the queries by the class min(30, count >> 3) of their own cell;
    -> per octet of the order (the eight queries a wave advances in lockstep) the set of layouts (True = three rows)"""
    out = []
    for at in range(0, len(own), qpb):
        blk = np.asarray(own[at:at + qpb])
        order = np.argsort(np.minimum(30, blk >> 3), kind="stable")
        for o in range(0, len(blk), 8):
            out.append(set((blk[order[o:o + 8]] < ROWS_BELOW).tolist()))
    return out


# ------------------------------------------------------------------------------------------------ grid borders
def border_scene(plane):
    S = Scene()
    spots = [(-63.5, -63.5), (63.5, -63.5), (-63.5, 63.5), (63.5, 63.5), (-63.5, 10.5), (63.5, -24.5), (17.5, -63.5), (-31.5, 63.5),   # cells 0 and 127
             (70.0, 10.5), (-80.0, -75.0), (66.5, 90.0), (-100.0, 30.5), (24.5, -120.0),                                            # saturated cells
             (20.0, 30.0), (-33.0, 21.0), (40.0, -40.0), (-64.0, 0.0), (0.0, 64.0), (64.0, 40.0), (-25.0, -64.0)]                     # integer coordinates
    for i, xy in enumerate(spots):
        pred = 10 + 2 * i; rc = pred
        p = S.query(xy, pred)
        if xy == (70.0, 10.5):                          # the query at 70 m has its neighbour at 72 m, in the same saturated cell
            S.point(p, (2.0, 0.0, 0.0), rc); S.point(p, (2.5, 0.25, 0.125), rc + 1); S.point(p, (2.25, -1.0, 0.0), rc - 1)
            S.point(p, (3.0, 0.5, 0.0), rc + 2); S.point(p, (2.5, -0.5, 0.0625), rc)
            continue
        S.point(p, (0.0625, 0.0, 0.0), rc)
        S.point(p, (-0.4375, 0.25, 0.125), rc + 1); S.point(p, (0.25, -1.0, 0.0), rc - 1); S.point(p, (-1.0, 0.5, 0.0), rc + 2)
        S.point(p, (-0.5, -0.5, 0.0625), rc)
        if plane:
            S.point(p, (1.0, 1.0, 0.0), rc)
    return S.finish()


def one_cell_scene(plane, seed):
    """the whole target inside one cell (84, 70); queries in it, beside it and some metres away"""
    rng = np.random.default_rng(seed)
    S = Scene()
    xy = (20.5, 6.5); pred = 30
    zc = z_of(np.hypot(*xy), pred)
    for k in range(40):
        S.point(np.array([xy[0], xy[1], zc]) + rng.uniform(-0.45, 0.45, 3), (0, 0, 0), pred + k // 8 - 2)
    for k in range(40):
        off = rng.uniform(-0.4, 0.4, 3) if k < 20 else rng.uniform(-1.0, 1.0, 3) * (1.5, 1.5, 0.3) if k < 32 else rng.uniform(-1.0, 1.0, 3) * (4.5, 4.5, 0.3)
        S.query(xy, pred + k % 5 - 2, tuple(off))
    return S.finish()


def border_cases():
    a = border_scene(False); b = border_scene(True)
    c = one_cell_scene(False, 600); d = one_cell_scene(True, 601)
    return {"borders": case("borders", "borders", a[0], a[1], b[0], b[1]), "one-cell": case("borders", "one-cell", c[0], c[1], d[0], d[1])}


# ------------------------------------------------------------------------------------------------ the cases
@functools.lru_cache(maxsize=None)
def cases():
    out = {}
    for fn in (model_cases, tie_cases, displaced_cases, vnm_cases, invalid_cases, far_cases, dense_cases, border_cases):
        out.update(fn())
    for name, c in out.items():
        assert c["name"] == name
    return out


NAMES = ("inside", "edges-delta", "edges-low", "edges-high", "bypass") + tuple(f"nearby-{nb}" for nb in NEARBY_VALUES) + \
        tuple(f"size-{n}" for n in SIZES) + ("ties", "ties-rounding", "displaced", "vnm", "invalid-ring200", "invalid-ahead", "far", "far-round2", "dense", "borders", "one-cell")
FAMILIES = ("inside", "edges", "bypass", "nearby", "sizes", "ties", "displaced", "vnm", "invalid", "far", "dense", "borders")
MONOTONE_FAMILIES = ("inside", "edges", "bypass", "nearby", "sizes", "ties", "displaced", "far", "dense", "borders")
ZERO_OK = ("nearby-0.5",)                               # the only case without any correspondence, by the rule itself: its window is ring rc alone


def family(name):
    return tuple(n for n in NAMES if cases()[n]["family"] == name)


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> (corner correspondences, plane correspondences, the corner queries' details, the plane queries' details)"""
    c = cases()[name]
    ec = np_associate(c["pose"], c["sharp"], c["corner"], False, c["nearby"], c["dmax"], detail=True)
    pc = np_associate(c["pose"], c["flat"], c["surf"], True, c["nearby"], c["dmax"], detail=True)
    return ec[:3], pc[:4], ec[3], pc[4]


def wrong_reference(name, wrong, loop=False):
    c = cases()[name]
    return (np_associate(c["pose"], c["sharp"], c["corner"], False, c["nearby"], c["dmax"], wrong=wrong, loop=loop),
            np_associate(c["pose"], c["flat"], c["surf"], True, c["nearby"], c["dmax"], wrong=wrong, loop=loop))
