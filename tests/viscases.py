"""An independent numpy restatement of ll_visibility (include/lightloam_hip.h) and the inputs of its tests.

np_pixel / np_images are the range image in float32 numpy, operation by operation as the header states it; angles come from the host
atan2f (oracle.orc.libm), to which tests/test_exact_math.py pins ll_atan2f.  np_to_world / np_to_frame are the two transforms in
float64 with the header's operation order, each coordinate rounded to float once.  np_vote is the vote, np_removed the rule.  No
expected value of any test comes from the library.  tests/test_vis_cases.py checks, without a GPU, that the crafted inputs sit where
they claim and what the default parameters do on the street scene.
"""
import numpy as np

F = np.float32
TWO_PI_F = F(6.2831855)
INF = F(np.inf)
DEFAULTS = dict(width=360, height=90, el_min_deg=-45.0, el_max_deg=45.0, min_range=1.0, max_range=120.0, margin_abs=0.5, margin_rel=0.02,
                radius=40.0)
DEFAULT_RULE = (2, 255)
IDENTITY = np.array([0, 0, 0, 1, 0, 0, 0], np.float64)


def cfg(**kw):
    """the parameters as the library holds them (floats) and the derived constants ka, ke, el_min"""
    c = dict(DEFAULTS); c.update(kw)
    for k in ("el_min_deg", "el_max_deg", "min_range", "max_range", "margin_abs", "margin_rel", "radius"):
        c[k] = F(c[k])
    rad = np.pi / 180.0
    c["el_min"] = F(np.float64(c["el_min_deg"]) * rad)
    c["ka"] = F(np.float64(c["width"]) / (2.0 * np.pi))
    c["ke"] = F(np.float64(c["height"]) / ((np.float64(c["el_max_deg"]) - np.float64(c["el_min_deg"])) * rad))
    return c


def lib_params(c):
    """the keyword arguments of Context.visibility for cfg c"""
    return {k: (int(c[k]) if k in ("width", "height") else float(c[k])) for k in DEFAULTS}


def np_pixel(p, c):
    """points (n, >= 3) float32 in a sensor frame -> (pix (n,) int64, row * width + col or -1 for no pixel, r (n,) float32)"""
    from oracle import orc
    p = np.asarray(p, F)
    p = p.reshape(-1, p.shape[-1] if p.ndim == 2 else 3)
    n = len(p)
    pix = np.full(n, -1, np.int64)
    if n == 0:
        return pix, np.zeros(0, F)
    x, y, z = (np.ascontiguousarray(p[:, k]) for k in range(3))
    with np.errstate(all="ignore"):
        xy2 = x * x + y * y                                          # float32 throughout: every product and sum rounded
        r = np.sqrt(xy2 + z * z)
        ok = (r >= c["min_range"]) & (r < c["max_range"])            # a NaN fails
        a = orc.libm(1, y, x)
        a = np.where(a < 0, a + TWO_PI_F, a).astype(F)
        col = np.minimum(c["width"] - 1, np.where(ok, a * c["ka"], F(0)).astype(np.int32))
        e = orc.libm(1, z, np.sqrt(xy2))
        fr = np.floor((e - c["el_min"]) * c["ke"])
        ok &= (fr >= 0) & (fr < c["height"])
        row = np.where(ok, fr, F(0)).astype(np.int32)
    pix[ok] = row[ok].astype(np.int64) * c["width"] + col[ok]
    return pix, r.astype(F)


def np_images(corner, surf, c):
    """(raw, img) [height][width] float32 of a frame with the two clouds; +inf: empty"""
    W, H = c["width"], c["height"]
    raw = np.full(W * H, INF, F)
    for cloud in (corner, surf):
        pix, r = np_pixel(np.asarray(cloud, F).reshape(-1, 4)[:, :3], c)
        np.minimum.at(raw, pix[pix >= 0], r[pix >= 0])
    raw = raw.reshape(H, W)
    img = np.full((H, W), INF, F)
    for dr in (-1, 0, 1):
        lo, hi = max(0, -dr), min(H, H - dr)                         # rows outside the image are left out
        for dc in (-1, 0, 1):
            img[lo:hi] = np.minimum(img[lo:hi], np.roll(raw, -dc, axis=1)[lo + dr:hi + dr])   # columns wrap
    return raw, img


def _rot(u, w, v):
    """v + w * 2 (u x v) + u x (2 (u x v)) in float64, the products and sums in ll_map_to_world's order"""
    ux, uy, uz = u
    v0, v1, v2 = v
    uvx = uy * v2 - uz * v1; uvy = uz * v0 - ux * v2; uvz = ux * v1 - uy * v0
    uvx = uvx + uvx; uvy = uvy + uvy; uvz = uvz + uvz
    return ((v0 + w * uvx) + (uy * uvz - uz * uvy), (v1 + w * uvy) + (uz * uvx - ux * uvz), (v2 + w * uvz) + (ux * uvy - uy * uvx))


def np_to_world(pose, p):
    """pointAssociateToMap: points (n, 3) float32 of a sensor frame -> world, float32, the pose (qx, qy, qz, qw, tx, ty, tz) as given"""
    P = np.asarray(pose, np.float64)
    v = np.asarray(p, F)[:, :3].astype(np.float64)
    with np.errstate(all="ignore"):
        s = _rot(P[0:3], P[3], (v[:, 0], v[:, 1], v[:, 2]))
        return np.stack([(s[k] + P[4 + k]).astype(F) for k in range(3)], axis=1)


def np_to_frame(pose, w):
    """R(q)^-1 (w - t): world points (n, 3) float32 -> the frame of `pose`, float32; the conjugate quaternion, the pose as given"""
    P = np.asarray(pose, np.float64)
    w = np.asarray(w, F).astype(np.float64)
    with np.errstate(all="ignore"):
        v = (w[:, 0] - P[4], w[:, 1] - P[5], w[:, 2] - P[6])
        s = _rot(-P[0:3], P[3], v)
        return np.stack([s[k].astype(F) for k in range(3)], axis=1)


def np_observers(poses, radius):
    """per list position the positions of its observers, ascending: another frame within radius (float64, squares summed left to right)"""
    t = np.asarray(poses, np.float64).reshape(-1, 7)[:, 4:]
    r2 = np.float64(F(radius)) * np.float64(F(radius))
    out = []
    for a in range(len(t)):
        d = t[a] - t
        d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
        out.append([b for b in range(len(t)) if b != a and d2[b] <= r2])
    return out


def np_vote(frames, poses, c):
    """frames: a list of (corner (n, 4), surf (m, 4)) float32, one drive; poses [n_frames][7] -> (per frame (corner counts (n, 2),
    surf counts (m, 2)) uint8: through, hit, saturating at 255;  the ordered frame pairs)"""
    poses = np.asarray(poses, np.float64).reshape(-1, 7)
    imgs = [np_images(co, su, c)[1].reshape(-1) for co, su in frames]
    obs = np_observers(poses, c["radius"])
    out = []
    for a, (co, su) in enumerate(frames):
        pts = np.concatenate([np.asarray(co, F).reshape(-1, 4), np.asarray(su, F).reshape(-1, 4)])[:, :3]
        through = np.zeros(len(pts), np.int64); hit = np.zeros(len(pts), np.int64)
        w = np_to_world(poses[a], pts)
        for b in obs[a]:
            pix, r = np_pixel(np_to_frame(poses[b], w), c)
            ok = pix >= 0
            d = np.where(ok, imgs[b][np.where(ok, pix, 0)], INF)
            ok &= d != INF
            with np.errstate(all="ignore"):
                m = c["margin_abs"] + c["margin_rel"] * r
                far = r + m; near = r - m
                through += ok & (d > far)
                hit += ok & (d >= near) & (d <= far)
        cnt = np.stack([np.minimum(through, 255), np.minimum(hit, 255)], axis=1).astype(np.uint8)
        n = len(np.asarray(co, F).reshape(-1, 4))
        out.append((cnt[:n], cnt[n:]))
    return out, sum(len(o) for o in obs)


def np_removed(cnt, rule=DEFAULT_RULE):
    """counts (n, 2) uint8 -> (n,) bool: through >= min_through and hit <= max_hit"""
    cnt = np.asarray(cnt).reshape(-1, 2).astype(np.int64)
    return (cnt[:, 0] >= rule[0]) & (cnt[:, 1] <= rule[1])


# ---------------------------------------------------------------------------------------------- crafted inputs
def pts4(xyz):
    """(n, 3) -> (n, 4) float32 clouds with the index as intensity"""
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    return np.concatenate([xyz, np.arange(len(xyz), dtype=F)[:, None]], axis=1)


def _first_float(lo, hi, pred):
    """the first float32 f in (lo, hi] with pred(f), pred monotone false -> true over the interval (bisection over the bits)"""
    lo, hi = F(lo), F(hi)
    assert 0 < lo < hi and not pred(lo) and pred(hi)
    a, b = int(lo.view(np.uint32)), int(hi.view(np.uint32))
    while b - a > 1:
        mid = (a + b) // 2
        if pred(np.uint32(mid).view(F)):
            b = mid
        else:
            a = mid
    return np.uint32(a).view(F), np.uint32(b).view(F)


def column_edge(c, col, r=10.0):
    """two points at range ~r whose y differ by one ulp: one in column col - 1, the next float in column col (0 < col < width / 4)"""
    th = col * 2.0 * np.pi / c["width"]
    x = F(r * np.cos(th)); y0 = r * np.sin(th)
    col_of = lambda y: int(np_pixel([[x, y, F(0.3)]], c)[0][0]) % c["width"]                   # noqa: E731
    below, at = _first_float(y0 * 0.999, y0 * 1.001, lambda y: col_of(y) >= col)
    return [x, below, F(0.3)], [x, at, F(0.3)]


def row_edge(c, row, r=10.0):
    """two points whose z differ by one ulp: one in row row - 1, the next float in row row (a row above the horizon)"""
    el = np.float64(c["el_min"]) + row / np.float64(c["ke"])
    assert el > 0.01
    x = F(r * np.cos(el) * np.cos(0.3)); y = F(r * np.cos(el) * np.sin(0.3)); z0 = r * np.sin(el)
    row_of = lambda z: int(np_pixel([[x, y, z]], c)[0][0]) // c["width"]                       # noqa: E731
    below, at = _first_float(z0 * 0.999, z0 * 1.001, lambda z: row_of(z) >= row)
    return [x, y, below], [x, y, at]


def image_cases(c):
    """name -> (corner (n, 4), surf (m, 4)) float32: the clouds of one frame each"""
    W, H = c["width"], c["height"]
    rmax = c["max_range"]; rmin = c["min_range"]
    cases = {}
    edge = []
    for col in sorted({1, W // 8, 3 * W // 16}):
        edge += column_edge(c, col)
    for row in sorted({H // 2 + 1, H - 1}):
        edge += row_edge(c, row)
    cases["pixel_edges"] = (pts4(edge[0::2]), pts4(edge[1::2]))
    # azimuth just below 2 pi (a barely negative angle becomes 6.2831855f, and 6.2831855f * ka is width or more: the clamp) and just above 0
    wrap = [[10, -1e-30, 1], [30, -1e-7, 2], [50, -1e-20, -3], [12, 1e-30, 1], [31, 1e-7, 2], [9, -0.01, 0.5], [9, 0.01, 0.5], [-10, 0.0, 1], [-10, -0.0, 1]]
    cases["wrap_column"] = (pts4(wrap[:5]), pts4(wrap[5:]))
    up = np.tan(np.radians(float(c["el_max_deg"]) + 0.5)); dn = np.tan(np.radians(float(c["el_min_deg"]) - 0.5))
    out = [[10, 0, 10 * up], [10, 3, 11 * dn], [0, 0, 5], [0, 0, -5], [0.0, -0.0, 20],                                   # elevation window
           [rmax, 0, 0], [0, np.nextafter(rmax, F(0)), 0], [0, 0.5 * rmin, 0.2 * rmin], [np.nextafter(rmin, F(0)), 0, 0], [0, -rmin, 0],
           [3 * rmax, 1, 1], [np.inf, 1, 1], [1, -np.inf, 1],                                                             # range window
           [np.nan, 1, 1], [1, np.nan, 1], [1, 1, np.nan], [np.nan, np.nan, np.nan], [7, 7, 1]]                            # NaN; one plain point
    cases["windows_and_nan"] = (pts4(out[:9]), pts4(out[9:]))
    cases["no_corner"] = (pts4(np.zeros((0, 3))), pts4([[5, 5, 0.5], [-8, 2, 1]]))
    cases["no_surf"] = (pts4([[5, -5, 0.5], [2, 8, -1]]), pts4(np.zeros((0, 3))))
    cases["empty"] = (pts4(np.zeros((0, 3))), pts4(np.zeros((0, 3))))
    # both types in one pixel: the nearer one is the corner point in the first pair, the surf point in the second
    cases["both_types"] = (pts4([[6, 6, 1], [-14, 7, 2], [3, -9, 0.5]]), pts4([[9, 9, 1.5], [-8, 4, 8.0 / 7.0], [3, -9, 0.5]]))
    rng = np.random.default_rng(20261020)
    cases["random"] = (random_cloud(rng, 700), random_cloud(rng, 2300))        # more than one tile of a type, several points per pixel
    return cases


def random_cloud(rng, n, r_lo=1.5, r_hi=60.0):
    r = rng.uniform(r_lo, r_hi, n); az = rng.uniform(-np.pi, np.pi, n); el = rng.uniform(-0.6, 0.6, n)
    return pts4(np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el)], axis=1))


def quat(yaw, pitch, roll):
    cy, sy, cp, sp, cr, sr = np.cos(yaw / 2), np.sin(yaw / 2), np.cos(pitch / 2), np.sin(pitch / 2), np.cos(roll / 2), np.sin(roll / 2)
    return np.array([sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy])


def margin_case(c, r=20.0):
    """Two frames at the origin under the identity, so l == p.  Frame 0 (the subject) has four points at range r on the +x, +y, -x, -y
    axes; frame 1 (the observer) has one point per axis whose range is, in that order: the first float above r + m (seen through),
    r + m itself (hit), r - m itself (hit), the last float below r - m (occluded) -- plus one subject point at (0.6 r, 0.6 r, r / 3) whose
    pixel neighbourhood is empty in the observer, and one far behind a near observer point (occluded by a wide margin).
    -> (frames, poses, expect): expect[i] = (through, hit) of subject point i"""
    r = F(r)
    m = c["margin_abs"] + c["margin_rel"] * r
    far, near = r + m, r - m
    d = [np.nextafter(far, INF), far, near, np.nextafter(near, F(0))]
    ax = [(1, 0), (0, 1), (-1, 0), (0, -1)]
    sub = [[r * ux, r * uy, 0] for ux, uy in ax] + [[0.6 * r, 0.6 * r, r / 3], [-0.6 * r, 0.6 * r, -r / 3]]
    obs = [[d[i] * ux, d[i] * uy, 0] for i, (ux, uy) in enumerate(ax)] + [[-0.2 * r, 0.2 * r, -r / 9]]
    frames = [(pts4(sub[:3]), pts4(sub[3:])), (pts4(obs[:2]), pts4(obs[2:]))]
    expect = [(1, 0), (0, 1), (0, 1), (0, 0), (0, 0), (0, 0)]
    return frames, np.stack([IDENTITY, IDENTITY]), expect


def random_drive(seed=7, n_frames=6, n_points=300, spread=25.0, far=(4, 5)):
    """n_frames frames of about n_points random points under random poses (yaw, pitch, roll, translation); the frames `far` stand
    beyond the default radius from the first ones.  -> (frames, poses)"""
    rng = np.random.default_rng(seed)
    frames, poses = [], []
    for k in range(n_frames):
        n = n_points + int(rng.integers(-20, 20))
        nc = n // 5
        frames.append((random_cloud(rng, nc, 2.0, 50.0), random_cloud(rng, n - nc, 2.0, 50.0)))
        t = rng.uniform(-spread / 2, spread / 2, 3) * np.array([1, 1, 0.1])
        if k in far:
            t[0] += 45.0
        poses.append(np.concatenate([quat(rng.uniform(-np.pi, np.pi), rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2)), t]))
    return frames, np.array(poses)


# ---------------------------------------------------------------------------------------------- the street scene
STREET = dict(n_frames=12, step=4.0, sensor_z=1.8, wall_y=12.0, wall_h=8.0, end_lo=-10.0, end_hi=54.0, rings=64, el_lo=-24.8, el_hi=2.0,
              az_step=0.5, leaf=0.4, box_frame=3, box_centre=(21.0, -1.5, 0.75), box_size=(4.5, 1.8, 1.5))


def _cast(o, d, S, with_box):
    """rays from o along unit d (n, 3), float64 -> (t (n,), is_box (n,)); inf: no hit"""
    n = len(d)
    t = np.full(n, np.inf); box = np.zeros(n, bool)
    with np.errstate(all="ignore"):
        def plane(axis, value, ok):
            tt = (value - o[axis]) / d[:, axis]
            h = o + tt[:, None] * d
            good = (tt > 1e-6) & ok(h)
            return np.where(good, tt, np.inf)
        in_street = lambda h: (np.abs(h[:, 1]) <= S["wall_y"]) & (h[:, 0] >= S["end_lo"]) & (h[:, 0] <= S["end_hi"])        # noqa: E731
        t = np.minimum(t, plane(2, 0.0, in_street))
        for y in (-S["wall_y"], S["wall_y"]):
            t = np.minimum(t, plane(1, y, lambda h: (h[:, 2] >= 0) & (h[:, 2] <= S["wall_h"]) & (h[:, 0] >= S["end_lo"]) & (h[:, 0] <= S["end_hi"])))
        for x in (S["end_lo"], S["end_hi"]):
            t = np.minimum(t, plane(0, x, lambda h: (h[:, 2] >= 0) & (h[:, 2] <= S["wall_h"]) & (np.abs(h[:, 1]) <= S["wall_y"])))
        if with_box:
            lo = np.array(S["box_centre"]) - np.array(S["box_size"]) / 2; hi = np.array(S["box_centre"]) + np.array(S["box_size"]) / 2
            t0 = (lo - o) / d; t1 = (hi - o) / d
            tn = np.minimum(t0, t1).max(axis=1); tf = np.maximum(t0, t1).min(axis=1)
            hitb = (tn <= tf) & (tn > 1e-6) & (tn < t)
            t = np.where(hitb, tn, t); box = hitb
    return t, box


def _voxel(p, leaf):
    """one centroid per occupied leaf-sized voxel, in the order of the voxels' first points"""
    if len(p) == 0:
        return p.reshape(0, 3)
    key = np.floor(p / leaf).astype(np.int64)
    _, first, inv = np.unique(key, axis=0, return_index=True, return_inverse=True)
    inv = inv.reshape(-1)
    s = np.zeros((len(first), 3)); np.add.at(s, inv, p)
    cen = s / np.bincount(inv)[:, None]
    return cen[np.argsort(first)]


def street_scene(S=None):
    """-> (frames, poses, is_box): per frame (corner (n, 4), surf (m, 4)) float32 in the sensor frame, poses [12][7], per frame
    (corner (n,), surf (m,)) bool: the point comes from the box.  A ground plane, two side walls and two end walls, ray-cast from
    12 sensor poses 4 m apart with a 64-ring, 0.5 degree scan, each scan down-sized to one centroid per 0.4 m voxel (static and box
    returns apart, so that every point has one label); the box stands in the scan of frame 3 only.  Every fifth point goes to the
    corner cloud, the rest to the surf cloud: the test does not care which is which."""
    S = dict(STREET) if S is None else S
    el = np.radians(np.linspace(S["el_lo"], S["el_hi"], S["rings"]))
    az = np.radians(np.arange(0.0, 360.0, S["az_step"]))
    E, A = np.meshgrid(el, az, indexing="ij")
    d = np.stack([np.cos(E) * np.cos(A), np.cos(E) * np.sin(A), np.sin(E)], axis=-1).reshape(-1, 3)
    frames, poses, is_box = [], [], []
    for k in range(S["n_frames"]):
        o = np.array([k * S["step"], 0.0, S["sensor_z"]])
        t, box = _cast(o, d, S, k == S["box_frame"])
        ok = np.isfinite(t)
        local = t[:, None] * d                                       # the pose is a pure translation: sensor frame = world - o
        stat = _voxel(local[ok & ~box], S["leaf"]); bx = _voxel(local[ok & box], S["leaf"])
        pts = np.concatenate([stat, bx]); lab = np.concatenate([np.zeros(len(stat), bool), np.ones(len(bx), bool)])
        corner = np.arange(len(pts)) % 5 == 0
        frames.append((pts4(pts[corner]), pts4(pts[~corner])))
        is_box.append((lab[corner], lab[~corner]))
        poses.append(np.concatenate([[0, 0, 0, 1], o]))
    return frames, np.array(poses), is_box
