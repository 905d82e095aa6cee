"""TransformToStart + TransformToEnd (laserOdometry.cpp:77-114, DISTORTION 1) restated in numpy, independent of the library and of
the oracle, and the crafted inputs the deskew tests share.

Per point p = (x, y, z, intensity) and a frame pose q = (x, y, z, w), t -- used as given, never normalised:
    s   = (intensity - (float)(int)intensity) / 0.1          float subtraction, f64 division (:81-82)
    un  = Identity.slerp(s, q) * p + s * t                    f64, STORED TO f32 (:86-93)
    end = q.inverse() * ((double)un - t)                      f64, stored to f32 (:105-110)
    intensity = (float)(int)intensity                         (:113)
with Eigen 3.3's formulas: slerp = QuaternionBase::slerp (scale0 / scale1 from acos|d| and three sines, the linear branch at
|d| >= 1 - eps, scale1 negated for d < 0), inverse = conjugate / squaredNorm (the zero quaternion unless squaredNorm > 0),
q * v = _transformVector (uv = 2 u x v; v + w uv + u x uv).  `dt` is the type the f64 steps run in: np.float64 is the restatement,
np.longdouble the same formulas with more bits (tests/test_deskew_cases.py measures one against the other)."""
import numpy as np

EPS64 = float(np.finfo(np.float64).eps)          # NumTraits<double>::epsilon(): the branch is the f64 one in either type


def point_s(pts, dt=np.float64):
    w = np.ascontiguousarray(pts, np.float32).reshape(-1, 4)[:, 3]
    frac = w - w.astype(np.int32).astype(np.float32)    # f32 - f32, exact or rounded as the reference's float subtraction
    return frac.astype(dt) / dt(0.1)


def slerp_identity(s, q, dt=np.float64):
    """Identity.slerp(s, q) for an array of s: (n, 4) coefficients x, y, z, w"""
    q = np.asarray(q, dt)
    one = dt(1.0) - dt(EPS64)
    d = q[3]
    absd = abs(d)
    if absd >= one:
        scale0 = dt(1.0) - s; scale1 = s.copy()
    else:
        theta = np.arccos(absd); sin_t = np.sin(theta)
        scale0 = np.sin((dt(1.0) - s) * theta) / sin_t
        scale1 = np.sin(s * theta) / sin_t
    if d < 0:
        scale1 = -scale1
    return np.stack([scale1 * q[0], scale1 * q[1], scale1 * q[2], scale0 + scale1 * q[3]], axis=1)


def transform_vector(q, v):
    """Eigen's _transformVector; q (4,) or (n, 4), v (n, 3)"""
    q = np.atleast_2d(q)
    u, w = q[:, :3], q[:, 3:4]
    uv = np.cross(u, v); uv = uv + uv
    return v + w * uv + np.cross(u, uv)


def inverse(q, dt=np.float64):
    q = np.asarray(q, dt)
    n2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]
    if not n2 > 0:
        return np.zeros(4, dt)
    return np.array([-q[0] / n2, -q[1] / n2, -q[2] / n2, q[3] / n2], dt)


def to_start(pts, q, t, dt=np.float64):
    """un as the reference stores it: (n, 3) float32"""
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 4)
    s = point_s(pts, dt)
    t = np.asarray(t, dt)
    un = transform_vector(slerp_identity(s, q, dt), pts[:, :3].astype(dt)) + s[:, None] * t
    return un.astype(np.float32)


def deskew(pts, q, t, dt=np.float64):
    """TransformToEnd of every point: (n, 4) float32"""
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 4)
    if len(pts) == 0:
        return pts.copy()
    t = np.asarray(t, dt)
    un = to_start(pts, q, t, dt)
    end = transform_vector(inverse(q, dt), un.astype(dt) - t)
    out = np.empty_like(pts)
    out[:, :3] = end.astype(np.float32)
    out[:, 3] = pts[:, 3].astype(np.int32).astype(np.float32)      # (float)(int): -0.05 becomes +0, not the -0 of trunc
    return out


def ulp_distance(a, b):
    """per value: how many representable f32 lie between a and b (0 = the same bits, 1 = adjacent); NaN anywhere = a large number"""
    a = np.ascontiguousarray(a, np.float32); b = np.ascontiguousarray(b, np.float32)
    def key(x):
        i = x.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    d = np.abs(key(a) - key(b))
    return np.where(np.isnan(a) | np.isnan(b), 1 << 40, d)


def check_close(got, want, what):
    """the cap every deskew comparison uses: each f32 coordinate equal or adjacent, at least 99.9 % of them the same bits; the
    intensities exact.  Returns (share of identical coordinates, largest distance) for the caller to print."""
    got = np.ascontiguousarray(got, np.float32).reshape(-1, 4); want = np.ascontiguousarray(want, np.float32).reshape(-1, 4)
    assert got.shape == want.shape, f"{what}: {got.shape} vs {want.shape}"
    bad = np.flatnonzero(got[:, 3].view(np.uint32) != want[:, 3].view(np.uint32))
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(got)} intensities differ, first at row {bad[0]}: {got[bad[0]]!r} vs {want[bad[0]]!r}"
    if len(got) == 0:
        return 1.0, 0
    d = ulp_distance(got[:, :3], want[:, :3])
    same = float((d == 0).mean())
    assert d.max() <= 1, f"{what}: a coordinate is {int(d.max())} f32 apart (row {int(np.argmax(d.max(axis=1)))})"
    assert same >= 0.999, f"{what}: only {same:.5f} of the coordinates are bit-identical"
    return same, int(d.max())


# ---- the crafted cases
S_VALUES = (0.0, 1e-6, 0.5, 0.999999)
RANGES = (0.5, 100.0)
RINGS = (0, 15)


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def poses():
    """(name, q, t): slerp's sign branch, its linear branch (the identity, and |q.w| one step below 1 with q.w >= 1 - eps), a
    rotation well inside the trigonometric branch, a non-unit q; t of 1 m and of 0"""
    qa = _unit([0.02, -0.035, 0.06, 1.0])
    near = np.array([1e-9, -2e-9, 0.0, 1.0 - EPS64 / 2])       # |q.w| = the largest double below 1: >= 1 - eps, the linear branch
    out = []
    # 1 m along a direction without short binary fractions: with t = (0.8, 0.6, 0) and s = f32(0.05) / 0.1 the sum p + s t of the
    # linear branch falls, in exact arithmetic, ON the middle between two f32 for every fourth point (s t is then an odd multiple of
    # 2^-27), and which way such a tie goes is decided by the last bit of an f64 product -- nothing the cap is meant to measure
    t1 = _unit([0.8, 0.57, -0.13])
    for tname, t in (("t1m", t1), ("t0", np.zeros(3))):
        out += [("rot_" + tname, qa, t), ("wneg_" + tname, -qa, t), ("identity_" + tname, np.array([0.0, 0.0, 0.0, 1.0]), t),
                ("linear_" + tname, near, t), ("norm1.01_" + tname, qa * 1.01, t),
                ("big_" + tname, _unit([0.3, -0.2, 0.5, 0.7]), t)]
    return out


def points(seed=5):
    """one cloud, ring-sorted as the registration node publishes: for ring ids 0 and 15, ranges 0.5 m and 100 m, every intensity
    fraction 0.1 * s of S_VALUES as f32 can hold it beside the ring id (beside 15 the fractions 1e-7 and 0.0999999 round to 0 and
    0.1: s = 0 and s just above 1 -- what a real cloud's last firing also does), in a handful of directions"""
    rng = np.random.default_rng(seed)
    rows = []
    for ring in RINGS:
        for rg in RANGES:
            for s in S_VALUES:
                for _ in range(6):
                    d = _unit(rng.normal(size=3) * [1.0, 1.0, 0.2])
                    rows.append(list(d * rg) + [np.float32(ring) + np.float32(0.1 * s)])
    return np.array(rows, np.float32)


def random_points(n, seed):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3)) * [1.0, 1.0, 0.2]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rg = np.exp(rng.uniform(np.log(0.5), np.log(100.0), n))
    inten = rng.integers(0, 16, n).astype(np.float32) + (0.1 * rng.uniform(0.0, 1.0, n)).astype(np.float32)
    return np.concatenate([d * rg[:, None], inten[:, None]], axis=1).astype(np.float32)
