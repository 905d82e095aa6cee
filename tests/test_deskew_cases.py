"""The numpy restatement of TransformToStart + TransformToEnd (tests/deskewcases.py) against itself, without a GPU: the f64
formulas against the same formulas in np.longdouble stay inside the cap the GPU test holds the kernel to -- f64 rounding errors near
1e-16 against an f32 spacing of 6e-8 put a value across an f32 rounding boundary about once in 1e8 coordinates --, and the closed
forms at the ends of the sweep."""
import numpy as np

import deskewcases as dc

assert np.finfo(np.longdouble).eps < np.finfo(np.float64).eps, "np.longdouble must be wider than f64 for this file to measure anything"


def test_restatement_against_longdouble_on_the_crafted_cases():
    pts = dc.points()
    assert len(pts) == len(dc.RINGS) * len(dc.RANGES) * len(dc.S_VALUES) * 6
    got, want = [], []
    for name, q, t in dc.poses():
        got.append(dc.deskew(pts, q, t)); want.append(dc.deskew(pts, q, t, np.longdouble))
        assert np.isfinite(got[-1]).all(), name
        d = dc.ulp_distance(got[-1][:, :3], want[-1][:, :3])
        assert d.max() <= 1, (name, int(d.max()))
    same, worst = dc.check_close(np.concatenate(got), np.concatenate(want), "crafted")
    print(f"crafted: {same:.6f} bit-identical, worst {worst} ulp")


def test_restatement_against_longdouble_on_random_points():
    rng = np.random.default_rng(17)
    pts = dc.random_points(20000, 3)
    got, want = [], []
    for k in range(4):                                    # 4 poses x 5000 points: rotations up to ~0.2 rad, one with q.w < 0
        axis = rng.normal(size=3); axis /= np.linalg.norm(axis)
        ang = rng.uniform(0.01, 0.2)
        q = np.concatenate([np.sin(ang / 2) * axis, [np.cos(ang / 2)]]) * (-1.0 if k == 3 else 1.0)
        t = rng.normal(size=3) * [1.0, 0.2, 0.05]
        p = pts[5000 * k:5000 * (k + 1)]
        got.append(dc.deskew(p, q, t)); want.append(dc.deskew(p, q, t, np.longdouble))
    same, worst = dc.check_close(np.concatenate(got), np.concatenate(want), "random")
    print(f"random: {same:.6f} bit-identical, worst {worst} ulp")


def test_the_s_values_the_crafted_cloud_holds():
    pts = dc.points()
    s = dc.point_s(pts)
    ring0 = pts[:, 3] < 1.0
    for want in dc.S_VALUES:                              # beside ring id 0 every fraction survives the f32 store
        assert np.isclose(s[ring0], want, rtol=1e-6, atol=1e-12).any(), want
    assert (np.trunc(pts[~ring0, 3]) == 15).all() and (s[~ring0] >= 0).all() and s[~ring0].max() < 1.0001
    assert {round(float(np.linalg.norm(p[:3])), 3) for p in pts} == {0.5, 100.0}


def test_start_of_the_sweep_is_the_inverse_pose():
    """s = 0: slerp gives the identity and un = p exactly, so end = q^-1 (p - t)"""
    pts = dc.points()
    pts = pts[dc.point_s(pts) == 0.0]
    assert len(pts) >= 24
    for name, q, t in dc.poses():
        q = np.asarray(q, np.float64)
        want = dc.transform_vector(dc.inverse(q), pts[:, :3].astype(np.float64) - t).astype(np.float32)
        got = dc.deskew(pts, q, t)
        assert got[:, :3].tobytes() == want.tobytes(), name


def test_end_of_the_sweep_stays_where_it_is():
    """s -> 1, unit q: un -> q p + t and end -> p.  What separates end from p: the f32 store of un (half a spacing per coordinate at
    |un| <= |p| + |t|; a rotation keeps its length) and of end, and the (1 - s) of the sweep left: |1 - s| (theta |p| + |t|)."""
    pts = dc.points()
    s = dc.point_s(pts)
    pts, s = pts[np.abs(s - 1.0) < 1e-4], s[np.abs(s - 1.0) < 1e-4]
    assert len(pts) >= 12
    for name, q, t in dc.poses():
        if name.startswith("norm1.01"):
            continue                                      # not a rotation: q^-1 (q p) is p only for a unit q
        got = dc.deskew(pts, q, t).astype(np.float64)
        p = pts[:, :3].astype(np.float64)
        theta = 2.0 * np.arccos(min(1.0, abs(q[3])))
        reach = np.linalg.norm(p, axis=1) + np.linalg.norm(t)
        bound = 2.0 * np.sqrt(3.0) * np.spacing(reach.astype(np.float32)) + 1.01 * np.abs(1.0 - s) * (theta * np.linalg.norm(p, axis=1) + np.linalg.norm(t))
        err = np.linalg.norm(got[:, :3] - p, axis=1)
        assert (err <= bound).all(), (name, float((err / bound).max()))


def test_intensity_becomes_the_ring_id():
    pts = np.concatenate([dc.points(), dc.random_points(500, 9)])
    out = dc.deskew(pts, *dc.poses()[0][1:])
    assert out[:, 3].tobytes() == pts[:, 3].astype(np.int32).astype(np.float32).tobytes()
    assert set(np.unique(out[:, 3])) <= set(range(16))
