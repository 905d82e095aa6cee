"""The numpy restatement of ll_entropy (tests/entropycases.py) on inputs whose answer is known, without a GPU: a sampled plane, a ball,
the crafted inputs sitting where they claim, and the street scene of tests/viscases.py under growing drift."""
import numpy as np

import entropycases as ec


def test_plane_of_known_thickness():
    rng = np.random.default_rng(1)
    c = ec.cfg()
    sigma = 0.02
    p = ec.plane_cloud(rng, 6000, sigma)
    mom = ec.np_moments(p.astype(np.float32), c)
    core = (np.abs(p[:, 0]) < 0.4) & (np.abs(p[:, 1]) < 0.4)          # whole neighbourhoods, away from the patch's rim
    assert core.sum() > 500 and mom["nn"][core].min() > 300
    l0 = mom["lam"][core, 0]
    assert abs(l0.mean() / sigma ** 2 - 1.0) < 0.05                   # the sample variance of ~1000 draws, averaged over ~1000 points
    # in the plane a disc of radius r has variance r^2 / 4 per axis
    assert np.allclose(mom["lam"][core, 1:].mean(axis=0), 0.25 * 0.25, rtol=0.1)
    h, pv, _ = ec.np_values(mom, c)
    assert np.allclose(pv[core], l0) and np.isfinite(h[core]).all()


def test_ball_is_isotropic():
    rng = np.random.default_rng(2)
    c = ec.cfg()
    p = ec.ball_cloud(rng, 4000, 0.25)                                # every point sees the whole ball: variance R^2 / 5 per axis
    mom = ec.np_moments(p.astype(np.float32), c)
    assert (mom["nn"] == 4000).all()
    lam = mom["lam"][0]
    assert np.allclose(lam, 0.25 ** 2 / 5.0, rtol=0.08) and lam[2] / lam[0] < 1.15


def test_crafted_inputs_sit_where_they_claim():
    c = ec.cfg()
    r = c["radius"]
    # distance radius is a neighbour, one step beyond is not
    w = np.array([[0, 0, 0], [r, 0, 0], [0, np.nextafter(r, np.float32(1)), 0]], np.float32)
    assert ec.np_moments(w, c)["nn"].tolist() == [2, 2, 1]
    nn = ec.np_moments(ec.edge_pairs(c).astype(np.float32), c)["nn"]
    assert len(set(nn.tolist())) > 3                                    # the steps about the radius do change the counts
    # the range's end: 65536 cell has no cell, the float below it has one
    edge = np.float32(ec.HALF) * c["cell"]
    out = ec.np_outside(np.array([[edge, 0, 0], [np.nextafter(edge, np.float32(0)), 0, 0], [0, -edge, 0], [0, 0, np.nextafter(-edge, np.float32(-1e9))]], np.float32), c)
    assert out.tolist() == [True, False, False, True]
    assert ec.np_outside(ec.BAD_POINTS.astype(np.float32), c).all()
    re = ec.range_edge(c).astype(np.float32)
    o = ec.np_outside(re, c)
    assert 0 < o.sum() < len(re)
    mom = ec.np_moments(re, c)
    assert (mom["nn"][o] == 0).all() and (mom["nn"][~o] >= 1).all() and mom["nn"].max() < (~o).sum()
    # cells of 1, 63, 64, 65 and 300 points, each cluster in one cell and alone
    pts, sizes = ec.cell_clusters(c)
    cells = np.floor(pts.astype(np.float32) / c["cell"]).astype(np.int64)
    at = 0
    for m in sizes:
        assert len(np.unique(cells[at:at + m], axis=0)) == 1
        at += m
    assert sizes[-1] > ec.CHUNK                                         # a neighbourhood longer than one LDS staging chunk
    nn = ec.np_moments(pts.astype(np.float32), c)["nn"]
    assert nn.tolist() == sum(([m] * m for m in sizes), [])
    # min_neighbours - 1 and min_neighbours
    nn = ec.np_moments(ec.min_edge_clusters(c).astype(np.float32), c)["nn"]
    m = c["min_neighbours"]
    assert nn.tolist() == [m - 1] * (m - 1) + [m] * m
    # exactly planar, exactly collinear: the smallest eigenvalue is zero up to rounding, h is finite through the floor
    for cloud, zeros in zip(ec.flat_and_line(), (1, 2)):
        mom = ec.np_moments(cloud.astype(np.float32), c)
        h, pv, _ = ec.np_values(mom, c)
        assert (mom["nn"] >= m).all() and np.abs(mom["lam"][:, :zeros]).max() < 1e-15 and np.isfinite(h).all() and (pv < 1e-15).all()
    # the faces: the points about a corner lie in the eight cells that meet there, the point on a face in the upper one
    fp = ec.face_points(c).astype(np.float32)
    assert len(fp) == 4 * 343
    for j, k in enumerate((-1, 0, 1, 2)):
        cells = np.floor(fp[343 * j:343 * (j + 1)] / c["cell"])
        assert len(np.unique(cells, axis=0)) == 8 and set(np.unique(cells).tolist()) == {k - 1, k}
        on = fp[343 * j:343 * (j + 1)] == np.float32(k) * c["cell"]
        assert on.all(axis=1).sum() == 1 and (cells[on.all(axis=1)] == k).all()


def test_street_scene_crispness_grows_with_drift():
    frames, poses, ops = ec.street()
    recs = [o["rec"] for o in ops]
    n = sum(len(a) + len(b) for a, b in frames)
    print([(r["mme"], r["mpv"], r["n_valid"]) for r in recs])
    for r in recs:
        assert r["n_points"] == n == r["n_valid"] + r["n_sparse"] + r["n_outside"] and r["n_outside"] == 0
        assert r["n_valid"] >= 0.95 * r["n_points"]                    # a mean over a remnant cannot pass
    assert recs[0]["mme"] < recs[1]["mme"] < recs[2]["mme"]
    assert recs[0]["mpv"] < recs[1]["mpv"] < recs[2]["mpv"]
