"""tests/rebuildcases.py's expected_insert -- the numpy restatement the GPU tests of ll_cubemaps_insert_keyframes compare against --
checked against its own invariants, with the CPU oracle only (no GPU, no library under test)."""
import numpy as np

import rebuildcases as rc
from rebuildcases import EMPTY, IDENT, LEAF, W, H, expected_insert, yaw_pose


def pt(x, y, z, i=0.0):
    return np.array([[x, y, z, i]], np.float32)


def test_identity_into_an_empty_map_is_binning_and_voxel_grid(orc):
    rng = np.random.default_rng(1)
    f = rc.frame(rng, 800, 1200, half=(60.0, 40.0, 10.0))
    want, added, dropped = expected_insert(orc, {}, (10, 10, 5), [f], [IDENT])
    assert added == [800, 1200] and dropped == [0, 0]
    for w in (0, 1):
        c = rc.cubes_of(f[w], (10, 10, 5))
        assert len(np.unique(c)) >= 4
        for cube in np.unique(c):
            exp = orc.voxel_grid(f[w][c == cube], LEAF[w])                         # the identity keeps every coordinate's bits
            assert want[(w, int(cube))].tobytes() == exp.tobytes()
        assert {k[1] for k in want if k[0] == w} == set(np.unique(c).tolist())


def test_points_on_the_negative_side_get_the_decrement(orc):
    """x + 25 = -0.5 truncates to 0 and must land one cube lower (:2112-2114); the same on y and z"""
    cen = (10, 10, 5)
    mid = 10 + W * 10 + W * H * 5
    cases = [(pt(-25.5, 0, 0), mid - 1), (pt(-24.5, 0, 0), mid), (pt(0, -25.5, 0), mid - W), (pt(0, 0, -25.5), mid - W * H),
             (pt(-75.5, -75.5, -75.5), mid - 2 - 2 * W - 2 * W * H), (pt(24.9, 24.9, 24.9), mid), (pt(25.1, 0, 0), mid + 1)]
    for p, cube in cases:
        want, added, dropped = expected_insert(orc, {}, cen, [(p, EMPTY)], [IDENT])
        assert list(want) == [(0, cube)] and added == [1, 0] and dropped == [0, 0], (p, cube, list(want))


def test_points_outside_the_array_are_dropped_and_counted(orc):
    """centre (10, 10, 5): x in [-525, 525), z in [-275, 275); a translation pushes part of a cloud over the edge"""
    cloud = np.concatenate([pt(524.0, 0, 0), pt(526.0, 0, 0), pt(-524.0, 0, 0), pt(-526.0, 0, 0), pt(0, 0, 276.0), pt(0, 0, -274.0)])
    want, added, dropped = expected_insert(orc, {}, (10, 10, 5), [(cloud, cloud[:2])], [IDENT])
    assert added == [3, 1] and dropped == [3, 1]
    assert sum(len(v) for k, v in want.items() if k[0] == 0) == 3
    want, added, dropped = expected_insert(orc, {}, (10, 10, 5), [(cloud, EMPTY)], [yaw_pose(0.0, (10.0, 0.0, 0.0))])
    assert added == [3, 0] and dropped == [3, 0]                                    # 534 and 536 out, -514 and -516 in
    want, added, dropped = expected_insert(orc, {}, (9, 10, 5), [(cloud, EMPTY)], [IDENT])
    assert added == [3, 0] and dropped == [3, 0]                                    # the centre moves the array: x in [-475, 575)
    assert sorted(float(v[0, 0]) for v in want.values()) == [0.0, 524.0, 526.0]


def test_a_repeated_frame_contributes_twice(orc):
    rng = np.random.default_rng(2)
    f = rc.frame(rng, 40, 60, half=(3.0, 3.0, 1.0))
    P = yaw_pose(12.0, (1.0, 2.0, 0.0))
    once = expected_insert(orc, {}, (10, 10, 5), [f], [P])
    twice = expected_insert(orc, {}, (10, 10, 5), [f, f], [P, P])
    assert twice[1] == [2 * a for a in once[1]]
    doubled = (np.concatenate([f[0], f[0]]), np.concatenate([f[1], f[1]]))
    assert {k: v.tobytes() for k, v in twice[0].items()} == {k: v.tobytes() for k, v in expected_insert(orc, {}, (10, 10, 5), [doubled], [P])[0].items()}
    # centroids of doubled voxels are those of the single ones up to rounding; the counts per cube are the same
    assert {k: len(v) for k, v in twice[0].items()} == {k: len(v) for k, v in once[0].items()}


def test_the_list_order_decides_the_order_of_the_filter_input(orc, monkeypatch):
    """the filter input of a cube is the old cloud, then the listed frames' points in LIST order: recorded by a stand-in filter"""
    rng = np.random.default_rng(3)
    a, b = rc.frame(rng, 30, 0, half=(3.0, 3.0, 1.0)), rc.frame(rng, 20, 0, half=(3.0, 3.0, 1.0))
    old = rc.box(rng, 10, (-3.0, -3.0, -1.0), (3.0, 3.0, 1.0))
    mid = 10 + W * 10 + W * H * 5
    seen = []
    monkeypatch.setattr(orc, "voxel_grid", lambda cloud, leaf: (seen.append(cloud.copy()), cloud)[1])
    expected_insert(orc, {(0, mid): old}, (10, 10, 5), [a, b], [IDENT, IDENT])
    expected_insert(orc, {(0, mid): old}, (10, 10, 5), [b, a], [IDENT, IDENT])
    assert seen[0].tobytes() == np.concatenate([old, a[0], b[0]]).tobytes()
    assert seen[1].tobytes() == np.concatenate([old, b[0], a[0]]).tobytes()
    assert seen[0].tobytes() != seen[1].tobytes()


def test_scenes_are_what_they_claim(orc):
    frames, poses, cen = rc.moved_centre_scene(2)
    want, added, dropped = expected_insert(orc, {}, cen, frames, poses)
    for w in (0, 1):
        assert dropped[w] > 200 and added[w] > 500 and added[w] + dropped[w] == sum(len(f[w]) for f in frames)
    xs = np.concatenate([v[:, 0] for v in want.values()])
    assert (xs < -25.0).any() and (xs > -25.0).any() and (xs > 850.0).any() and not (xs >= 875.0).any()
    frames, poses = rc.spread_scene(5)
    want, _, _ = expected_insert(orc, {}, (10, 10, 5), frames, poses)
    assert len({c for w, c in want if w == 0}) > 8
    frames, poses = rc.one_cube_scene(6)
    want, _, _ = expected_insert(orc, {}, (10, 10, 5), frames, poses)
    assert {c for w, c in want} == {10 + W * 10 + W * H * 5}
    frames, poses, dst = rc.general_scene(1)
    pre = {}
    want, added, dropped = expected_insert(orc, {}, (10, 10, 5), frames, poses, pre)
    assert len({c for w, c in want if w == 0}) >= 4 and dropped == [0, 0]
