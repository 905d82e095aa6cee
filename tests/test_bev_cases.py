"""The numpy restatement of ll_bev (tests/bevcases.py) on its own, without a GPU and without the library: hand-computed tiny cases, that
the crafted inputs sit where they claim, and what the default parameters do on the yard scene -- every listed displacement is found
within one cell and one yaw step with score > second, and with the ground layer in (z_min = -3) the zero shift wins, which is why the
default z_min is -1."""
import math

import numpy as np
import pytest

import bevcases as bc

C = bc.cfg(**bc.SMALL)
CASES = bc.crafted_cases(C)


def test_one_hot_under_90_degrees_by_hand():
    """query (2.2, 0.3) turns to (-0.3, 2.2): cell (-1, 4); the target point (0.7, 3.3) is cell (1, 6): sx = sy = 2"""
    grid, vol, res = bc.np_match(CASES["one_hot_90"], C)
    h = C["half"]
    assert grid.sum() == 2 and grid[6 + h, 1 + h] == 1 << 1                                      # z = z_min + 1.5: layer 1, bit 1
    assert vol.sum() == 1 and vol[0, 2 + 4, 2 + 4] == 1
    assert (res["score"], res["second"], res["iyaw"], res["sx"], res["sy"], res["n_query"]) == (1, 0, 0, 2, 2, 1)
    assert res["yaw"] == math.pi / 2.0
    assert res["D"].tolist() == [0.0, 0.0, math.sin(math.pi / 4.0), math.cos(math.pi / 4.0), 1.0, 1.0, 0.0]


def test_one_hot_grid_bit():
    grid = bc.np_grid(np.array([[0.7, 3.3, -1.0 + 1.5]], np.float32), C)
    assert np.argwhere(grid).tolist() == [[6 + 16, 1 + 16]] and grid[22, 17] == 2


def test_layer_limits_by_hand():
    """layers -1 and 8 are dropped, 0 and 7 kept: cell (2, 2) holds bits 0 and 7, cell (-5, 0) nothing (z just below z_min, z_min + 8)"""
    grid, vol, res = bc.np_match(CASES["layer_limits"], C)
    assert np.argwhere(grid).tolist() == [[2 + 16, 2 + 16]] and grid[18, 18] == 0x81
    assert res["n_query"] == 2 and res["score"] == 2 and (res["sx"], res["sy"]) == (0, 0) and res["second"] == 0


def test_ties_go_to_the_lowest_flat_index():
    grid, vol, res = bc.np_match(CASES["tie_two_peaks"], C)
    assert np.argwhere(vol == 1).tolist() == [[0, 3, 6], [0, 6, 1], [1, 3, 6], [1, 6, 1]]        # (j, sy + 4, sx + 4): two shifts, two equal yaws
    assert (res["score"], res["iyaw"], res["sx"], res["sy"]) == (1, 0, 2, -1)
    assert res["second"] == 1                                                                      # the other peak lies outside the window
    _, vol0, res0 = bc.np_match(CASES["tie_all_zero"], C)
    assert vol0.sum() == 0 and (res0["score"], res0["second"], res0["iyaw"], res0["sx"], res0["sy"]) == (0, 0, 0, -4, -4)


def test_peaks_at_the_corners_and_the_window():
    _, vol, res = bc.np_match(CASES["peak_at_corner"], C)
    assert vol.sum() == 1 and vol[0, 7, 7] == 1 and (res["sx"], res["sy"], res["second"]) == (3, 3, 0)
    _, vol, res = bc.np_match(CASES["peak_at_first_corner"], C)
    assert vol[0, 0, 0] == 2 and vol[0, 4, 5] == 1 and (res["score"], res["sx"], res["sy"], res["second"]) == (2, -4, -4, 1)
    cw, case = bc.window_case()
    _, vol, res = bc.np_match(case, cw)
    assert res["second"] == -1 and res["score"] == vol.max() > 50


def test_empty_and_tiny_sides():
    for name in ("empty_query", "empty_target", "no_layer_at_all"):
        grid, vol, res = bc.np_match(CASES[name], C)
        assert vol.sum() == 0 and (res["score"], res["second"], res["iyaw"], res["sx"], res["sy"]) == (0, 0, 0, -4, -4), name
    assert bc.np_match(CASES["empty_query"], C)[2]["n_query"] == 0 and bc.np_match(CASES["empty_target"], C)[0].sum() == 0
    assert bc.np_match(CASES["no_layer_at_all"], C)[0].sum() == 0 and bc.np_match(CASES["no_layer_at_all"], C)[2]["n_query"] > 0
    _, vol, res = bc.np_match(CASES["one_point_query"], C)
    assert res["n_query"] == 1 and res["score"] == 1 and vol[1, 2 + 4, -1 + 4] == 1               # the point's own cell, a cell left and two up


def test_crafted_inputs_sit_where_they_claim():
    cell = float(C["cell"])
    e = np.concatenate(CASES["cell_edges_same"]["frames"][0])[:, :3]
    fx = np.floor(e[:, 0] * C["inv"])
    for k in (-3, -1, 0, 1, 2, 5):                                                                 # one ulp below k * cell is the cell before
        below, at, above = (np.float32(v) for v in bc._ulps(k * cell))
        got = {float(np.floor(v * C["inv"])) for v in (below, at, above)}
        assert got == {k - 1.0, float(k)} and (e[:, 0] == below).any() and (e[:, 0] == at).any() and (e[:, 1] == above).any()
    assert len(np.unique(fx)) >= 8
    lay = bc.np_layer(e, C)
    assert {-1, 0, 1, 3, 4, 6, 7} <= set(lay.tolist())
    ring = np.concatenate(CASES["square_edges"]["frames"][0])[:, :3]
    ix, iy, inside = bc.np_cell(ring[:, 0], ring[:, 1], C)
    assert (~inside).sum() >= 8 and {-16, 15} <= set(ix[inside].tolist()) and {-16, 15} <= set(iy[inside].tolist())
    bad = np.concatenate(CASES["bad_values"]["frames"][0])[:, :3]
    assert np.isnan(bad).any() and np.isposinf(bad).any() and np.isneginf(bad).any() and (np.abs(bad) == np.float32(1e30)).any()
    grid, vol, res = bc.np_match(CASES["bad_values"], C)
    plain = (np.abs(bad) < 100).all(axis=1)                                                       # NaN compares false
    assert plain.sum() == 40 and res["n_query"] == int((bc.np_layer(bad[plain], C) >= 0).sum()) + 3   # (1e30, 1, 0), (1, -1e30, 0), (3e38, 3e38, 0.5) have a layer
    for n in (1023, 1024, 1025, 2049):
        case = CASES[f"chunk_{n}"]
        assert sum(len(x) for x in case["frames"][1]) == n
        assert 0 < bc.np_match(case, C)[2]["n_query"] < n                                          # some points have no layer: -1 entries in the list
    assert CASES["max_yaws"]["n_yaws"] == C["max_yaws"] == 16
    m = CASES["multi_frame_stored"]
    assert m["target"].count(1) == 2 and np.abs(m["poses"][:, :2]).min() > 1e-4                  # a repeated id; roll and pitch are not zero
    for c, case in bc.shift_limit_cases():
        assert (2 * c["half"] + 2 * c["shift_half"]) ** 2 + 4096 <= 160 * 1024
        _, vol, res = bc.np_match(case, c)
        assert vol.shape == (3, 2 * c["shift_half"], 2 * c["shift_half"]) and res["score"] > res["second"] >= 0


def test_multi_frame_sides_use_every_listed_frame():
    m = CASES["multi_frame_stored"]
    l = bc.np_side([m["frames"][i] for i in m["target"]], [m["poses"][i] for i in m["target"]])
    assert len(l) == sum(len(a) + len(b) for a, b in (m["frames"][i] for i in m["target"]))
    anchor = np.concatenate(m["frames"][0])[:, :3]
    assert np.abs(l[:len(anchor)] - anchor).max() < 1e-5                                           # the anchor's own points come back, to rounding
    g = CASES["multi_frame_given"]
    assert bc.np_match(g, C)[1].max() > 0 and np.allclose(g["poses"], bc.IDENTITY * 3.0)         # the stored poses must not be read


def test_guess_against_matrices():
    """np_guess spells ll_bev_guess; the 4 x 4 product is the independent statement.  Unit quaternions, translations below 64 m: the
    entries are sums of a few products of numbers below 64, each rounded to 2^-53 relative"""
    rng = np.random.default_rng(9)
    for _ in range(20):
        P = []
        for _ in range(3):
            q = rng.normal(size=4); q /= np.linalg.norm(q)
            P.append(np.concatenate([q, rng.uniform(-60, 60, 3)]))
        T = bc.np_guess(*P)
        M = bc.pose_matrix(P[0]) @ bc.pose_matrix(P[1]) @ np.linalg.inv(bc.pose_matrix(P[2]))
        assert np.abs(bc.pose_matrix(T) - M).max() < 64 * 3 * 40 * 2.0 ** -53
    assert np.allclose(bc.np_guess(bc.IDENTITY, bc.IDENTITY, bc.IDENTITY), bc.IDENTITY, atol=0)


@pytest.mark.parametrize("k", range(len(bc.DISPLACEMENTS)))
def test_yard_displacements_are_found(k):
    c = bc.cfg()
    grid, vol, res = bc.yard_reference(k)
    print(f"yard {bc.DISPLACEMENTS[k]}: score {res['score']} second {res['second']} n_query {res['n_query']} yaw {math.degrees(res['yaw']):.1f} "
          f"t ({res['D'][4]}, {res['D'][5]})")
    assert bc.yard_found(res, k, c), res
    assert res["score"] > res["second"] > 0


def test_yard_second_seed():
    """the scene is not tuned to one draw of the boxes"""
    c = bc.cfg()
    for k in (0, 2):
        _, _, res = bc.yard_reference(k, seed=5)
        assert bc.yard_found(res, k, c) and res["score"] > res["second"], (k, res)


def test_the_ground_trap_is_why_z_min_is_minus_one():
    """with the ground in (z_min = -3: the plane 1.8 m below the sensor is layer 1) the sensor-centred ground rings of the two scans
    coincide at zero shift whatever the displacement is: zero shift wins, and by a wide margin over the true peak"""
    c = bc.cfg()
    for k in (0, 1):
        _, vol, res = bc.yard_reference(k, z_min=-3.0)
        _, _, good = bc.yard_reference(k)
        print(f"yard {k} with the ground: best {res['score']} at ({res['sx']}, {res['sy']}); without: {good['score']}")
        assert (res["sx"], res["sy"]) == (0, 0) and not bc.yard_found(res, k, c)
        assert res["score"] > 3 * good["score"]
