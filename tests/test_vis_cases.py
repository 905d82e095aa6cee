"""The inputs of the visibility tests checked against their own preconditions, on the numpy restatement alone (tests/viscases.py): no GPU
and no library.  The crafted "edge" points really sit where they claim, and on the ray-cast street scene the default parameters and
rule remove no static point and at least half of the box's points."""
import numpy as np
import pytest

import viscases as vc

F = np.float32
SIZES = [dict(width=16, height=4), dict()]


@pytest.fixture(scope="module")
def street(orc):
    frames, poses, is_box = vc.street_scene()
    c = vc.cfg()
    counts, pairs = vc.np_vote(frames, poses, c)
    return frames, poses, is_box, counts, pairs


def _ulp_apart(a, b):
    return int(F(b).view(np.uint32)) - int(F(a).view(np.uint32)) == 1


@pytest.mark.parametrize("size", SIZES, ids=["16x4", "default"])
def test_column_and_row_edges_are_one_ulp_wide(orc, size):
    c = vc.cfg(**size)
    W, H = c["width"], c["height"]
    for col in sorted({1, W // 8, 3 * W // 16}):
        below, at = vc.column_edge(c, col)
        assert below[0] == at[0] and below[2] == at[2] and _ulp_apart(below[1], at[1])
        pix, _ = vc.np_pixel([below, at], c)
        assert (pix >= 0).all() and list(pix % W) == [col - 1, col] and pix[0] // W == pix[1] // W
    for row in sorted({H // 2 + 1, H - 1}):
        below, at = vc.row_edge(c, row)
        assert below[0] == at[0] and below[1] == at[1] and _ulp_apart(below[2], at[2])
        pix, _ = vc.np_pixel([below, at], c)
        assert (pix >= 0).all() and list(pix // W) == [row - 1, row] and pix[0] % W == pix[1] % W


@pytest.mark.parametrize("size", SIZES, ids=["16x4", "default"])
def test_wrap_column_and_windows(orc, size):
    c = vc.cfg(**size)
    W = c["width"]
    cases = vc.image_cases(c)
    co, su = cases["wrap_column"]
    pix, _ = vc.np_pixel(co[:, :3], c)
    assert (pix >= 0).all() and list(pix[:3] % W) == [W - 1] * 3 and list(pix[3:] % W) == [0, 0]      # just below 2 pi: the clamp; just above 0
    a = orc.libm(1, co[:3, 1], co[:3, 0])
    assert (a < 0).all() and ((a + vc.TWO_PI_F).astype(F) * c["ka"] >= W).all()                       # without the min the column would be `width`
    pix, _ = vc.np_pixel(su[:, :3], c)
    assert list(pix[:2] % W) == [W - 1, 0] and list(pix[2:] % W) == [W // 2, W // 2]                  # either side of the seam; +-pi
    co, su = cases["windows_and_nan"]
    pix, r = vc.np_pixel(np.concatenate([co, su])[:, :3], c)
    used = pix >= 0
    assert list(np.flatnonzero(used)) == [6, 9, 17]                 # the last float below max_range, exactly min_range, the plain point
    assert r[5] == c["max_range"] and r[6] < c["max_range"] and r[8] < c["min_range"] and r[9] == c["min_range"]
    raw, img = vc.np_images(co, su, c)
    assert np.isfinite(raw).sum() == 3 and not np.isnan(raw).any() and not np.isnan(img).any()
    co, su = cases["both_types"]
    pc, rc = vc.np_pixel(co[:, :3], c); ps, rs = vc.np_pixel(su[:, :3], c)
    assert (pc == ps).all() and (pc >= 0).all() and rc[0] < rs[0] and rs[1] < rc[1] and rc[2] == rs[2]
    raw, _ = vc.np_images(co, su, c)
    assert [raw.reshape(-1)[p] for p in pc] == [rc[0], rs[1], rc[2]]
    for name in ("no_corner", "no_surf", "empty"):
        raw, img = vc.np_images(*cases[name], c)
        assert np.isfinite(raw).sum() == (0 if name == "empty" else 2)


def test_erosion_wraps_columns_and_stops_at_rows(orc):
    c = vc.cfg(width=16, height=4)
    raw, img = vc.np_images(vc.pts4([[10, -0.5, 9.9]]), vc.pts4(np.zeros((0, 3))), c)       # the last column, the top row
    assert np.isfinite(raw).sum() == 1 and raw[3, 15] < np.inf
    want = np.zeros((4, 16), bool); want[2:4, [14, 15, 0]] = True
    assert (np.isfinite(img) == want).all() and (img[want] == raw[3, 15]).all()


def test_margin_case_sits_one_ulp_either_side_of_both_margins(orc):
    c = vc.cfg()
    frames, poses, expect = vc.margin_case(c)
    sub = np.concatenate(frames[0])[:, :3]; obs = np.concatenate(frames[1])[:, :3]
    assert (vc.np_to_frame(poses[1], vc.np_to_world(poses[0], sub)) == sub).all()              # identity poses: l == p, bit for bit
    _, r = vc.np_pixel(sub[:4], c); _, d = vc.np_pixel(obs[:4], c)
    m = c["margin_abs"] + c["margin_rel"] * r
    far, near = r + m, r - m
    assert d[0] == np.nextafter(far[0], F(np.inf)) and d[1] == far[1] and d[2] == near[2] and d[3] == np.nextafter(near[3], F(0))
    counts, pairs = vc.np_vote(frames, poses, c)
    got = [tuple(int(v) for v in row) for row in np.concatenate(counts[0])]
    assert got == expect and pairs == 2
    _, img = vc.np_images(*frames[1], c)
    pix, _ = vc.np_pixel(sub[4:], c)
    assert img.reshape(-1)[pix[0]] == np.inf and img.reshape(-1)[pix[1]] < near[0]            # the empty pixel; the occluded point


def test_random_drive_has_every_kind_of_evidence(orc):
    frames, poses = vc.random_drive()
    obs = vc.np_observers(poses, 40.0)
    assert any(len(o) == len(poses) - 1 for o in obs) or max(len(o) for o in obs) >= 3
    assert any(len(o) < len(poses) - 1 for o in obs)                # some pairs are outside the radius
    c = vc.cfg(width=48, height=12)
    counts, _ = vc.np_vote(frames, poses, c)
    allc = np.concatenate([np.concatenate(x) for x in counts])
    assert (allc[:, 0] > 0).sum() > 50 and (allc[:, 1] > 0).sum() > 50 and (allc.sum(axis=1) == 0).sum() > 50 and allc[:, 0].max() >= 2


def test_street_scene_is_what_it_claims(street):
    frames, poses, is_box, _, pairs = street
    S = vc.STREET
    assert len(frames) == S["n_frames"] == 12 and pairs == 12 * 11 - 2                          # 4 m apart: only (0, 11) and (11, 0) are beyond the radius of 40
    n = [len(co) + len(su) for co, su in frames]
    assert min(n) > 4000 and max(n) < 16000
    nbox = [int(bc.sum() + bs.sum()) for bc, bs in is_box]
    assert nbox[S["box_frame"]] >= 30 and sum(nbox) == nbox[S["box_frame"]]


def test_street_scene_default_rule_keeps_the_static_world_and_removes_the_box(street):
    """The prototype the feature was specified with (float64, its own generator) flagged 0 of 96 483 static points and 41 of 58 box points; this scene is the
    committed generator under the float32 restatement.  It gives 0 of 86 236 static points and 47 of the box's 56.  The bounds are the specification's: no static point, at least half
    of the box."""
    frames, poses, is_box, counts, _ = street
    n_static = n_box = gone_static = gone_box = 0
    for (cc, cs), (bc, bs) in zip(counts, is_box):
        gone = vc.np_removed(np.concatenate([cc, cs])); box = np.concatenate([bc, bs])
        n_static += int((~box).sum()); n_box += int(box.sum())
        gone_static += int((gone & ~box).sum()); gone_box += int((gone & box).sum())
    print(f"street scene: static points flagged {gone_static} of {n_static}, box points flagged {gone_box} of {n_box}")
    assert gone_static == 0
    assert 2 * gone_box >= n_box
