"""laserMapping's five-nearest search and line / plane fits on the device (ll_map_search.h under k_map_knn, k_map_knn_partial and
k_map_fit_merged) against the independent numpy reference of mapsearchcases.py, at crafted inputs: exact ties, degenerate grids,
tiny maps, queries outside the box and on cell boundaries, the 1 m gate to the ulp, stack sizes around the workgroup sizes,
eigenvalue-ratio and residual ladders, degenerate fits and the candidate merge.  The search and the gate are exact (ids, xyz
bits, distance bits); the fitted values are held to 1e-9 * max(1, |value|); no case is excluded (test_map_search_cases.py shows
that no fit decision lies within 1e-9 of its threshold).

Largest |device - numpy| per family, measured on an MI355X (line points a / b, unit normal n, negative_OA_dot_norm d; absolute):
  ties              a/b 0        n 4.6e-14  d 2.9e-13        gate              a/b 5.6e-17  n 8.9e-15  d 1.6e-14
  grid              a/b 8.9e-16  n 2.2e-12  d 7.2e-10 (*)    stack             a/b 1.8e-15  n 1.0e-14  d 2.4e-13
  mapsize           a/b 0        n 2.0e-15  d 2.0e-14        ratio ladder      a/b 3.6e-15
  box               a/b 8.9e-16  n 3.6e-14  d 4.7e-13        eigen degenerate  a/b 1.4e-17
  plane fits        a/b -        n 2.6e-11  d 5.7e-09 (*)    residual ladder   n 1.3e-14  d 1.2e-14
  plane, all z = 0  n 1.0e-14    d 4.8e-14                   merge             a/b 3.6e-15  n 4.4e-14  d 1.4e-12
(*) at |d| = 1000 m (plane fits) and about 540 m (the far cluster): 5.7e-12 and 1.3e-12 relative.  Every search result and every
block list was exact.  The bound REL leaves more than 30x headroom over the worst value (n at 1000 m).
"""
import numpy as np
import pytest

import mapsearchcases as ms

pytestmark = pytest.mark.gpu

REL = 1e-9                                              # test_gpu_mapping.REL


@pytest.fixture(scope="module")
def ctx1(api):
    ctx = api.Context(api.default_params(16, batch=1, max_points=4096))
    yield ctx
    ctx.close()


def _map(api, ctx, c, gids=False):
    """a fresh map sized to the case"""
    m = api.Map(ctx, max(1, len(c["cm"])), max(1, len(c["sm"])), max(1, len(c["cs"])), max(1, len(c["ss"])))
    m.set_map(c["cm"], c["sm"])
    m.set_scan(c["cs"], c["ss"])
    if gids and c["gid_c"] is not None:
        m.set_map_ids(c["gid_c"], c["gid_s"])
    return m


def _blocks(m):
    e_src, a, b = m.edges()
    p_src, n, d = m.planes()
    assert m.counts() == (len(e_src), len(p_src))
    return e_src.copy(), a.copy(), b.copy(), p_src.copy(), n.copy(), d.copy()


def _check_blocks(name, got, ref):
    bad, worst = ms.block_differences(got, ref[:6], REL)
    what = f"{name} [{'map' if name in ms.MAP_NAMES else 'merged'}]: largest |device - numpy| in a/b {worst[0]:.3e}, n {worst[1]:.3e}, d {worst[2]:.3e}"
    print(what)
    assert not bad, (what, bad)
    if len(got[4]):
        assert np.abs(np.linalg.norm(got[4], axis=1) - 1.0).max() <= 1e-12, what
    return worst


# ------------------------------------------------------------------------------------------------ 1. the search itself
def _check_knn(name, which, world, cloud, gid, nn, ids):
    """Map.knn_partial's rows of one cloud type against the brute force, per query"""
    n = len(world)
    assert nn.shape == (n, 5, 4) and ids.shape == (n, 5)
    if n == 0:
        return
    pos, d, _ = ms.np_search5(world, cloud, gid)
    key = np.arange(len(cloud), dtype=np.int64) if gid is None else np.asarray(gid, np.int64)
    back = {int(k): i for i, k in enumerate(key)}
    inside = (d < np.float32(1.0)) & (pos >= 0)                                           # ascending rows: a prefix
    for i in range(n):
        k = int(inside[i].sum())
        where = (name, which, i)
        for j in range(k):                                                               # exact within 1 m: id, xyz bits, distance bits
            p = int(pos[i, j])
            assert ids[i, j] == key[p], where
            assert nn[i, j, :3].tobytes() == cloud[p, :3].tobytes() and nn[i, j, 3:].tobytes() == d[i, j:j + 1].tobytes(), where
        for j in range(k, 5):                                                            # beyond: padding, or a genuine map point at >= 1 m
            if ids[i, j] == ms.INT_MAX:
                assert np.isposinf(nn[i, j, 3]), where
                assert (ids[i, j:] == ms.INT_MAX).all(), where
                continue
            p = back.get(int(ids[i, j]))
            assert p is not None, where
            assert nn[i, j, :3].tobytes() == cloud[p, :3].tobytes(), where
            dj = ms.sq_dist(world[i:i + 1], cloud[p:p + 1])[0, 0]
            assert nn[i, j, 3] == dj and dj >= np.float32(1.0), where
        for j in range(4):                                                               # ascending by (distance, id)
            assert (nn[i, j, 3], ids[i, j]) < (nn[i, j + 1, 3], ids[i, j + 1]) or ids[i, j + 1] == ms.INT_MAX, where


@pytest.mark.parametrize("name", ms.MAP_NAMES)
def test_knn_partial_equals_the_brute_force(api, ctx1, name):
    c = ms.map_cases()[name]
    m = _map(api, ctx1, c, gids=True)
    cn, ci, sn, si = m.knn_partial(c["pose"])
    m.close()
    _check_knn(name, "corner", ms.np_to_world(c["pose"], c["cs"]), c["cm"], c["gid_c"], cn, ci)
    _check_knn(name, "surf", ms.np_to_world(c["pose"], c["ss"]), c["sm"], c["gid_s"], sn, si)


# ------------------------------------------------------------------------------------------------ 2. search + fit + compaction
@pytest.mark.parametrize("name", ms.MAP_NAMES)
def test_associate_equals_the_reference(api, ctx1, name):
    c = ms.map_cases()[name]
    m = _map(api, ctx1, c)
    m.associate(c["pose"])
    got = _blocks(m)
    m.close()
    _check_blocks(name, got, ms.reference_by_position(name))
    if c["family"] == "gate":
        assert np.array_equal(got[0], np.flatnonzero(c["expect"]))                       # blocks only where the f32 distance is < 1.0f


# ------------------------------------------------------------------------------------------------ 3. merge + fit + compaction
def _merged(api, ctx, cn, ci, sn, si):
    nc, ns = ci.shape[1], si.shape[1]
    m = api.Map(ctx, 8, 8, max(1, nc), max(1, ns))
    pt = np.zeros((1, 4), np.float32)
    m.set_map(pt, pt)
    m.set_scan(np.zeros((nc, 4), np.float32), np.zeros((ns, 4), np.float32))
    m.associate_merged(cn, ci, sn, si, ms.IDENT)
    got = _blocks(m)
    m.close()
    return got


@pytest.mark.parametrize("name", ms.MERGED_NAMES)
def test_associate_merged_equals_the_reference(api, ctx1, name):
    c = ms.merged_cases()[name]
    got = _merged(api, ctx1, c["cn"], c["ci"], c["sn"], c["si"])
    _check_blocks(name, got, ms.reference(name))


# ------------------------------------------------------------------------------------------------ 4. the two routes agree bit for bit
@pytest.mark.parametrize("name", [n for n in ms.MAP_NAMES if n != "ties-gid"])
def test_associate_equals_knn_partial_then_associate_merged(api, ctx1, name):
    c = ms.map_cases()[name]
    m = _map(api, ctx1, c)
    m.associate(c["pose"])
    one = _blocks(m)
    cn, ci, sn, si = m.knn_partial(c["pose"])
    m.associate_merged(cn[None], ci[None], sn[None], si[None], c["pose"])
    two = _blocks(m)
    m.close()
    for a, b in zip(one, two):
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), name


def test_gids_order_the_ties_of_the_merged_route(api, ctx1):
    """with gids (a tile shard) the partial search and the merge order ties by gid: the blocks are those of the gid-ordered reference,
    while Map.associate on the same map still orders by position (test_associate_equals_the_reference)"""
    c = ms.map_cases()["ties-gid"]
    m = _map(api, ctx1, c, gids=True)
    cn, ci, sn, si = m.knn_partial(c["pose"])
    m.associate_merged(cn[None], ci[None], sn[None], si[None], c["pose"])
    got = _blocks(m)
    m.close()
    _check_blocks("ties-gid", got, ms.reference("ties-gid"))
    assert ms.block_differences(ms.reference("ties-gid")[:6], ms.reference_by_position("ties-gid")[:6], REL)[0]      # and the two orders differ here
