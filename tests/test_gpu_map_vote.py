"""The graph-based correspondence vote of the mapping stage on the device (ll_map_vote.hip; laserMapping.cpp:836-1030 and the
Corre_Match of :1993-2003): the crafted cases of mapvotecases.py through ll_map_vote_host, the centroid and the vote inside a map
against numpy and the oracle, the voted solve against an un-voted one on the selected points, the loops against their parts,
off-means-off, and the refusals."""
import ctypes as C

import numpy as np
import pytest

import mapvotecases as mc
from conftest import assert_bit_equal
from test_gpu_drives import CAP, NAN7, compose, qmul, qrot
from test_gpu_mapping_sequences import _assert_same, _ctx, _guesses
from test_gpu_sequences import drives, max_points

pytestmark = pytest.mark.gpu

REL = 1e-9                                             # tests/test_gpu_mapping.py's tolerance


def close(a, b, what):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    assert a.shape == b.shape, what
    scale = max(1.0, float(np.abs(b).max()) if b.size else 1.0)
    assert (float(np.abs(a - b).max()) if a.size else 0.0) <= REL * scale, what


@pytest.fixture(scope="module")
def ctx1(api):
    ctx = api.Context(api.default_params(16, batch=1, max_points=4096))
    yield ctx
    ctx.close()


# ------------------------------------------------------------------------------------------------ 1. crafted cases
@pytest.mark.parametrize("name", mc.CASE_NAMES)
def test_crafted_cases_equal_np_map_vote(api, ctx1, name):
    src, tgt = mc.all_cases()[name]
    cnt, sel = mc.reference(name)
    gcnt, gsel = api.map_vote_host(ctx1, src, tgt)
    assert np.array_equal(gcnt, cnt), (name, np.flatnonzero(gcnt != cnt)[:8])
    assert np.array_equal(gsel, sel), (name, np.flatnonzero(gsel != sel)[:8])


# ------------------------------------------------------------------------------------------------ the jittered room
BOX = np.array([10.0, 8.0, 3.0])


def _on_box(rng, n, jitter):
    """n points on the six faces of the box [0, BOX], area-weighted, jittered by `jitter` along the face normal -> (points, axis, side)"""
    areas = np.array([BOX[1] * BOX[2], BOX[1] * BOX[2], BOX[0] * BOX[2], BOX[0] * BOX[2], BOX[0] * BOX[1], BOX[0] * BOX[1]])
    face = rng.choice(6, n, p=areas / areas.sum())
    p = rng.uniform(0, 1, (n, 3)) * BOX
    ax = face // 2; side = face % 2
    p[np.arange(n), ax] = side * BOX[ax] + rng.normal(0, jitter, n)
    return p, ax, side


def room(seed):
    """a map of ~3000 surf and ~500 corner points, a corner stack and a surf stack of 20 tight patches of 35 points in patch order
    (as a sweep delivers them), a third of them displaced by 0.3 .. 0.8 m along the wall's normal, either way"""
    rng = np.random.default_rng(seed)
    surf_map, _, _ = _on_box(rng, 3000, 0.01)
    edges = []
    for a in range(3):                                   # the 12 edges of the box
        for u in (0.0, 1.0):
            for v in (0.0, 1.0):
                e = np.zeros((42, 3)); e[:, a] = rng.uniform(0, BOX[a], 42)
                b, c = [k for k in range(3) if k != a]
                e[:, b] = u * BOX[b]; e[:, c] = v * BOX[c]
                edges.append(e + rng.normal(0, 0.01, e.shape))
    corner_map = np.concatenate(edges)
    corner_stack = corner_map[rng.choice(len(corner_map), 120, replace=False)] + rng.normal(0, 0.02, (120, 3))
    centres, ax, side = _on_box(rng, 20, 0.0)
    pts = []
    for c, a, s in zip(centres, ax, side):
        c = np.clip(c, 1.3, BOX - 1.3); c[a] = s * BOX[a]   # away from the other walls
        q = np.tile(c, (35, 1))
        b, d = [k for k in range(3) if k != a]
        r = 0.6 * np.sqrt(rng.uniform(0, 1, 35)); th = rng.uniform(0, 2 * np.pi, 35)
        q[:, b] += r * np.cos(th); q[:, d] += r * np.sin(th)
        q[:, a] += rng.normal(0, 0.01, 35)
        out = rng.uniform(0, 1, 35) < 1 / 3
        q[out, a] += rng.uniform(0.3, 0.8, out.sum()) * rng.choice([-1.0, 1.0], out.sum())
        pts.append(q)
    surf_stack = np.concatenate(pts)
    # the stack is in the lidar frame: the world points carried back through a small pose, which is then the guess
    yaw = 0.02
    pose = np.array([0.0, 0.0, np.sin(yaw / 2), np.cos(yaw / 2), 0.3, -0.2, 0.05])
    cs, sn = np.cos(yaw), np.sin(yaw)
    R = np.array([[cs, -sn, 0], [sn, cs, 0], [0, 0, 1.0]])
    to_lidar = lambda w: (w - pose[4:]) @ R                 # R^T (w - t)
    return dict(corner_map=mc.f4(corner_map), surf_map=mc.f4(surf_map), corner_stack=mc.f4(to_lidar(corner_stack)),
                surf_stack=mc.f4(to_lidar(surf_stack)), pose=pose)


def np_centroids(orc, sc):
    """per surf stack point: the f32 FLANN distances to every map point at the oracle's pointAssociateToMap, the five nearest in
    ascending order, their float sum in that order / 5 in float; and whether the six nearest distances are all distinct"""
    w = np.ascontiguousarray(orc.point_associate_to_map(sc["pose"][:4], sc["pose"][4:], sc["surf_stack"]), np.float32)
    m = sc["surf_map"]
    d = (w[:, None, 0] - m[None, :, 0]) ** 2
    d = d + (w[:, None, 1] - m[None, :, 1]) ** 2
    d = d + (w[:, None, 2] - m[None, :, 2]) ** 2
    assert d.dtype == np.float32
    order = np.argsort(d, axis=1, kind="stable")[:, :6]
    d6 = np.take_along_axis(d, order, axis=1)
    untied = (np.diff(d6, axis=1) > 0).all()
    c = np.zeros((len(w), 3), np.float32)
    for j in range(5):
        c = c + m[order[:, j], :3]
    return c / np.float32(5), untied


@pytest.fixture(scope="module")
def scene(orc):
    sc = room(7)
    q, t = sc["pose"][:4], sc["pose"][4:]
    sc["blocks"] = orc.map_associate(q, t, sc["corner_stack"], sc["corner_map"], sc["surf_stack"], sc["surf_map"])
    sc["ctr"], sc["untied"] = np_centroids(orc, sc)
    p_src = sc["blocks"][3]
    tgt = np.zeros((len(p_src), 4), np.float32); tgt[:, :3] = sc["ctr"][p_src]
    sc["tgt"] = tgt
    sc["cnt"], sc["sel"] = mc.np_map_vote(sc["surf_stack"][p_src], tgt)
    return sc


def _map(api, ctx, sc, surf_stack=None, vote=True):
    ss = sc["surf_stack"] if surf_stack is None else surf_stack
    m = api.Map(ctx, len(sc["corner_map"]) + 8, len(sc["surf_map"]) + 8, len(sc["corner_stack"]) + 8, len(sc["surf_stack"]) + 8)
    m.set_map(sc["corner_map"], sc["surf_map"])
    m.set_scan(sc["corner_stack"], ss)
    if vote:
        m.set_vote(True)
    return m


# ------------------------------------------------------------------------------------------------ 2. centroid and vote inside the map
def test_scene_is_what_the_test_needs(scene):
    """conditions on the INPUT, checked on the CPU side: no tied neighbour distances; kept and dropped blocks in at least two regions"""
    assert scene["untied"]
    assert len(scene["surf_map"]) == 3000 and len(scene["corner_map"]) == 504 and len(scene["surf_stack"]) == 700
    n = len(scene["blocks"][3])
    assert n > 400 and len(scene["blocks"][0]) > 20, (n, len(scene["blocks"][0]))
    mixed = [r for r, (b0, b1) in enumerate(mc.region_bounds(n)) if scene["sel"][b0:b1].any() and (~scene["sel"][b0:b1]).any()]
    print("candidates", n, "selected", int(scene["sel"].sum()), "regions with both kept and dropped:", mixed)
    assert len(mixed) >= 2


def test_centroid_and_vote_inside_the_map(api, ctx1, scene):
    e_src, e_a, e_b, p_src, p_n, p_d = scene["blocks"]
    m = _map(api, ctx1, scene)
    m.associate(scene["pose"])
    src, cnt, sel, tgt = m.download_vote()
    assert np.array_equal(src, p_src)
    assert_bit_equal(tgt, scene["ctr"][p_src], "centroids")
    assert np.array_equal(cnt, scene["cnt"]) and np.array_equal(sel, scene["sel"])
    ne, npl = m.counts()
    assert (ne, npl) == (len(e_src), int(scene["sel"].sum()))
    s2, n2, d2 = m.planes()
    keep = scene["sel"]
    assert np.array_equal(s2, p_src[keep])
    close(n2, p_n[keep], "plane normals"); close(d2, p_d[keep], "negative_OA_dot_norm")
    # a second association leaves the same candidates (the compaction of the first one is not its input)
    m.associate(scene["pose"])
    src3, cnt3, sel3, tgt3 = m.download_vote()
    assert np.array_equal(src3, p_src) and np.array_equal(cnt3, cnt) and np.array_equal(sel3, sel)
    # off again: all blocks, and the candidates of the last voted association stay readable
    m.set_vote(False)
    m.associate(scene["pose"])
    assert m.counts() == (len(e_src), len(p_src))
    assert np.array_equal(m.planes()[0], p_src)
    m.close()


# ------------------------------------------------------------------------------------------------ 3. voted solve against an un-voted one
def test_voted_normal_equations_equal_the_oracle_over_the_selected_blocks(api, ctx1, scene, orc):
    e_src, e_a, e_b, p_src, p_n, p_d = scene["blocks"]
    keep = scene["sel"]
    m = _map(api, ctx1, scene)
    m.associate(scene["pose"])
    for dp in ([0, 0, 0], [0.01, 0.02, -0.01]):
        pose = scene["pose"].copy(); pose[4:] += dp
        Ho, go, co = orc.map_normal_equations(pose[:4], pose[4:], scene["corner_stack"], e_src, e_a, e_b, scene["surf_stack"],
                                              p_src[keep], p_n[keep], p_d[keep])
        H, g, cost = m.normal_equations(pose)
        close(H, Ho, "H"); close(g, go, "g"); close(cost, co, "cost")
    m.close()


def test_voted_solve_equals_the_unvoted_solve_on_the_selected_points(api, ctx1, scene):
    p_src = scene["blocks"][3]
    guess = scene["pose"].copy(); guess[4:] += [0.04, -0.03, 0.01]
    a = _map(api, ctx1, scene)
    a.associate(guess)
    src, cnt, sel, _ = a.download_vote()
    assert sel.any() and (~sel).any()
    pa = a.solve(guess)
    b = _map(api, ctx1, scene, surf_stack=scene["surf_stack"][src[sel]], vote=False)
    b.associate(guess)
    assert b.counts() == a.counts()
    assert np.array_equal(b.planes()[0], np.arange(int(sel.sum())))
    pb = b.solve(guess)
    assert_bit_equal(pa, pb, "voted solve vs un-voted solve on the selected points")
    assert np.asarray(pa, np.float64).tobytes() == np.asarray(pb, np.float64).tobytes()
    a.close(); b.close()


# ------------------------------------------------------------------------------------------------ 4. loops equal their parts
def _same64(a, b, what):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    assert a.shape == b.shape and a.tobytes() == b.tobytes(), (what, a, b)


def test_optimize_equals_associate_and_solve(api, ctx1, scene):
    guess = scene["pose"].copy(); guess[4:] += [0.04, -0.03, 0.01]
    a = _map(api, ctx1, scene)
    pa, ran = a.optimize(guess, n_outer=2)
    assert ran
    b = _map(api, ctx1, scene)
    p = guess.copy()
    for _ in range(2):
        b.associate(p)
        p = b.solve(p)
    _same64(pa, p, "optimize vs associate + solve")
    assert a.counts() == b.counts()
    for x, y in zip(a.download_vote(), b.download_vote()):
        assert np.array_equal(x, y)
    c = _map(api, ctx1, scene, vote=False)                         # and the vote does something here
    pc, _ = c.optimize(guess, n_outer=2)
    assert c.counts()[1] > a.counts()[1]
    a.close(); b.close(); c.close()


@pytest.fixture(scope="module")
def seqs(api, synth):
    S, n = 3, 4
    cfgs, scans, _ = drives(synth, 16, S, n)
    ctx = _ctx(api, 16, scans)
    yield dict(S=S, n=n, cfgs=cfgs, scans=scans, ctx=ctx)
    ctx.close()


def test_cubemap_process_equals_its_parts(api, synth, seqs):
    ctx, cfgs, n = seqs["ctx"], seqs["cfgs"], seqs["n"]
    c, s, pool = CAP[16]
    a = api.CubeMap(ctx, c, s, pool_points=pool); b = api.CubeMap(ctx, c, s, pool_points=pool); off = api.CubeMap(ctx, c, s, pool_points=pool)
    a.set_vote(True); b.set_vote(True)
    differs = False
    for k in range(n):
        guess = _guesses(synth, cfgs[:1], k, [(0.0, 0.0, 0.0)])[0]
        f = ctx.features(k * seqs["S"])
        pa, ra = a.process(guess, f["less_sharp"], f["less_flat"])
        b.prepare(guess[4:], f["less_sharp"], f["less_flat"])
        pb, rb = b.optimize(guess, 2)
        b.update(pb)
        po, ro = off.process(guess, f["less_sharp"], f["less_flat"])
        assert ra == rb == ro == (k > 0)
        _same64(pa, pb, f"frame {k}")
        if ra:
            n_all = off.map().counts()[1]
            src, cnt, sel, _ = a.map().download_vote()
            assert a.map().counts()[1] == int(sel.sum())
            differs = differs or int(sel.sum()) < len(sel)
    assert a.info() == b.info()
    for which in range(4):
        assert_bit_equal(a.cloud(which), b.cloud(which), f"cloud {which}")
    print("the vote dropped blocks in some frame:", differs)
    a.close(); b.close(); off.close()


def test_cubemaps_equal_single_maps_with_flags_1_0_1(api, synth, seqs):
    """ll_cubemaps_process_slots over three sequences with flags [1, 0, 1]: sequence 2 starts one frame late, so that it is below the
    :1822 gate beside running ones; then one more frame through ll_cubemaps_process in which sequence 0 brings an empty stack.
    Every sequence equals its own ll_cubemap, and sequence 1 equals the un-voted run."""
    ctx, cfgs, S, n = seqs["ctx"], seqs["cfgs"], seqs["S"], seqs["n"]
    c, s, pool = CAP[16]
    flags = [1, 0, 1]
    many = api.CubeMaps(ctx, S, c, s, pool_points=pool)
    many.set_vote(flags)
    ones = [api.CubeMap(ctx, c, s, pool_points=pool) for _ in range(S)]
    for q in range(S):
        ones[q].set_vote(flags[q])
    plain = api.CubeMap(ctx, c, s, pool_points=pool)                # sequence 1, never voted
    gate_seen = False
    for k in range(n):
        guess = _guesses(synth, cfgs, k, [(0.0, 0.0, 0.0)] * S)
        slots = [k * S + q for q in range(S)]
        if k == 0:
            slots[2] = -1
        poses, ran = many.process_slots(guess, slots)
        for q in range(S):
            if slots[q] < 0:
                continue
            p1, r1 = ones[q].process_slot(guess[q], slots[q])
            assert bool(ran[q]) == bool(r1), (k, q)
            _same64(poses[q], p1, f"frame {k} sequence {q}")
        if k == 1:
            assert not ran[2] and ran[0] and ran[1]                 # the gate is shut for sequence 2 beside two running ones
            gate_seen = True
        p2, _ = plain.process_slot(guess[1], slots[1])
        _same64(poses[1], p2, f"frame {k}: sequence 1 against the un-voted run")
    assert gate_seen
    # one more frame from host clouds: sequence 0's stack is empty
    empty = np.zeros((0, 4), np.float32)
    guess = _guesses(synth, cfgs, n - 1, [(0.0, 0.0, 0.0)] * S)
    feats = [ctx.features((n - 1) * S + q) for q in range(S)]
    corners = [f["less_sharp"] for f in feats]; surfs = [f["less_flat"] for f in feats]
    corners[0] = empty; surfs[0] = empty
    poses, ran = many.process(guess, corners, surfs)
    for q in range(S):
        p1, r1 = ones[q].process(guess[q], corners[q], surfs[q])
        assert bool(ran[q]) == bool(r1), q
        _same64(poses[q], p1, f"host frame, sequence {q}")
    p2, _ = plain.process(guess[1], corners[1], surfs[1])
    _same64(poses[1], p2, "host frame: sequence 1 against the un-voted run")
    for q in range(S):
        _assert_same(many, q, ones[q], f"sequence {q}")
    _assert_same(many, 1, plain, "sequence 1 un-voted")
    for o in ones:
        o.close()
    plain.close(); many.close()


def _chain_with_vote(api, rings, scans, pose0, vote_from):
    """test_gpu_drives.single_chain with the map's vote switched on by hand for the frames with index > vote_from"""
    n = len(scans)
    ctx = api.Context(api.default_params(rings, batch=n, max_points=max(map(len, scans))))
    for k, s in enumerate(scans):
        ctx.upload_scan(k, s)
    ctx.extract(0, n)
    ctx.set_target_from_slot(0)
    rel = ctx.odometry_frames(1, n - 1, pose0=pose0, n_outer=3, first_frame_index=1)
    c, s_, pool = CAP[rings]
    cm = api.CubeMap(ctx, c, s_, pool_points=pool)
    qw, tw = [0.0, 0.0, 0.0, 1.0], [0.0, 0.0, 0.0]
    qm, tm = [0.0, 0.0, 0.0, 1.0], [0.0, 0.0, 0.0]
    odom, mapped = [], []
    for k in range(n):
        if k > 0:
            qw, tw = compose(qw, tw, list(rel[k - 1, :4]), list(rel[k - 1, 4:]))
        r = qrot(qm, tw)
        guess = np.array(qmul(qm, qw) + [r[i] + tm[i] for i in range(3)])
        cm.set_vote(vote_from >= 0 and k > vote_from)
        p, rn = cm.process_slot(guess, k)
        n2 = qw[0] * qw[0] + qw[1] * qw[1] + qw[2] * qw[2] + qw[3] * qw[3]
        inv = [-qw[0] / n2, -qw[1] / n2, -qw[2] / n2, qw[3] / n2]
        qm = qmul(list(p[:4]), inv)
        r = qrot(qm, tw)
        tm = [p[4 + i] - r[i] for i in range(3)]
        odom.append(np.array(qw + tw)); mapped.append(p)
    return np.array(odom), np.array(mapped), ctx, cm


def _run_drives(api, rings, scans, pose0, vote_from):
    L, F = len(scans), len(scans[0])
    ctx = api.Context(api.default_params(rings, batch=2 * L, max_points=max_points(scans)))
    c, s_, pool = CAP[rings]
    dr = api.Drives(ctx, L, c, s_, pool_points=pool)
    if vote_from is not None:
        dr.set_map_vote(vote_from)
    out = []
    for k in range(F):
        slots = dr.slots()
        for q in range(L):
            ctx.upload_scan(int(slots[q]), scans[q][k])
        cmd = np.full(L, api.START if k == 0 else api.RUN, np.int32)
        odom, mapped, ran = dr.step(cmd, np.array(pose0) if k == 0 else np.array([NAN7] * L))
        out.append((odom.copy(), mapped.copy()))
    return out, dr, ctx


def test_drive_lanes_vote_from_frame_21(api, synth):
    """2 lanes x 25 frames, from_frame = 20: equal to the single-drive chain with the vote switched on by hand after frame 20, and
    bit-identical to a run with the vote off up to frame 20"""
    rings, L, F, FROM = 16, 2, 25, 20
    cfgs, scans, pose0 = drives(synth, rings, L, F)
    on, dr_on, ctx_on = _run_drives(api, rings, scans, pose0, FROM)
    off, dr_off, ctx_off = _run_drives(api, rings, scans, pose0, None)
    for k in range(FROM + 1):
        _same64(on[k][0], off[k][0], f"frame {k} odom, before the gate opens")
        _same64(on[k][1], off[k][1], f"frame {k} mapped, before the gate opens")
    later = any(on[k][1].tobytes() != off[k][1].tobytes() for k in range(FROM + 1, F))
    print("the voted frames differ from the un-voted run:", later)
    assert dr_on.stats() == dr_off.stats()                         # no host synchronisation added
    for q in range(L):
        odom, mapped, c1, cm = _chain_with_vote(api, rings, scans[q], pose0[q], FROM)
        for k in range(F):
            _same64(on[k][0][q], odom[k], f"lane {q} frame {k} odom")
            _same64(on[k][1][q], mapped[k], f"lane {q} frame {k} mapped")
        _assert_same(dr_on.cubemaps, q, cm, f"lane {q}")
        cm.close(); c1.close()
    dr_on.close(); ctx_on.close(); dr_off.close(); ctx_off.close()


# ------------------------------------------------------------------------------------------------ 5. off means off
def test_off_means_off_and_no_synchronisation_is_added(api, synth, seqs):
    ctx, cfgs, S, n = seqs["ctx"], seqs["cfgs"], seqs["S"], seqs["n"]
    c, s, pool = CAP[16]
    never = api.CubeMaps(ctx, S, c, s, pool_points=pool)
    toggled = api.CubeMaps(ctx, S, c, s, pool_points=pool)
    toggled.set_vote([1] * S); toggled.set_vote([0] * S)
    voted = api.CubeMaps(ctx, S, c, s, pool_points=pool)
    voted.set_vote([1] * S)
    for k in range(n):
        guess = _guesses(synth, cfgs, k, [(0.0, 0.0, 0.0)] * S)
        slots = [k * S + q for q in range(S)]
        p0, r0 = never.process_slots(guess, slots)
        p1, r1 = toggled.process_slots(guess, slots)
        voted.process_slots(guess, slots)
        assert (r0 == r1).all()
        _same64(p0, p1, f"frame {k}")
    for q in range(S):
        assert never.info(q) == toggled.info(q)
        for which in range(4):
            assert_bit_equal(never.cloud(q, which), toggled.cloud(q, which), f"sequence {q} cloud {which}")
        cubes = [(s_, i) for s_ in (0, 1) for i in range(api.N_CUBES) if len(never.cube(q, s_, i))]
        for s_, i in cubes:
            assert_bit_equal(never.cube(q, s_, i), toggled.cube(q, s_, i), f"sequence {q} cube {s_} {i}")
    assert never.stats() == toggled.stats() == voted.stats()       # the same host synchronisations per frame, vote on or off
    never.close(); toggled.close(); voted.close()


# ------------------------------------------------------------------------------------------------ 6. errors
def test_refusals(api, ctx1, scene):
    lib = ctx1.lib
    m = _map(api, ctx1, scene, vote=False)
    m.set_row_shard(1, 2)
    assert lib.ll_map_set_vote(m.h, 1) == -7                        # LL_ERR_STATE: a row shard
    m.set_row_shard(0, 1)
    gid_c = np.arange(len(scene["corner_map"]), dtype=np.int32); gid_s = np.arange(len(scene["surf_map"]), dtype=np.int32)
    m.set_map_ids(gid_c, gid_s)
    assert lib.ll_map_set_vote(m.h, 1) == -7                        # ... the merged (tile-parallel) association
    m.set_map_ids(None, None)
    m.set_vote(True)
    assert lib.ll_map_set_row_shard(m.h, 1, 2) == -7 and lib.ll_map_set_map_ids(m.h, gid_c.ctypes.data_as(C.c_void_p), gid_s.ctypes.data_as(C.c_void_p)) == -7
    assert lib.ll_map_set_vote(m.h, 2) == -2
    m.close()
    big = api.Map(ctx1, 64, 64, 64, 200000)                        # a region of 10 019 candidates needs 280 KB of LDS
    assert lib.ll_map_set_vote(big.h, 1) == -2
    assert lib.ll_map_set_vote(big.h, 0) == 0
    big.close()
    ok = api.Map(ctx1, 64, 64, 64, 116000)                         # 5 819 candidates: 162 932 B fit
    assert lib.ll_map_set_vote(ok.h, 1) == 0
    ok.close()
    n = C.c_int(0)
    assert lib.ll_map_set_vote(None, 1) == -2 and lib.ll_map_download_vote(None, None, None, None, None, 0, C.byref(n)) == -2
    assert lib.ll_map_vote_host(None, None, None, 0, None, None) == -2 and lib.ll_map_vote_host(ctx1.h, None, None, 4, None, None) == -2
    assert lib.ll_cubemap_set_vote(None, 1) == -2 and lib.ll_cubemaps_set_vote(None, None) == -2 and lib.ll_drives_set_map_vote(None, 3) == -2
    cms = api.CubeMaps(ctx1, 2, 256, 256, pool_points=4096)
    assert lib.ll_cubemaps_set_vote(cms.h, None) == -2
    cms.close()
