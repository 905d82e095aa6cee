"""ll_drives with localising lanes (ll_drives_set_localize): a lane that reads another lane's frozen map must equal, bit for bit,
the single chain -- ll_odometry_frames, WorldPose::compose, transformAssociateToMap, CubeMap.prepare + optimize on an imported
copy of that map (a localisation frame: no update), transformUpdate -- started from the same map-to-odom pose."""
import numpy as np
import pytest

from conftest import assert_bit_equal
from test_gpu_drives import CAP, NAN7, compose, qmul, qrot, single_chain
from test_gpu_sequences import drives, max_points

pytestmark = pytest.mark.gpu

RINGS, S, N_MAP, N_LOC, J = 16, 3, 7, 5, 2       # lanes, frames mapped, frames localised, lane 2's first frame
IDENT = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])
FIT_FIELDS = ("n_edge", "n_plane", "cost", "sq_edge", "sq_plane")


def fit_tuple(rec):
    return tuple(getattr(rec, f) for f in FIT_FIELDS)


def make_drives(api, scans, keep_registered=False):
    ctx = api.Context(api.default_params(RINGS, batch=2 * S, max_points=max_points(scans)))
    c, s_, pool = CAP[RINGS]
    return ctx, api.Drives(ctx, S, c, s_, pool_points=pool, keep_registered=keep_registered)


def step(api, ctx, dr, frames, scans, pose0, started):
    """one step: frames = {lane: (drive, frame)}; a lane STARTs when it is not in `started`"""
    cmd = np.zeros(S, np.int32)
    slots = dr.slots()
    for q, (d, k) in frames.items():
        cmd[q] = api.RUN if q in started else api.START
        ctx.upload_scan(int(slots[q]), scans[d][k])
    p0 = np.array([pose0[frames[q][0]] if q in frames else NAN7 for q in range(S)])
    out = dr.step(cmd, p0)
    started.update(frames)
    return out


def registered(cloud, p):
    """pointAssociateToMap of laserCloud by pose p (LaserMapping::qrot + t in f64, stored as f32), as test_registered_clouds"""
    ux, uy, uz, w = p[:4]
    v = cloud[:, :3].astype(np.float64)
    uvx = uy * v[:, 2] - uz * v[:, 1]; uvy = uz * v[:, 0] - ux * v[:, 2]; uvz = ux * v[:, 1] - uy * v[:, 0]
    uvx = uvx + uvx; uvy = uvy + uvy; uvz = uvz + uvz
    x = ((v[:, 0] + w * uvx) + (uy * uvz - uz * uvy)) + p[4]
    y = ((v[:, 1] + w * uvy) + (uz * uvx - ux * uvz)) + p[5]
    z = ((v[:, 2] + w * uvz) + (ux * uvy - uy * uvx)) + p[6]
    return np.stack([x.astype(np.float32), y.astype(np.float32), z.astype(np.float32), cloud[:, 3]], axis=1)


def localize_chain(api, scans, pose0, start, map_pts, layout):
    """single_chain (test_gpu_drives) with the mapping frame replaced by CubeMap.prepare + optimize on an imported copy of the map,
    and the map-to-odom pose starting at `start`; also the fit records ll_cubemaps_localize_slots gives for the same frames and
    guesses (a one-sequence CubeMaps holding the same map) and the registered clouds"""
    n = len(scans)
    ctx = api.Context(api.default_params(RINGS, batch=n, max_points=max(map(len, scans))))
    for k, s in enumerate(scans):
        ctx.upload_scan(k, s)
    ctx.extract(0, n)
    ctx.set_target_from_slot(0)
    rel = ctx.odometry_frames(1, n - 1, pose0=pose0, n_outer=3, first_frame_index=1)
    c, s_, pool = CAP[RINGS]
    cm = api.CubeMap(ctx, c, s_, pool_points=pool)
    cm.import_map(map_pts, layout)
    cms = api.CubeMaps(ctx, 1, c, s_, pool_points=pool)
    cms.import_maps(map_pts, [0, len(map_pts)], [layout])
    qw, tw = [0.0, 0.0, 0.0, 1.0], [0.0, 0.0, 0.0]
    qm, tm = [float(x) for x in start[:4]], [float(x) for x in start[4:]]
    odom, mapped, ran, fits, regs = [], [], [], [], []
    for k in range(n):
        if k > 0:
            qw, tw = compose(qw, tw, list(rel[k - 1, :4]), list(rel[k - 1, 4:]))
        r = qrot(qm, tw)
        guess = np.array(qmul(qm, qw) + [r[i] + tm[i] for i in range(3)])          # transformAssociateToMap
        f = ctx.features(k)
        cm.prepare(guess[4:], f["less_sharp"], f["less_flat"])
        p, rn = cm.optimize(guess)
        p2, rn2, fit = cms.localize_slots(guess[None, :], [k])
        assert (p2[0] == p).all() and bool(rn2[0]) == rn
        n2 = qw[0] * qw[0] + qw[1] * qw[1] + qw[2] * qw[2] + qw[3] * qw[3]         # transformUpdate
        inv = [-qw[0] / n2, -qw[1] / n2, -qw[2] / n2, qw[3] / n2]
        qm = qmul(list(p[:4]), inv)
        r = qrot(qm, tw)
        tm = [p[4 + i] - r[i] for i in range(3)]
        odom.append(np.array(qw + tw)); mapped.append(p); ran.append(rn); fits.append(fit_tuple(fit[0]))
        regs.append(registered(ctx.cloud(k)[0], p))
    cms.close(); cm.close(); ctx.close()
    return np.array(odom), np.array(mapped), np.array(ran), fits, regs


def map_state(api, dr, lane):
    cms = dr.cubemaps
    pts, off = cms.export([api.MAP_ALL if q == lane else api.MAP_NONE for q in range(S)])
    return pts[off[lane]:off[lane + 1]].copy(), cms.layout(lane), cms.info(lane)


def same_map(a, b):
    return a[0].tobytes() == b[0].tobytes() and all(np.array_equal(x, y) for x, y in zip(a[1], b[1])) and a[2] == b[2]


class Base:
    """drives A, B (scans, warm starts); a Drives whose lane 0 has mapped drive A for N_MAP frames and gone IDLE; that lane's
    mapped poses, its checkpoint and its map"""

    def __init__(self, api, synth):
        _, self.scans, self.pose0 = drives(synth, RINGS, 2, N_MAP)
        self.ctx, self.dr = make_drives(api, self.scans, keep_registered=True)
        started, self.mapped0 = set(), []
        for k in range(N_MAP):
            _, mapped, ran = step(api, self.ctx, self.dr, {0: (0, k)}, self.scans, self.pose0, started)
            assert bool(ran[0]) == (k > 0)
            self.mapped0.append(mapped[0].copy())
        self.blob = self.dr.save([1, 0, 0])
        self.dr.step(np.zeros(S, np.int32))                                         # lane 0 goes IDLE
        self.map0 = map_state(api, self.dr, 0)

    def close(self):
        self.dr.close(); self.ctx.close()


@pytest.fixture(scope="module")
def base(api, synth):
    b = Base(api, synth)
    yield b
    b.close()


def test_lanes_equal_the_single_localising_chain(api, base):
    dr, ctx, scans, pose0 = base.dr, base.ctx, base.scans, base.pose0
    start = np.tile(IDENT, (S, 1)); start[2] = base.mapped0[J]
    dr.set_localize([-1, 0, 0], start)
    first = {1: 0, 2: J}
    started, got = set(), {1: [], 2: []}
    for t in range(N_LOC):
        s0, c0 = dr.stats()[0], dr.cubemaps.stats()[0]
        odom, mapped, ran = step(api, ctx, dr, {q: (0, first[q] + t) for q in (1, 2)}, scans, pose0, started)
        s1, c1 = dr.stats()[0], dr.cubemaps.stats()[0]
        assert s1 - s0 == c1 - c0 <= 3, (t, s1 - s0, c1 - c0)                       # headers, prepare, poses + fit
        assert np.isnan(odom[0]).all() and np.isnan(mapped[0]).all() and not ran[0] and len(dr.registered(0)) == 0
        fit = dr.fit()
        assert fit_tuple(fit[0]) == (0, 0, 0.0, 0.0, 0.0)
        for q in (1, 2):
            got[q].append((odom[q], mapped[q], bool(ran[q]), fit_tuple(fit[q]), dr.registered(q)))
    assert same_map(map_state(api, dr, 0), base.map0)                               # nothing of lane 0's map has moved
    assert dr.cubemaps.info(1)[1][:2] != (0, 0)                                     # lane 1 did gather map 0 into its own workspace
    for q in (1, 2):
        sub = scans[0][first[q]:first[q] + N_LOC]
        odom, mapped, ran, fits, regs = localize_chain(api, sub, pose0[0], start[q], base.map0[0], base.map0[1])
        for k in range(N_LOC):
            o, m, r, f, reg = got[q][k]
            assert (o == odom[k]).all(), f"lane {q} frame {k} odom"
            assert (m == mapped[k]).all(), f"lane {q} frame {k} mapped"
            assert r == bool(ran[k]) and r, (q, k)                                  # the map is there from frame 0 on
            assert f == fits[k], (q, k, f, fits[k])
            assert f[0] > 10 and f[1] > 50 and f[2] > 0.0
            assert_bit_equal(reg, regs[k], f"lane {q} frame {k} registered cloud")
    dr.set_localize([-1, -1, -1])
    dr.step(np.zeros(S, np.int32))
    assert [fit_tuple(f) for f in dr.fit()] == [(0, 0, 0.0, 0.0, 0.0)] * S


def test_mixed_step_and_the_write_guard(api, base):
    scans, pose0 = base.scans, base.pose0
    ctx, dr = make_drives(api, scans)
    dr.restore(base.blob, [2])                                                      # lane 2: drive A's map, left idle
    map2 = map_state(api, dr, 2)
    assert map2[0].tobytes() == base.map0[0].tobytes()
    dr.set_localize([-1, 2, -1])
    started, lane0, lane1 = set(), [], []
    for t in range(3):                                                              # lane 0 maps drive B, lane 1 localises drive A in lane 2's map
        s0 = dr.stats()[0]
        odom, mapped, ran = step(api, ctx, dr, {0: (1, t), 1: (0, t)}, scans, pose0, started)
        assert dr.stats()[0] - s0 <= 5 + 3, t
        lane0.append((odom[0], mapped[0], bool(ran[0]))); lane1.append((odom[1], mapped[1], bool(ran[1])))
        assert dr.fit()[0].n_plane == 0 and dr.fit()[1].n_plane > 50
    assert same_map(map_state(api, dr, 2), map2)
    # lane 1 would read lane 0's map while lane 0 maps into it: refused, nothing enqueued
    dr.set_localize([-1, 0, -1])
    stats0 = (dr.stats(), dr.cubemaps.stats())
    slots = dr.slots()
    ctx.upload_scan(int(slots[0]), scans[1][3]); ctx.upload_scan(int(slots[1]), scans[0][3])
    for cmd1 in (api.RUN, api.START):
        with pytest.raises(api.LightLoamError) as e:
            dr.step(np.array([api.RUN, cmd1, api.IDLE], np.int32))
        assert e.value.code == -2 and "lane 1" in str(e.value) and "lane 0" in str(e.value), e.value
    assert (dr.stats(), dr.cubemaps.stats()) == stats0 and (dr.slots() == slots).all()
    for t in (3, 4):                                                                # lane 1 idle: lane 0 runs on as if nothing had been refused
        odom, mapped, ran = step(api, ctx, dr, {0: (1, t)}, scans, pose0, started)
        lane0.append((odom[0], mapped[0], bool(ran[0])))
    odom, mapped, ran, c1, cm = single_chain(api, RINGS, scans[1][:5], pose0[1])
    for k in range(5):
        assert (lane0[k][0] == odom[k]).all() and (lane0[k][1] == mapped[k]).all() and lane0[k][2] == bool(ran[k]), f"lane 0 frame {k}"
    cm.close(); c1.close()
    odom, mapped, ran, _, _ = localize_chain(api, scans[0][:3], pose0[0], IDENT, base.map0[0], base.map0[1])
    for k in range(3):
        assert (lane1[k][0] == odom[k]).all() and (lane1[k][1] == mapped[k]).all() and lane1[k][2] == bool(ran[k]), f"lane 1 frame {k}"
    # bad arguments of the mode itself
    for bad in ([-1, S, -1], [-2, -1, -1]):
        with pytest.raises(api.LightLoamError) as e:
            dr.set_localize(bad)
        assert e.value.code == -2
    with pytest.raises(api.LightLoamError) as e:
        dr.set_localize([-1, 0, -1], np.full((S, 7), np.nan))
    assert e.value.code == -2
    dr.close(); ctx.close()


def test_mode_is_not_part_of_a_checkpoint(api, base):
    scans, pose0 = base.scans, base.pose0
    start = np.tile(IDENT, (S, 1)); start[1] = base.mapped0[1]

    def run(interrupted):
        ctx, dr = make_drives(api, scans)
        dr.restore(base.blob, [0])
        dr.set_localize([-1, 0, -1], start)
        started, rows, lane, desc = set(), [], 1, None
        for t in range(N_LOC):
            if interrupted and t == 3:
                blob = dr.save([0, 1, 0])
                desc = api.describe_checkpoint(blob)
                dr.step(np.zeros(S, np.int32))                                      # lane 1 stops
                dr.restore(blob, [2])                                               # ... and goes on as lane 2
                dr.set_localize([-1, -1, 0])                                        # the mode comes from here, not from the blob
                lane = 2; started.add(2)
            odom, mapped, ran = step(api, ctx, dr, {lane: (0, 1 + t)}, scans, pose0, started)
            rows.append((odom[lane].copy(), mapped[lane].copy(), bool(ran[lane]), fit_tuple(dr.fit()[lane])))
        assert same_map(map_state(api, dr, 0)[:2] + (None,), base.map0[:2] + (None,))
        dr.close(); ctx.close()
        return rows, desc

    whole, _ = run(False)
    parts, desc = run(True)
    for k in range(N_LOC):
        for a, b, what in zip(whole[k][:2], parts[k][:2], ("odom", "mapped")):
            assert (a == b).all(), f"frame {k} {what}"
        assert whole[k][2:] == parts[k][2:] and whole[k][2], k
    assert sorted(desc) == sorted(api.describe_checkpoint(base.blob))               # the same fields: no mode in the blob
    assert desc["version"] == 1 and desc["n_records"] == 1
    assert sorted(desc["records"][0]) == ["bytes", "frame_index", "lane", "n_corner", "n_features", "n_surf", "offset"]
    assert desc["records"][0]["lane"] == 1 and desc["records"][0]["frame_index"] == 2
    assert (desc["records"][0]["n_corner"], desc["records"][0]["n_surf"]) == (0, 0)  # a localising lane's own map stays empty
