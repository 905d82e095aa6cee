#!/usr/bin/env python3
"""Regenerates tests/golden/*.npz.

WHAT THESE ARE: regression snapshots of inputs and expected outputs for the hot path, produced by OUR CPU oracle
(oracle/ll_oracle.c) on deterministic synthetic scans.  They are NOT outputs of the reference: BrenYi/Light-LOAM ships
no tests or fixtures and none of its translation units builds in this image (ROS1 / PCL / Eigen / Ceres are absent and
no stand-in headers are written for them), so no reference-generated vector of these stages exists ("parity unpinned").
They travel to the GPU box (which has no /root/reference and must not need the generator) and pin both the oracle
(tests/test_golden.py, CPU) and the HIP path (-m gpu) against silent drift.

The files under tests/golden/reference/ are different: they ARE reference output.  scanRegistration.cpp is the one
translation unit of the reference that compiles without Eigen / Ceres / FLANN; oracle/ref.py builds it unchanged against
declared container doubles (variant f32, see there), and record_reference() below keeps what that binary published for one
scan per case: laserCloud, cloudCurvature and cloudLabel (int8) on [5, n-5), the sharp / less-sharp / flat topics, and the
per-ring VoxelGrid INPUTS as laserCloud indices (the filter itself is a pass-through double; its output is not recorded).
The input scans are not stored: tests regenerate them from synth by the case's settings.  They live in a directory of their
own because tests/test_golden.py and tests/test_gpu_variants.py take every *.npz beside this script as an oracle snapshot.
Recording needs the reference tree; tests/test_ref_scan_registration.py compares the oracle with these files everywhere.

    python tests/golden/make_golden.py              # the oracle snapshots
    python tests/golden/make_golden.py reference    # the recorded reference output
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import lightloam_amd  # noqa: E402,F401
from lightloam_amd import synth  # noqa: E402
from oracle import orc  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))

CASES = {
    # name: (rings, azimuths, synth overrides, pose guess)
    "vlp16_450": (16, 450, dict(), [0, 0, 0, 1, 0.9, 0.0, 0.0]),
    "hdl64_256_azmajor": (64, 256, dict(order=1, az_jitter_deg=0.4, drop_prob=0.02, emit_nan=1), [0.001, -0.002, 0.004, 1, 0.8, 0.02, -0.01]),
}


def build(name):
    rings, az, kw, pose = CASES[name]
    cfg = synth.default_cfg(rings, azimuths=az, **kw)
    P = orc.params(rings)
    scans = [synth.scan(cfg, k) for k in range(2)]
    ex = [orc.extract(s, P) for s in scans]
    q = np.array(pose[:4], float); q /= np.linalg.norm(q); t = np.array(pose[4:], float)
    es, ea, eb = orc.associate_corner(q, t, ex[1]["sharp"], ex[0]["less_sharp"])
    ps, pa, pb, pc = orc.associate_plane(q, t, ex[1]["flat"], ex[0]["less_flat"])
    cnt, sidx, sw = orc.vote(ex[1]["flat"][ps], ex[0]["less_flat"][pa])
    order = np.sort(sidx); wmap = np.ones(len(ps), np.float32); wmap[sidx] = sw
    H, g, cost = orc.normal_equations(q, t, ex[1]["sharp"], es, ex[0]["less_sharp"], ea, eb, ex[1]["flat"], ps[order],
                                      ex[0]["less_flat"], pa[order], pb[order], pc[order], wmap[order], 0.1)
    rc, d = orc.gn_solve(H, g)
    q1, t1 = orc.pose_update(q, t, d)
    out = dict(rings=rings, pose=np.concatenate([q, t]), scan0=scans[0], scan1=scans[1])
    for k in (0, 1):
        for key in ("cloud", "label", "scan_start", "scan_end", "sharp", "less_sharp", "flat", "less_flat"):
            out[f"s{k}_{key}"] = ex[k][key]
        out[f"s{k}_curv"] = ex[k]["curv"]
    sel = np.zeros(len(ps), bool); sel[sidx] = True
    out.update(e_src=es, e_a=ea, e_b=eb, p_src=ps, p_a=pa, p_b=pb, p_c=pc, v_count=cnt, v_sel=sel, v_w=wmap,
               H=H, g=g, cost=cost, pose_after=np.concatenate([q1, t1]))
    return out


REF_DIR = os.path.join(HERE, "reference")
REF_CASES = {
    # name: (rings, scan index, synth overrides); the 32- and 64-ring scans are decimated in azimuth to ~30 k points so that
    # every file stays well below the size limit of a committed file
    "scanreg_s16": (16, 1, dict()),
    "scanreg_s32": (32, 1, dict(azimuths=900)),
    "scanreg_s64_azmajor_jitter_nan": (64, 1, dict(azimuths=480, order=1, az_jitter_deg=0.4, drop_prob=0.03, emit_nan=1)),
}


def reference_input(name):
    rings, k, kw = REF_CASES[name]
    return rings, synth.scan(synth.default_cfg(rings, **kw), k)


def record_reference(name):
    from oracle import ref
    rings, scan = reference_input(name)
    r = ref.extract([scan], rings, orc.params(rings).minimum_range, variant="f32")[0]
    n = len(r["cloud"])
    curv = np.zeros(n, np.float32); curv[5:n - 5] = r["curv"][5:n - 5]          # outside [5, n-5) the globals hold leftovers
    label = np.zeros(n, np.int8); label[5:n - 5] = r["label"][5:n - 5]
    ss, se = r["scan_start"], r["scan_end"]
    rings_picked = [i for i in range(rings) if se[i] - ss[i] >= 6]
    assert len(rings_picked) == len(r["voxel_inputs"])
    index = []
    for i, pts in zip(rings_picked, r["voxel_inputs"]):
        idx = np.concatenate([np.arange(ss[i] + (se[i] - ss[i]) * j // 6, ss[i] + (se[i] - ss[i]) * (j + 1) // 6) for j in range(6)])
        idx = idx[r["label"][idx] <= 0]                                          # scanRegistration.cpp:361-367, with the REFERENCE's labels
        assert r["cloud"][idx].tobytes() == pts.tobytes(), "the recorded indices must reproduce the reference's filter input"
        index.append(idx.astype(np.int32))
    return dict(rings=rings, n_in=len(scan), cloud=r["cloud"], curv=curv, label=label, sharp=r["sharp"], less_sharp=r["less_sharp"],
                flat=r["flat"], voxel_ring=np.array(rings_picked, np.int32), voxel_count=np.array([len(i) for i in index], np.int32),
                voxel_index=np.concatenate(index))


if __name__ == "__main__":
    if sys.argv[1:] == ["reference"]:
        os.makedirs(REF_DIR, exist_ok=True)
        for name in REF_CASES:
            data = record_reference(name)
            path = os.path.join(REF_DIR, name + ".npz")
            np.savez_compressed(path, **data)
            print(f"{path}: {os.path.getsize(path) / 1024:.0f} KiB, n_in {data['n_in']}, laserCloud {len(data['cloud'])}, "
                  f"sharp / less sharp / flat {len(data['sharp'])} / {len(data['less_sharp'])} / {len(data['flat'])}")
        sys.exit(0)
    for name in CASES:
        data = build(name)
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **data)
        print(f"{path}: {os.path.getsize(path) / 1024:.0f} KiB, n_in {len(data['scan1'])}, edges {len(data['e_src'])}, planes {len(data['p_src'])}")
