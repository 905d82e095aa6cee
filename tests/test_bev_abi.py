"""The bev ABI without a GPU: the built library and api.EXPORTS hold the new symbols, the three new structs that cross the boundary
have the same size and field offsets in include/lightloam_hip.h (compiled with the host C compiler) and in ctypes, the defaults are the
header's, ll_bev_guess (plain host C) agrees with the numpy restatement, and the C++ wrapper compiles."""
import ctypes as C
import os
import subprocess

import numpy as np

import bevcases as bc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SYMBOLS = ["ll_bev_default_params", "ll_bev_create", "ll_bev_destroy", "ll_bev_last_error", "ll_bev_match", "ll_bev_volume", "ll_bev_grid", "ll_bev_reset",
           "ll_bev_timing", "ll_bev_guess"]

STRUCTS = {"ll_bev_params": ("BevParams", ["cell", "half", "shift_half", "z_min", "z_layer", "excl_yaw", "excl_shift", "max_ops", "max_yaws", "max_points"]),
           "ll_bev_op": ("BevOp", ["n_target", "target", "target_poses_w7", "n_query", "query", "query_poses_w7", "yaw0", "yaw_step", "n_yaws"]),
           "ll_bev_result": ("BevResult", ["score", "second", "iyaw", "sx", "sy", "n_query", "yaw", "D_w7"])}


def test_symbols_exist_in_the_library_and_in_exports(api):
    lib = api.load_library()
    for s in SYMBOLS:
        assert hasattr(lib, s), s
        assert s in api.EXPORTS, s
    assert lib.ll_abi_version() == 3                                  # functions only: the version stays
    from lightloam_amd import build as b
    assert "ll_bev.hip" in b.HIP_SOURCES


def test_struct_layouts_match_the_header(api, tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "lightloam_hip.h"', 'int main(void) {']
    for cname, (_, fields) in STRUCTS.items():
        lines.append(f'  printf("{cname} size %zu\\n", sizeof({cname}));')
        for f in fields:
            lines.append(f'  printf("{cname} {f} %zu\\n", offsetof({cname}, {f}));')
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = {}
    for line in subprocess.check_output([str(exe)], text=True).splitlines():
        cname, field, value = line.split()
        got[(cname, field)] = int(value)
    for cname, (pyname, fields) in STRUCTS.items():
        T = getattr(api, pyname)
        assert [n for n, _ in T._fields_] == fields, cname
        assert got[(cname, "size")] == C.sizeof(T), cname
        for f in fields:
            assert got[(cname, f)] == getattr(T, f).offset, (cname, f)


def test_default_params_are_the_headers(api):
    p = api.bev_params()
    assert (p.cell, p.half, p.shift_half, p.z_min, p.z_layer, p.excl_yaw, p.excl_shift, p.max_ops, p.max_yaws, p.max_points) == \
        (0.5, 128, 16, -1.0, 1.0, 1, 2, 64, 16, 1 << 21)
    assert {k: getattr(p, k) for k in bc.DEFAULTS} == bc.DEFAULTS
    assert api.bev_params(half=64, max_ops=8).half == 64
    assert (2 * p.half + 2 * p.shift_half) ** 2 + 4096 <= 160 * 1024      # the default fits LDS


def test_guess_agrees_with_the_numpy_product(api):
    rng = np.random.default_rng(4)
    for k in range(50):
        P = []
        for _ in range(3):
            q = rng.normal(size=4); q /= np.linalg.norm(q)
            P.append(np.concatenate([q, rng.uniform(-60, 60, 3) * (1.0 if k % 2 else 0.01)]))
        got = api.bev_guess(*P)
        want = bc.np_guess(*P)
        assert np.abs(got - want).max() <= 1e-15, (k, got, want)
    D = np.array([0.0, 0.0, np.sin(0.4), np.cos(0.4), 3.0, -2.0, 0.0])
    Pc = np.array([0, 0, 0, 1, 10.0, 20.0, 1.8])
    assert np.abs(api.bev_guess(Pc, D, bc.IDENTITY) - [0, 0, np.sin(0.4), np.cos(0.4), 13.0, 18.0, 1.8]).max() <= 1e-15      # P_q = identity: T0 = P_c o D
    assert np.abs(api.bev_guess(Pc, bc.IDENTITY, Pc) - bc.IDENTITY).max() <= 1e-15                                          # P_c o P_c^-1
    lib = api.load_library()
    assert lib.ll_bev_guess(None, D.ctypes.data, D.ctypes.data, D.ctypes.data) == -2


def test_python_methods_exist(api):
    for name in ("match", "volume", "grid", "reset", "timing"):
        assert callable(getattr(api.Bev, name)), name
    assert callable(api.Context.bev) and callable(api.bev_params) and callable(api.bev_guess)


def test_null_handles_are_refused_without_a_device(api):
    lib = api.load_library()
    assert lib.ll_bev_create(None, None, None) == -2 and lib.ll_bev_match(None, None, 1, None) == -2
    assert lib.ll_bev_volume(None, 0, None) == -2 and lib.ll_bev_grid(None, 0, None) == -2 and lib.ll_bev_reset(None) == -2
    assert lib.ll_bev_timing(None, None, None) == -2 and lib.ll_bev_last_error(None) == b"null bev"


def test_host_wrapper_compiles_as_cxx14(tmp_path):
    src = tmp_path / "use_bev.cpp"
    src.write_text("#include \"lightloam_host.hpp\"\n"
                   "long long run(lightloam::Context &c) {\n"
                   "    lightloam::Keyframes kf(c, 64, 1 << 18, 1 << 20);\n"
                   "    ll_bev_params p = lightloam::Bev::default_params();\n"
                   "    p.max_ops = 4;\n"
                   "    lightloam::Bev bev(kf, p), bev2(kf);\n"
                   "    const int t[1] = {0}, q[2] = {1, 2};\n"
                   "    ll_bev_op op = {1, t, nullptr, 2, q, nullptr, 0.1, 0.0174, 13};\n"
                   "    const std::vector<ll_bev_result> r = bev.match(std::vector<ll_bev_op>(1, op));\n"
                   "    const std::vector<int> vol = bev.volume(0);\n"
                   "    const std::vector<unsigned char> grid = bev.grid(0);\n"
                   "    double ms[3]; long long n[3];\n"
                   "    bev.timing(ms, n);\n"
                   "    const double I[7] = {0, 0, 0, 1, 0, 0, 0};\n"
                   "    double T0[7];\n"
                   "    lightloam::Bev::guess(I, r[0].D_w7, I, T0);\n"
                   "    bev.reset();\n"
                   "    return r[0].score + r[0].second + n[2] + (long long)(vol.size() + grid.size()) + bev2.params().half + (long long)T0[4];\n"
                   "}\n")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])
