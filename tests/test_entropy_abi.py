"""The entropy ABI without a GPU: the built library and api.EXPORTS hold the new symbols, the three new structs that cross the
boundary have the same size and field offsets in include/lightloam_hip.h (compiled with the host C compiler) and in ctypes, the
defaults are the header's, and the C++ wrapper compiles."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SYMBOLS = ["ll_entropy_default_params", "ll_entropy_create", "ll_entropy_destroy", "ll_entropy_last_error", "ll_entropy_run", "ll_entropy_values",
           "ll_entropy_reset", "ll_entropy_timing"]

STRUCTS = {"ll_entropy_params": ("EntropyParams", ["radius", "min_neighbours", "lambda_floor", "max_points"]),
           "ll_entropy_op": ("EntropyOp", ["n_frames", "frames", "poses_w7"]),
           "ll_entropy_rec": ("EntropyRec", ["n_points", "n_valid", "n_sparse", "n_outside", "n_pairs", "sum_h", "sum_pv", "mme", "mpv"])}


def test_symbols_exist_in_the_library_and_in_exports(api):
    lib = api.load_library()
    for s in SYMBOLS:
        assert hasattr(lib, s), s
        assert s in api.EXPORTS, s
    assert lib.ll_abi_version() == 3                                  # functions only: the version stays


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
    p = api.entropy_params()
    assert (p.radius, p.min_neighbours, p.lambda_floor, p.max_points) == (0.5, 6, C.c_float(1e-6).value, 1 << 20)
    assert api.entropy_params(radius=1.0, max_points=4096).max_points == 4096
    import entropycases as ec
    assert {k: getattr(p, k) for k in ec.DEFAULTS} == {k: (v if isinstance(v, int) else C.c_float(v).value) for k, v in ec.DEFAULTS.items()}


def test_python_methods_exist(api):
    for name in ("run", "values", "reset", "timing", "close"):
        assert callable(getattr(api.Entropy, name)), name
    assert callable(api.Context.entropy) and callable(api.entropy_params)
    assert api.EntropyOp._fields_ == api.VisibilityOp._fields_         # an op is (n_frames, frames, poses_w7), as ll_visibility_op


def test_host_wrapper_compiles_as_cxx14(tmp_path):
    src = tmp_path / "use_entropy.cpp"
    src.write_text("#include \"lightloam_host.hpp\"\n"
                   "double run(lightloam::Context &c, const double *before, const double *after) {\n"
                   "    lightloam::Keyframes kf(c, 64, 1 << 18, 1 << 20);\n"
                   "    ll_entropy_params p = lightloam::Entropy::default_params();\n"
                   "    p.max_points = 1 << 16; p.radius = 0.75f;\n"
                   "    lightloam::Entropy en(kf, p), en2(kf);\n"
                   "    std::vector<int> ids(2, 0); ids[1] = 1;\n"
                   "    std::vector<ll_entropy_op> ops(2);\n"
                   "    ops[0].n_frames = 2; ops[0].frames = ids.data(); ops[0].poses_w7 = before;\n"
                   "    ops[1].n_frames = 2; ops[1].frames = ids.data(); ops[1].poses_w7 = after;\n"
                   "    const std::vector<ll_entropy_rec> rec = en.run(ops);\n"
                   "    const lightloam::Entropy::Values v = en.values(3);\n"
                   "    double ms[5]; long long n[5];\n"
                   "    en.timing(ms, n);\n"
                   "    en.reset();\n"
                   "    return rec[1].mme - rec[0].mme + rec[0].mpv + (double)(rec[0].n_valid + rec[0].n_pairs + n[4]) + ms[3] + v.h[0] + v.pv[0] + v.nn[0] + en2.params().radius\n"
                   "           + (en.get() != nullptr);\n"
                   "}\n")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])
