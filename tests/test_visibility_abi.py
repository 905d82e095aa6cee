"""The visibility ABI without a GPU: the built library and api.EXPORTS hold the new symbols, the three new structs that cross the
boundary have the same size and field offsets in include/lightloam_hip.h (compiled with the host C compiler) and in ctypes, the
defaults are the header's, and the C++ wrapper compiles."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SYMBOLS = ["ll_visibility_default_params", "ll_visibility_create", "ll_visibility_destroy", "ll_visibility_last_error", "ll_visibility_run",
           "ll_visibility_counts", "ll_visibility_images", "ll_visibility_reset", "ll_visibility_timing", "ll_cubemaps_insert_keyframes_filtered"]

STRUCTS = {"ll_visibility_params": ("VisibilityParams", ["width", "height", "el_min_deg", "el_max_deg", "min_range", "max_range", "margin_abs",
                                                         "margin_rel", "radius", "max_images"]),
           "ll_visibility_op": ("VisibilityOp", ["n_frames", "frames", "poses_w7"]),
           "ll_visibility_rule": ("VisibilityRule", ["min_through", "max_hit"])}


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
    p = api.visibility_params()
    assert (p.width, p.height, p.el_min_deg, p.el_max_deg, p.min_range, p.max_range, p.radius) == (360, 90, -45.0, 45.0, 1.0, 120.0, 40.0)
    assert (p.margin_abs, p.margin_rel, p.max_images) == (0.5, C.c_float(0.02).value, 256)
    assert api.visibility_params(width=720, max_images=8).width == 720
    import viscases as vc
    assert {k: getattr(p, k) for k in vc.DEFAULTS} == {k: (v if isinstance(v, int) else C.c_float(v).value) for k, v in vc.DEFAULTS.items()}


def test_python_methods_exist(api):
    for name in ("run", "counts", "images", "reset", "timing"):
        assert callable(getattr(api.Visibility, name)), name
    assert callable(api.Context.visibility) and callable(api.visibility_params)
    import inspect
    sig = inspect.signature(api.CubeMaps.insert_keyframes)
    assert list(sig.parameters)[1:] == ["kf", "ops", "visibility", "rule"] and sig.parameters["visibility"].default is None and sig.parameters["rule"].default is None
    assert api._BorrowedCubeMaps.insert_keyframes is api.CubeMaps.insert_keyframes   # Drives.cubemaps.insert_keyframes needs nothing more


def test_host_wrapper_compiles_as_cxx14(tmp_path):
    src = tmp_path / "use_visibility.cpp"
    src.write_text("#include \"lightloam_host.hpp\"\n"
                   "long long run(lightloam::Context &c) {\n"
                   "    lightloam::Keyframes kf(c, 64, 1 << 18, 1 << 20);\n"
                   "    lightloam::LaserMappingSequences m(c, 2, 0.4f, 0.8f, 4096, 32768, 1 << 18);\n"
                   "    lightloam::Drives d(c, 2, 4096, 32768, 1 << 18);\n"
                   "    ll_visibility_params p = lightloam::Visibility::default_params();\n"
                   "    p.max_images = 16;\n"
                   "    lightloam::Visibility vis(kf, p), vis2(kf);\n"
                   "    std::vector<int> ids(2, 0); ids[1] = 1;\n"
                   "    ll_visibility_op vop = {2, ids.data(), nullptr};\n"
                   "    const std::vector<long long> pairs = vis.run(std::vector<ll_visibility_op>(1, vop));\n"
                   "    const lightloam::Visibility::Counts cnt = vis.counts(0);\n"
                   "    std::vector<float> raw, img;\n"
                   "    vis.images(0, &raw, &img);\n"
                   "    double ms[3]; long long n[3];\n"
                   "    vis.timing(ms, n);\n"
                   "    ll_insert_op op = {0, 2, ids.data(), nullptr, 1, {10, 10, 5}};\n"
                   "    const ll_visibility_rule rule = {2, 255};\n"
                   "    std::vector<long long> added, dropped, removed;\n"
                   "    m.insert_keyframes_filtered(kf, vis, rule, std::vector<ll_insert_op>(1, op), &added, &dropped, &removed);\n"
                   "    const int rc = lightloam::LaserMappingSequences::insert_filtered_into(d.cubemaps(), kf, vis, rule, std::vector<ll_insert_op>(1, op));\n"
                   "    vis.reset();\n"
                   "    return pairs[0] + added[0] + dropped[1] + removed[0] + rc + n[2] + (long long)(cnt.corner.size() + raw.size()) + vis2.params().width;\n"
                   "}\n")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])
