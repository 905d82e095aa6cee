"""The keyframes ABI without a GPU: the built library and api.EXPORTS hold the new symbols, and the two new structs that cross the
boundary have the same size and field offsets in include/lightloam_hip.h (compiled with the host C compiler) and in ctypes."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SYMBOLS = ["ll_keyframes_create", "ll_keyframes_destroy", "ll_keyframes_last_error", "ll_keyframes_size", "ll_keyframes_reset",
           "ll_keyframes_info", "ll_keyframes_add_cubemaps", "ll_keyframes_add_points", "ll_keyframes_export",
           "ll_cubemaps_insert_keyframes", "ll_cubemaps_insert_timing", "ll_drives_set_keyframes", "ll_drives_correct"]

STRUCTS = {"ll_insert_op": ("InsertOp", ["dst", "n_frames", "frames", "poses_w7", "reset", "cen"]),
           "ll_keyframe_info": ("KeyframeInfo", ["lane", "frame_index", "n", "offset", "pose_w7"]),
           "ll_keyframes_params": ("KeyframesParams", ["max_frames", "cap_corner", "cap_surf"])}


def test_symbols_exist_in_the_library_and_in_exports(api):
    lib = api.load_library()
    for s in SYMBOLS:
        assert hasattr(lib, s), s
        assert s in api.EXPORTS, s


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


def test_python_methods_exist(api):
    for name in ("add_cubemaps", "add_points", "export", "info", "size", "reset"):
        assert callable(getattr(api.Keyframes, name)), name
    assert callable(api.Context.keyframes) and callable(api.CubeMaps.insert_keyframes) and callable(api.CubeMaps.insert_timing)
    assert callable(api.Drives.set_keyframes) and callable(api.Drives.correct)
    assert api._BorrowedCubeMaps.insert_keyframes is api.CubeMaps.insert_keyframes   # Drives.cubemaps.insert_keyframes needs nothing more


def test_host_wrapper_compiles_as_cxx14(tmp_path):
    src = tmp_path / "use_keyframes.cpp"
    src.write_text("#include \"lightloam_host.hpp\"\n"
                   "long long run(lightloam::Context &c) {\n"
                   "    lightloam::Keyframes kf(c, 64, 1 << 18, 1 << 20);\n"
                   "    lightloam::LaserMappingSequences m(c, 2, 0.4f, 0.8f, 4096, 32768, 1 << 18);\n"
                   "    lightloam::Drives d(c, 2, 4096, 32768, 1 << 18);\n"
                   "    d.set_keyframes(&kf, 2);\n"
                   "    std::vector<double> poses(14, 0.0);\n"
                   "    const int first = kf.add_cubemaps(m.get(), std::vector<int>(2, 1), poses.data());\n"
                   "    const int id = kf.add_points(std::vector<lightloam::PointXYZI>(3), std::vector<lightloam::PointXYZI>(), poses.data());\n"
                   "    std::vector<int> ids(1, id);\n"
                   "    ll_insert_op op = {0, 1, ids.data(), nullptr, 1, {10, 10, 5}};\n"
                   "    std::vector<long long> added, dropped;\n"
                   "    m.insert_keyframes(kf, std::vector<ll_insert_op>(1, op), &added, &dropped);\n"
                   "    const int rc = lightloam::LaserMappingSequences::insert_into(d.cubemaps(), kf, std::vector<ll_insert_op>(1, op));\n"
                   "    d.correct(std::vector<int>(2, 1), poses.data());\n"
                   "    d.set_keyframes(nullptr);\n"
                   "    const lightloam::Keyframes::Exported x = kf.export_frames(0, kf.size());\n"
                   "    return added[0] + dropped[1] + rc + first + kf.info(0).n[0] + (long long)x.points.size();\n"
                   "}\n")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])
