"""Map export at the boundary, without a GPU: the library exports the entry points, the header declares them and the LL_MAP_*
values, api.py binds them, the ABI version has not moved, and the C++ host wrappers compile as C++14."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ll_cubemaps_export", "ll_cubemaps_export_sizes", "ll_cubemap_export"]


def test_library_exports_map_export(api):
    lib = api.load_library()
    for name in NAMES + ["ll_cubemaps_export_timing"]:
        assert hasattr(lib, name), name
        assert name in api.EXPORTS, name
    lib.ll_abi_version.restype = int
    assert lib.ll_abi_version() == 3


def test_header_declares_the_calls_and_the_selectors():
    text = open(os.path.join(ROOT, "include", "lightloam_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
    for name, value in (("LL_MAP_NONE", "(-1)"), ("LL_MAP_SURROUND", "0"), ("LL_MAP_ALL", "1")):
        assert re.search(r"#define\s+" + name + r"\s+" + re.escape(value) + r"\s", text), name


def test_python_binding(api):
    assert (api.MAP_NONE, api.MAP_SURROUND, api.MAP_ALL) == (-1, 0, 1)
    for m in ("export", "export_sizes"):
        assert callable(getattr(api.CubeMaps, m))
    assert callable(api.CubeMap.export) and callable(api.Drives.export_maps)


def test_host_wrappers_compile_as_cxx14(tmp_path):
    src = tmp_path / "use_map_export.cpp"
    src.write_text("#include \"lightloam_host.hpp\"\n"
                   "void publish(lightloam::Context &c) {\n"
                   "    std::vector<lightloam::PointXYZI> pts;\n"
                   "    std::vector<long long> off;\n"
                   "    lightloam::LaserMappingSequences m(c, 3, 0.4f, 0.8f, 4096, 32768, 1 << 18);\n"
                   "    m.export_maps({LL_MAP_ALL, LL_MAP_NONE, LL_MAP_SURROUND}, pts, off);\n"
                   "    lightloam::LaserMapping one(c);\n"
                   "    one.export_map(LL_MAP_SURROUND, pts);\n"
                   "    lightloam::Drives d(c, 3, 4096, 32768, 1 << 18);\n"
                   "    d.export_maps({LL_MAP_ALL, LL_MAP_ALL, LL_MAP_ALL}, pts, off);\n"
                   "}\n")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_kitti_drives_tool_compiles(tmp_path):
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tools", "ll_kitti_drives.cpp")])
