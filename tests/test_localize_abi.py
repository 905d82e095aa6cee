"""Localisation against frozen cube maps at the boundary, without a GPU: the library exports the three entry points, api.EXPORTS
lists them, the ABI version and the checkpoint format stay where they were, api.LocalizeFit mirrors ll_localize_fit, the Python
methods exist, the C++ host wrappers compile as C++14 and tools/ll_kitti_drives.cpp compiles against the header."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ll_cubemaps_localize_slots", "ll_drives_set_localize", "ll_drives_fit"]
GXX = ["g++", "-std=c++14", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include")]


def test_library_exports_localisation(api):
    lib = api.load_library()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in api.EXPORTS, name
    assert lib.ll_abi_version() == 3
    for name in ("llcms_localize_slots_dev", "ll_launch_cms_fit"):
        assert not hasattr(lib, name), name


def test_header_declares_them():
    text = open(os.path.join(ROOT, "include", "lightloam_hip.h")).read()
    for name in NAMES:
        assert name + "(" in text, name
    assert "typedef struct { int n_edge, n_plane; double cost, sq_edge, sq_plane; } ll_localize_fit;" in text
    assert "#define LL_ABI_VERSION 3 " in text


def test_fit_record_layout(api):
    assert [f for f, _ in api.LocalizeFit._fields_] == ["n_edge", "n_plane", "cost", "sq_edge", "sq_plane"]
    assert [t for _, t in api.LocalizeFit._fields_] == [C.c_int, C.c_int, C.c_double, C.c_double, C.c_double]
    assert C.sizeof(api.LocalizeFit) == 32 and api.LocalizeFit.cost.offset == 8


def test_python_methods_exist(api):
    assert callable(api.CubeMaps.localize_slots) and callable(api.Drives.set_localize) and callable(api.Drives.fit)
    assert [f for f, _ in api.DrivesParams._fields_] == ["n_lanes", "base", "line_res", "plane_res", "max_scan_corner", "max_scan_surf",
                                                          "pool_points", "n_outer", "keep_registered"]      # the mode is no create-time parameter


def test_host_wrappers_compile_as_cxx14(tmp_path):
    src = tmp_path / "use_localize.cpp"
    src.write_text("#include \"lightloam_host.hpp\"\n"
                   "double run(lightloam::Context &c) {\n"
                   "    lightloam::LaserMappingSequences m(c, 3, 0.4f, 0.8f, 4096, 32768, 1 << 18);\n"
                   "    m.process_slots({0, -1, -1});\n"
                   "    m.localize_slots({-1, 4, 5}, {0, 0, 0});\n"
                   "    m.localize_slots({-1, 4, 5}, std::vector<int>(), false);\n"
                   "    lightloam::Drives d(c, 3, 4096, 32768, 1 << 18);\n"
                   "    const double start[21] = {0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1, 2.5, 0, 0};\n"
                   "    d.set_localize({-1, 0, 0}, start);\n"
                   "    d.step({LL_DRIVE_IDLE, LL_DRIVE_START, LL_DRIVE_START});\n"
                   "    const std::vector<ll_localize_fit> f = d.fit();\n"
                   "    d.set_localize({-1, -1, -1});\n"
                   "    return f[1].cost + f[1].sq_edge + f[2].sq_plane + f[1].n_edge + f[2].n_plane + m.fit[1].cost;\n"
                   "}\n")
    subprocess.check_call(GXX + [str(src)])


def test_kitti_drives_tool_compiles_with_localize_in():
    path = os.path.join(ROOT, "tools", "ll_kitti_drives.cpp")
    text = open(path).read()
    assert "--localize-in" in text and "--start-pose" in text and "set_localize" in text
    subprocess.check_call(GXX + [path])
