"""ll_drives at the boundary, without a GPU: the library exports it (and ll_cubemaps_reset), api.EXPORTS lists it, the Python
classes exist, the C++ host wrapper lightloam::Drives compiles as C++14 and tools/ll_kitti_drives.cpp compiles against the header."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ll_cubemaps_reset", "ll_drives_create", "ll_drives_destroy", "ll_drives_last_error", "ll_drives_slots", "ll_drives_step",
         "ll_drives_registered", "ll_drives_stats", "ll_drives_cubemaps"]


def test_library_exports_drives(api):
    lib = api.load_library()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in api.EXPORTS, name


def test_internal_entry_points_stay_hidden(api):
    lib = api.load_library()
    for name in ("llcms_process_slots_dev", "llcms_begin", "llcms_stage"):
        assert not hasattr(lib, name), name


def test_python_classes_exist(api):
    for m in ("slots", "step", "registered", "stats"):
        assert callable(getattr(api.Drives, m))
    assert isinstance(api.Drives.cubemaps, property)
    assert callable(api.CubeMaps.reset)
    assert (api.IDLE, api.RUN, api.START) == (0, 1, 2)
    assert [f for f, _ in api.DrivesParams._fields_] == ["n_lanes", "base", "line_res", "plane_res", "max_scan_corner", "max_scan_surf",
                                                          "pool_points", "n_outer", "keep_registered"]


def test_host_wrapper_compiles_as_cxx14(tmp_path):
    src = tmp_path / "use_drives.cpp"
    src.write_text("#include \"lightloam_host.hpp\"\n"
                   "void run(lightloam::Context &c, const std::string &path) {\n"
                   "    lightloam::Drives d(c, 4, 4096, 32768, 1 << 18, 0, true);\n"
                   "    const std::vector<int> s = d.slots();\n"
                   "    std::vector<int> cmd = {LL_DRIVE_START, LL_DRIVE_START, LL_DRIVE_IDLE, LL_DRIVE_START};\n"
                   "    const double pose0[28] = {0};\n"
                   "    d.step(cmd, pose0);\n"
                   "    cmd = {LL_DRIVE_RUN, LL_DRIVE_IDLE, LL_DRIVE_START, LL_DRIVE_RUN};\n"
                   "    d.step(cmd);\n"
                   "    lightloam::TrajectoryWriter w(path);\n"
                   "    w.append(d.mapped_pose(0));\n"
                   "    std::vector<lightloam::PointXYZI> reg = d.registered(3);\n"
                   "    long long syncs = 0, frames = 0; d.stats(syncs, frames);\n"
                   "    (void)s; (void)reg; (void)d.odom[7 * 3]; (void)d.ran[0]; (void)ll_cubemaps_reset(d.cubemaps(), 1); (void)d.get();\n"
                   "}\n")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_kitti_drives_tool_compiles():
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tools", "ll_kitti_drives.cpp")])
