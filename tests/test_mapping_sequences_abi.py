"""ll_cubemaps at the boundary, without a GPU: the library exports it, api.EXPORTS lists it, and the C++ host wrapper
lightloam::LaserMappingSequences compiles as C++14."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ll_cubemaps_create", "ll_cubemaps_destroy", "ll_cubemaps_last_error", "ll_cubemaps_process_slots", "ll_cubemaps_process",
         "ll_cubemaps_info", "ll_cubemaps_download_cloud", "ll_cubemaps_download_cube", "ll_cubemaps_stats"]


def test_library_exports_cubemaps(api):
    lib = api.load_library()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in api.EXPORTS, name


def test_python_class_exists(api):
    for m in ("process_slots", "process", "info", "cloud", "cube", "stats"):
        assert callable(getattr(api.CubeMaps, m))


def test_host_wrapper_compiles_as_cxx14(tmp_path):
    src = tmp_path / "use_mapping_sequences.cpp"
    src.write_text("#include \"lightloam_host.hpp\"\n"
                   "void frame(lightloam::Context &c, const double *q_odom, const double *t_odom) {\n"
                   "    lightloam::LaserMappingSequences m(c, 4, 0.4f, 0.8f, 4096, 32768, 1 << 18);\n"
                   "    const int run[4] = {1, 1, 0, 1};\n"
                   "    m.transformAssociateToMap(q_odom, t_odom, run);\n"
                   "    m.process_slots(std::vector<int>{0, 1, -1, 3});\n"
                   "    m.transformUpdate(q_odom, t_odom, run);\n"
                   "    std::vector<lightloam::PointXYZI> a(3), b(5);\n"
                   "    m.process({&a, &a, nullptr, &a}, {&b, &b, nullptr, &b});\n"
                   "    (void)m.parameters[7 * 3 + 4]; (void)m.ran[0]; (void)m.get();\n"
                   "}\n")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])
