"""TransformToEnd at the boundary, without a GPU: the library exports the two entry points, api.EXPORTS lists them, the header
declares them with the argument counts the Python wrapper's ctypes signatures have, the ABI version stays 3, the Python methods
exist, and the C++ host wrappers and the many-drive tool compile as C++14."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ll_set_deskew", "ll_deskew_slots"]
GXX = ["g++", "-std=c++14", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include")]


def test_library_exports_the_deskew(api):
    lib = api.load_library()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in api.EXPORTS, name
    assert lib.ll_abi_version() == 3
    assert not hasattr(lib, "ll_launch_deskew")                     # the launcher stays inside the library (C++ linkage)


def _header_arguments(text, name):
    """the number of top-level commas + 1 in the declaration of `name`, comments removed"""
    decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    assert decl, name
    return decl.group(1).count(",") + 1


def test_signatures_match_the_header(api):
    text = open(os.path.join(ROOT, "include", "lightloam_hip.h")).read()
    lib = api.load_library()
    for name, n in (("ll_set_deskew", 2), ("ll_deskew_slots", 5)):
        assert _header_arguments(text, name) == n == len(getattr(lib, name).argtypes), name
    assert "#define LL_ABI_VERSION 3 " in text
    plain = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    assert "int ll_set_deskew(ll_ctx *ctx, int mode);" in plain
    assert "int ll_deskew_slots(ll_ctx *ctx, int first, int count, const double *host_pose7 , int mode );" in plain


def test_python_methods_exist(api):
    assert callable(api.Context.set_deskew) and callable(api.Context.deskew_slots)


def test_host_wrappers_compile_as_cxx14(tmp_path):
    src = tmp_path / "use_deskew.cpp"
    src.write_text("#include \"lightloam_host.hpp\"\n"
                   "int run() {\n"
                   "    lightloam::Context c(16, 4, 0, -1.0, -24.9f, 2.0f, 1);\n"
                   "    c.set_deskew(2);\n"
                   "    std::vector<double> rel = lightloam::odometry_frames(c, 1, 3);\n"
                   "    c.set_deskew(0);\n"
                   "    const double pose[14] = {0, 0, 0, 1, 0.9, 0, 0, 0, 0, 0, 1, 0.8, 0, 0};\n"
                   "    c.deskew_slots(0, 2, pose, 1);\n"
                   "    c.deskew_slots(2, 1);\n"
                   "    try { c.deskew_slots(2, 1, nullptr, 2); } catch (const lightloam::Error &e) { return e.code == LL_ERR_STATE ? (int)rel.size() : -1; }\n"
                   "    return 0;\n"
                   "}\n")
    subprocess.check_call(GXX + [str(src)])
    subprocess.check_call(GXX + [os.path.join(ROOT, "tools", "ll_kitti_drives.cpp")])
