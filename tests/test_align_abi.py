"""Map alignment at the boundary, without a GPU: the library exports the two entry points, api.EXPORTS lists them, the header
declares them with the argument counts the Python wrapper's ctypes signatures have, the ABI version stays 3, the Python methods
exist (also on the handle a Drives object lends) and the C++ host wrappers and the native test program compile as C++14."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ll_cubemaps_align", "ll_cubemaps_align_timing"]
GXX = ["g++", "-std=c++14", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include")]


def test_library_exports_the_alignment(api):
    lib = api.load_library()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in api.EXPORTS, name
    assert lib.ll_abi_version() == 3
    for name in ("llal_free", "llcms_align_state"):
        assert not hasattr(lib, name), name


def _header_arguments(text, name):
    """the number of top-level commas + 1 in the declaration of `name`, comments removed"""
    decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    assert decl, name
    return decl.group(1).count(",") + 1


def test_signatures_match_the_header(api):
    text = open(os.path.join(ROOT, "include", "lightloam_hip.h")).read()
    lib = api.load_library()
    for name, n in (("ll_cubemaps_align", 8), ("ll_cubemaps_align_timing", 3)):
        assert _header_arguments(text, name) == n == len(getattr(lib, name).argtypes), name
    assert "#define LL_ABI_VERSION 3 " in text
    assert "typedef struct { int dst, src; double T_w7[7]; } ll_merge_op;" in text  # the op's layout is the merge's


def test_python_methods_exist(api):
    assert callable(api.CubeMaps.align) and callable(api.CubeMaps.align_timing)
    assert api._BorrowedCubeMaps.align is api.CubeMaps.align                       # Drives.cubemaps.align needs nothing more


def test_host_wrappers_compile_as_cxx14(tmp_path):
    src = tmp_path / "use_align.cpp"
    src.write_text("#include \"lightloam_host.hpp\"\n"
                   "double run(lightloam::Context &c) {\n"
                   "    lightloam::LaserMappingSequences m(c, 3, 0.4f, 0.8f, 4096, 32768, 1 << 18);\n"
                   "    std::vector<ll_merge_op> ops(2);\n"
                   "    ops[0].dst = 0; ops[0].src = 2; ops[1].dst = 1; ops[1].src = 2;\n"
                   "    for (int k = 0; k < 7; ++k) ops[0].T_w7[k] = ops[1].T_w7[k] = k == 3 ? 1.0 : 0.0;\n"
                   "    std::vector<double> T; std::vector<int> ran; std::vector<ll_localize_fit> fit;\n"
                   "    m.align_maps(ops, 2, &T, &ran, &fit);\n"
                   "    m.align_maps(ops, 0, &T);\n"
                   "    for (int i = 0; i < 2; ++i) for (int k = 0; k < 7; ++k) ops[i].T_w7[k] = T[7 * i + k];\n"
                   "    m.merge_maps(ops);\n"
                   "    lightloam::Drives d(c, 3, 4096, 32768, 1 << 18);\n"
                   "    const int rc = lightloam::LaserMappingSequences::align_into(d.cubemaps(), ops, 2, &T, nullptr, &fit);\n"
                   "    return T[0] + fit[1].cost + ran[0] + rc;\n"
                   "}\n")
    subprocess.check_call(GXX + [str(src)])
    subprocess.check_call(GXX + [os.path.join(ROOT, "tests", "native", "align_host.cpp")])
