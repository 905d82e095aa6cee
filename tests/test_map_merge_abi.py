"""Map merge at the boundary, without a GPU: the library exports the two entry points, api.EXPORTS lists them, the header declares
them and ll_merge_op (64 bytes), the ABI version stays 3, the Python methods exist and the C++ host wrapper compiles as C++14."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ll_cubemaps_merge", "ll_cubemaps_merge_timing"]
GXX = ["g++", "-std=c++14", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include")]


def test_library_exports_the_merge(api):
    lib = api.load_library()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in api.EXPORTS, name
    assert lib.ll_abi_version() == 3
    for name in ("llmm_free", "llcms_merge_state", "llcms_fail"):
        assert not hasattr(lib, name), name


def test_header_declares_them():
    text = open(os.path.join(ROOT, "include", "lightloam_hip.h")).read()
    for name in NAMES:
        assert name + "(" in text, name
    assert "typedef struct { int dst, src; double T_w7[7]; } ll_merge_op;" in text
    assert "#define LL_ABI_VERSION 3 " in text


def test_merge_op_layout(api, tmp_path):
    assert [f for f, _ in api.MergeOp._fields_] == ["dst", "src", "T_w7"]
    assert C.sizeof(api.MergeOp) == 64 and api.MergeOp.T_w7.offset == 8
    src = tmp_path / "size.c"
    src.write_text("#include <stddef.h>\n#include \"lightloam_hip.h\"\n"
                   "_Static_assert(sizeof(ll_merge_op) == 64, \"ll_merge_op is 64 bytes\");\n"
                   "_Static_assert(offsetof(ll_merge_op, T_w7) == 8, \"T_w7 at 8\");\n"
                   "_Static_assert(LL_ABI_VERSION == 3, \"ABI 3\");\n")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_python_methods_exist(api):
    assert callable(api.CubeMaps.merge) and callable(api.CubeMaps.merge_timing)
    assert api._BorrowedCubeMaps.merge is api.CubeMaps.merge                       # Drives.cubemaps.merge needs nothing more


def test_host_wrapper_compiles_as_cxx14(tmp_path):
    src = tmp_path / "use_merge.cpp"
    src.write_text("#include \"lightloam_host.hpp\"\n"
                   "long long run(lightloam::Context &c) {\n"
                   "    lightloam::LaserMappingSequences m(c, 3, 0.4f, 0.8f, 4096, 32768, 1 << 18);\n"
                   "    std::vector<ll_merge_op> ops(2);\n"
                   "    ops[0].dst = 0; ops[0].src = 2; ops[1].dst = 1; ops[1].src = 2;\n"
                   "    for (int k = 0; k < 7; ++k) ops[0].T_w7[k] = ops[1].T_w7[k] = k == 3 ? 1.0 : 0.0;\n"
                   "    std::vector<long long> added, dropped;\n"
                   "    m.merge_maps(ops, &added, &dropped);\n"
                   "    m.merge_maps(ops);\n"
                   "    lightloam::Drives d(c, 3, 4096, 32768, 1 << 18);\n"
                   "    const int rc = lightloam::LaserMappingSequences::merge_into(d.cubemaps(), ops, &added);\n"
                   "    return added[0] + dropped[3] + rc;\n"
                   "}\n")
    subprocess.check_call(GXX + ["-fsyntax-only", str(src)])
