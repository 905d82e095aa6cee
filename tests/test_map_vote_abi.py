"""The mapping vote at the boundary, without a GPU: the library exports the six entry points, api.EXPORTS lists them, the header
declares them with the argument counts the Python wrapper's ctypes signatures have, the ABI version stays 3, the Python methods
exist, the kernels' file is one of the library's sources, and the C++ host wrappers and the many-drive tool compile as C++14."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"ll_map_set_vote": 2, "ll_map_download_vote": 7, "ll_map_vote_host": 6, "ll_cubemap_set_vote": 2, "ll_cubemaps_set_vote": 2,
         "ll_drives_set_map_vote": 2}
GXX = ["g++", "-std=c++14", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include")]


def test_library_exports_the_map_vote(api):
    lib = api.load_library()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in api.EXPORTS, name
    assert lib.ll_abi_version() == 3
    for name in ("ll_map_launch_vote", "ll_map_launch_vote_only", "k_map_vote"):      # the launchers stay inside the library (C++ linkage)
        assert not hasattr(lib, name), name


def _header_arguments(text, name):
    """the number of top-level commas + 1 in the declaration of `name`, comments removed"""
    decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    assert decl, name
    return decl.group(1).count(",") + 1


def test_signatures_match_the_header(api):
    text = open(os.path.join(ROOT, "include", "lightloam_hip.h")).read()
    lib = api.load_library()
    for name, n in NAMES.items():
        assert _header_arguments(text, name) == n == len(getattr(lib, name).argtypes), name
    assert "#define LL_ABI_VERSION 3 " in text
    plain = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    assert "int ll_map_set_vote(ll_map *m, int on);" in plain
    assert "int ll_map_download_vote(ll_map *m, int *src, int *count, uint8_t *selected, float *tgt3, int cap, int *n);" in plain
    assert "int ll_map_vote_host(ll_ctx *ctx, const ll_point *src, const ll_point *tgt, int n, int *count, uint8_t *selected);" in plain
    assert "int ll_cubemap_set_vote(ll_cubemap *cm, int on);" in plain
    assert "int ll_cubemaps_set_vote(ll_cubemaps *cms, const int *on );" in plain
    assert "int ll_drives_set_map_vote(ll_drives *d, int from_frame);" in plain


def test_python_methods_and_sources_exist(api):
    for f in (api.Map.set_vote, api.Map.download_vote, api.map_vote_host, api.CubeMap.set_vote, api.CubeMaps.set_vote, api.Drives.set_map_vote):
        assert callable(f)
    import lightloam_amd  # noqa: F401
    from lightloam_amd import build as b
    assert "ll_map_vote.hip" in b.HIP_SOURCES
    assert os.path.exists(os.path.join(ROOT, "light-loam_amd", "csrc", "ll_map_vote.hip"))


def test_host_wrappers_compile_as_cxx14(tmp_path):
    src = tmp_path / "use_map_vote.cpp"
    src.write_text("#include \"lightloam_host.hpp\"\n"
                   "int run() {\n"
                   "    lightloam::Context c(16, 4);\n"
                   "    lightloam::MapOptimizer m(c, 4096, 4096, 512, 2048);\n"
                   "    m.set_vote(true);\n"
                   "    std::vector<int> src, count; std::vector<unsigned char> sel; std::vector<float> tgt;\n"
                   "    m.download_vote(src, count, sel, tgt);\n"
                   "    std::vector<lightloam::Corre_Match> cor(40);\n"
                   "    lightloam::map_vote_host(c, cor, count, sel);\n"
                   "    lightloam::LaserMapping lm(c, 0.4f, 0.8f, 2048, 8192, 1 << 16);\n"
                   "    lm.set_vote(true);\n"
                   "    lightloam::LaserMappingSequences s(c, 2, 0.4f, 0.8f, 2048, 8192, 1 << 16);\n"
                   "    s.set_vote(std::vector<int>{1, 0});\n"
                   "    lightloam::Drives d(c, 2, 2048, 8192, 1 << 16);\n"
                   "    d.set_map_vote(20);\n"
                   "    d.set_map_vote(-1);\n"
                   "    return (int)src.size();\n"
                   "}\n")
    subprocess.check_call(GXX + [str(src)])
    subprocess.check_call(GXX + [os.path.join(ROOT, "tools", "ll_kitti_drives.cpp")])
