"""The measured-information feature at the boundary, without a GPU: the library exports the entry points, api.EXPORTS lists them, the
header declares them with the argument counts the ctypes signatures have, the two new structs have the C sizes, the ABI version stays 3
(functions and new structs only), the kernels stay inside, the Python methods exist and the new lightloam_host.hpp members compile as
C++14."""
import ctypes as C
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"ll_cubemaps_localize_slots_info": 7, "ll_cubemaps_align_info": 9, "ll_drives_set_info": 2, "ll_drives_info": 2,
         "ll_pg_edge_from_info": 5, "ll_posegraphs_evaluate6": 9, "ll_posegraphs_solve6": 9}
GXX = ["g++", "-std=c++14", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include")]


def test_library_exports_the_entry_points(api):
    lib = api.load_library()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in api.EXPORTS, name
    assert lib.ll_abi_version() == 3
    for name in ("k_cms_info", "k_al_infosum", "ll_launch_cms_info", "ll_info_finish", "ll_info_eig"):    # kernels and helpers stay inside
        assert not hasattr(lib, name), name


def _header_arguments(text, name):
    """the number of top-level commas + 1 in the declaration of `name`, comments removed"""
    decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    assert decl, name
    return decl.group(1).count(",") + 1


def test_signatures_and_structs_match_the_header(api):
    text = open(os.path.join(ROOT, "include", "lightloam_hip.h")).read()
    lib = api.load_library()
    for name, n in NAMES.items():
        assert _header_arguments(text, name) == n == len(getattr(lib, name).argtypes), name
    assert "#define LL_ABI_VERSION 3 " in text
    plain = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    assert "typedef struct { double H[36]; double g[6]; double eig[6]; double sigma2; int rows; int flags; } ll_pose_info;" in plain
    assert "typedef struct { int i, j; double Z_w7[7]; double S[36]; double huber; } ll_pg_edge6;" in plain
    assert "int ll_pg_edge_from_info(const ll_pose_info *info, const double *X_w7, double sigma, double floor, double S36[36]);" in plain
    assert C.sizeof(api.PoseInfo) == 400                            # 49 doubles and two ints
    assert [n for n, _ in api.PoseInfo._fields_] == ["H", "g", "eig", "sigma2", "rows", "flags"]
    assert (api.PoseInfo.g.offset, api.PoseInfo.eig.offset, api.PoseInfo.sigma2.offset, api.PoseInfo.rows.offset, api.PoseInfo.flags.offset) == (288, 336, 384, 392, 396)
    assert C.sizeof(api.PgEdge6) == 360 == api.PG_EDGE6.itemsize    # two ints, 7 + 36 + 1 doubles
    assert [n for n, _ in api.PgEdge6._fields_] == list(api.PG_EDGE6.names)
    assert [api.PG_EDGE6.fields[n][1] for n in api.PG_EDGE6.names] == [getattr(api.PgEdge6, n).offset for n in api.PG_EDGE6.names]
    assert C.sizeof(api.PgEdge) == 120 == api.PG_EDGE.itemsize      # the diagonal edge is what it was


def test_python_methods_exist(api):
    for f in (api.Drives.set_info, api.Drives.info, api.edge_from_info, api.pg_edges6):
        assert callable(f)
    assert inspect.signature(api.CubeMaps.localize_slots).parameters["info"].default is False
    assert inspect.signature(api.CubeMaps.align).parameters["info"].default is False
    sig = inspect.signature(api.edge_from_info)
    assert list(sig.parameters) == ["info", "X", "sigma", "floor"] and sig.parameters["sigma"].default == 0.0 and sig.parameters["floor"].default == 0.0
    import lightloam_amd  # noqa: F401
    from lightloam_amd import build as b
    for src in ("ll_localize.hip", "ll_map_align.hip", "ll_posegraph.hip"):
        assert src in b.HIP_SOURCES
    assert os.path.exists(os.path.join(ROOT, "light-loam_amd", "csrc", "ll_pose_info.h"))


def test_host_wrapper_compiles_as_cxx14(tmp_path):
    src = tmp_path / "use_info.cpp"
    src.write_text("#include \"lightloam_host.hpp\"\n"
                   "static_assert(sizeof(lightloam::PoseInfo) == 400 && sizeof(ll_pg_edge6) == 360, \"layout\");\n"
                   "int run(lightloam::LaserMappingSequences &seq, lightloam::Drives &drives, lightloam::Context &c) {\n"
                   "    std::vector<int> slots((size_t)seq.S, 0), map_of((size_t)seq.S, 0), ran;\n"
                   "    std::vector<lightloam::PoseInfo> info;\n"
                   "    seq.localize_slots(slots, map_of, true, &info);\n"
                   "    seq.localize_slots(slots, map_of, false, &info);\n"
                   "    seq.localize_slots(slots);\n"
                   "    std::vector<ll_merge_op> ops(1);\n"
                   "    std::vector<double> T;\n"
                   "    std::vector<ll_localize_fit> fit;\n"
                   "    std::vector<lightloam::PoseInfo> ainfo;\n"
                   "    seq.align_maps(ops, 2, &T, &ran, &fit, &ainfo);\n"
                   "    seq.align_maps(ops, 0, &T, &ran, &fit);\n"
                   "    drives.set_info(true);\n"
                   "    std::vector<lightloam::PoseInfo> dinfo = drives.info();\n"
                   "    double S[36], Z[7];\n"
                   "    lightloam::PoseGraphs::edge_from_info(info[0], &seq.parameters[0], 0.05, 1e-6, S);\n"
                   "    lightloam::PoseGraphs pg(c, 4, 100, 200);\n"
                   "    std::vector<lightloam::PoseGraphs::Graph6> graphs(1);\n"
                   "    graphs[0].poses = {0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1, 1, 0, 0};\n"
                   "    lightloam::PoseGraphs::relative_pose(&graphs[0].poses[0], &graphs[0].poses[7], Z);\n"
                   "    graphs[0].edges.push_back(lightloam::PoseGraphs::edge6(0, 1, Z, S, 0.5));\n"
                   "    graphs[0].edges.push_back(lightloam::PoseGraphs::edge6(lightloam::PoseGraphs::edge(1, 0, Z, 10.0, 1.0)));\n"
                   "    lightloam::PoseGraphs::Evaluation ev = pg.evaluate(graphs);\n"
                   "    std::vector<ll_pg_record> rec = pg.solve(graphs);\n"
                   "    return rec[0].termination + (int)ev.cost[0] + dinfo[0].rows + ainfo[0].flags;\n"
                   "}\n")
    subprocess.check_call(GXX + [str(src)])


def test_the_drives_tool_takes_info():
    path = os.path.join(ROOT, "tools", "ll_kitti_drives.cpp")
    text = open(path).read()
    assert '"--info"' in text and "_info.txt" in text and "d.set_info(true)" in text
    subprocess.check_call(GXX + [path])
