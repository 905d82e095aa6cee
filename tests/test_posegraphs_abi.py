"""ll_posegraphs at the boundary, without a GPU: the library exports the entry points, api.EXPORTS lists them, the header declares them
with the argument counts the Python wrapper's ctypes signatures have, the structs have the C sizes, the ABI version stays 3 (functions
and new structs only), the kernels stay inside, the file is one of the library's sources, the default options need no device, and
lightloam::PoseGraphs compiles as C++14."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"ll_pg_default_options": 1, "ll_posegraphs_create": 5, "ll_posegraphs_destroy": 1, "ll_posegraphs_last_error": 1,
         "ll_posegraphs_evaluate": 9, "ll_posegraphs_solve": 9, "ll_posegraphs_timing": 3}
GXX = ["g++", "-std=c++14", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include")]


def test_library_exports_the_posegraphs(api):
    lib = api.load_library()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in api.EXPORTS, name
    assert lib.ll_abi_version() == 3
    for name in ("k_pg_solve", "pg_run", "pg_linearise", "pg_residual"):      # kernels and helpers stay inside the library
        assert not hasattr(lib, name), name


def _header_arguments(text, name):
    """the number of top-level commas + 1 in the declaration of `name`, comments removed"""
    decl = re.search(r"\b(?:int|void|char)\s*\*?\s*" + name + r"\s*\(([^;]*)\)\s*;", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    assert decl, name
    return decl.group(1).count(",") + 1


def test_signatures_match_the_header(api):
    text = open(os.path.join(ROOT, "include", "lightloam_hip.h")).read()
    lib = api.load_library()
    for name, n in NAMES.items():
        assert _header_arguments(text, name) == n == len(getattr(lib, name).argtypes), name
    assert "#define LL_ABI_VERSION 3 " in text
    plain = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    assert "typedef struct { int i, j; double Z_w7[7]; double sqrt_info[6]; double huber; } ll_pg_edge;" in plain
    assert ("typedef struct { double cost0, cost, grad_max; int lm_iterations, lm_successes, pcg_iterations, termination; } "
            "ll_pg_record;") in plain
    assert "int ll_posegraphs_create(ll_ctx *ctx, int max_graphs, int max_nodes_total, int max_edges_total, ll_posegraphs **out);" in plain
    assert ("int ll_posegraphs_solve(ll_posegraphs *pg, int n_graphs, const int *node_off, const int *edge_off, double *poses_w7, "
            "const unsigned char *fixed, const ll_pg_edge *edges, const ll_pg_options *opt, ll_pg_record *rec);") in plain
    assert C.sizeof(api.PgEdge) == 120 == api.PG_EDGE.itemsize
    assert C.sizeof(api.PgOptions) == 88 and C.sizeof(api.PgRecord) == 40
    assert [n for n, _ in api.PgEdge._fields_] == list(api.PG_EDGE.names)
    assert [api.PG_EDGE.fields[n][1] for n in api.PG_EDGE.names] == [getattr(api.PgEdge, n).offset for n in api.PG_EDGE.names]


def test_python_methods_and_sources_exist(api):
    P = api.PoseGraphs
    for f in (P.evaluate, P.solve, P.timing, api.Context.posegraphs, api.relative_pose, api.pg_options, api.pg_edges):
        assert callable(f)
    import lightloam_amd  # noqa: F401
    from lightloam_amd import build as b
    assert "ll_posegraph.hip" in b.HIP_SOURCES
    assert os.path.exists(os.path.join(ROOT, "light-loam_amd", "csrc", "ll_posegraph.hip"))


def test_default_options_need_no_device(api):
    o = api.PgOptions()
    api.load_library().ll_pg_default_options(C.byref(o))
    assert (o.max_lm_iterations, o.max_pcg_iterations, o.eta) == (50, 1000, 0.1)
    lm = api.LmOptions()
    api.load_library().ll_lm_default_options(C.byref(lm))
    for name in ("initial_radius", "max_radius", "min_radius", "min_relative_decrease", "min_lm_diagonal", "max_lm_diagonal",
                 "function_tolerance", "gradient_tolerance", "parameter_tolerance"):
        assert getattr(o, name) == getattr(lm, name), name
    assert api.pg_options(eta=0.01, max_lm_iterations=7).eta == 0.01


def test_packing_and_relative_pose(api):
    import numpy as np
    import posegraphcases as pc
    rng = np.random.default_rng(0)
    Pi, Pj = pc.random_pose(rng), pc.random_pose(rng)
    assert np.allclose(api.relative_pose(Pi, Pj), pc.relative(Pi, Pj), rtol=0, atol=1e-14)
    e = api.pg_edges([(0, 1, Pi, 2.0, 0.5), (1, 0, Pj, np.arange(6.0))])
    assert e.dtype == api.PG_EDGE and e["sqrt_info"][0].tolist() == [2.0] * 6 and e["huber"].tolist() == [0.5, 0.0]
    no, eo, poses, fixed, edges = api.PoseGraphs._pack([(np.stack([Pi, Pj]), e), (np.stack([Pj, Pi, Pi]), e[:1], [0, 0, 1])])
    assert no.tolist() == [0, 2, 5] and eo.tolist() == [0, 2, 3] and fixed.tolist() == [1, 0, 0, 0, 1] and poses.shape == (5, 7)


def test_host_wrapper_compiles_as_cxx14(tmp_path):
    src = tmp_path / "use_posegraphs.cpp"
    src.write_text("#include \"lightloam_host.hpp\"\n"
                   "int run() {\n"
                   "    lightloam::Context c(16, 4);\n"
                   "    lightloam::PoseGraphs pg(c, 4, 100, 200);\n"
                   "    std::vector<lightloam::PoseGraphs::Graph> graphs(2);\n"
                   "    for (auto &g : graphs) {\n"
                   "        g.poses = {0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1, 1, 0, 0};\n"
                   "        double Z[7];\n"
                   "        lightloam::PoseGraphs::relative_pose(&g.poses[0], &g.poses[7], Z);\n"
                   "        g.edges.push_back(lightloam::PoseGraphs::edge(0, 1, Z, 10.0, 1.0));\n"
                   "        g.edges.push_back(lightloam::PoseGraphs::edge(1, 0, Z, 10.0, 1.0, 0.5));\n"
                   "    }\n"
                   "    graphs[1].fixed = {0, 1};\n"
                   "    lightloam::PoseGraphs::Evaluation ev = pg.evaluate(graphs);\n"
                   "    ll_pg_options o = lightloam::PoseGraphs::default_options();\n"
                   "    o.max_lm_iterations = 10;\n"
                   "    std::vector<ll_pg_record> rec = pg.solve(graphs, &o);\n"
                   "    std::vector<ll_pg_record> rec2 = pg.solve(graphs);\n"
                   "    double ms[2]; long long counts[3];\n"
                   "    pg.timing(ms, counts);\n"
                   "    return rec[0].termination + rec2[1].lm_iterations + (int)ev.cost[0] + (int)ev.grad[1].size();\n"
                   "}\n")
    subprocess.check_call(GXX + [str(src)])
