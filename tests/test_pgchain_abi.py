"""The chain preconditioner at the boundary, without a GPU: the library exports the four entry points, api.EXPORTS lists them, the
header declares them word for word with the argument counts of the ctypes signatures, the two kinds are defined, the structs keep their
sizes, the kernels stay inside, the Python methods exist, a NULL handle is refused without a device, and lightloam::PoseGraphs compiles
as C++14 with the new members."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"ll_posegraphs_set_preconditioner": 2, "ll_posegraphs_preconditioner": 1, "ll_posegraphs_precond_stats": 2,
         "ll_posegraphs_chain_solve": 8}
LINES = ["#define LL_PG_PRECOND_BLOCK_JACOBI 0",
         "#define LL_PG_PRECOND_CHAIN 1",
         "int ll_posegraphs_set_preconditioner(ll_posegraphs *pg, int kind);",
         "int ll_posegraphs_preconditioner(const ll_posegraphs *pg);",
         "int ll_posegraphs_precond_stats(ll_posegraphs *pg, long long counts2[2]);",
         "int ll_posegraphs_chain_solve(ll_posegraphs *pg, int n_systems, const int *node_off, const double *diag36, const double *upper36, "
         "const double *rhs6, double *out6, int *status);"]
GXX = ["g++", "-std=c++14", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include")]


def test_library_exports_the_preconditioner(api):
    lib = api.load_library()
    for name, n in NAMES.items():
        assert hasattr(lib, name), name
        assert name in api.EXPORTS, name
        assert len(getattr(lib, name).argtypes) == n, name
    assert lib.ll_abi_version() == 3                                # functions only
    for name in ("k_pg_chain_solve", "pg_chain_factor", "pg_chain_apply", "pg_chain_matrix", "pg_chain_alloc"):
        assert not hasattr(lib, name), name


def test_the_header_declares_them_word_for_word(api):
    text = open(os.path.join(ROOT, "include", "lightloam_hip.h")).read()
    plain = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    for line in LINES:
        assert line in plain, line
    assert "#define LL_ABI_VERSION 3 " in text
    assert C.sizeof(api.PgOptions) == 88 and C.sizeof(api.PgRecord) == 40          # the switch lives on the object
    assert (api.PG_PRECOND_BLOCK_JACOBI, api.PG_PRECOND_CHAIN) == (0, 1)
    assert api.PG_PRECOND_NAMES == {"jacobi": 0, "chain": 1}


def test_python_methods_exist(api):
    P = api.PoseGraphs
    for f in (P.set_preconditioner, P.precond_stats, P.chain_solve):
        assert callable(f)
    assert isinstance(P.preconditioner, property)


def test_a_null_handle_is_refused_without_a_device(api):
    lib = api.load_library()
    counts = (C.c_longlong * 2)()
    assert lib.ll_posegraphs_set_preconditioner(None, 1) == -2
    assert lib.ll_posegraphs_preconditioner(None) == -2
    assert lib.ll_posegraphs_precond_stats(None, C.addressof(counts)) == -2
    assert lib.ll_posegraphs_chain_solve(None, 0, None, None, None, None, None, None) == -2


def test_host_wrapper_compiles_as_cxx14(tmp_path):
    src = tmp_path / "use_pgchain.cpp"
    src.write_text("#include \"lightloam_host.hpp\"\n"
                   "int run() {\n"
                   "    lightloam::Context c(16, 4);\n"
                   "    lightloam::PoseGraphs pg(c, 4, 100, 200);\n"
                   "    pg.set_preconditioner(LL_PG_PRECOND_CHAIN);\n"
                   "    const lightloam::PoseGraphs &cpg = pg;\n"
                   "    int kind = cpg.preconditioner();\n"
                   "    std::vector<lightloam::PoseGraphs::Graph> graphs(1);\n"
                   "    graphs[0].poses = {0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1, 1, 0, 0};\n"
                   "    double Z[7];\n"
                   "    lightloam::PoseGraphs::relative_pose(&graphs[0].poses[0], &graphs[0].poses[7], Z);\n"
                   "    graphs[0].edges.push_back(lightloam::PoseGraphs::edge(0, 1, Z, 10.0, 1.0));\n"
                   "    std::vector<ll_pg_record> rec = pg.solve(graphs);\n"
                   "    long long counts[2];\n"
                   "    pg.precond_stats(counts);\n"
                   "    std::vector<int> node_off = {0, 2};\n"
                   "    std::vector<double> diag(72, 0.0), upper(72, 0.0), rhs(12, 1.0);\n"
                   "    for (int k = 0; k < 12; ++k) diag[(k / 6) * 36 + (k % 6) * 7] = 2.0;\n"
                   "    lightloam::PoseGraphs::ChainSolution s = pg.chain_solve(node_off, diag, upper, rhs);\n"
                   "    pg.set_preconditioner(LL_PG_PRECOND_BLOCK_JACOBI);\n"
                   "    return kind + rec[0].termination + (int)counts[0] + (int)counts[1] + s.status[0] + (int)s.x.size();\n"
                   "}\n")
    subprocess.check_call(GXX + [str(src)])
