"""ll_posegraphs_covariances and ll_pg_edge_gate at the boundary, without a GPU: the library exports the entry points, api.EXPORTS lists
them, the header declares them word for word with the argument counts of the ctypes signatures, the structs have the header's sizes,
the kernels stay inside, the defaults are the header's, a NULL handle is refused without a device, lightloam::PoseGraphs compiles as
C++14 with the new members, and the gate -- host arithmetic -- equals the numpy restatement and returns each of its errors."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import pgcovcases as cv
import posegraphcases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"ll_pg_cov_default_options": 1, "ll_posegraphs_covariances": 12, "ll_posegraphs_covariances6": 12, "ll_posegraphs_cov_timing": 3,
         "ll_pg_edge_gate": 7}
LINES = ["typedef struct { int graph, a, b; } ll_pg_cov_query;",
         "typedef struct { int max_pcg_iterations; double tolerance; } ll_pg_cov_options;",
         "typedef struct { int status, pcg_iterations; double residual; } ll_pg_cov_record;",
         "void ll_pg_cov_default_options(ll_pg_cov_options *o);",
         "int ll_posegraphs_covariances(ll_posegraphs *pg, int n_graphs, const int *node_off, const int *edge_off, const double *poses_w7, "
         "const unsigned char *fixed, const ll_pg_edge *edges, int n_queries, const ll_pg_cov_query *q, const ll_pg_cov_options *opt, "
         "double *joint144, ll_pg_cov_record *rec);",
         "int ll_posegraphs_covariances6(ll_posegraphs *pg, int n_graphs, const int *node_off, const int *edge_off, const double *poses_w7, "
         "const unsigned char *fixed, const ll_pg_edge6 *edges, int n_queries, const ll_pg_cov_query *q, const ll_pg_cov_options *opt, "
         "double *joint144, ll_pg_cov_record *rec);",
         "int ll_posegraphs_cov_timing(ll_posegraphs *pg, double ms2[2], long long counts3[3]);",
         "int ll_pg_edge_gate(const double *Pa_w7, const double *Pb_w7, const double *Z_w7, const double *S36, const double joint144[144], "
         "double *chi2, double cov36[36]);"]
GXX = ["g++", "-std=c++14", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include")]


def test_library_exports_the_covariances(api):
    lib = api.load_library()
    for name, n in NAMES.items():
        assert hasattr(lib, name), name
        assert name in api.EXPORTS, name
        assert len(getattr(lib, name).argtypes) == n, name
    assert lib.ll_abi_version() == 3                                # functions and structs of their own only
    for name in ("k_pg_cov_prepare", "k_pg_cov_columns", "k_pg_cov_gather", "pg_cov_run", "pg_error", "pg_jacobians", "pg_error_z"):
        assert not hasattr(lib, name), name


def test_the_header_declares_them_word_for_word(api):
    text = open(os.path.join(ROOT, "include", "lightloam_hip.h")).read()
    plain = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    for line in LINES:
        assert line in plain, line
    assert "4 x the rotation block" in re.sub(r"\s+", " ", text)  # the rotation-vector covariance
    assert "NOT in the graph" in text                               # what the gate's chi-square is valid for
    assert C.sizeof(api.PgCovQuery) == 12 and C.sizeof(api.PgCovOptions) == 16 and C.sizeof(api.PgCovRecord) == 16
    assert api.PG_COV_QUERY.itemsize == 12
    assert C.sizeof(api.PgOptions) == 88 and C.sizeof(api.PgRecord) == 40          # the solves' structs keep their sizes


def test_default_options(api):
    o = api.pg_cov_options()
    assert (o.max_pcg_iterations, o.tolerance) == (1000, 1e-10)
    o = api.pg_cov_options(max_pcg_iterations=7)
    assert (o.max_pcg_iterations, o.tolerance) == (7, 1e-10)
    api.load_library().ll_pg_cov_default_options(None)              # a NULL pointer is ignored
    with pytest.raises(AttributeError):
        api.pg_cov_options(eta=0.5)


def test_python_methods_exist(api):
    P = api.PoseGraphs
    for f in (P.covariances, P.cov_timing, api.edge_gate, api.pg_cov_options):
        assert callable(f)
    assert api.PG_COV_STATUS == {0: "converged", 1: "iterations", 2: "breakdown"}


def test_a_null_handle_is_refused_without_a_device(api):
    lib = api.load_library()
    ms = (C.c_double * 2)(); counts = (C.c_longlong * 3)()
    assert lib.ll_posegraphs_covariances(None, 0, None, None, None, None, None, 0, None, None, None, None) == -2
    assert lib.ll_posegraphs_covariances6(None, 0, None, None, None, None, None, 0, None, None, None, None) == -2
    assert lib.ll_posegraphs_cov_timing(None, C.addressof(ms), C.addressof(counts)) == -2


# ------------------------------------------------------------------------------------------------ the gate
def gate_case():
    """the 40-node chain at its start poses (the gate does not need an optimum), a 5 m false loop and a true one"""
    truth, start, edges = pc.noisy_chain("cm")
    S, _ = cv.sigma(start, edges)
    return truth, start, S


def test_the_gate_matches_the_restatement(api):
    truth, x, S = gate_case()
    rng = np.random.default_rng(8)
    full = np.triu(rng.normal(size=(6, 6))) + 3.0 * np.eye(6)
    worst = 0.0
    for a, b in ((20, 2), (2, 20), (35, 3), (10, 30), (7, 7 + 1)):
        J = cv.joint(S, a, b)
        for Z in (pc.relative(truth[a], truth[b]), pc.false_loop(truth, a, b)[2], 3.0 * pc.relative(truth[a], truth[b])):
            for info in (None, np.array([2.0, 3.0, 4.0, 0.5, 1.0, 1.5]), full):
                want, Cw = cv.gate(x[a], x[b], Z, info, J)
                got, Cg = api.edge_gate(x[a], x[b], Z, info, J, with_cov=True)
                assert api.edge_gate(x[a], x[b], Z, info, J) == got
                worst = max(worst, abs(got - want) / want, np.abs(Cg - Cw).max() / np.abs(Cw).max())
    print(f"gate: worst relative difference of chi2 and C from the restatement {worst:.3g}")
    assert worst <= 1e-12


def test_the_gate_scales_unnormalised_quaternions_away(api):
    truth, x, S = gate_case()
    a, b = 20, 2
    Z = pc.false_loop(truth)[2]
    J = cv.joint(S, a, b)
    one = api.edge_gate(x[a], x[b], Z, None, J)
    Pa = x[a].copy(); Pa[:4] *= 2.0
    Pb = x[b].copy(); Pb[:4] *= -0.5
    assert api.edge_gate(Pa, Pb, Z, None, J) == pytest.approx(one, rel=1e-12)


def test_the_gate_returns_each_of_its_errors(api):
    lib = api.load_library()
    truth, x, S = gate_case()
    a, b = 20, 2
    good = dict(Pa=x[a].copy(), Pb=x[b].copy(), Z=pc.relative(truth[a], truth[b]), S=np.eye(6), J=cv.joint(S, a, b))

    def call(**kw):
        v = {k: (None if k in kw and kw[k] is None else np.ascontiguousarray(kw.get(k, good[k]), np.float64)) for k in good}
        chi2 = C.c_double(-1.0); cov = np.full(36, -1.0)
        ptr = lambda arr: None if arr is None else arr.ctypes.data
        rc = lib.ll_pg_edge_gate(ptr(v["Pa"]), ptr(v["Pb"]), ptr(v["Z"]), ptr(v["S"]), ptr(v["J"]), C.addressof(chi2), cov.ctypes.data)
        if rc != 0:
            assert chi2.value == -1.0 and (cov == -1.0).all()       # the outputs are untouched
        return rc

    assert call() == 0 and call(S=None) == 0
    for key in ("Pa", "Pb", "Z", "J"):
        assert call(**{key: None}) == -2, key
        for junk in (np.nan, np.inf):
            arr = good[key].copy().reshape(-1); arr[-1] = junk
            assert call(**{key: arr}) == -2, (key, junk)
    bad_S = np.eye(6); bad_S[2, 3] = np.nan
    assert call(S=bad_S) == -2
    for key in ("Pa", "Pb", "Z"):
        arr = good[key].copy(); arr[:4] = 0.0
        assert call(**{key: arr}) == -2, key                        # a zero quaternion
    rank5 = np.eye(6); rank5[5, 5] = 0.0
    assert call(S=rank5) == -2                                      # S^T S is not positive definite
    assert call(J=np.zeros((12, 12)), S=None) == -2                 # C = 0 is not positive definite
    assert call(J=-good["J"], S=None) == -2
    assert call(J=np.zeros((12, 12))) == 0                          # the edge's own covariance carries C
    assert lib.ll_pg_edge_gate(good["Pa"].ctypes.data, good["Pb"].ctypes.data, good["Z"].ctypes.data, None, good["J"].ctypes.data, None, None) == -2
    with pytest.raises(api.LightLoamError) as ei:
        api.edge_gate(good["Pa"], good["Pb"], good["Z"], rank5, good["J"])
    assert ei.value.code == -2


def test_host_wrapper_compiles_as_cxx14(tmp_path):
    src = tmp_path / "use_pgcov.cpp"
    src.write_text("#include \"lightloam_host.hpp\"\n"
                   "int run() {\n"
                   "    lightloam::Context c(16, 4);\n"
                   "    lightloam::PoseGraphs pg(c, 4, 100, 200);\n"
                   "    std::vector<lightloam::PoseGraphs::Graph> graphs(1);\n"
                   "    graphs[0].poses = {0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1, 1, 0, 0};\n"
                   "    double Z[7];\n"
                   "    lightloam::PoseGraphs::relative_pose(&graphs[0].poses[0], &graphs[0].poses[7], Z);\n"
                   "    graphs[0].edges.push_back(lightloam::PoseGraphs::edge(0, 1, Z, 10.0, 1.0));\n"
                   "    std::vector<ll_pg_cov_query> q = {{0, 1, -1}, {0, 0, 1}};\n"
                   "    ll_pg_cov_options o = lightloam::PoseGraphs::default_cov_options();\n"
                   "    lightloam::PoseGraphs::Covariances cv = pg.covariances(graphs, q, &o);\n"
                   "    std::vector<lightloam::PoseGraphs::Graph6> graphs6(1);\n"
                   "    graphs6[0].poses = graphs[0].poses;\n"
                   "    graphs6[0].edges.push_back(lightloam::PoseGraphs::edge6(graphs[0].edges[0]));\n"
                   "    lightloam::PoseGraphs::Covariances cv6 = pg.covariances(graphs6, q);\n"
                   "    double ms[2]; long long counts[3];\n"
                   "    pg.cov_timing(ms, counts);\n"
                   "    double C36[36];\n"
                   "    double chi2 = lightloam::PoseGraphs::edge_gate(&graphs[0].poses[0], &graphs[0].poses[7], Z, nullptr, &cv.joint[144], C36);\n"
                   "    return cv.records[0].status + cv6.records[1].pcg_iterations + (int)counts[0] + (int)cv.joint.size() + (chi2 > 22.46);\n"
                   "}\n")
    subprocess.check_call(GXX + [str(src)])
