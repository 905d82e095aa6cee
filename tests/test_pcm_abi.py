"""The pcm ABI without a GPU: the built library and api.EXPORTS hold the new symbols, the header declares them verbatim and compiles as C,
the structs that cross the boundary have the same size and field offsets in C and in ctypes, the ABI version stays, NULL handles are
refused, and the C++ wrapper compiles."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SYMBOLS = ["ll_pcm_default_params", "ll_pcm_create", "ll_pcm_destroy", "ll_pcm_last_error", "ll_pcm_run", "ll_pcm_select", "ll_pcm_adjacency",
           "ll_pcm_timing", "ll_pcm_host"]

DECLARATIONS = [
    "typedef struct ll_pcm ll_pcm;",
    "typedef struct { double rot_tol, trans_tol, rot_rate, trans_rate; } ll_pcm_params;",
    "typedef struct { int i, j; double Z_w7[7]; } ll_pcm_candidate;",
    "typedef struct { int n_candidates, n_selected, start /* original index, -1: none */, max_degree; long long n_consistent_pairs; } ll_pcm_record;",
    "void ll_pcm_default_params(ll_pcm_params *p);",
    "int  ll_pcm_create(ll_ctx *ctx, int max_graphs, int max_nodes_total, int max_candidates_total, ll_pcm **out);",
    "void ll_pcm_destroy(ll_pcm *pcm);",
    "const char *ll_pcm_last_error(const ll_pcm *pcm);",
    "int  ll_pcm_run(ll_pcm *pcm, int n_graphs, const int *node_off, const int *cand_off, const double *poses_w7,",
    "int  ll_pcm_select(ll_pcm *pcm, int n_graphs, const int *cand_off, const unsigned long long *words, unsigned char *selected,",
    "int  ll_pcm_adjacency(ll_pcm *pcm, int graph, unsigned long long *words_out);",
    "int  ll_pcm_timing(const ll_pcm *pcm, double *ms /* [5] */, long long *counts /* [4] */);",
    "int  ll_pcm_host(int n_nodes, const double *poses_w7, int n_candidates, const ll_pcm_candidate *candidates, const ll_pcm_params *params,",
]

STRUCTS = {"ll_pcm_params": ("PcmParams", ["rot_tol", "trans_tol", "rot_rate", "trans_rate"]),
           "ll_pcm_record": ("PcmRecord", ["n_candidates", "n_selected", "start", "max_degree", "n_consistent_pairs"])}


def test_symbols_exist_in_the_library_and_in_exports(api):
    lib = api.load_library()
    for s in SYMBOLS:
        assert hasattr(lib, s), s
        assert s in api.EXPORTS, s
    assert lib.ll_abi_version() == 3                                  # functions and structs of their own only: the version stays


def test_header_declares_them_verbatim():
    text = open(os.path.join(ROOT, "include", "lightloam_hip.h")).read()
    for d in DECLARATIONS:
        assert d in text, d
    assert "#define LL_ABI_VERSION 3 " in text


def test_header_compiles_as_c_and_layouts_match(api, tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "lightloam_hip.h"', 'int main(void) {']
    for cname, (_, fields) in STRUCTS.items():
        lines.append(f'  printf("{cname} size %zu\\n", sizeof({cname}));')
        for f in fields:
            lines.append(f'  printf("{cname} {f} %zu\\n", offsetof({cname}, {f}));')
    lines.append('  printf("ll_pcm_candidate size %zu\\n", sizeof(ll_pcm_candidate));')
    for f in ("i", "j", "Z_w7"):
        lines.append(f'  printf("ll_pcm_candidate {f} %zu\\n", offsetof(ll_pcm_candidate, {f}));')
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = {}
    for line in subprocess.check_output([str(exe)], text=True).splitlines():
        cname, field, value = line.split()
        got[(cname, field)] = int(value)
    for cname, (pyname, fields) in STRUCTS.items():
        T = getattr(api, pyname)
        assert [n for n, _ in T._fields_] == fields, cname
        assert got[(cname, "size")] == C.sizeof(T), cname
        for f in fields:
            assert got[(cname, f)] == getattr(T, f).offset, (cname, f)
    d = api.PCM_CANDIDATE                                              # the candidate crosses as a numpy record
    assert got[("ll_pcm_candidate", "size")] == d.itemsize == 64
    for f in ("i", "j", "Z_w7"):
        assert got[("ll_pcm_candidate", f)] == d.fields[f][1], f


def test_default_params_are_the_headers(api):
    import pcmcases as pc
    p = api.pcm_params()
    assert (p.rot_tol, p.trans_tol, p.rot_rate, p.trans_rate) == (0.05, 0.5, 2e-4, 0.02)
    assert {k: getattr(p, k) for k in pc.DEFAULT} == pc.DEFAULT
    assert api.pcm_params(trans_tol=1.0).trans_tol == 1.0


def test_null_handles_are_refused(api):
    lib = api.load_library()
    one = (C.c_int * 2)(0, 0)
    assert lib.ll_pcm_run(None, 0, one, one, None, None, None, None, None, None) == -2
    assert lib.ll_pcm_select(None, 0, one, None, None, None, None) == -2
    assert lib.ll_pcm_adjacency(None, 0, None) == -2
    assert lib.ll_pcm_timing(None, None, None) == -2
    out = C.c_void_p()
    assert lib.ll_pcm_create(None, 1, 1, 1, C.byref(out)) == -2 and not out.value
    assert lib.ll_pcm_last_error(None)                                 # a text, not a crash
    lib.ll_pcm_destroy(None); lib.ll_pcm_default_params(None)


def test_python_methods_exist(api):
    for name in ("run", "select", "adjacency", "timing", "close"):
        assert callable(getattr(api.Pcm, name)), name
    assert callable(api.Context.pcm) and callable(api.pcm_params) and callable(api.pcm_host)
    e = api.pg_edges([(0, 1, [0, 0, 0, 1, 1, 2, 3], 1.0, 0.0)])
    c = api.pcm_candidates(e)                                          # a pose-graph edge passes as it is, as a record array or as a tuple
    assert (c["i"], c["j"]) == (0, 1) and c["Z_w7"][0].tolist() == [0, 0, 0, 1, 1, 2, 3]
    assert api.pcm_candidates([(0, 1, [0, 0, 0, 1, 1, 2, 3], 1.0, 0.0)]).tobytes() == c.tobytes()


def test_host_wrapper_compiles_as_cxx14(tmp_path):
    src = tmp_path / "use_pcm.cpp"
    src.write_text("#include \"lightloam_host.hpp\"\n"
                   "int run(lightloam::Context &c, const ll_pg_edge &e) {\n"
                   "    lightloam::Pcm pcm(c, 4, 100, 100);\n"
                   "    lightloam::Pcm::Graph g; g.poses.assign(14, 0.0);\n"
                   "    const double Z[7] = {0, 0, 0, 1, 0, 0, 0};\n"
                   "    g.candidates.push_back(lightloam::Pcm::candidate(0, 1, Z));\n"
                   "    g.candidates.push_back(lightloam::Pcm::candidate(e));\n"
                   "    ll_pcm_params p = lightloam::Pcm::default_params();\n"
                   "    lightloam::Pcm::Result r = pcm.run(std::vector<lightloam::Pcm::Graph>(1, g), &p);\n"
                   "    std::vector<unsigned long long> w = pcm.adjacency(0, 2);\n"
                   "    r = pcm.select(std::vector<std::vector<unsigned long long> >(1, w), std::vector<int>(1, 2));\n"
                   "    double ms[5]; long long n[4];\n"
                   "    pcm.timing(ms, n);\n"
                   "    std::vector<unsigned char> sel; std::vector<int> deg; ll_pcm_record rec;\n"
                   "    return lightloam::Pcm::host(g, &p, &w, sel, &deg, &rec) + r.rec[0].n_selected + r.selected[0][0] + r.degree[0][0] + (int)n[3]\n"
                   "           + (int)lightloam::Pcm::words(65) + (pcm.get() != nullptr);\n"
                   "}\n")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])
