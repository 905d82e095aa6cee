"""ll_odometry_sequences at the boundary, without a GPU: the library exports it, the ctypes layout follows the header, and the C++
host mirror's wrapper compiles as C++14."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_odometry_sequences(api):
    lib = api.load_library()
    assert hasattr(lib, "ll_odometry_sequences")
    assert "ll_odometry_sequences" in api.EXPORTS


def test_seq_layout_matches_the_header():
    from lightloam_amd import api
    text = open(os.path.join(ROOT, "include", "lightloam_hip.h")).read()
    m = re.search(r"typedef struct \{([^{}]*)\}\s*ll_seq_layout;", text)
    assert m, "ll_seq_layout not declared"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = re.findall(r"\bint\s+(\w+)\s*;", body)
    assert fields == [f for f, _ in api.SeqLayout._fields_] == ["base", "n_seq", "ring_rows"]
    assert api.sequence_slot(api.SeqLayout(4, 3, 5), 7, 2) == 4 + (7 % 5) * 3 + 2


def test_host_wrapper_compiles_as_cxx14(tmp_path):
    src = tmp_path / "use_sequences.cpp"
    src.write_text("#include \"lightloam_host.hpp\"\n"
                   "std::vector<double> run(lightloam::Context &c) {\n"
                   "    ll_seq_layout L; L.base = 0; L.n_seq = 4; L.ring_rows = 8;\n"
                   "    const int rows[4] = {7, 7, 3, 0};\n"
                   "    return lightloam::odometry_sequences(c, L, 1, 7, rows);\n"
                   "}\n")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])
