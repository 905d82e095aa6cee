"""ll_places at the boundary, without a GPU: the library exports the entry points, api.EXPORTS lists them, the header declares them
with the argument counts the Python wrapper's ctypes signatures have, the ABI version stays 3 (functions only, no struct changed),
the Python methods exist, the kernels' file is one of the library's sources, and lightloam::Places compiles as C++14."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"ll_places_default_params": 2, "ll_places_create": 3, "ll_places_destroy": 1, "ll_places_last_error": 1, "ll_places_size": 1,
         "ll_places_reset": 1, "ll_places_add_slots": 4, "ll_places_add_points": 4, "ll_places_upload": 4, "ll_places_download": 4,
         "ll_places_distances": 7, "ll_places_match": 10, "ll_places_timing": 3}
GXX = ["g++", "-std=c++14", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include")]


def test_library_exports_the_places(api):
    lib = api.load_library()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in api.EXPORTS, name
    assert lib.ll_abi_version() == 3
    for name in ("k_pl_gram", "k_pl_describe", "pl_describe"):      # kernels and helpers stay inside the library (C++ linkage)
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
    assert "typedef struct { int capacity; float max_radius, z_offset; } ll_places_params;" in plain
    assert "int ll_places_add_slots(ll_places *db, const int *slots, int count, int *first_id);" in plain
    assert "int ll_places_add_points(ll_places *db, const ll_point *host, int n, int *id);" in plain
    assert "int ll_places_upload(ll_places *db, int first, int count, const float *desc1200);" in plain
    assert "int ll_places_distances(ll_places *db, int q0, int nq, int c0, int nc, float *dist, unsigned char *shift);" in plain
    assert ("int ll_places_match(ll_places *db, int q0, int nq, int c0, int nc, const int *c_end, int K, int *id, float *dist, "
            "unsigned char *shift);") in plain
    import ctypes as C
    assert C.sizeof(api.PlacesParams) == 12


def test_python_methods_and_sources_exist(api):
    P = api.Places
    for f in (P.add_slots, P.add_points, P.upload, P.download, P.distances, P.match, P.timing, P.reset, api.Context.places):
        assert callable(f)
    import lightloam_amd  # noqa: F401
    from lightloam_amd import build as b
    assert "ll_place.hip" in b.HIP_SOURCES
    assert os.path.exists(os.path.join(ROOT, "light-loam_amd", "csrc", "ll_place.hip"))


def test_default_params_need_no_device(api):
    p = api.PlacesParams()
    api.load_library().ll_places_default_params(__import__("ctypes").byref(p), 77)
    assert (p.capacity, p.max_radius, p.z_offset) == (77, 80.0, 2.0)


def test_host_wrapper_compiles_as_cxx14(tmp_path):
    src = tmp_path / "use_places.cpp"
    src.write_text("#include \"lightloam_host.hpp\"\n"
                   "int run() {\n"
                   "    lightloam::Context c(16, 4);\n"
                   "    lightloam::Places db(c, 1024);\n"
                   "    lightloam::Places db2(c, 64, 100.0f, 1.73f);\n"
                   "    int first = db.add_slots(std::vector<int>{0, 1, 2});\n"
                   "    std::vector<lightloam::PointXYZI> cloud(100);\n"
                   "    int id = db.add_points(cloud);\n"
                   "    std::vector<float> desc = db.download(first, 3);\n"
                   "    db2.upload(0, desc);\n"
                   "    lightloam::Places::Match all = db.distances(id, 1, 0, 3);\n"
                   "    lightloam::Places::Match best = db.match(id, 1, 0, 3, 2);\n"
                   "    lightloam::Places::Match past = db.match(id, 1, 0, 3, 1, std::vector<int>{2});\n"
                   "    double ms[3]; long long counts[2];\n"
                   "    db.timing(ms, counts);\n"
                   "    db.reset();\n"
                   "    return db.size() + best.id[0] + past.id[0] + (int)all.shift[0];\n"
                   "}\n")
    subprocess.check_call(GXX + [str(src)])
