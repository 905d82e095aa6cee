"""The tile / segment vocabulary of the tiled kernels (csrc/ll_tiles.h: LLTiler's numbering, ll_tile_find's binary search over the
segments' first tiles) against prefix sums and a linear scan, on the host alone: tests/native/tiles_host.cpp is a stand-alone program
that includes nothing but that header.  It is built with AddressSanitizer and UBSan and run as a child process."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "light-loam_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "native", "tiles_host.cpp")


def test_header_needs_no_hip():
    text = open(os.path.join(CSRC, "ll_tiles.h")).read()
    includes = [ln.split()[1] for ln in text.splitlines() if ln.startswith("#include")]
    assert includes == []                         # plain C++: no HIP header, nothing of the library
    program = [ln.split()[1] for ln in open(SRC).read().splitlines() if ln.startswith("#include")]
    assert sorted(program) == ['"ll_tiles.h"', "<cstdio>", "<cstdlib>", "<vector>"]


def test_tiler_and_find_on_crafted_segments(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the host program"
    exe = str(tmp_path / "tiles_host")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                    "-I", CSRC, "-o", exe, SRC], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.startswith("tables "), run.stdout
    tables, tiles = int(run.stdout.split()[1]), int(run.stdout.split()[3])
    assert tables == 2 * (6 + 36 + 216 + 3) and tiles > 2 * 3 * 300        # every crafted table ran, the large ones tile by tile
