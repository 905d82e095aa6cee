"""The cube map's pair-table bookkeeping (csrc/ll_cubemap_tables.h: centre cube, shift loops, valid list, the update's plan / fit /
commit) against a naive one-cloud-per-cube model, on the host alone: tests/native/cubemap_tables_host.cpp is a stand-alone program
that includes nothing but that header.  It is built with AddressSanitizer and UBSan and run as a child process."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "light-loam_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "native", "cubemap_tables_host.cpp")


def test_header_needs_no_hip():
    text = open(os.path.join(CSRC, "ll_cubemap_tables.h")).read()
    includes = [ln.split()[1] for ln in text.splitlines() if ln.startswith("#include")]
    assert sorted(includes) == ["<algorithm>", "<cstddef>", "<string>", "<vector>"]


def test_tables_against_the_naive_model(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the host program"
    exe = str(tmp_path / "cubemap_tables_host")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                    "-I", CSRC, "-o", exe, SRC], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.startswith("frames "), run.stdout
