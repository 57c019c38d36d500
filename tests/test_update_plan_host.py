"""The index arithmetic of vers_ivf_update_batch on the HOST (no GPU): tests/cpp/update_plan_demo.cpp includes
vers_amd/csrc/update_plan.hpp -- a header without a HIP dependency, the one the kernels include -- under the host compiler, built as a
stand-alone program with -fsanitize=address,undefined.  It emulates the locate classification and the in-place backward merge on
std::vectors, tile by tile in descending order with every load of a tile before its stores, and compares ids and row payloads with the
plain restatement (retain + insert at the partition point): lists of 0 / 1 / 63 / 64 / 65 / 130 / 200 rows; insertions at the head, at the
tail, in the middle and on a tile boundary; more than 64 rows into one list; a list that loses and gains; every row leaving; rows into an
empty list; a list exactly at capacity (the grow flag); random cases from a fixed seed."""
import os
import subprocess

from tests.test_seg_plan_host import host_compilers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_backward_merge_and_locate_match_the_restatement(tmp_path):
    cxx = next(iter(host_compilers()), None)
    assert cxx is not None, "no host compiler"
    exe = str(tmp_path / "update_plan_demo")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-fsanitize=address,undefined", "-I" + os.path.join(ROOT, "vers_amd", "csrc"),
                        os.path.join(ROOT, "tests", "cpp", "update_plan_demo.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, r.stdout[-1000:] + r.stderr[-2000:]
    words = r.stdout.split()
    assert words[0] == "OK" and int(words[1]) >= 400, r.stdout


def test_the_kernels_include_the_header():
    src = open(os.path.join(ROOT, "vers_amd", "csrc", "ivf_build.hip")).read()
    assert '#include "update_plan.hpp"' in src
    for fn in ("upd::merge_source", "upd::insertion_point", "upd::list_of_row", "upd::classify", "upd::plan_lengths"):
        assert fn in src, fn
