"""fetch_tiles_kernel on the HOST: tests/cpp/fetch_kernel_emu.cpp includes the kernel's text as it stands in vers_amd/csrc/fetch.hip.h
(between its two marker comments), runs every block as 256 threads and compares the fetched rows bit for bit with a plain restatement -- at
ld 64 (d = 1), 320 (d = 300: two column passes, the second ragged) and 768, with tiles of which 1, T - 1, T and 64 rows are wanted (T = the
library's threshold between reading the wanted rows' pieces directly and turning the whole tile through LDS, read from ivf_fetch.hip; every
layout runs with the threshold forced to 1 and to 1000 too), a repeated id with two destinations, ids in no list (rows of zeros), an output
pitch above d whose padding keeps its sentinel, an output the 16-byte stores cannot serve, slack rows holding NaN and 1e30, and lists that
end at 1, 63, 64 and 65 rows.  Built with AddressSanitizer as a stand-alone program: an index outside a buffer is an error here, before the
kernel ever runs on a GPU.

The second test builds tests/cpp/fetch_plan_demo.cpp: the map's refresh decision (full / appended range / none) as a pure function of the
counters, and the tile jobs of both passes, from vers_amd/csrc/fetch_plan.hpp with the host compiler alone."""
import os
import re
import subprocess

import pytest

from tests.test_compact_kernel_host import host_clang

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BEGIN, END = "// [fetch gather kernel: begin]", "// [fetch gather kernel: end]"


def threshold():
    m = re.search(r"constexpr uint32_t kFetchLdsMin = (\d+);", open(os.path.join(ROOT, "vers_amd", "csrc", "ivf_fetch.hip")).read())
    assert m, "kFetchLdsMin"
    return int(m.group(1))


def test_fetch_tiles_kernel_on_the_host_under_address_sanitizer(tmp_path):
    cxx = host_clang()
    if cxx is None:
        pytest.skip("no clang++ under the hipcc prefix (the emulation needs ext_vector_type)")
    src = open(os.path.join(ROOT, "vers_amd", "csrc", "fetch.hip.h")).read()
    assert src.count(BEGIN) == 1 and src.count(END) == 1
    snip = src[src.index(BEGIN):src.index(END)]
    lds = "extern __shared__ __attribute__((aligned(16))) f32x4 tl[];"
    assert snip.count(lds) == 1 and "fetch_tiles_kernel" in snip and "rows_rm" not in snip and "row_ids" not in snip
    (tmp_path / "kernel_snip.h").write_text(snip.replace(lds, "f32x4* tl = g_lds;"))
    exe = str(tmp_path / "fetch_kernel_emu")
    subprocess.check_call([cxx, "-std=c++20", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address", "-pthread", "-I" + str(tmp_path),
                           os.path.join(ROOT, "tests", "cpp", "fetch_kernel_emu.cpp"), "-o", exe])
    T = threshold()
    assert 1 <= T <= 64
    r = subprocess.run([exe, str(T)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "MISMATCH" not in r.stdout and r.stdout.count(": ok") == 15, r.stdout + r.stderr


def test_map_refresh_decision_and_jobs_on_the_host(tmp_path):
    cxx = host_clang() or "c++"
    exe = str(tmp_path / "fetch_plan_demo")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-I" + os.path.join(ROOT, "vers_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "fetch_plan_demo.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "all ok" in r.stdout, r.stdout + r.stderr
