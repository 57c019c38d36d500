"""tiles_to_live_rows_kernel on the HOST: tests/cpp/recluster_gather_emu.cpp includes the kernel's text as it stands in
vers_amd/csrc/ivf_build.hip (between its two marker comments), runs every block as 256 threads and compares X' bit for bit with a plain
restatement -- at ld 64 (one partial column pass), 320 (two, the second ragged), 768 and 1536 (whole passes), with lists that end at 1, 63,
64 and 65 rows, slack rows holding NaN and 1e30 under row_ids entries that look live, a rank table with holes at id 0 and at the last id,
and d < pitch <= ld (the padding columns are written as zeros whatever the tile holds there).  Built with AddressSanitizer as a
stand-alone program: an index outside a buffer is an error here, before the kernel ever runs on a GPU."""
import os
import subprocess

import pytest

from tests.test_compact_kernel_host import host_clang

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BEGIN, END = "// [recluster gather kernel: begin]", "// [recluster gather kernel: end]"


def test_tiles_to_live_rows_kernel_on_the_host_under_address_sanitizer(tmp_path):
    cxx = host_clang()
    if cxx is None:
        pytest.skip("no clang++ under the hipcc prefix (the emulation needs ext_vector_type)")
    src = open(os.path.join(ROOT, "vers_amd", "csrc", "ivf_build.hip")).read()
    assert src.count(BEGIN) == 1 and src.count(END) == 1
    snip = src[src.index(BEGIN):src.index(END)]
    lds = "extern __shared__ __attribute__((aligned(16))) f32x4 tl[];"
    assert snip.count(lds) == 1 and "tiles_to_live_rows_kernel" in snip and "rows_rm" not in snip
    (tmp_path / "kernel_snip.h").write_text(snip.replace(lds, "f32x4* tl = g_lds;"))
    exe = str(tmp_path / "recluster_gather_emu")
    subprocess.check_call([cxx, "-std=c++20", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address", "-pthread", "-I" + str(tmp_path),
                           os.path.join(ROOT, "tests", "cpp", "recluster_gather_emu.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "MISMATCH" not in r.stdout and r.stdout.count(": ok") == 7, r.stdout + r.stderr
