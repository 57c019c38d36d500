"""compact_tiles_kernel on the HOST: tests/cpp/compact_kernel_emu.cpp includes the kernel's text as it stands in
vers_amd/csrc/ivf_build.hip, runs every block as 256 threads and compares the f32 tiles, the fp16 shadow tiles, the row-major rows,
row_ids, xnorm and both maxima bit for bit with restatements of row_to_f16 / row_norm_blocked / row_shadow_residual -- at ld 64
(one partial column pass), 320 (two, the second ragged), 768 and 1536 (whole passes), with and without a shadow and a row-major
copy, with slack rows holding NaN and 1e30, an element beyond fp16's range and a NaN row.  Built with AddressSanitizer as a
stand-alone program: an index outside a buffer is an error here, before the kernel ever runs on a GPU."""
import os
import subprocess

import pytest

from vers_amd import build as vbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host_clang():
    prefix = os.path.dirname(os.path.dirname(vbuild._hipcc()))
    for c in (os.path.join(prefix, "llvm", "bin", "clang++"), os.path.join(prefix, "lib", "llvm", "bin", "clang++")):
        if os.path.exists(c):
            return c
    return None


def test_compact_tiles_kernel_on_the_host_under_address_sanitizer(tmp_path):
    cxx = host_clang()
    if cxx is None:
        pytest.skip("no clang++ under the hipcc prefix (the emulation needs ext_vector_type and _Float16)")
    src = open(os.path.join(ROOT, "vers_amd", "csrc", "ivf_build.hip")).read()
    begin, end = src.index("struct CompactJob {"), src.index("// ---- vers_ivf_remove_batch: marking")
    snip = src[begin:end]
    lds = "extern __shared__ __attribute__((aligned(16))) f32x4 tl[];"
    assert snip.count(lds) == 1 and "compact_tiles_kernel" in snip
    (tmp_path / "kernel_snip.h").write_text(snip.replace(lds, "f32x4* tl = g_lds;"))
    exe = str(tmp_path / "compact_kernel_emu")
    subprocess.check_call([cxx, "-std=c++20", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address", "-pthread", "-I" + str(tmp_path),
                           os.path.join(ROOT, "tests", "cpp", "compact_kernel_emu.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "MISMATCH" not in r.stdout and r.stdout.count(": ok") == 12, r.stdout + r.stderr
