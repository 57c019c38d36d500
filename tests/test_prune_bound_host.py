"""The list scan's early-abandon bound on the HOST (no GPU): tests/cpp/prune_bound_demo.cpp includes the text of pre_bound,
prune_tail_entry and prune_lower as it stands in vers_amd/csrc/prescan.hip.h and checks, for more than 10^5 (row, query, columns
consumed) triples -- clustered rows, rows equal to the query, rows whose whole distance sits in the prefix / in the suffix,
magnitudes in fp16's subnormal range and scaled by 300 --, that the bound never exceeds the f32 value the kernel's arithmetic
produces for the whole row (fp16-rounded operands, f32 accumulation in shuffled orders)."""
import os
import re
import shutil
import subprocess

from vers_amd import build as vbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host_compilers():
    prefix = os.path.dirname(os.path.dirname(vbuild._hipcc()))
    cands = [os.path.join(prefix, "llvm", "bin", "clang++"), os.path.join(prefix, "lib", "llvm", "bin", "clang++"), shutil.which("clang++"), shutil.which("g++")]
    return [c for c in cands if c and os.path.exists(c)]


def test_prune_bound_never_exceeds_the_kernels_value(tmp_path):
    src = open(os.path.join(ROOT, "vers_amd", "csrc", "prescan.hip.h")).read()
    begin = src.index("struct PreBound {")
    end = src.index("// The table of a batch: a wave per query.")
    snip = src[begin:end]
    assert "prune_lower" in snip and "prune_tail_entry" in snip and "pre_bound" in snip and "__global__" not in snip
    (tmp_path / "prune_snip.h").write_text("#include <cstdint>\nnamespace vers {\n" + snip + "\n}\n")
    exe = str(tmp_path / "prune_bound_demo")
    # which compiler: the first that builds a one-line _Float16 / __builtin_bit_cast probe (clang -- hipcc's own is always there --, or
    # g++ from 12 on).  The demo itself must then build: a compile error in the text cut from the header is a failure.
    (tmp_path / "probe.cpp").write_text("int main() { _Float16 h = (_Float16)1.5f; return __builtin_bit_cast(unsigned, (float)h) == 0u; }\n")
    cxx = next((c for c in host_compilers() if subprocess.run([c, "-std=c++17", str(tmp_path / "probe.cpp"), "-o", str(tmp_path / "probe")],
                                                              capture_output=True).returncode == 0), None)
    assert cxx is not None, "no host compiler builds a _Float16 probe (hipcc's clang++ should): " + repr(host_compilers())
    r = subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-fsanitize=address,undefined", "-I" + str(tmp_path),
                        os.path.join(ROOT, "tests", "cpp", "prune_bound_demo.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout[-2000:])
    m = re.search(r"TRIPLES (\d+) VIOLATIONS (\d+)", r.stdout)
    assert r.returncode == 0 and m, r.stdout[-2000:] + r.stderr[-2000:]
    assert int(m.group(1)) >= 100000 and int(m.group(2)) == 0, r.stdout[-2000:]
