"""The int8 head's bound on the HOST (no GPU): tests/cpp/head_bound_demo.cpp includes the text of head_scale, head_quant, head_resid,
head_extra and head_lower as it stands in vers_amd/csrc/prescan.hip.h (next to pre_bound and prune_tail_entry) and checks, for random
and adversarial inputs -- elements at the clamp, an outlier that sets the scale 50x the typical element, all-zero head columns,
residuals aligned with the query, negative I --, that the bound never exceeds the val computed in f64 from the fp16 operands minus
pre_bound's `common`, per row and with a tile's minima; and that a NaN in any input makes the test say "not dead".  Built with
-fsanitize=address,undefined."""
import os
import re
import subprocess

from tests.test_prune_bound_host import ROOT, host_compilers


def test_head_bound_never_exceeds_the_f64_value(tmp_path):
    src = open(os.path.join(ROOT, "vers_amd", "csrc", "prescan.hip.h")).read()
    begin = src.index("struct PreBound {")
    end = src.index("// The table of a batch: a wave per query.")
    snip = src[begin:end]
    for name in ("head_scale", "head_quant", "head_resid", "head_extra", "head_lower", "prune_tail_entry", "pre_bound"):
        assert name in snip, name
    assert "__global__" not in snip
    (tmp_path / "prune_snip.h").write_text("#include <cstdint>\nnamespace vers {\n" + snip + "\n}\n")
    exe = str(tmp_path / "head_bound_demo")
    (tmp_path / "probe.cpp").write_text("int main() { _Float16 h = (_Float16)1.5f; return __builtin_bit_cast(unsigned, (float)h) == 0u; }\n")
    cxx = next((c for c in host_compilers() if subprocess.run([c, "-std=c++17", str(tmp_path / "probe.cpp"), "-o", str(tmp_path / "probe")],
                                                              capture_output=True).returncode == 0), None)
    assert cxx is not None, "no host compiler builds a _Float16 probe (hipcc's clang++ should): " + repr(host_compilers())
    r = subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-fsanitize=address,undefined", "-I" + str(tmp_path),
                        os.path.join(ROOT, "tests", "cpp", "head_bound_demo.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    m = re.search(r"CHECKS (\d+) TILES (\d+) NANS (\d+) VIOLATIONS (\d+)", r.stdout)
    assert r.returncode == 0 and m, r.stdout[-2000:] + r.stderr[-2000:]
    assert int(m.group(1)) >= 50000 and int(m.group(2)) >= 500 and int(m.group(3)) >= 10 and int(m.group(4)) == 0, r.stdout[-2000:]
