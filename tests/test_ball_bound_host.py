"""The sub-cluster ball bound on the HOST (no GPU): tests/cpp/ball_bound_demo.cpp includes the text of ball_bracket and ball_lower as it
stands in vers_amd/csrc/prescan.hip.h (next to pre_bound, prune_lower and head_lower) and checks, for random and adversarial (row, query,
sub-cluster) triples at d = 64, 300 and 768 -- the adversarial rows lie on the side of the query and set r_j; each is also taken as a
sub-cluster of its own, at distance exactly r_j after its fp16 rounding, where Cauchy-Schwarz is attained --, that the bound never exceeds the val computed in f64 from the fp16 operands minus
pre_bound's `common`, with the centre's dot product summed in f32 forwards, backwards and pairwise; and that a NaN or an infinity in
any input makes the test say "not dead".  Built with -fsanitize=address,undefined."""
import os
import re
import subprocess

from tests.test_prune_bound_host import ROOT, host_compilers


def test_ball_bound_never_exceeds_the_f64_value(tmp_path):
    src = open(os.path.join(ROOT, "vers_amd", "csrc", "prescan.hip.h")).read()
    begin = src.index("struct PreBound {")
    end = src.index("// The table of a batch: a wave per query.")
    snip = src[begin:end]
    for name in ("ball_bracket", "ball_lower", "prune_round_up", "prune_eps", "pre_bound"):
        assert name in snip, name
    assert "__global__" not in snip
    (tmp_path / "prune_snip.h").write_text("#include <cstdint>\nnamespace vers {\n" + snip + "\n}\n")
    exe = str(tmp_path / "ball_bound_demo")
    (tmp_path / "probe.cpp").write_text("int main() { _Float16 h = (_Float16)1.5f; return __builtin_bit_cast(unsigned, (float)h) == 0u; }\n")
    cxx = next((c for c in host_compilers() if subprocess.run([c, "-std=c++17", str(tmp_path / "probe.cpp"), "-o", str(tmp_path / "probe")],
                                                              capture_output=True).returncode == 0), None)
    assert cxx is not None, "no host compiler builds a _Float16 probe (hipcc's clang++ should): " + repr(host_compilers())
    r = subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-fsanitize=address,undefined", "-I" + str(tmp_path),
                        os.path.join(ROOT, "tests", "cpp", "ball_bound_demo.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    m = re.search(r"CHECKS (\d+) ADVERSARIAL (\d+) NANS (\d+) VIOLATIONS (\d+) SLACK (\S+) ADVMIN (\S+) ADVMAX (\S+)", r.stdout)
    assert r.returncode == 0 and m, r.stdout[-2000:] + r.stderr[-2000:]
    assert int(m.group(1)) >= 30000 and int(m.group(2)) >= 600 and int(m.group(3)) >= 12 and int(m.group(4)) == 0, r.stdout[-2000:]
    # the test must REACH the bound: a row exactly at r_j leaves only the rounding terms between bound and val -- E_dot = 1.01 (ld + 2) u
    # sn nq', r nq' eps = (ld + 2) u r nq', 16 u S and the 1e-12 factors.  With sn nq' and r nq' each <= 2 (|q|^2 + max|x|^2) (AM-GM, nq' =
    # 2 |q|) their sum, normalised by |q|^2 + max|x|^2, stays below 4.02 (ld + 2) u + 16 u + 1e-11 < 2e-4 at ld = 768; a demo whose
    # adversarial rows miss r_j (3.7e-3 when the random rows set the radius) fails here
    assert 0.0 <= float(m.group(5)) and 0.0 <= float(m.group(6)) and float(m.group(7)) < 2e-4, r.stdout[-2000:]
