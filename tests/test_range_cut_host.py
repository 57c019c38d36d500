"""The range pre-filter's cut on the HOST (no GPU): tests/cpp/range_cut_demo.cpp includes the text of pre_bound (prescan.hip.h) and of
range_cut (range_prescan.hip.h) as they stand and sweeps d_pad 64 / 320 / 768, both metrics, radii 0 .. 4, R^2 0 / 1e-7 / inf and vals on a
grid round each cut: `val > cut` in f32 must imply that pre_bound's f64 lower bound of the reference's distance exceeds the radius, and
with a non-finite input no val may pass."""
import os
import re
import subprocess

from tests.test_prune_bound_host import ROOT, host_compilers


def test_a_val_above_the_cut_is_provably_beyond_the_radius(tmp_path):
    pre = open(os.path.join(ROOT, "vers_amd", "csrc", "prescan.hip.h")).read()
    rng = open(os.path.join(ROOT, "vers_amd", "csrc", "range_prescan.hip.h")).read()
    snip = pre[pre.index("struct PreBound {"):pre.index("// The table of a batch: a wave per query.")]
    snip += rng[rng.index("// ---- range_cut: host + device"):rng.index("// ---- the kernels' parameters")]
    assert "range_cut" in snip and "pre_bound" in snip and "__global__" not in snip
    (tmp_path / "range_cut_snip.h").write_text("#include <cstdint>\nnamespace vers {\n" + snip + "\n}\n")
    (tmp_path / "probe.cpp").write_text("int main() { _Float16 h = (_Float16)1.5f; return __builtin_bit_cast(unsigned, (float)h) == 0u; }\n")
    cxx = next((c for c in host_compilers() if subprocess.run([c, "-std=c++17", str(tmp_path / "probe.cpp"), "-o", str(tmp_path / "probe")],
                                                              capture_output=True).returncode == 0), None)
    assert cxx is not None, repr(host_compilers())
    exe = str(tmp_path / "range_cut_demo")
    r = subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-fsanitize=address,undefined", "-I" + str(tmp_path),
                        os.path.join(ROOT, "tests", "cpp", "range_cut_demo.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    m = re.search(r"PAIRS (\d+) RULED_OUT (\d+) VIOLATIONS (\d+) NONFINITE_PASSED (\d+)", r.stdout)
    assert r.returncode == 0 and m, r.stdout[-2000:] + r.stderr[-2000:]
    assert int(m.group(1)) >= 100000 and int(m.group(2)) >= 10000 and int(m.group(3)) == 0 and int(m.group(4)) == 0, r.stdout[-2000:]
