"""The list scan's hand-out of quads on the HOST (no GPU): tests/cpp/handout_demo.cpp includes the text of pre_run_len as it stands
in vers_amd/csrc/prescan.hip.h and replays the hand-out of 1 .. 512 blocks against one counter under random interleavings (the
counter moves between a block's load and its add) for 0 .. 5763 quads and hot counts of 0, 1, half, all and more than there are
quads: every quad exactly once, runs of 1 .. kPreMaxRun, single quads inside the hot region, no run computed behind the hot region
starting inside it, and the guided rule unchanged where there is no hot count."""
import os
import re
import subprocess

from tests.test_prune_bound_host import ROOT, host_compilers


def test_every_quad_is_handed_out_once_and_hot_quads_singly(tmp_path):
    src = open(os.path.join(ROOT, "vers_amd", "csrc", "prescan.hip.h")).read()
    begin = src.index("constexpr uint32_t kPreMaxRun")
    end = src.index("// ----", begin)
    snip = src[begin:end]
    assert "pre_run_len" in snip and "__global__" not in snip and snip.count("{") == snip.count("}")
    (tmp_path / "handout_snip.h").write_text("#include <cstdint>\nnamespace vers {\n" + snip + "\n}\n")
    exe = str(tmp_path / "handout_demo")
    (tmp_path / "probe.cpp").write_text("#include <cstdint>\nint main() { return 0; }\n")
    cxx = next((c for c in host_compilers() if subprocess.run([c, "-std=c++17", "-fsanitize=address,undefined", str(tmp_path / "probe.cpp"), "-o", str(tmp_path / "probe")],
                                                              capture_output=True).returncode == 0), None)
    assert cxx is not None, "no host compiler builds a sanitized probe: " + repr(host_compilers())
    r = subprocess.run([cxx, "-std=c++17", "-O2", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + str(tmp_path),
                        os.path.join(ROOT, "tests", "cpp", "handout_demo.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout[-2000:])
    m = re.search(r"CASES (\d+) HANDOUTS (\d+) VIOLATIONS (\d+)", r.stdout)
    assert r.returncode == 0 and m, r.stdout[-2000:] + r.stderr[-2000:]
    assert int(m.group(1)) >= 5 * 5 * 7 * 5 and int(m.group(2)) > 100000 and int(m.group(3)) == 0, r.stdout[-2000:]
