"""The head filter's stream of tile prefixes on the HOST (no GPU): tests/cpp/head_stream_demo.cpp includes the text of kHeadPrefix,
head_stream_len and head_stream_pos as it stands in vers_amd/csrc/prescan.hip.h (next to pre_run_len) and replays a wave's ring of
R = 2 .. 4 slots over segments of 0 .. 12 tiles: every position issued maps inside [0, n_tiles) x [0, kHeadPrefix), each (tile, step)
of the prefix stream is requested exactly once and consumed in order, positions past the end repeat the last valid step, and a segment
without tiles issues nothing.  Built with -fsanitize=address,undefined."""
import os
import re
import subprocess

from tests.test_prune_bound_host import ROOT, host_compilers


def test_stream_positions_stay_inside_the_segment_and_visit_each_step_once(tmp_path):
    src = open(os.path.join(ROOT, "vers_amd", "csrc", "prescan.hip.h")).read()
    begin = src.index("constexpr uint32_t kHeadPrefix")
    end = src.index("// ----", begin)
    snip = src[begin:end]
    assert "head_stream_pos" in snip and "head_stream_len" in snip and "__global__" not in snip and snip.count("{") == snip.count("}")
    (tmp_path / "head_stream_snip.h").write_text("#include <cstdint>\nnamespace vers {\n" + snip + "\n}\n")
    exe = str(tmp_path / "head_stream_demo")
    (tmp_path / "probe.cpp").write_text("#include <cstdint>\nint main() { return 0; }\n")
    cxx = next((c for c in host_compilers() if subprocess.run([c, "-std=c++17", "-fsanitize=address,undefined", str(tmp_path / "probe.cpp"), "-o", str(tmp_path / "probe")],
                                                              capture_output=True).returncode == 0), None)
    assert cxx is not None, "no host compiler builds a sanitized probe: " + repr(host_compilers())
    r = subprocess.run([cxx, "-std=c++17", "-O2", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + str(tmp_path),
                        os.path.join(ROOT, "tests", "cpp", "head_stream_demo.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout[-2000:])
    m = re.search(r"CASES (\d+) ISSUES (\d+) VIOLATIONS (\d+)", r.stdout)
    assert r.returncode == 0 and m, r.stdout[-2000:] + r.stderr[-2000:]
    assert int(m.group(1)) == 13 * 3 and int(m.group(2)) > 1000 and int(m.group(3)) == 0, r.stdout[-2000:]
