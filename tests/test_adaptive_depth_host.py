"""The adaptive filtered search's depth rule on the HOST (no GPU): tests/cpp/adaptive_depth_demo.cpp includes vers_amd/csrc/adaptive_depth.hpp
-- a header without a HIP dependency, the one the plan kernel applies rank by rank -- under the host compiler and walks a query's ranks with
it; the expected depth is the definition restated by brute force: the smallest P in [P_min, P_max] with a_0 + ... + a_{P-1} >= min_allowed,
or P_max if there is none."""
import os
import subprocess

import numpy as np

from tests.test_seg_plan_host import host_compilers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def brute_depth(a, nprobe_min, nprobe_max, min_allowed):
    k = len(a)
    p_min, p_max = min(nprobe_min, k), min(nprobe_max, k)
    for p in range(p_min, p_max + 1):
        if int(np.sum(a[:p], dtype=np.int64)) >= min_allowed:
            return p
    return p_max


def cases():
    rng = np.random.default_rng(0xADA9)
    out = []
    for k in (1, 63, 64, 65, 129, 200):
        vecs = [rng.integers(0, 4, k), rng.integers(0, 40, k) * (rng.random(k) < 0.2), np.zeros(k, dtype=np.int64)]   # dense, sparse, all-zero counts
        for a in vecs:
            a = np.asarray(a, dtype=np.int64)
            total = int(a.sum())
            pref = np.cumsum(a)
            exact = sorted({int(pref[p - 1]) for p in (1, min(k, 63), min(k, 64), min(k, 65), min(k, 128), (k + 1) // 2, k)})   # exactly A_P for some P
            for m in [0, 1, total, total + 1] + exact:
                for lo, hi in ((1, k), (1, k + 9), (k + 3, k + 9), (4, 4), (min(k, 64), min(k, 64)), (1, 1), (2, max(2, k - 1)), (min(k, 65), k)):
                    out.append((a, lo, hi, m))
    return out


def test_depth_rule_matches_the_brute_force_definition(tmp_path):
    cxx = next(iter(host_compilers()), None)
    assert cxx is not None, "no host compiler"
    exe = str(tmp_path / "adaptive_depth_demo")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-fsanitize=address,undefined", "-I" + os.path.join(ROOT, "vers_amd", "csrc"),
                        os.path.join(ROOT, "tests", "cpp", "adaptive_depth_demo.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    table = cases()
    text = "".join("%d %d %d %d %s\n" % (len(a), lo, hi, m, " ".join(str(int(v)) for v in a)) for a, lo, hi, m in table)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, r.stdout[-1000:] + r.stderr[-2000:]
    got = [tuple(int(x) for x in line.split()) for line in r.stdout.splitlines()]
    assert len(got) == len(table)
    depths = set()
    for (a, lo, hi, m), (depth, prefix) in zip(table, got):
        assert prefix == 1, (len(a), lo, hi, m)
        assert depth == brute_depth(a, lo, hi, m), (len(a), lo, hi, m, depth)
        depths.add(depth)
    # the table reaches both ends and the chunk boundaries of the kernel's 64-rank walk
    assert {1, 63, 64, 65, 128, 129, 200} <= depths, sorted(depths)
