"""The exhaustive scans' segment plan on the HOST (no GPU): tests/cpp/seg_plan_demo.cpp includes vers_amd/csrc/seg_plan.hpp -- a header
without a HIP dependency -- under the host compiler and prints seg_plan() for a table of inputs; the expected values are a restatement of
the sizing sequence as the five call sites spelled it out before they shared it (target_items, per, seg_rows, n_segs, n_segs_pad, n_items
and the 2^32 refusal of the calls that count slots), written here in Python integers with the 32-bit truncations made explicit."""
import itertools
import os
import shutil
import subprocess

from vers_amd import build as vbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host_compilers():
    prefix = os.path.dirname(os.path.dirname(vbuild._hipcc()))
    cands = [os.path.join(prefix, "llvm", "bin", "clang++"), os.path.join(prefix, "lib", "llvm", "bin", "clang++"), shutil.which("clang++"), shutil.which("g++")]
    return [c for c in cands if c and os.path.exists(c)]


U32 = 0xFFFFFFFF
K_WAVE, K_WAVES_PER_BLOCK = 64, 4


def max_seg_rows(ld):
    return ((1 << 31) // (ld * 4)) // 64 * 64


def blocks_per_cu(qg, ld):
    if qg == 1:
        return 3
    lds = ld * qg * 4 + 16
    return max(1, min(2, (160 * 1024) // lds))


def expected(n_rows, b, ld, n_cu, fixed):
    qg = 1 if b == 1 else 8
    n_qg = (b + qg - 1) // qg
    target_items = (n_cu * blocks_per_cu(qg, ld) * K_WAVES_PER_BLOCK) & U32
    per = (n_rows * n_qg + target_items - 1) // target_items
    want = fixed if fixed > 0 else (per if per else 1)
    seg_rows = min((want + K_WAVE - 1) // K_WAVE * K_WAVE, max_seg_rows(ld)) & U32
    n_segs = ((n_rows + seg_rows - 1) // seg_rows) & U32
    if n_segs == 0:
        n_segs = 1
    n_segs_pad = n_segs if qg == 1 else (((n_segs + 3) & U32) // 4 * 4) & U32
    n_items = (n_segs_pad * n_qg) & U32
    too_large = b * n_segs >= U32 or n_segs_pad * n_qg >= U32
    return (seg_rows, n_segs, n_segs_pad, n_items, n_qg, qg, int(too_large))


def cases():
    out = list(itertools.product((0, 1, 63, 64, 65, 3000), (1, 7, 8, 9), (16, 768), (1, 256), (0, 64, 256)))
    for ld in (16, 768):  # option "seg_rows" on either side of the cap a buffer descriptor sets, and on it
        cap = max_seg_rows(ld)
        out += [(10 * cap, b, ld, 256, f) for b in (1, 8) for f in (cap - 64, cap, cap + 64)]
    # sized, not fixed, at the cap: a corpus so long that one item per resident wave would exceed it (d = 768: 2^24 rows short of 2^32 a segment)
    out += [(1 << 36, 1, 768, 1, 0), (max_seg_rows(768) * 12 - 1, 1, 768, 1, 0), (max_seg_rows(768) * 12 + 1, 1, 768, 1, 0)]
    # the 2^32 limits: b * n_segs (slots) and n_segs_pad * n_qg (items), the last plan that fits and the first that does not
    out += [((1 << 35) - 64, 8, 16, 256, 64), (1 << 35, 8, 16, 256, 64), ((1 << 35) - 64, 9, 16, 256, 64),
            (64 * (U32 - 1), 1, 16, 256, 64), (64 * U32, 1, 16, 256, 64),
            ((1 << 32) - 64, 64, 16, 256, 64), ((1 << 32) - 1, 64, 16, 256, 64)]  # (the last two: as many rows as a handle holds)
    return out


def test_seg_plan_matches_the_restated_formula(tmp_path):
    cxx = next(iter(host_compilers()), None)
    assert cxx is not None, "no host compiler"
    exe = str(tmp_path / "seg_plan_demo")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-fsanitize=address,undefined", "-I" + os.path.join(ROOT, "vers_amd", "csrc"),
                        os.path.join(ROOT, "tests", "cpp", "seg_plan_demo.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    table = cases()
    r = subprocess.run([exe], input="".join("%d %d %d %d %d\n" % c for c in table), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, r.stdout[-1000:] + r.stderr[-2000:]
    got = [tuple(int(x) for x in line.split()) for line in r.stdout.splitlines()]
    assert len(got) == len(table)
    refused = 0
    for c, g in zip(table, got):
        assert g == expected(*c), (c, g, expected(*c))
        seg_rows, n_segs, n_segs_pad, n_items, n_qg, qg, too_large = g
        b = c[1]
        assert n_segs >= 1 and seg_rows % 64 == 0 and 64 <= seg_rows <= max_seg_rows(c[2])
        assert n_segs_pad == n_segs if b == 1 else (n_segs_pad % 4 == 0 and 0 <= n_segs_pad - n_segs < 4)
        if not too_large:
            assert n_segs * seg_rows >= c[0] and n_items == n_segs_pad * n_qg
        refused += too_large
    assert refused == 4, refused  # (of the seven cases at the limit; nothing else comes near it)
