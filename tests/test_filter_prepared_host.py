"""A prepared filter's tail refresh on the HOST (no GPU): tests/cpp/filter_tail_plan_demo.cpp includes vers_amd/csrc/filter_prepared.hpp -- a
header without a HIP dependency: which lists grew since the snapshot, the 64-row tiles of each that can hold a changed bit, and the shortcut
when no id handed out since is below n_bits -- under the host compiler with -fsanitize=address,undefined.  Every case is checked twice: by
the demo against a row-by-row restatement, and here against the tile ranges written out by hand."""
import os
import subprocess

from tests.test_seg_plan_host import host_compilers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (snap_len, len) -> the tiles that must be recomputed, first and last
GROWTH = {(0, 3): (0, 0), (10, 12): (0, 0), (60, 70): (0, 1), (60, 64): (0, 0), (64, 65): (1, 1), (127, 129): (1, 2)}


def cases():
    """-> [(k, rank, owned, first_new_id, n_bits, [(snap, len, owner)], expected items)]"""
    out = []
    for (a, b), (t0, t1) in GROWTH.items():
        out.append((1, 0, 0, 100, 1000, [(a, b, 0)], [(0, a, b, t0, t1)]))
    # all of them in one index, between a list that did not grow, an empty one and one that another rank owns (and that grew there)
    lists = [(5, 5, 0), (0, 0, 0)] + [(a, b, 0) for a, b in GROWTH] + [(7, 9, 1), (200, 200, 0), (130, 131, 0)]
    want = [(2 + i, a, b, *GROWTH[(a, b)]) for i, (a, b) in enumerate(GROWTH)] + [(len(lists) - 1, 130, 131, 2, 2)]
    out.append((len(lists), 0, 1, 5000, 6000, lists, want))
    # the same lengths seen by the other rank: only its own list
    out.append((len(lists), 1, 1, 5000, 6000, lists, [(8, 7, 9, 0, 0)]))
    # without an owner table every list is this rank's
    out.append((len(lists), 0, 0, 5000, 6000, lists, want[:-1] + [(8, 7, 9, 0, 0), want[-1]]))
    # the first new id is at or beyond n_bits: no new row can be allowed, the plan is empty (equal and beyond; n_bits == 0)
    out.append((len(lists), 0, 1, 6000, 6000, lists, []))
    out.append((len(lists), 0, 1, 6001, 6000, lists, []))
    out.append((1, 0, 0, 0, 0, [(0, 3, 0)], []))
    out.append((len(lists), 0, 1, 5999, 6000, lists, want))   # one id below n_bits is enough for the whole plan
    # nothing grew
    out.append((3, 0, 0, 10, 1000, [(4, 4, 0), (64, 64, 0), (0, 0, 0)], []))
    return out


def test_tail_plan_matches_the_brute_force_restatement(tmp_path):
    cxx = next(iter(host_compilers()), None)
    assert cxx is not None, "no host compiler"
    exe = str(tmp_path / "filter_tail_plan_demo")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I" + os.path.join(ROOT, "vers_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "filter_tail_plan_demo.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    table = cases()
    text = "".join("%d %d %d %d %d\n%s" % (k, rank, owned, first, n_bits, "".join("%d %d %d\n" % l for l in lists)) for k, rank, owned, first, n_bits, lists, _ in table)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, r.stdout[-1000:] + r.stderr[-2000:]
    lines = [tuple(int(x) for x in line.split()) for line in r.stdout.splitlines()]
    at = 0
    for k, rank, owned, first, n_bits, lists, want in table:
        n_items, rows, ok = lines[at]
        got = lines[at + 1:at + 1 + n_items]
        at += 1 + n_items
        assert ok == 1, (k, rank, owned, first, n_bits)
        assert got == want, (k, rank, owned, first, n_bits, got)
        assert rows == sum(b - a for _, a, b, _, _ in want)
    assert at == len(lines)
