"""The head filter's ring of tile prefixes (csrc/head_filter.hip.h: a wave keeps kHeadRing steps of its segment's prefix stream in flight
across tile ends, and its next segment's first loads go out ahead of the quad change): ids, distance bits and counts must equal, with
no tolerance, those of the same handle with pre_head = 0 for EVERY query and the oracle's for every 7th.  The lists are built by hand --
one tight mode each, d = 768 -- so that their segments have the tile counts the ring can go wrong at:
  tiles  lists whose four segments have 1, 2, 4 (= R), 5 (= R + 1) and ~20 tiles with partial last tiles, a list of 40 rows (one partial
         tile and three segments WITHOUT tiles in one quad) and one whose segments differ in their tile counts; batches of 8, 40 and 72
         queries; then the slack rows poisoned (1e30, NaN): a prefetched slack or foreign tile must never take part in a verdict
  late   rows and queries whose energy sits in columns 256 .. 383 (those columns scaled, rows renormalised) mixed with ordinary lists in
         one index: their tiles survive the test at 256 columns and die at 320 or 384 -- steps read on demand while the next tile's
         prefix waits in the ring.  Every list is probed, so the cold tiles are known: head_steps must exceed 4 x (tiles of the cold
         lists) >= 4 x (tiles of dead quads)
  live   700 short lists, more cold quads than the filter has blocks, twenty of which hold rows that are true neighbours of a query of
         another list: live quads in the middle of a block's stride -- the block's next quad must start correctly
As in test_head_filter_gpu.py every case must show some dead quad: a filter that never fires does not pass."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BODY = r'''
import sys
import numpy as np
from oracle import c_oracle as co
from vers_amd import capi, testhooks
from vers_amd.index import IVFFlatIndex

CASE = sys.argv[1]
D = 768
capi.set_option("pre_head", 1)

def run(ix, Q, top_k, nprobe, head):
    capi.set_option("pre_head", head)
    f0 = ix.prescan_stats()["fallback_queries"]
    ids, dist, cnt = ix.search_batch(Q, top_k, nprobe)
    st = ix.head_state()
    capi.set_option("pre_head", 1)
    return ids, dist, cnt, ix.prescan_stats()["fallback_queries"] - f0, st

def both(ix, Q, top_k, nprobe, tag=""):
    """pre_head = 1 against pre_head = 0 for every query, against the oracle for every 7th; returns the filter's counters of the split scan"""
    i1, d1, c1, f1, s1 = run(ix, Q, top_k, nprobe, 1)
    i0, d0, c0, f0, s0 = run(ix, Q, top_k, nprobe, 0)
    print("FIG", CASE, tag, "b", Q.shape[0], "last", s1["last"], "off", s0["last"], "fallback on/off", f1, f0)
    assert s0["last"] == dict(quads_tested=0, quads_dead=0, head_steps=0), s0
    assert np.array_equal(c1, c0), (tag, np.flatnonzero(c1 != c0))
    assert np.array_equal(i1, i0), (tag, np.flatnonzero((i1 != i0).any(axis=1)))
    assert np.array_equal(d1.view(np.uint32), d0.view(np.uint32)), (tag, np.flatnonzero((d1.view(np.uint32) != d0.view(np.uint32)).any(axis=1)))
    assert f1 == f0, (tag, f1, f0)
    for qi in range(0, Q.shape[0], 7):
        oi, od = co.search_nprobe(ix.values, ix.centroids, ix.ids, Q[qi], top_k, nprobe)
        assert c1[qi] == len(oi) and np.array_equal(i1[qi, :len(oi)], oi), (tag, qi)
        assert np.array_equal(d1[qi, :len(oi)].view(np.uint32), od.view(np.uint32)), (tag, qi)
    return s1

def unit(v):
    return (v / np.sqrt((v.astype(np.float64) ** 2).sum(axis=-1, keepdims=True))).astype(np.float32)

def mode(rng, late):
    c = rng.standard_normal(D)
    if late:
        c[256:384] *= 8.0
    return unit(c)

def around(rng, c, n):
    return unit(c[None, :] + 0.01 * rng.standard_normal((n, D)))

def index_of(lists):
    """an index whose lists are the given row blocks, uploaded as they are (centroid = the list's mean)"""
    ix = IVFFlatIndex(D)
    ix.values = np.concatenate(lists).astype(np.float32)
    ix.centroids = np.stack([l.astype(np.float64).mean(axis=0) for l in lists]).astype(np.float32)
    ix.assignments = np.concatenate([np.full(len(l), i, dtype=np.uint64) for i, l in enumerate(lists)])
    off = np.concatenate([[0], np.cumsum([len(l) for l in lists])])
    ix.ids = [list(range(int(off[i]), int(off[i + 1]))) for i in range(len(lists))]
    ix.num_centroids = len(lists)
    ix._upload()
    return ix

def dead_some(st, tag):
    assert st["valid"] and st["last"]["quads_tested"] > 0 and st["last"]["quads_dead"] > 0, (tag, st)

def tiles_of(n):   # a list of n rows: four segments of whole tiles, nearly equal (one quad per list at these lengths)
    per = (-(-n // 4) + 63) // 64 * 64
    return sum(-(-max(0, min(per, n - s * per)) // 64) for s in range(4))

if CASE == "tiles":
    rng = np.random.default_rng(0x901)
    # rows per list -> tiles per segment: 40 -> 1 0 0 0 | 200 -> 1 1 1 1 (8 rows) | 450 -> 2 2 2 2 (66 rows) | 1000 -> 4 4 4 4 (232) | 1230 -> 5 5 5 5 (270)
    # | 700 -> 3 3 3 2 | 5000 -> 20 20 20 19 (1280 1280 1280 1160), and ordinary ones
    lens = [40, 200, 450, 1000, 1230, 700, 5000] + [1250 + 37 * i for i in range(9)]
    modes = [mode(rng, False) for _ in lens]
    ix = index_of([around(rng, c, n) for c, n in zip(modes, lens)])
    assert ix.head_state()["valid"] and ix.head_state()["cols"] == 384, ix.head_state()
    homes = [7, 8, 9]   # the queries' own lists: every other list is cold
    def queries(b):
        return np.concatenate([around(rng, modes[h], -(-b // 3)) for h in homes])[:b]
    for b in (8, 40, 72):
        dead_some(both(ix, queries(b), 10, 16, tag="b%d" % b), "b%d" % b)
    for v in (1.0e30, float("nan")):
        testhooks.poison_slack(ix, v)
        dead_some(both(ix, queries(40), 10, 16, tag="slack %r" % v), "slack %r" % v)
elif CASE == "late":
    rng = np.random.default_rng(0x902)
    lens = [1250 + 41 * i for i in range(12)]
    late = [i % 2 == 1 for i in range(12)]
    modes = [mode(rng, l) for l in late]
    ix = index_of([around(rng, c, n) for c, n in zip(modes, lens)])
    homes = [0, 1, 2]   # two ordinary lists and a late one
    Q = np.concatenate([around(rng, modes[h], 3) for h in homes])[:8]
    st = both(ix, Q, 10, 12, tag="late")   # nprobe = every list: the nine other lists are cold and all of them are tested
    dead_some(st, "late")
    cold_tiles = sum(tiles_of(n) for i, n in enumerate(lens) if i not in homes)
    print("FIG late cold tiles", cold_tiles, "head steps", st["last"]["head_steps"])
    assert st["last"]["head_steps"] > 4 * cold_tiles, (st, cold_tiles)
elif CASE == "live":
    rng = np.random.default_rng(0x903)
    n_lists = 700
    modes = [mode(rng, False) for _ in range(n_lists)]
    homes = [0, 1, 2]
    lists = [around(rng, c, 70 + (i % 5) * 30) for i, c in enumerate(modes)]
    for j, i in enumerate(range(20, 700, 34)):   # twenty lists far from every query that hold six rows next to a home mode
        lists[i] = np.concatenate([lists[i], unit(modes[homes[j % 3]][None, :] + 0.002 * rng.standard_normal((6, D)))])
    ix = index_of(lists)
    Q = np.concatenate([around(rng, modes[h], 24) for h in homes])
    st = both(ix, Q, 10, 700, tag="live")   # every list is probed: ~700 cold quads
    dead_some(st, "live")
    t, dd = st["last"]["quads_tested"], st["last"]["quads_dead"]
    # more quads than blocks (two per compute unit); the twenty planted lists' quads stayed live, and their rows -- nearer to every
    # query than its own list's -- are what the search returns
    assert t > 2 * 256 and t - dd >= 20, st
    off = np.concatenate([[0], np.cumsum([len(l) for l in lists])])
    planted = np.concatenate([np.arange(off[i + 1] - 6, off[i + 1]) for i in range(20, 700, 34)])
    ids, _, _ = ix.search_batch(Q, 10, 700)
    assert np.isin(ids, planted).all(), np.flatnonzero(~np.isin(ids, planted).all(axis=1))
print("DONE", CASE)
'''


def run(case):
    env = dict(os.environ); env["PYTHONPATH"] = ROOT
    r = subprocess.run([sys.executable, "-c", BODY, case], capture_output=True, text=True, env=env, cwd=ROOT, timeout=600)
    print(r.stdout[-4000:])
    assert r.returncode == 0 and ("DONE " + case) in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


@pytest.mark.parametrize("case", ["tiles", "late", "live"])
def test_prefetched_prefixes_change_no_bit(case):
    run(case)
