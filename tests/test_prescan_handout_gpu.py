"""The list scan's hand-out of quads (csrc/prescan.hip.h, pre_run_len; option "pre_hot_single"): where tiles are abandoned early the
blocks take the quads of the hot lists -- some query's nearest, the first of the work order -- one at a time and the rest in guided
runs.  Which block scans which quad decides nothing: ids, distance bits, counts and the number of re-scanned queries must equal
those of pre_hot_single = 0 for EVERY query, and the oracle's for every 7th -- with a hot list of four quads next to one of a single
quad, a list probed by two query groups, nprobe = 1 (every probed list hot: the hot region is the whole launch), nprobe = nlist with
two home lists (most lists cold), a batch of 4, and after add_batch / remove_batch / compact.

Grids: ONE block, TWO blocks and the default.  The launcher puts min(2, 160 KiB / LDS of a block) blocks on each compute unit it may
use (launch_prescan), so "one" / "two" reserve every compute unit but one / but two AND ask for a result wide enough that a block
needs more than 80 KiB of LDS: top_k = 17 keeps 41 keys per query, whose buffers are 128 keys long -- 64 queries x 128 x 8 B = 64 KiB
next to the 32 KiB query block of d = 256 (at d = 768 the query block alone is 96 KiB).  With one block the hand-out is sequential:
every hot quad goes singly to the same block, and the quads of a hot list of several quads meet back to back and are merged.  The
default grid runs the same cases at top_k = 10 (64-key buffers, two blocks per compute unit).

That the scan is told the RIGHT hot count is checked on what the planner published: vers_ivf_last_scan prints the batch's work order
under option "scan_debug" = 16 (items, of which hot), and the test works both figures out from the queries' probes and the planner's
cut of the lists (plan.hip.h list_seg_rows; ivf_plan.hip: segments of round_up(max(256, mean length / 4), 64) rows, a quad = four)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BODY = r'''
import os
import re
import sys
import tempfile
import numpy as np
import torch
from oracle import c_oracle as co
from tests import datagen as dg
from vers_amd import capi
from vers_amd.index import IVFFlatIndex

CASE, GRID = sys.argv[1], sys.argv[2]
N_CU = torch.cuda.get_device_properties(0).multi_processor_count
capi.set_option("scan_reserve_cus", {"one": 1 << 20, "two": N_CU - 2, "all": -1}[GRID])
MPL = 8   # modes per list
QG = 64   # queries per block at these shapes (the planner takes 64-query hi-only blocks wherever they fit 160 KiB)

def top_k_for(d):
    """the grid's top_k (docstring), with the floor of a block's LDS it implies: query block (fp16) + candidate buffers"""
    top_k = 17 if (GRID != "all" and d == 256) else 10   # (d = 768: the query block alone is 96 KiB)
    kp = min(64, top_k + max(24, top_k))                       # ivf_plan.hip: keys kept per query on the fp16 shadow
    cap = 64 if kp <= 40 else 128                              # prescan.hip.h pre_cap
    lds_floor = d * QG * 2 + QG * cap * 8
    if GRID != "all":
        assert 80 * 1024 < lds_floor <= 150 * 1024, (d, top_k, lds_floor)   # one block per compute unit, and 64-query blocks still fit
    return top_k

def make(seed, counts, d):
    """Lists of the given lengths: list c holds rows of its own MPL modes (vec ids shuffled over the lists), centroid = its rows' mean"""
    k, n = len(counts), int(sum(counts))
    centres = dg.dist_u(seed ^ 0xC0FFEE, k * MPL, d)
    lst = np.random.default_rng(seed).permutation(np.repeat(np.arange(k), counts))
    X = dg.normalize_rows(centres[lst * MPL + np.arange(n) % MPL] + dg.default_sigma(d) * dg.noise(seed, np.arange(n), d))
    ix = IVFFlatIndex(d)
    ix.values, ix.assignments, ix.num_centroids = X, lst.astype(np.uint64), k
    ix.centroids = np.stack([X[lst == c].mean(axis=0) for c in range(k)]).astype(np.float32)
    ix.ids = [np.flatnonzero(lst == c).tolist() for c in range(k)]
    ix._upload()
    return centres, ix

def queries(seed, centres, b, homes, d):
    """b queries drawn from the modes of the lists `homes` only (round robin)"""
    i = np.arange(b)
    mode = np.asarray(homes)[i % len(homes)] * MPL + (i // len(homes)) % MPL
    return dg.normalize_rows(centres[mode] + dg.default_sigma(d) * dg.noise(seed, np.arange(b), d))

def probes(ix, Q, nprobe):
    return np.argsort(((Q[:, None, :] - ix.centroids[None]) ** 2).sum(-1), axis=1, kind="stable")[:, :nprobe]

def seg_target(n_total, k):   # ivf_plan.hip: the matrix-core scan's segment length
    return (max(256, (n_total // k + 3) // 4) + 63) // 64 * 64

def quads(length, target):   # plan.hip.h list_seg_rows: nearly equal whole-tile segments, four to a quad
    return max(1, (length + 4 * target - 1) // (4 * target))

def items_of(length, target, n_queries):
    """work items of a list probed by n_queries: (query groups) x (segments padded to whole quads)"""
    nq = quads(length, target)
    seg = ((length + 4 * nq - 1) // (4 * nq) + 63) // 64 * 64
    return (n_queries + QG - 1) // QG * (((length + seg - 1) // seg + 3) // 4 * 4)

def published_work_order(ix):
    """(items, hot items) of the last planned batch as the device holds them: vers_ivf_last_scan's diagnostic line"""
    capi.set_option("scan_debug", 16)
    saved = os.dup(2)
    try:
        with tempfile.TemporaryFile() as f:
            os.dup2(f.fileno(), 2)
            try:
                ix.last_scan()
            finally:
                os.dup2(saved, 2)
            f.seek(0)
            txt = f.read().decode()
    finally:
        os.close(saved)
        capi.set_option("scan_debug", 0)
    m = re.search(r"work order: (\d+) items, the first (\d+) of hot lists", txt)
    assert m, txt
    return int(m.group(1)), int(m.group(2))

def check_hot_count(ix, Q, nprobe, counts, tag):
    """the hot count the scan's hand-out reads = the items of the lists that are some query's nearest"""
    pr = probes(ix, Q, nprobe)
    per_list = np.bincount(pr.ravel(), minlength=len(counts))
    target = seg_target(int(sum(counts)), len(counts))
    want = {L: items_of(int(counts[L]), target, int(per_list[L])) for L in np.flatnonzero(per_list)}
    hot = set(pr[:, 0].tolist())
    items, hot_items = published_work_order(ix)
    print("FIG", CASE, GRID, tag, "work order", items, "items, hot", hot_items, "expected", sum(want.values()), sum(want[L] for L in hot))
    assert items == sum(want.values()) == ix.last_scan()["items"], (tag, items, want)
    assert hot_items == sum(want[L] for L in hot) and 0 < hot_items <= items and hot_items % 4 == 0, (tag, hot_items, sorted(hot), want)
    return hot_items, items

def run(ix, Q, top_k, nprobe, single):
    capi.set_option("pre_hot_single", single)
    f0 = ix.prescan_stats()["fallback_queries"]
    ids, dist, cnt = ix.search_batch(Q, top_k, nprobe)
    return ids, dist, cnt, ix.prescan_stats()["fallback_queries"] - f0, ix.prune_stats()["last"]

def both(ix, Q, top_k, nprobe, tag="", must_skip=True, counts=None):
    i1, d1, c1, f1, s1 = run(ix, Q, top_k, nprobe, 1)
    i0, d0, c0, f0, s0 = run(ix, Q, top_k, nprobe, 0)
    print("FIG", CASE, GRID, tag, "single", s1, "runs", s0, "re-scanned", f1, f0)
    assert np.array_equal(c1, c0), (tag, np.flatnonzero(c1 != c0))
    assert np.array_equal(i1, i0), (tag, np.flatnonzero((i1 != i0).any(axis=1)))
    assert np.array_equal(d1.view(np.uint32), d0.view(np.uint32)), (tag, np.flatnonzero((d1.view(np.uint32) != d0.view(np.uint32)).any(axis=1)))
    assert f1 == f0, (tag, f1, f0)
    for qi in range(0, Q.shape[0], 7):
        oi, od = co.search_nprobe(ix.values, ix.centroids, ix.ids, Q[qi], top_k, nprobe)
        assert c1[qi] == len(oi) and np.array_equal(i1[qi, :len(oi)], oi), (tag, qi)
        assert np.array_equal(d1[qi, :len(oi)].view(np.uint32), od.view(np.uint32)), (tag, qi)
    # the case must run the kernel whose hand-out the option changes (the one that abandons tiles: its counters are the evidence), and on
    # the smallest grid -- where the work is walked in its planned order, hot lists first -- tiles of the cold lists must have been let go
    assert s1["steps_executed"] > 0 and s0["steps_executed"] > 0, (tag, "the scan that abandons tiles did not run: the case exercises nothing")
    if must_skip and GRID == "one":
        assert s1["steps_skipped"] > 0, (tag, "nothing was abandoned: the case exercises nothing")
    if counts is not None:
        return check_hot_count(ix, Q, nprobe, counts, tag)

COUNTS = [5400, 600, 1200, 900, 1500, 1100, 800, 788]   # 12288 rows in 8 lists: quads of 4 x 384 rows -> four quads, one quad, ...
if CASE in ("hot3", "hot3_d768"):   # a hot list of three quads next to a hot list of a single quad; the other six are cold
    d = 768 if CASE == "hot3_d768" else 256
    centres, ix = make(0x901, COUNTS, d)
    Q = queries(0x911, centres, 64, [0, 1], d)
    near = probes(ix, Q, 1)[:, 0]
    T = seg_target(sum(COUNTS), len(COUNTS))
    assert T == 384 and quads(COUNTS[0], T) >= 3 and quads(COUNTS[1], T) == 1 and set(near.tolist()) == {0, 1}, (T, np.bincount(near))
    hot_items, items = both(ix, Q, top_k_for(d), 4, counts=COUNTS)
    assert hot_items == 4 * (quads(COUNTS[0], T) + 1) and items > hot_items   # the two hot lists' quads (one query group each), cold ones behind
elif CASE == "two_groups":          # 160 queries of two home lists: both lists are scanned for three groups of up to 64 queries
    centres, ix = make(0x902, COUNTS, 256)
    Q = queries(0x912, centres, 160, [0, 1], 256)
    assert np.bincount(probes(ix, Q, 4).ravel(), minlength=8).max() > 64
    both(ix, Q, top_k_for(256), 4, counts=COUNTS)
elif CASE == "nprobe1":             # every probed list is hot: the hot region is the whole launch (nothing cold to abandon)
    centres, ix = make(0x903, COUNTS, 256)
    Q = queries(0x913, centres, 64, list(range(8)), 256)
    assert np.unique(probes(ix, Q, 1)).size == 8
    hot_items, items = both(ix, Q, top_k_for(256), 1, must_skip=False, counts=COUNTS)
    assert hot_items == items   # the hot region is the whole launch
elif CASE == "all_lists":           # nprobe = nlist, two home lists of 12: ten lists are cold
    counts = [2700, 700, 1300, 900, 1500, 1100, 800, 788, 600, 500, 450, 950]
    centres, ix = make(0x904, counts, 256)
    Q = queries(0x914, centres, 64, [2, 5], 256)
    assert set(probes(ix, Q, 1)[:, 0].tolist()) == {2, 5}
    hot_items, items = both(ix, Q, top_k_for(256), 12, counts=counts)
    assert 4 * hot_items < items   # two hot lists of twelve
elif CASE == "batch4":              # the smallest batch on this path
    centres, ix = make(0x905, COUNTS, 256)
    Q = queries(0x915, centres, 4, [0, 1], 256)
    both(ix, Q, top_k_for(256), 4, must_skip=False, counts=COUNTS)
elif CASE == "mutate":              # add_batch, remove_batch and compact on one index
    centres, ix = make(0x906, COUNTS, 256)
    Q = queries(0x916, centres, 64, [0, 1], 256)
    extra = dg.normalize_rows(centres[(np.arange(700) * 5) % (8 * MPL)] + dg.default_sigma(256) * dg.noise(0x926, np.arange(700), 256))
    ix.add_batch(extra)
    TK = top_k_for(256)
    both(ix, Q, TK, 4, tag="add")
    ix.remove_batch(np.arange(0, 12288, 3))
    both(ix, Q, TK, 4, tag="remove", must_skip=False)
    ix.compact()
    both(ix, Q, TK, 4, tag="compact", must_skip=False)
print("DONE", CASE, GRID)
'''


def run(case, grid):
    env = dict(os.environ); env["PYTHONPATH"] = ROOT
    r = subprocess.run([sys.executable, "-c", BODY, case, grid], capture_output=True, text=True, env=env, cwd=ROOT, timeout=600)
    print(r.stdout[-4000:])
    assert r.returncode == 0 and ("DONE %s %s" % (case, grid)) in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


@pytest.mark.parametrize("grid", ["one", "two", "all"])
@pytest.mark.parametrize("case", ["hot3", "hot3_d768", "two_groups", "nprobe1", "all_lists", "batch4", "mutate"])
def test_hot_quads_singly_changes_no_bit(case, grid):
    run(case, grid)
