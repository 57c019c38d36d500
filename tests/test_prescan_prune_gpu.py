"""Early abandon of the batched list scan (csrc/prescan.hip.h, prune_lower; option "pre_prune"): a wave stops reading a 64-row
tile once the columns read so far prove that none of its rows can pass any of its queries' thresholds.  The skipped rows would
have been dropped by the threshold anyway, so ids, distance bits and counts must equal those of pre_prune = 0 for EVERY query
(and the oracle's for every 7th) -- on clustered rows of 12 / 4 / 2 / 5 column steps, ragged lists, queries whose neighbours sit
in a list scanned late, a NaN in a column the abandon would skip, poisoned slack rows, after add / remove / compact, on a
cosine-distance index and with every certificate forced to fail."""
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
from tests import datagen as dg
from tests.golden import make_golden as mg
from vers_amd import capi, testhooks
from vers_amd.index import IVFFlatIndex

CASE = sys.argv[1]
# A threshold reaches a list through the query's other blocks.  These indexes are far smaller than the chip: with a block on every
# compute unit all lists are scanned at the same moment and no list ever sees a tight threshold.  ONE block (option
# "scan_reserve_cus": every compute unit but one left free) walks the work in its planned order -- every query's nearest list
# first, then the others -- which is what a full-size launch does to the bulk of its lists.  "all": the default launch.
ONE_BLOCK = sys.argv[2] == "one"
capi.set_option("scan_reserve_cus", (1 << 20) if ONE_BLOCK else -1)

def run(ix, Q, top_k, nprobe, prune):
    capi.set_option("pre_prune", prune)
    f0 = ix.prescan_stats()["fallback_queries"]
    ids, dist, cnt = ix.search_batch(Q, top_k, nprobe)
    st = ix.prune_stats()["last"]
    return ids, dist, cnt, ix.prescan_stats()["fallback_queries"] - f0, st

def both(ix, Q, top_k, nprobe, metric=0, oracle=True, tag=""):
    """pre_prune = 1 against pre_prune = 0 for every query, against the oracle for every 7th; returns the skipped-steps counter"""
    i1, d1, c1, f1, s1 = run(ix, Q, top_k, nprobe, 1)
    i0, d0, c0, f0, s0 = run(ix, Q, top_k, nprobe, 0)
    print("FIG", CASE, tag, "top_k", top_k, "on", s1, "off", s0, "fallback on/off", f1, f0)
    assert s0["steps_skipped"] == 0 and s0["tiles_abandoned"] == 0, s0
    assert np.array_equal(c1, c0), (tag, np.flatnonzero(c1 != c0))
    assert np.array_equal(i1, i0), (tag, np.flatnonzero((i1 != i0).any(axis=1)))
    assert np.array_equal(d1.view(np.uint32), d0.view(np.uint32)), (tag, np.flatnonzero((d1.view(np.uint32) != d0.view(np.uint32)).any(axis=1)))
    assert f1 == f0, (tag, f1, f0)
    if oracle:
        for qi in range(0, Q.shape[0], 7):
            oi, od = co.search_nprobe(ix.values, ix.centroids, ix.ids, Q[qi], top_k, nprobe, metric=metric)
            assert c1[qi] == len(oi) and np.array_equal(i1[qi, :len(oi)], oi), (tag, qi)
            assert np.array_equal(d1[qi, :len(oi)].view(np.uint32), od.view(np.uint32)), (tag, qi)
    return s1["steps_skipped"]

def clustered(seed, n, d, k, modes, b, home_lists=2):
    """Rows of `modes` modes in k lists; b queries drawn from the modes of `home_lists` of the lists only.  A tile holds rows of every
    mode of its list, so a list is abandoned early only where NO query of the group has its own mode there: with queries of every
    mode every list is some query's home and nothing could ever be skipped.  The other lists are probed as 2nd .. 4th nearest."""
    X = dg.dist_c(seed, n, d, modes, dg.default_sigma(d))
    ix = IVFFlatIndex.build_index(k, 1, 3, X, init_indices=mg.init_draws(seed, 1, k, n))
    pool = dg.dist_c(seed + 0x100, 16 * b, d, modes, dg.default_sigma(d), seed_c=seed ^ 0xC0FFEE)   # (the rows' own modes)
    near = np.argmin(((pool[:, None, :] - ix.centroids[None]) ** 2).sum(-1), axis=1)
    sizes = np.bincount(near, minlength=k)
    homes = np.argsort(-sizes)[:home_lists]
    Q = pool[np.isin(near, homes)][:b]
    assert Q.shape[0] == b, Q.shape
    global HOMES
    HOMES = homes
    return X, ix, Q

if CASE == "clustered768":   # 12 steps; ~190 rows per mode, ~24 tiles per list
    X, ix, Q = clustered(0x701, 12288, 768, 8, 64, 64)
    sk = both(ix, Q, 10, 4)
    assert sk > 0 or not ONE_BLOCK, "nothing was abandoned: the case exercises nothing"
    # top_k = 26 keeps 52 keys per query: 64-query blocks no longer fit next to their buffers and the planner takes 32-query blocks with
    # BOTH halves of the query's fp16 split, which the early abandon does not cover (counter 0) ...
    both(ix, Q, 26, 4, tag="hi+lo")
    # ... with the hi-only query block forced the 32-query blocks abandon tiles too
    capi.set_option("pre_hi_only", 1)
    sk = both(ix, Q, 26, 4, tag="hi-only")
    capi.set_option("pre_hi_only", 0)
    # (prescan = 2: after 256 failed queries the failure watch has switched the shadow off for the handle -- nothing left to abandon)
    assert sk > 0 or not ONE_BLOCK or capi.env_option("prescan", 1) == 2, "nothing was abandoned: the case exercises nothing"
elif CASE == "steps":        # 4 steps | 2 steps: nothing to skip | 300 columns: padded to 320, 5 steps
    for d, must in ((256, None), (128, 0), (300, None)):
        X, ix, Q = clustered(0x710 + d, 6144, d, 8, 64, 64)
        sk = both(ix, Q, 10, 4, tag="d%d" % d)
        if must is not None:
            assert sk == must, (d, sk)
        else:
            assert sk > 0 or not ONE_BLOCK, (d, "nothing was abandoned: the case exercises nothing")
elif CASE == "widths":       # the other instantiations in scope: 16-query hi-only blocks, and wide candidate lists (top_k 64: 96 keys, 32-query blocks)
    X, ix, Q = clustered(0x771, 12288, 768, 8, 64, 64)
    capi.set_option("pre_narrow", 1); capi.set_option("pre_hi_only", 1)
    sk = both(ix, Q, 10, 4, tag="narrow16 hi-only")
    capi.set_option("pre_narrow", 0); capi.set_option("pre_hi_only", 0)
    assert sk > 0 or not ONE_BLOCK, "narrow blocks: nothing was abandoned"
    sk = both(ix, Q, 64, 4, tag="wide lists")
    assert sk > 0 or not ONE_BLOCK, "wide lists: nothing was abandoned"
elif CASE == "ragged":       # one-tile items, items whose second wave has no tile, partially filled last tiles
    X, ix, Q = clustered(0x721, 1000, 768, 12, 48, 64)
    both(ix, Q, 10, 4)
    both(ix, Q, 26, 6)
elif CASE == "late":         # neighbours in two lists: the second is scanned after the query's threshold is tight
    X, ix, _ = clustered(0x731, 12288, 768, 8, 64, 64)
    asg = ix.assignments.astype(np.int64)
    big = np.argsort(-np.bincount(asg, minlength=8))[:3]   # a and b from three of the lists: the others stay nobody's home
    rng = np.random.default_rng(0x731)
    Q = np.zeros((64, 768), dtype=np.float32)
    for i in range(64):
        a = int(rng.choice(np.flatnonzero(np.isin(asg, big))))
        others = np.flatnonzero(np.isin(asg, big) & (asg != asg[a]))
        b = int(others[rng.integers(0, others.size)])
        Q[i] = co.normalize((X[a] + X[b]).astype(np.float32))
    sk = both(ix, Q, 10, 4)
    both(ix, Q, 26, 8)
    print("FIG late skipped", sk)
elif CASE == "nonfinite":    # a NaN in a last-step column of one row of a list that otherwise prunes; poisoned slack rows
    X, ix, Q = clustered(0x741, 12288, 768, 8, 64, 64)
    sk_clean = both(ix, Q, 10, 4, tag="clean")
    assert sk_clean > 0 or not ONE_BLOCK
    # the same lists with a NaN in the last column of one row of a list that is NOBODY's home -- one whose tiles the clean run abandons
    # (uploaded as they are: add() would refuse the row).  The reference panics on a NaN distance: a batch that probes the row's list
    # must end in the same status either way, one that does not in the same results.
    nan_row = int(np.flatnonzero(~np.isin(ix.assignments.astype(np.int64), HOMES))[100])
    X2 = X.copy(); X2[nan_row, 767] = np.float32("nan")
    ix2 = IVFFlatIndex(768)
    ix2.values, ix2.centroids, ix2.assignments, ix2.ids, ix2.num_centroids = X2, ix.centroids, ix.assignments, ix.ids, ix.num_centroids
    ix2._upload()
    lst = int(ix.assignments[nan_row])
    near = np.argsort(((Q[:, None, :] - ix.centroids[None]) ** 2).sum(-1), axis=1)[:, :4]
    hit = np.flatnonzero((near == lst).any(axis=1)); miss = np.flatnonzero(~(near == lst).any(axis=1))
    print("FIG nan: queries probing the list", hit.size, "not probing it", miss.size)
    assert hit.size and miss.size
    sk = both(ix2, Q[miss], 10, 4, oracle=False, tag="nan-miss")
    assert sk > 0 or not ONE_BLOCK
    status = []
    for prune in (1, 0):
        try:
            out = run(ix2, Q[hit], 10, 4, prune)
            status.append(("ok", out[0].tobytes(), out[1].tobytes(), out[2].tobytes(), out[3]))
        except capi.VersError as e:
            status.append(("err", e.status))
    print("FIG nan-hit", status[0][:2] if status[0][0] == "err" else ("ok", status[0][4]))
    assert status[0] == status[1], "a NaN row: pruning on and off disagree"
    for v in (float("inf"), float("nan"), -1.0e30):
        testhooks.poison_slack(ix, v)
        sk = both(ix, Q, 10, 4, tag="slack %r" % v)
        assert sk > 0 or not ONE_BLOCK
elif CASE == "mutate":       # add_batch, remove_batch and compact on one small index
    X, ix, Q = clustered(0x751, 4096, 768, 8, 32, 64)
    ix.add_batch(dg.dist_c(0x752, 700, 768, 32, dg.default_sigma(768), seed_c=0x751 ^ 0xC0FFEE))
    both(ix, Q, 10, 4, tag="add")
    ix.remove_batch(np.arange(0, 4096, 3))
    both(ix, Q, 10, 4, tag="remove")
    ix.compact()
    sk = both(ix, Q, 10, 4, tag="compact")
    print("FIG mutate skipped", sk)
elif CASE == "cosine":       # the bound is squared L2's: nothing is abandoned on a cosine-distance index
    X = dg.dist_c(0x761, 6144, 768, 64, dg.default_sigma(768))
    ix = IVFFlatIndex.build_index(8, 1, 3, X, init_indices=mg.init_draws(0x761, 1, 8, 6144), metric=capi.METRIC_COSDIST)
    Q = dg.dist_c(0x861, 64, 768, 64, dg.default_sigma(768), seed_c=0x761 ^ 0xC0FFEE)
    sk = both(ix, Q, 10, 4, metric=1)
    assert sk == 0, sk
print("DONE", CASE)
'''


def run(case, env_extra=None, blocks="one"):
    env = dict(os.environ); env.update(env_extra or {}); env["PYTHONPATH"] = ROOT
    r = subprocess.run([sys.executable, "-c", BODY, case, blocks], capture_output=True, text=True, env=env, cwd=ROOT, timeout=600)
    print(r.stdout[-4000:])
    assert r.returncode == 0 and ("DONE " + case) in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


@pytest.mark.parametrize("case", ["clustered768", "steps", "widths", "ragged", "late", "nonfinite", "mutate", "cosine"])
def test_abandoning_tiles_changes_no_bit(case):
    run(case)


def test_abandoning_tiles_on_the_default_launch():
    """A block per compute unit (the default): on an index this small nothing need be abandoned, and nothing may change."""
    run("clustered768", blocks="all")
    run("ragged", blocks="all")


def test_abandoning_tiles_with_every_certificate_forced_to_fail():
    """prescan = 2: every query is re-scanned exactly whatever the list scan kept."""
    run("clustered768", {"VERS_OPTIONS": "prescan=2"})
