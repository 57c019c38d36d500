"""The list of LIVE cold quads that the split scan's last launch draws from (csrc/head_filter.hip.h appends it, csrc/prescan.hip.h hands
out its positions; option "pre_live_list", vers_ivf_cold_state).  Which block scans which quad was never deterministic and a dead quad
holds no row a threshold would have kept, so ids, distance bits, counts and the fallback count with pre_live_list = 1 must equal, with
no tolerance, those of the same handle with pre_live_list = 0 -- the walk over every cold quad that skips the dead ones by their mark --
for EVERY query, and the oracle's for every 7th.  Every cold quad is either ruled out by one of the two filters or listed:
live + dead = tested, and the cold launch scans exactly the live ones, whichever way it finds them.

The indexes are the small ones of tests/test_ball_filter_gpu.py with "pre_ball_min_quads" = 1, the smallest shapes at which the hand-out
can go wrong: an empty list (every cold quad dies; one and two query groups per list), dead and live quads mixed (700 lists, 20 of them
with planted rows), a unit of several quads kept live by planted rows (also with the scan on ONE block, so that a run holds several
positions of the list; whether two entries of the unit then stand adjacent and ascending, and merge, is up to the order in which the
filter's blocks appended them -- either way the results must be the oracle's, which a slot filled twice or not at all would break),
a NaN row, the head's filter alone (pre_ball = 0), rows without contrast
(nothing dies: the list holds every cold quad, and the back-off still engages) and a cold region below the ball pass's engaging rule
(identity survivor list)."""
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
from vers_amd import capi
from vers_amd.index import IVFFlatIndex

CASE = sys.argv[1]
D = 768
capi.set_option("pre_head", 1)
capi.set_option("pre_ball", 1)
capi.set_option("pre_ball_min_quads", 1)
capi.set_option("pre_head_backoff", 0)     # two scans of one handle are compared: the second must not sit the split out

def run(ix, Q, top_k, nprobe, live):
    capi.set_option("pre_live_list", live)
    f0 = ix.prescan_stats()["fallback_queries"]
    try:
        ids, dist, cnt = ix.search_batch(Q, top_k, nprobe)
    finally:
        capi.set_option("pre_live_list", 1)
    return ids, dist, cnt, ix.prescan_stats()["fallback_queries"] - f0, ix.head_state()["last"], ix.ball_state()["last"], ix.cold_state()["last"]

def accounted(h, c, tag):
    """every cold quad is dead or listed, and the cold launch scanned the live ones and nothing else"""
    assert h["quads_tested"] > 0, (tag, h)
    assert c["quads_live"] + h["quads_dead"] == h["quads_tested"], (tag, h, c)
    assert c["quads_scanned"] == c["quads_live"], (tag, c)

def both(ix, Q, top_k, nprobe, tag="", oracle=True):
    """pre_live_list = 1 against 0 for every query, against the oracle for every 7th; returns the counters of the run through the list"""
    i1, d1, c1, f1, h1, b1, s1 = run(ix, Q, top_k, nprobe, 1)
    i0, d0, c0, f0, h0, b0, s0 = run(ix, Q, top_k, nprobe, 0)
    print("FIG", CASE, tag, "b", Q.shape[0], "balls", b1, "head", h1, "cold, list", s1, "cold, walk", s0, "fallback", f1, f0)
    assert np.array_equal(c1, c0), (tag, np.flatnonzero(c1 != c0))
    assert np.array_equal(i1, i0), (tag, np.flatnonzero((i1 != i0).any(axis=1)))
    assert np.array_equal(d1.view(np.uint32), d0.view(np.uint32)), (tag, np.flatnonzero((d1.view(np.uint32) != d0.view(np.uint32)).any(axis=1)))
    assert f1 == f0, (tag, f1, f0)
    accounted(h1, s1, tag + " list")
    accounted(h0, s0, tag + " walk")
    # (how many die may differ by a quad between two scans: the thresholds the hot launch leaves depend on its blocks' order)
    assert (h1["quads_tested"], b1["units_tested"]) == (h0["quads_tested"], b0["units_tested"]), (tag, h1, h0, b1, b0)
    if oracle:
        for qi in range(0, Q.shape[0], 7):
            oi, od = co.search_nprobe(ix.values, ix.centroids, ix.ids, Q[qi], top_k, nprobe)
            assert c1[qi] == len(oi) and np.array_equal(i1[qi, :len(oi)], oi), (tag, qi)
            assert np.array_equal(d1[qi, :len(oi)].view(np.uint32), od.view(np.uint32)), (tag, qi)
    return h1, b1, s1, i1

def home_queries(ix, seed, d, modes, b, home_lists):
    """b queries from the rows' own modes, those of `home_lists` of the lists only: the other lists are nobody's nearest -- cold"""
    pool = dg.dist_c(seed + 0x100, 24 * b, d, modes, dg.default_sigma(d), seed_c=seed ^ 0xC0FFEE)
    near = np.argmin(((pool[:, None, :] - ix.centroids[None]) ** 2).sum(-1), axis=1)
    homes = np.argsort(-np.bincount(near, minlength=ix.centroids.shape[0]))[:home_lists]
    Q = pool[np.isin(near, homes)][:b]
    assert Q.shape[0] == b, Q.shape
    return Q

def dist_c_index(seed, n, d, k, modes):
    X = dg.dist_c(seed, n, d, modes, dg.default_sigma(d))
    return X, IVFFlatIndex.build_index(k, 1, 3, X, init_indices=mg.init_draws(seed, 1, k, n))

def unit(v):
    return (v / np.sqrt((v.astype(np.float64) ** 2).sum(axis=-1, keepdims=True))).astype(np.float32)

def around(rng, c, n, s=0.01):
    return unit(c[None, :] + s * rng.standard_normal((n, D)))

def index_of(lists):
    """an index whose lists are the given row blocks, uploaded as they are (centroid = the list's mean)"""
    ix = IVFFlatIndex(D)
    ix.values = np.concatenate(lists).astype(np.float32)
    ix.centroids = np.stack([np.nan_to_num(l.astype(np.float64)).mean(axis=0) for l in lists]).astype(np.float32)
    ix.assignments = np.concatenate([np.full(len(l), i, dtype=np.uint64) for i, l in enumerate(lists)])
    off = np.concatenate([[0], np.cumsum([len(l) for l in lists])])
    ix.ids = [list(range(int(off[i]), int(off[i + 1]))) for i in range(len(lists))]
    ix.num_centroids = len(lists)
    ix._upload()
    return ix

def twelve(rng):
    """twelve single-mode lists, the first three of them the queries' homes"""
    lens = [1250 + 41 * i for i in range(12)]
    modes = [unit(rng.standard_normal(D)) for _ in lens]
    lists = [around(rng, c, n) for c, n in zip(modes, lens)]
    Q = np.concatenate([around(rng, modes[h], 3) for h in (0, 1, 2)])[:8]
    return modes, lists, Q

if CASE == "empty":          # every cold quad dies: the list is empty and the cold launch leaves at its first draw
    X, ix = dist_c_index(0xB01, 40000, 768, 32, 128)
    for b in (8, 40, 72):    # groups of <= 32 queries | two query tiles | two groups per list
        h1, b1, s1, _ = both(ix, home_queries(ix, 0xB01, 768, 128, b, 3), 10, 32, tag="b%d" % b)
        assert h1["quads_dead"] == h1["quads_tested"] and s1 == dict(quads_live=0, quads_scanned=0), (b, h1, s1)
elif CASE == "planted":      # dead and live quads mixed: twenty cold lists hold six rows next to a home mode and stay live
    rng = np.random.default_rng(0xB04)
    modes = [unit(rng.standard_normal(D)) for _ in range(700)]
    homes = [0, 1, 2]
    lists = [around(rng, c, 70 + (i % 5) * 30) for i, c in enumerate(modes)]
    picks = list(range(20, 700, 34))
    for j, i in enumerate(picks):
        lists[i] = np.concatenate([lists[i], unit(modes[homes[j % 3]][None, :] + 0.002 * rng.standard_normal((6, D)))])
    Q = np.concatenate([around(rng, modes[h], 24) for h in homes])
    off = np.concatenate([[0], np.cumsum([len(l) for l in lists])])
    planted = np.concatenate([np.arange(off[i + 1] - 6, off[i + 1]) for i in picks])
    ix = index_of(lists)
    h1, b1, s1, ids = both(ix, Q, 10, 700, tag="planted")   # every list is probed: 697 cold lists, two groups each
    # all twenty planted lists for the group of queries 0 .. 63, the six next to the last home mode for the group of queries 64 .. 71
    assert s1["quads_live"] >= 26 and h1["quads_dead"] > 0, (h1, s1)
    assert np.isin(ids, planted).all(), np.flatnonzero(~np.isin(ids, planted).all(axis=1))
elif CASE == "multi":        # a unit of several quads: the verdict and the list cover each of them
    rng = np.random.default_rng(0xB0C)
    modes, lists, Q = twelve(rng)
    lists[7] = around(rng, modes[7], 8000)     # ~4 quads of ~2000 rows (the other lists: one quad each)
    planted = []
    for r0 in (100, 2100, 4100, 6100):        # six rows next to home mode 0 in every quarter of the long list
        lists[7][r0:r0 + 6] = around(rng, modes[0], 6, s=0.004)
        planted += list(range(r0, r0 + 6))
    ix = index_of(lists)
    base = sum(len(l) for l in lists[:7])
    for reserve in (-1, 1 << 20):             # the scan's own grid | ONE block: runs of several positions (entries merge where the list's order lets them)
        capi.set_option("scan_reserve_cus", reserve)
        h1, b1, s1, ids = both(ix, Q, 10, 12, tag="reserve %d" % reserve)
        assert b1 == dict(units_tested=9, units_dead=8), b1
        assert s1["quads_live"] >= 2 and h1["quads_dead"] >= 8, (h1, s1)   # the long list's quads, those that hold planted rows
        near0 = np.flatnonzero(np.argmin(((Q[:, None, :] - np.stack(modes[:3])[None]) ** 2).sum(-1), axis=1) == 0)
        assert np.isin(ids[near0], base + np.asarray(planted)).all(), ids[near0]
    capi.set_option("scan_reserve_cus", -1)
elif CASE == "nanrow":       # a NaN row: its list stays live, the batch ends in status 2 either way
    rng = np.random.default_rng(0xB03)
    modes, lists, Q = twelve(rng)
    ix = index_of(lists)     # without the NaN: every cold unit dies, nothing is listed
    h1, b1, s1, _ = both(ix, Q, 10, 12, tag="clean")
    assert b1 == dict(units_tested=9, units_dead=9) and s1 == dict(quads_live=0, quads_scanned=0), (b1, s1)
    lists[7][100, 767] = np.float32("nan")
    ix = index_of(lists)
    status = []
    for live in (1, 0):
        try:
            out = run(ix, Q, 10, 12, live)
            status.append(("ok", out[0].tobytes(), out[1].tobytes(), out[2].tobytes(), out[3]))
        except capi.VersError as e:
            status.append(("err", e.status))
        h, bl, c = ix.head_state()["last"], ix.ball_state()["last"], ix.cold_state()["last"]
        print("FIG nanrow live", live, status[-1][:2] if status[-1][0] == "err" else "ok", h, bl, c)
        accounted(h, c, "nanrow %d" % live)
        # the eight other cold units still die by their balls, every quad of theirs with them: what is listed is list 7's, the one
        # difference to the index above
        assert bl == dict(units_tested=9, units_dead=8) and c["quads_live"] >= 1, (bl, c)
    assert status[0] == status[1] == ("err", 2), [s[:2] for s in status]
elif CASE == "headonly":     # pre_ball = 0: the list comes from the head's filter alone
    capi.set_option("pre_ball", 0)
    rng = np.random.default_rng(0xB0D)
    modes, lists, Q = twelve(rng)
    lists[7][200:206] = around(rng, modes[0], 6, s=0.004)
    ix = index_of(lists)
    h1, b1, s1, _ = both(ix, Q, 10, 12, tag="head only")
    assert b1 == dict(units_tested=0, units_dead=0), b1
    assert s1["quads_live"] >= 1 and h1["quads_dead"] >= 1, (h1, s1)
elif CASE == "distu":        # rows without contrast: nothing dies, the list holds every cold quad -- and the back-off still engages
    X = dg.dist_u(0xB05, 20000, 768)
    ix = IVFFlatIndex.build_index(32, 1, 3, X, init_indices=mg.init_draws(0xB05, 1, 32, 20000))
    Q = dg.dist_u(0xB06, 40, 768)
    h1, b1, s1, _ = both(ix, Q, 10, 32, tag="distu")
    assert 8 * h1["quads_dead"] < h1["quads_tested"] and s1["quads_live"] == h1["quads_tested"] - h1["quads_dead"], (h1, s1)
    # fewer than 1/8 of the quads died in the split scans above: the filter's last block has set the handle's pinned word, and with the
    # back-off switched on the next batch reads it and sits the split out -- one launch, no list
    capi.set_option("pre_head_backoff", 1)
    ix.search_batch(Q, 10, 32)
    assert ix.head_state()["last"]["quads_tested"] == 0 and ix.cold_state()["last"] == dict(quads_live=0, quads_scanned=0), (ix.head_state(), ix.cold_state())
elif CASE == "identity":     # a cold region below the ball pass's engaging rule: the survivor list is the identity, the head's filter lists what it leaves
    capi.set_option("pre_ball_min_quads", 0)
    rng = np.random.default_rng(0xB0E)
    modes, lists, Q = twelve(rng)
    lists[7][200:206] = around(rng, modes[0], 6, s=0.004)
    ix = index_of(lists)
    assert ix.ball_state()["valid"], ix.ball_state()
    h1, b1, s1, _ = both(ix, Q, 10, 12, tag="identity")
    assert b1 == dict(units_tested=0, units_dead=0), b1
    assert h1["quads_tested"] >= 9 and s1["quads_live"] >= 1 and h1["quads_dead"] >= 1, (h1, s1)   # nine cold lists, every quad of theirs through the head's filter
print("DONE", CASE)
'''


def run(case):
    env = dict(os.environ); env["PYTHONPATH"] = ROOT
    r = subprocess.run([sys.executable, "-c", BODY, case], capture_output=True, text=True, env=env, cwd=ROOT, timeout=600)
    print(r.stdout[-4000:])
    assert r.returncode == 0 and ("DONE " + case) in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


@pytest.mark.parametrize("case", ["empty", "planted", "multi", "nanrow", "headonly", "distu", "identity"])
def test_cold_launch_over_the_live_list_changes_no_bit(case):
    run(case)
