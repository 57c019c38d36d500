"""The lists' sub-cluster balls and the pass that rules cold quads out with them before the int8 head's filter reads their rows
(csrc/ball_filter.hip.h; options "pre_ball", "pre_ball_cut", "pre_ball_min_quads").  A dropped quad holds only rows a threshold would
have dropped anyway, so ids, distance bits, counts and the fallback count must equal, with no tolerance, those of the same handle with
pre_ball = 0 for EVERY query and the oracle's for every 7th.  The indexes here are small -- tens of cold quads, where the pass stands
aside by default (it engages from twice the compute units' worth of cold quads) -- so every case lowers the threshold to one quad
through "pre_ball_min_quads"; the planted case has ~700 cold quads and runs at the default as well.  Cases: Dist-C at d = 768, 32 lists of
4 modes, every list probed, batches of 8, 40 and 72 (units must die, the head's filter must read fewer steps than without the pass),
the slack rows poisoned, a NaN row in a cold list (its sub-cluster is open), cold lists with six planted rows next to a home mode (their
units stay live, their rows are returned), Dist-U (no balls at all), d = 300, d = 128 (no split scan), add_batch / remove_batch /
compact, and a list of 40 modes (more than the cap of 32: no balls for it, the head handles it)."""
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
D = 768
capi.set_option("pre_head", 1)
capi.set_option("pre_ball", 1)             # (read when the index is built -- whether there are balls -- and per search -- whether they are used)
capi.set_option("pre_ball_min_quads", 1)   # the indexes here have tens of cold quads: the default threshold would keep the pass off
ZERO = dict(units_tested=0, units_dead=0)

def run(ix, Q, top_k, nprobe, ball):
    capi.set_option("pre_ball", ball)
    f0 = ix.prescan_stats()["fallback_queries"]
    try:
        ids, dist, cnt = ix.search_batch(Q, top_k, nprobe)
    finally:
        capi.set_option("pre_ball", 1)
    return ids, dist, cnt, ix.prescan_stats()["fallback_queries"] - f0, ix.head_state(), ix.ball_state()

def both(ix, Q, top_k, nprobe, tag="", oracle=True):
    """pre_ball = 1 against pre_ball = 0 for every query, against the oracle for every 7th; returns the head's and the balls' state of each"""
    i1, d1, c1, f1, h1, b1 = run(ix, Q, top_k, nprobe, 1)
    i0, d0, c0, f0, h0, b0 = run(ix, Q, top_k, nprobe, 0)
    print("FIG", CASE, tag, "b", Q.shape[0], "balls", {k: b1[k] for k in ("valid", "bytes", "lists_with_balls", "subclusters")}, "last", b1["last"],
          "head on", h1["last"], "head off", h0["last"], "fallback on/off", f1, f0)
    assert b0["last"] == ZERO, b0
    assert np.array_equal(c1, c0), (tag, np.flatnonzero(c1 != c0))
    assert np.array_equal(i1, i0), (tag, np.flatnonzero((i1 != i0).any(axis=1)))
    assert np.array_equal(d1.view(np.uint32), d0.view(np.uint32)), (tag, np.flatnonzero((d1.view(np.uint32) != d0.view(np.uint32)).any(axis=1)))
    assert f1 == f0, (tag, f1, f0)
    if oracle:
        for qi in range(0, Q.shape[0], 7):
            oi, od = co.search_nprobe(ix.values, ix.centroids, ix.ids, Q[qi], top_k, nprobe)
            assert c1[qi] == len(oi) and np.array_equal(i1[qi, :len(oi)], oi), (tag, qi)
            assert np.array_equal(d1[qi, :len(oi)].view(np.uint32), od.view(np.uint32)), (tag, qi)
    return h1, b1, h0

def fired(res, tag):
    """units died, and the head's filter read fewer steps than without the pass; the merged quad counts cover both filters"""
    h1, b1, h0 = res
    assert b1["valid"] and b1["last"]["units_tested"] > 0 and b1["last"]["units_dead"] > 0, (tag, b1)
    assert h1["last"]["head_steps"] < h0["last"]["head_steps"], (tag, h1, h0)
    assert h1["last"]["quads_tested"] == h0["last"]["quads_tested"] and h1["last"]["quads_dead"] >= b1["last"]["units_dead"], (tag, h1, h0, b1)

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

if CASE == "base":           # 40 k rows, 32 lists of 4 modes, EVERY list probed: 29 cold lists, one quad per (list, group)
    X, ix = dist_c_index(0xB01, 40000, 768, 32, 128)
    st = ix.ball_state()
    print("FIG base balls", st)
    assert st["valid"] and st["bytes"] > 0 and st["lists_with_balls"] >= 28 and st["lists_with_balls"] <= st["subclusters"] <= 32 * 32, st
    for b in (8, 40, 72):    # groups of <= 32 queries | two query tiles | more than one group per list
        fired(both(ix, home_queries(ix, 0xB01, 768, 128, b, 3), 10, 32, tag="b%d" % b), "b%d" % b)
elif CASE == "slack":        # the slack rows poisoned: a huge finite value, NaN (the derived arrays, the balls among them, are rebuilt)
    X, ix = dist_c_index(0xB02, 20000, 768, 32, 128)
    for v in (1.0e30, float("nan")):
        testhooks.poison_slack(ix, v)
        assert ix.ball_state()["valid"], ix.ball_state()
        fired(both(ix, home_queries(ix, 0xB02, 768, 128, 40, 3), 10, 32, tag="slack %r" % v), "slack %r" % v)
elif CASE == "nanrow":       # a stored row with a NaN in a cold list: its sub-cluster is open, its unit is not ruled out by the balls
    rng = np.random.default_rng(0xB03)
    lens = [1250 + 41 * i for i in range(12)]
    modes = [unit(rng.standard_normal(D)) for _ in lens]
    lists = [around(rng, c, n) for c, n in zip(modes, lens)]
    homes = [0, 1, 2]
    Q = np.concatenate([around(rng, modes[h], 3) for h in homes])[:8]
    ix = index_of(lists)
    h1, b1, h0 = both(ix, Q, 10, 12, tag="clean")
    assert b1["last"] == dict(units_tested=9, units_dead=9), b1    # one mode per list, one group: every cold unit dies
    lists[7][100, 767] = np.float32("nan")
    ix2 = index_of(lists)
    assert ix2.ball_state()["valid"], ix2.ball_state()
    # the reference panics on a NaN distance: the batch ends in the same status either way (tests/test_prescan_prune_gpu.py)
    status = []
    for ball in (1, 0):
        try:
            out = run(ix2, Q, 10, 12, ball)
            status.append(("ok", out[0].tobytes(), out[1].tobytes(), out[2].tobytes(), out[3]))
        except capi.VersError as e:
            status.append(("err", e.status))
        if ball == 1:
            b2 = ix2.ball_state()
    print("FIG nanrow", status[0][:2] if status[0][0] == "err" else ("ok", status[0][4]), b2["last"])
    assert status[0] == status[1], "a NaN row: the ball pass on and off disagree"
    assert b2["last"] == dict(units_tested=9, units_dead=8), b2    # the NaN row's list alone stays live
elif CASE == "planted":      # twenty cold lists hold six rows next to a home mode: their units stay live, their rows are what the search returns
    rng = np.random.default_rng(0xB04)
    n_lists = 700
    modes = [unit(rng.standard_normal(D)) for _ in range(n_lists)]
    homes = [0, 1, 2]
    lists = [around(rng, c, 70 + (i % 5) * 30) for i, c in enumerate(modes)]
    picks = list(range(20, 700, 34))
    for j, i in enumerate(picks):
        lists[i] = np.concatenate([lists[i], unit(modes[homes[j % 3]][None, :] + 0.002 * rng.standard_normal((6, D)))])
    Q = np.concatenate([around(rng, modes[h], 24) for h in homes])
    off = np.concatenate([[0], np.cumsum([len(l) for l in lists])])
    planted = np.concatenate([np.arange(off[i + 1] - 6, off[i + 1]) for i in picks])
    for mq in (1, 0):        # the lowered threshold, then the default one (twice the compute units: ~700 cold quads are above it on a full device)
        capi.set_option("pre_ball_min_quads", mq)
        # a handle of its own per round: the planted rows are near-ties, most queries are re-scanned exactly, and after a few such
        # batches the handle switches its fp16 shadow -- and with it the split scan -- off
        ix = index_of(lists)
        h1, b1, h0 = both(ix, Q, 10, 700, tag="min_quads %d" % mq)   # every list is probed: 697 cold lists, two groups each
        if mq == 1:
            fired((h1, b1, h0), "planted")
        t, dd = b1["last"]["units_tested"], b1["last"]["units_dead"]
        # a planted list's unit stays live for a group that holds a query of its home mode: all twenty for the group of queries 0 .. 63
        # (every home mode), the six planted next to the last home mode for the group of queries 64 .. 71
        assert t == 0 or (t - dd >= 26 and dd > 0), b1
        ids, _, _ = ix.search_batch(Q, 10, 700)
        assert np.isin(ids, planted).all(), np.flatnonzero(~np.isin(ids, planted).all(axis=1))
elif CASE == "distu":        # no clusters: no list gets balls, everything is released, the pass is never launched
    X = dg.dist_u(0xB05, 20000, 768)
    ix = IVFFlatIndex.build_index(32, 1, 3, X, init_indices=mg.init_draws(0xB05, 1, 32, 20000))
    st = ix.ball_state()
    assert not st["valid"] and st["bytes"] == 0 and st["lists_with_balls"] == 0 and st["subclusters"] == 0, st
    h1, b1, h0 = both(ix, dg.dist_u(0xB06, 40, 768), 10, 32)
    # (the head's own counters differ between the two runs: nothing dies on such rows and its back-off sits the second scan out)
    assert b1["last"] == ZERO and b1["total"] == ZERO, (b1, h1, h0)
elif CASE == "d300":         # ld 320: five steps of 64 columns, the centres' dot products in two shares of 160
    X, ix = dist_c_index(0xB07, 20000, 300, 32, 128)
    fired(both(ix, home_queries(ix, 0xB07, 300, 128, 40, 3), 10, 32), "d300")
elif CASE == "d128":         # two steps: no head, no split scan -- the pass never runs
    X, ix = dist_c_index(0xB08, 20000, 128, 32, 128)
    h1, b1, h0 = both(ix, home_queries(ix, 0xB08, 128, 128, 40, 3), 10, 32)
    assert b1["last"] == ZERO and b1["total"] == ZERO and h1["last"]["quads_tested"] == 0, (b1, h1)
elif CASE == "lifecycle":    # add_batch and remove_batch invalidate the balls with the head, compact derives them again
    X, ix = dist_c_index(0xB09, 20000, 768, 32, 128)
    Q = home_queries(ix, 0xB09, 768, 128, 40, 3)
    fired(both(ix, Q, 10, 32, tag="built"), "built")
    ix.add_batch(dg.dist_c(0xB0A, 700, 768, 128, dg.default_sigma(768), seed_c=0xB09 ^ 0xC0FFEE))
    h1, b1, h0 = both(ix, Q, 10, 32, tag="add")
    assert not b1["valid"] and b1["last"] == ZERO, b1
    ix.compact()
    fired(both(ix, Q, 10, 32, tag="compact"), "compact")
    ix.remove_batch(np.arange(0, 20000, 3))
    h1, b1, h0 = both(ix, Q, 10, 32, tag="remove")
    assert not b1["valid"] and b1["last"] == ZERO, b1
    ix.compact()
    fired(both(ix, Q, 10, 32, tag="compact 2"), "compact 2")
elif CASE == "cap":          # a list of 40 modes: more sub-clusters than the cap of 32 -- no balls for it, the head's filter handles it as before
    rng = np.random.default_rng(0xB0B)
    lens = [1250 + 41 * i for i in range(12)]
    modes = [unit(rng.standard_normal(D)) for _ in lens]
    lists = [around(rng, c, n) for c, n in zip(modes, lens)]
    lists[5] = np.concatenate([around(rng, unit(rng.standard_normal(D)), 30) for _ in range(40)])
    ix = index_of(lists)
    st = ix.ball_state()
    assert st["valid"] and st["lists_with_balls"] == 11 and st["subclusters"] == 11, st
    homes = [0, 1, 2]
    Q = np.concatenate([around(rng, modes[h], 3) for h in homes])[:8]
    h1, b1, h0 = both(ix, Q, 10, 12, tag="cap")
    assert b1["last"] == dict(units_tested=9, units_dead=8), b1
    assert h1["last"]["quads_dead"] == h1["last"]["quads_tested"] == h0["last"]["quads_tested"], (h1, h0)   # ... and the head rules the ninth list's quads out
    assert 0 < h1["last"]["head_steps"] < h0["last"]["head_steps"], (h1, h0)
print("DONE", CASE)
'''


def run(case):
    env = dict(os.environ); env["PYTHONPATH"] = ROOT
    r = subprocess.run([sys.executable, "-c", BODY, case], capture_output=True, text=True, env=env, cwd=ROOT, timeout=600)
    print(r.stdout[-4000:])
    assert r.returncode == 0 and ("DONE " + case) in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


@pytest.mark.parametrize("case", ["base", "slack", "nanrow", "planted", "distu", "d300", "d128", "lifecycle", "cap"])
def test_ruling_cold_units_out_by_their_balls_changes_no_bit(case):
    run(case)
