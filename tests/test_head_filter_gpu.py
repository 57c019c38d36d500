"""The int8 head of the stored rows and the filter that rules cold quads out with it (csrc/head_filter.hip.h; options "pre_head",
"pre_head_cols"): where tiles are abandoned early the list scan runs as three launches -- hot quads, filter, the cold quads it left.
A dropped quad holds only rows a threshold would have dropped anyway, so ids, distance bits and counts must equal, with no tolerance,
those of the same handle with pre_head = 0 for EVERY query and the oracle's for every 7th: on clustered rows (Dist-C, d = 768, 32
lists of 4 modes, nprobe 8) in batches of 8, 40 and 72 queries -- groups of up to 32, two query sets, more than one group per
list --, with a one-tile list, at d = 300 (head clipped to 256 columns) and d = 128 (no head: one launch), on rows without clusters
(Dist-U), after add_batch / remove_batch (head invalid, one launch) and compact (valid again), and with the slack rows poisoned.
A condition, not a measurement: in every Dist-C case some quad must die, in the base case at least half of those tested -- a filter
that never fires does not pass."""
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
capi.set_option("pre_head", 1)   # (read when the index is built -- whether there is a head -- and per search -- whether it is used)

def run(ix, Q, top_k, nprobe, head):
    capi.set_option("pre_head", head)
    f0 = ix.prescan_stats()["fallback_queries"]
    ids, dist, cnt = ix.search_batch(Q, top_k, nprobe)
    st = ix.head_state()
    capi.set_option("pre_head", 1)
    return ids, dist, cnt, ix.prescan_stats()["fallback_queries"] - f0, st

def both(ix, Q, top_k, nprobe, tag="", oracle=True):
    """pre_head = 1 against pre_head = 0 for every query, against the oracle for every 7th; returns the filter's counters of the split scan"""
    i1, d1, c1, f1, s1 = run(ix, Q, top_k, nprobe, 1)
    i0, d0, c0, f0, s0 = run(ix, Q, top_k, nprobe, 0)
    print("FIG", CASE, tag, "b", Q.shape[0], "head", {k: s1[k] for k in ("valid", "cols", "bytes")}, "last", s1["last"], "off", s0["last"], "fallback on/off", f1, f0)
    assert s0["last"] == dict(quads_tested=0, quads_dead=0, head_steps=0), s0
    assert np.array_equal(c1, c0), (tag, np.flatnonzero(c1 != c0))
    assert np.array_equal(i1, i0), (tag, np.flatnonzero((i1 != i0).any(axis=1)))
    assert np.array_equal(d1.view(np.uint32), d0.view(np.uint32)), (tag, np.flatnonzero((d1.view(np.uint32) != d0.view(np.uint32)).any(axis=1)))
    assert f1 == f0, (tag, f1, f0)
    if oracle:
        for qi in range(0, Q.shape[0], 7):
            oi, od = co.search_nprobe(ix.values, ix.centroids, ix.ids, Q[qi], top_k, nprobe)
            assert c1[qi] == len(oi) and np.array_equal(i1[qi, :len(oi)], oi), (tag, qi)
            assert np.array_equal(d1[qi, :len(oi)].view(np.uint32), od.view(np.uint32)), (tag, qi)
    return s1

def home_queries(ix, seed, d, modes, b, home_lists):
    """b queries from the rows' own modes, those of `home_lists` of the lists only: the other lists are nobody's nearest -- cold --
    and are probed as 2nd .. nprobe-th nearest"""
    pool = dg.dist_c(seed + 0x100, 24 * b, d, modes, dg.default_sigma(d), seed_c=seed ^ 0xC0FFEE)
    near = np.argmin(((pool[:, None, :] - ix.centroids[None]) ** 2).sum(-1), axis=1)
    homes = np.argsort(-np.bincount(near, minlength=ix.centroids.shape[0]))[:home_lists]
    Q = pool[np.isin(near, homes)][:b]
    assert Q.shape[0] == b, Q.shape
    return Q

def dist_c_index(seed, n, d, k, modes):
    X = dg.dist_c(seed, n, d, modes, dg.default_sigma(d))
    return X, IVFFlatIndex.build_index(k, 1, 3, X, init_indices=mg.init_draws(seed, 1, k, n))

def dead_some(st, tag, half=False):
    t, dd = st["last"]["quads_tested"], st["last"]["quads_dead"]
    assert st["valid"] and t > 0 and dd > 0, (tag, st)
    if half:
        assert 2 * dd >= t, (tag, st)

if CASE == "base":           # 40 k rows, 32 lists of 4 modes (~1250 rows, ~20 tiles, 2 quads each; lengths are no multiples of 64), nprobe 8
    X, ix = dist_c_index(0x801, 40000, 768, 32, 128)
    assert ix.head_state()["valid"] and ix.head_state()["cols"] == 384 and ix.head_state()["bytes"] > 0, ix.head_state()
    for b in (8, 40, 72):    # groups of <= 32 queries | two query sets | more than one group per list
        Q = home_queries(ix, 0x801, 768, 128, b, 3)
        dead_some(both(ix, Q, 10, 8, tag="b%d" % b), "b%d" % b, half=True)
    for v in (1.0e30, float("nan")):   # the slack rows poisoned: a huge finite value, NaN (the derived arrays, the head among them, are rebuilt)
        testhooks.poison_slack(ix, v)
        Q = home_queries(ix, 0x801, 768, 128, 40, 3)
        dead_some(both(ix, Q, 10, 8, tag="slack %r" % v), "slack %r" % v)
elif CASE == "onetile":      # a list of ONE partial tile (40 rows of a tight mode of their own) among the others
    rng = np.random.default_rng(0x811)
    unit = lambda v: (v / np.sqrt((v.astype(np.float64) ** 2).sum())).astype(np.float32)
    tiny = unit(rng.standard_normal(768))   # a mode of its own, as far from the others as they are from each other
    extra = np.stack([unit(tiny + 0.01 * rng.standard_normal(768)) for _ in range(40)])
    X, ixb = dist_c_index(0x811, 30000, 768, 32, 128)
    ix = IVFFlatIndex(768)      # the built lists + the extra rows as a 33rd, uploaded as they are
    ix.values = np.concatenate([X, extra]).astype(np.float32)
    ix.centroids = np.concatenate([ixb.centroids, extra.mean(axis=0, keepdims=True)]).astype(np.float32)
    ix.assignments = np.concatenate([ixb.assignments, np.full(40, 32, dtype=np.uint64)])
    ix.ids = [list(l) for l in ixb.ids] + [list(range(30000, 30040))]
    ix.num_centroids = 33
    ix._upload()
    ixb.close()
    lens = np.bincount(ix.assignments.astype(np.int64), minlength=33)
    print("FIG onetile: shortest lists", np.sort(lens)[:3])
    assert lens.min() <= 64 and (lens % 64 != 0).any()
    for b in (8, 40):
        Q = home_queries(ix, 0x811, 768, 128, b, 3)
        dead_some(both(ix, Q, 10, 8, tag="b%d" % b), "b%d" % b)
elif CASE == "d300":         # ld 320: the head is clipped to 256 columns, one boundary
    X, ix = dist_c_index(0x821, 20000, 300, 32, 128)
    assert ix.head_state()["cols"] == 256, ix.head_state()
    Q = home_queries(ix, 0x821, 300, 128, 40, 3)
    dead_some(both(ix, Q, 10, 8), "d300")
elif CASE == "d128":         # two steps: no head, one launch
    X, ix = dist_c_index(0x831, 20000, 128, 32, 128)
    st = ix.head_state()
    assert not st["valid"] and st["bytes"] == 0, st
    Q = home_queries(ix, 0x831, 128, 128, 40, 3)
    s1 = both(ix, Q, 10, 8)
    assert s1["last"]["quads_tested"] == 0, s1
elif CASE == "distu":        # no clusters: nothing dies, nothing changes
    X = dg.dist_u(0x841, 20000, 768)
    ix = IVFFlatIndex.build_index(32, 1, 3, X, init_indices=mg.init_draws(0x841, 1, 32, 20000))
    Q = dg.dist_u(0x842, 40, 768)
    s1 = both(ix, Q, 10, 8)
    assert s1["valid"], s1
    print("FIG distu dead", s1["last"])
elif CASE == "mutate":       # add_batch and remove_batch invalidate the head (one launch), compact builds it again
    X, ix = dist_c_index(0x851, 20000, 768, 32, 128)
    Q = home_queries(ix, 0x851, 768, 128, 40, 3)
    dead_some(both(ix, Q, 10, 8, tag="built"), "built")
    ix.add_batch(dg.dist_c(0x852, 700, 768, 128, dg.default_sigma(768), seed_c=0x851 ^ 0xC0FFEE))
    s1 = both(ix, Q, 10, 8, tag="add")
    assert not s1["valid"] and s1["last"]["quads_tested"] == 0, s1
    ix.compact()
    dead_some(both(ix, Q, 10, 8, tag="compact"), "compact")
    ix.remove_batch(np.arange(0, 20000, 3))
    s1 = both(ix, Q, 10, 8, tag="remove")
    assert not s1["valid"] and s1["last"]["quads_tested"] == 0, s1
    ix.compact()
    dead_some(both(ix, Q, 10, 8, tag="compact 2"), "compact 2")
print("DONE", CASE)
'''


def run(case):
    env = dict(os.environ); env["PYTHONPATH"] = ROOT
    r = subprocess.run([sys.executable, "-c", BODY, case], capture_output=True, text=True, env=env, cwd=ROOT, timeout=600)
    print(r.stdout[-4000:])
    assert r.returncode == 0 and ("DONE " + case) in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


@pytest.mark.parametrize("case", ["base", "onetile", "d300", "d128", "distu", "mutate"])
def test_ruling_cold_quads_out_changes_no_bit(case):
    run(case)
