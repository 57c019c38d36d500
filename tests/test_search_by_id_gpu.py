"""vers_ivf_search_by_id / _dev: a search whose queries are stored vectors.  Bit for bit, no tolerance:
  1. flags 0: equal to search_batch(values[ids]) for nprobe 0, 1, 4 and k, top_k 1, 10 and 55 (above the fast domain), b = 1, 33 and 64, through
     the host call and the device-pointer call, on indexes that went through test_recluster_gpu.py's `mutate`;
  2. squared L2 on a built index: the id itself comes first, at distance exactly 0.0;
  3. VERS_BYID_EXCLUDE_SELF: equal, row by row, to the ORACLE's search on the fields with that one id taken out of its list -- on a mutated
     index, on an index made by `upload` with assignments that are NOT the first-minimum centroid (the query's own list is one the probe does
     not reach: nothing of the row is dropped but its last entry), for a query whose list holds only itself, and with top_k at and above the
     rows in reach (the count shrinks by one);
  4. the refusals: the flag with nprobe == 0, an unknown flag bit, an id in no list, an id >= n -- outputs untouched."""
import numpy as np
import pytest

from oracle import c_oracle as co
from tests.test_recluster_gpu import build, mutate
from tests.test_remove_gpu import bits, live_ids
from vers_amd import capi
from vers_amd.capi import _ptr
from vers_amd.index import IVFFlatIndex

pytestmark = pytest.mark.gpu

CASES = ["n200_d7_k40_l2", "n333_d33_k5_cos", "n1500_d130_k10_l2", "n900_d300_k30_cos"]


def by_id_dev(ix, ids, top_k, nprobe, exclude_self=False, flags=None, poll=True):
    import torch
    b = len(ids)
    idd = torch.from_numpy(np.asarray(ids, dtype=np.uint64).view(np.int64).copy()).cuda()
    oi = torch.full((b, max(top_k, 1)), 13, dtype=torch.int64, device="cuda")
    od = torch.full((b, max(top_k, 1)), -2.0, dtype=torch.float32, device="cuda")
    oc = torch.full((b,), 17, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    try:
        ix.search_by_id_dev(idd.data_ptr(), b, top_k, nprobe, oi.data_ptr(), od.data_ptr(), oc.data_ptr(), exclude_self=exclude_self, flags=flags)
        torch.cuda.synchronize()
        if poll:
            ix.poll(0)
    finally:
        torch.cuda.synchronize()
        by_id_dev.last = (oi.cpu().numpy().view(np.uint64)[:, :top_k], od.cpu().numpy()[:, :top_k], oc.cpu().numpy().view(np.uint32))
    return by_id_dev.last


def same(got, want, what):
    assert np.array_equal(got[2], want[2]), (what, "counts", got[2], want[2])
    on = np.arange(got[0].shape[1])[None, :] < got[2][:, None]
    assert np.array_equal(got[0][on], want[0][on]), (what, "ids")
    assert np.array_equal(bits(got[1])[on], bits(want[1])[on]), (what, "distance bits")


@pytest.mark.parametrize("case_id", CASES)
def test_flags_0_is_the_search_with_the_stored_vectors(case_id):
    case, ix = build(case_id)
    live = mutate(case, ix)
    rng = np.random.default_rng(case.seed)
    k = ix.num_centroids
    for b in (1, 33, 64):
        ids = rng.choice(live, b, replace=b > live.size).astype(np.uint64)
        ids[0] = live[-1]                                   # (an added row)
        Q = ix.values[ids.astype(np.int64)]
        for nprobe in sorted({0, 1, 4, k}):
            for top_k in (1, 10, 55):
                want = ix.search_batch(Q, top_k, nprobe)
                same(ix.search_by_id(ids, top_k, nprobe), want, (case_id, "host", b, nprobe, top_k))
                same(by_id_dev(ix, ids, top_k, nprobe), want, (case_id, "dev", b, nprobe, top_k))
    ix.close()


def test_l2_the_id_itself_comes_first_at_distance_zero():
    case, ix = build("n1500_d130_k10_l2")
    ids = np.arange(0, case.n, 23, dtype=np.uint64)
    for got in (ix.search_by_id(ids, 5, 1), by_id_dev(ix, ids, 5, 1), ix.search_by_id(ids, 5, 0)):
        assert (got[2] == 5).all()
        assert np.array_equal(got[0][:, 0], ids) and (bits(got[1][:, 0]) == 0).all()     # exactly +0.0
    ix.close()


def oracle_without(ix, v, top_k, nprobe):
    """the oracle's nprobe search for values[v] on the mirror's fields with v alone taken out of its list"""
    lists = [[x for x in l if x != v] for l in ix.ids]
    return co.search_nprobe(ix.values, ix.centroids, lists, ix.values[v], top_k, nprobe, ix.metric)


def check_exclude(ix, ids, top_k, nprobe, what):
    ids = np.asarray(ids, dtype=np.uint64)
    for name, got in (("host", ix.search_by_id(ids, top_k, nprobe, exclude_self=True)), ("dev", by_id_dev(ix, ids, top_k, nprobe, exclude_self=True))):
        gi, gd, gc = got
        for q, v in enumerate(ids.tolist()):
            oi, od = oracle_without(ix, v, top_k, nprobe)
            assert gc[q] == len(oi), (what, name, q, v, int(gc[q]), len(oi))
            assert np.array_equal(gi[q, :len(oi)], oi) and np.array_equal(bits(gd[q, :len(oi)]), bits(od)), (what, name, q, v)
            assert v not in gi[q, :gc[q]].tolist()


@pytest.mark.parametrize("case_id", CASES)
def test_exclude_self_is_the_search_on_the_index_without_that_id(case_id):
    case, ix = build(case_id)
    live = mutate(case, ix)
    rng = np.random.default_rng(case.seed + 3)
    k = ix.num_centroids
    for b in (1, 33):
        ids = rng.choice(live, b, replace=b > live.size)
        for nprobe in sorted({1, 4, k}):
            for top_k in (1, 10, 55):
                check_exclude(ix, ids, top_k, nprobe, (case_id, b, nprobe, top_k))
    # top_k at and above the rows in reach: the count shrinks by one
    c = int(np.argmax([len(l) for l in ix.ids]))
    v = ix.ids[c][len(ix.ids[c]) // 2]
    for top_k in (len(ix.ids[c]) - 1, len(ix.ids[c]), len(ix.ids[c]) + 5):
        check_exclude(ix, [v], top_k, 1, (case_id, "reach", top_k))
    plain = ix.search_batch(ix.values[v], len(live) + 1, 1)
    reach = int(plain[2][0])
    there = v in plain[0][0, :reach].tolist()       # (the list v lies in is the nearest one unless the build's last centroid update moved it away)
    assert ix.search_by_id([v], reach + 5, 1, exclude_self=True)[2][0] == reach - (1 if there else 0)
    ix.close()


def test_exclude_self_when_the_own_list_is_not_the_nearest_and_when_it_holds_nothing_else():
    case, src = build("n333_d33_k5_l2")
    k, n = case.k, case.n
    # assignments of the caller's choice: every seventh id sits in the list of its FARTHEST centroid
    asg = src.assignments.copy()
    moved = np.arange(3, n, 7)
    d2 = ((src.values[moved, None, :].astype(np.float64) - src.centroids[None, :, :].astype(np.float64)) ** 2).sum(-1)
    asg[moved] = np.argmax(d2, axis=1).astype(np.uint64)
    assert (asg[moved] != src.assignments[moved]).all()
    ix = IVFFlatIndex(case.d, metric=case.metric)
    ix.num_centroids, ix.values, ix.centroids, ix.assignments = k, src.values.copy(), src.centroids.copy(), asg
    ix._upload()
    ix.ids = [np.flatnonzero(asg == c).tolist() for c in range(k)]
    ids = np.concatenate([moved[:20], np.arange(0, 40, 7)])
    for nprobe in (1, 2, k):
        for top_k in (1, 10, 55):
            check_exclude(ix, ids, top_k, nprobe, ("uploaded", nprobe, top_k))
    # with one probe the own list is out of reach: the row is the plain search's, which does not hold the id
    plain = ix.search_by_id(moved[:20], 10, 1)
    assert not (plain[0] == moved[:20, None].astype(np.uint64)).any()
    same(ix.search_by_id(moved[:20], 10, 1, exclude_self=True), plain, "nothing to drop but the last entry")
    # a query whose list holds only itself
    c = int(np.argmin([len(l) if l else n for l in ix.ids]))
    v = ix.ids[c][0]
    others = [x for x in ix.ids[c] if x != v]
    assert ix.remove_batch(others) == len(others) and ix.ids[c] == [v]
    for nprobe in (1, 2, k):
        check_exclude(ix, [v, ids[0]], 10, nprobe, ("alone in its list", nprobe))
    src.close()
    ix.close()


def test_refusals_leave_the_outputs_untouched():
    case, ix = build("n333_d33_k5_l2")
    live = mutate(case, ix)
    n = len(ix.assignments)
    gone = np.setdiff1d(np.arange(n), live)
    ok = live[:9].astype(np.uint64)
    lib = capi.lib()

    def refused(ids, top_k, nprobe, flags):
        ids = np.asarray(ids, dtype=np.uint64)
        oi = np.full((ids.size, top_k), 13, dtype=np.uint64); od = np.full((ids.size, top_k), -2.0, dtype=np.float32); oc = np.full(ids.size, 17, dtype=np.uint32)
        assert lib.vers_ivf_search_by_id(ix._h, _ptr(ids), ids.size, top_k, nprobe, flags, _ptr(oi), _ptr(od), _ptr(oc)) == capi.ERR_INVALID
        assert (oi == 13).all() and (od == -2.0).all() and (oc == 17).all()
        with pytest.raises(capi.VersError) as e:
            by_id_dev(ix, ids, top_k, nprobe, flags=flags)
        assert e.value.status == capi.ERR_INVALID
        gi, gd, gc = by_id_dev.last
        assert (gi == 13).all() and (gd == -2.0).all() and (gc == 17).all()

    refused(ok, 5, 0, capi.BYID_EXCLUDE_SELF)                       # the flag in the reference's mode
    refused(ok, 5, 1, 2)                                            # an unknown flag bit
    refused(ok, 5, 1, capi.BYID_EXCLUDE_SELF | 0x80000000)
    for flags in (0, capi.BYID_EXCLUDE_SELF):
        for bad in (int(gone[0]), int(gone[-1]), n, 1 << 40):       # in no list | at and beyond n
            ids = ok.copy(); ids[4] = bad
            refused(ids, 5, 1, flags)
    ix.poll(0)
    same(ix.search_by_id(ok, 5, 1), ix.search_batch(ix.values[ok.astype(np.int64)], 5, 1), "after the refusals")
    ix.close()
