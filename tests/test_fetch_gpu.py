"""vers_ivf_fetch / vers_ivf_fetch_dev: the stored vector, its list and whether it is still there, by vec id.  Every index goes through
test_recluster_gpu.py's `mutate` first -- a scattered removal with id 0 and id n - 1, a whole list removed, an add_batch of 65 rows, an
update_batch with movers, NO compact -- and everything is compared bit for bit with the IVFFlatIndex mirror: rows == values[v], clusters ==
assignments[v], status from list membership; an id in no list gives a row of zeros, UINT64_MAX and 2.
  1. all ids ascending, descending, a permutation with repeats, n = 1 / 64 / 65, through the host call and through the device-pointer call
     (whose rows have a pitch above d: the padding keeps its sentinel), under the default options, "memory" = 1 and "rowmajor" = 0 (the tile
     gather: with the threshold forced to 1 and to 1000 too, and without the id map), and after the slack was poisoned with NaN and 1e30;
  2. a batch larger than one staging chunk; each nullable output as NULL;
  3. the refusals: an id == n, an id far beyond, during a streamed upload, on a set_shard handle -- outputs untouched, the index searchable;
  4. the staleness protocol: a second fetch refreshes nothing, ids added into slack are found, removed ones are not."""
import ctypes as C

import numpy as np
import pytest

from tests import mutation_model as mm
from tests.test_recluster_gpu import METRICS, SHAPES, build, mutate
from tests.test_remove_gpu import bits, check_search, check_state, live_ids
from vers_amd import capi, testhooks
from vers_amd.capi import _ptr
from vers_amd.index import IVFFlatIndex

pytestmark = pytest.mark.gpu

GUARD = np.float32(-7.0)
CASE_IDS = [f"{s}_{m}" for s in SHAPES for m in METRICS]


def round_up(x, m):
    return (x + m - 1) // m * m


def expected(ix, ids):
    ids = np.asarray(ids, dtype=np.int64)
    n = len(ix.assignments)
    in_list = np.zeros(n, dtype=bool)
    in_list[live_ids(ix)] = True
    ok = in_list[ids]
    rows = np.where(ok[:, None], ix.values[ids], np.float32(0.0)).astype(np.float32)
    cl = np.where(ok, ix.assignments[ids], np.uint64(capi.NO_CLUSTER)).astype(np.uint64)
    st = np.where(ok, 0, 2).astype(np.uint8)
    return rows, cl, st


def fetch_dev(ix, ids, pad=3, rows=True, clusters=True, status=True):
    """the device-pointer call on sentinel-filled outputs -> (rows [n, ld], clusters, status, counts)"""
    import torch
    n, ld = len(ids), round_up(ix.d + pad, 4)
    idd = torch.from_numpy(np.asarray(ids, dtype=np.uint64).view(np.int64).copy()).cuda()
    R = torch.full((max(n, 1), ld), float(GUARD), dtype=torch.float32, device="cuda")
    Cl = torch.full((max(n, 1),), 9, dtype=torch.int64, device="cuda")
    St = torch.full((max(n, 1),), 5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    try:
        counts = ix.fetch_dev(idd.data_ptr(), n, R.data_ptr() if rows else 0, ld, Cl.data_ptr() if clusters else 0, St.data_ptr() if status else 0)
    finally:
        torch.cuda.synchronize()
        fetch_dev.last = (R.cpu().numpy()[:n], Cl.cpu().numpy().view(np.uint64)[:n], St.cpu().numpy()[:n])
    return fetch_dev.last + (counts,)


def check_ids(ix, ids, what):
    ids = np.asarray(ids, dtype=np.uint64)
    wr, wc, ws = expected(ix, ids)
    counts = (int((ws == 0).sum()), int((ws == 2).sum()))
    rows, cl, st = ix.fetch(ids, row_stride_floats=ix.d + 2, fill=GUARD)
    assert np.array_equal(bits(rows[:, :ix.d]), bits(wr)), (what, "host rows")
    assert (rows[:, ix.d:] == GUARD).all(), (what, "host padding")
    assert np.array_equal(cl, wc) and np.array_equal(st, ws) and ix.last_fetch_counts == counts, (what, "host clusters / status / counts")
    rows, cl, st, got = fetch_dev(ix, ids)
    assert np.array_equal(bits(rows[:, :ix.d]), bits(wr)), (what, "dev rows")
    assert (rows[:, ix.d:] == GUARD).all(), (what, "dev padding")
    assert np.array_equal(cl, wc) and np.array_equal(st, ws) and got == counts, (what, "dev clusters / status / counts")
    assert not np.isnan(rows[:, :ix.d]).any() and not (rows[:, :ix.d] == np.float32(1e30)).any(), (what, "slack reached the output")


def id_sets(ix, seed):
    n = len(ix.assignments)
    rng = np.random.default_rng(seed)
    asc = np.arange(n, dtype=np.uint64)
    yield "ascending", asc
    yield "descending", asc[::-1].copy()
    yield "permutation with repeats", rng.integers(0, n, size=n + 37).astype(np.uint64)
    for m in (1, 64, 65):
        yield f"n = {m}", rng.integers(0, n, size=m).astype(np.uint64)


def all_checks(ix, seed, what):
    for name, ids in id_sets(ix, seed):
        check_ids(ix, ids, (what, name))


OPTION_SETS = {
    "defaults": [],
    "memory1": [("memory", 1, 0)],
    "rowmajor0": [("rowmajor", 0, -1)],
}


@pytest.mark.parametrize("case_id", CASE_IDS)
def test_fetch_returns_the_mirror(case_id):
    for name, opts in OPTION_SETS.items():
        for opt, value, _ in opts:
            capi.set_option(opt, value)
        try:
            case, ix = build(case_id)
            mutate(case, ix)
            gone = np.setdiff1d(np.arange(len(ix.assignments)), live_ids(ix))
            assert gone.size and 0 in gone and case.n - 1 in gone
            if name != "defaults":
                assert ix.layout_bytes()["rowmajor"] == 0, name   # the rows come from the f32 tiles
            all_checks(ix, case.seed, name)
            r, c, s = expected(ix, gone)
            assert not r.any() and (c == capi.NO_CLUSTER).all() and (s == 2).all()
            if name == "rowmajor0":     # both forms of the tile gather, and the per-call table in the map's place
                perm = np.random.default_rng(case.seed + 1).integers(0, len(ix.assignments), size=len(ix.assignments) + 11).astype(np.uint64)
                for opt, value, default in (("fetch_lds_min", 1, 64), ("fetch_lds_min", 1000, 64), ("fetch_map", 0, 1)):
                    capi.set_option(opt, value)
                    try:
                        check_ids(ix, perm, (name, opt, value))
                    finally:
                        capi.set_option(opt, default)
            for poison in (float("nan"), 1e30):
                testhooks.poison_slack(ix, poison)
                check_ids(ix, np.arange(len(ix.assignments), dtype=np.uint64), (name, "poisoned slack", poison))
            ix.close()
        finally:
            for opt, _, default in opts:
                capi.set_option(opt, default)


def test_a_batch_larger_than_one_staging_chunk_and_the_nullable_outputs():
    case, ix = build("n1500_d130_k10_l2")
    mutate(case, ix)
    n = len(ix.assignments)
    ids = np.random.default_rng(5).integers(0, n, size=n + 3).astype(np.uint64)
    wr, wc, ws = expected(ix, ids)
    capi.set_option("add_batch_rows", 64)
    capi.set_option("remove_batch_ids", 7)
    try:
        check_ids(ix, ids, "chunks of 64")
        rows, cl, st = ix.fetch(ids[:100], want_rows=False)      # the membership query, chunks of 7 ids
        assert rows is None and np.array_equal(cl, wc[:100]) and np.array_equal(st, ws[:100])
    finally:
        capi.set_option("add_batch_rows", 131072)
        capi.set_option("remove_batch_ids", 1 << 20)
    lib = capi.lib()
    for want_rows, want_cl, want_st in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)):     # the host call, every output alone and none at all
        rows = np.full((ids.size, ix.d), GUARD, dtype=np.float32)
        cl = np.full(ids.size, 9, dtype=np.uint64); st = np.full(ids.size, 5, dtype=np.uint8)
        counts = np.zeros(2, dtype=np.uint64)
        capi.check(lib.vers_ivf_fetch(ix._h, _ptr(ids), ids.size, _ptr(rows) if want_rows else None, 4 * ix.d, _ptr(cl) if want_cl else None,
                                      _ptr(st) if want_st else None, counts.ctypes.data_as(C.POINTER(C.c_uint64))))
        assert np.array_equal(bits(rows), bits(wr)) if want_rows else (rows == GUARD).all()
        assert np.array_equal(cl, wc) if want_cl else (cl == 9).all()
        assert np.array_equal(st, ws) if want_st else (st == 5).all()
        assert counts.tolist() == [int((ws == 0).sum()), int((ws == 2).sum())]
        r, c, s, got = fetch_dev(ix, ids, rows=bool(want_rows), clusters=bool(want_cl), status=bool(want_st))
        assert np.array_equal(bits(r[:, :ix.d]), bits(wr)) if want_rows else (r == GUARD).all()
        assert np.array_equal(c, wc) if want_cl else (c == 9).all()
        assert np.array_equal(s, ws) if want_st else (s == 5).all()
        assert got == (int((ws == 0).sum()), int((ws == 2).sum()))
    capi.check(lib.vers_ivf_fetch(ix._h, _ptr(ids), ids.size, None, 0, None, None, None))   # (no counts either)
    counts = np.full(2, 7, dtype=np.uint64)
    capi.check(lib.vers_ivf_fetch(ix._h, None, 0, None, 0, None, None, counts.ctypes.data_as(C.POINTER(C.c_uint64))))    # n == 0: counts 0
    assert counts.tolist() == [0, 0]
    ix.close()


def refused(ix, ids, status):
    """both calls refuse with `status` and write nothing"""
    ids = np.asarray(ids, dtype=np.uint64)
    rows = np.full((ids.size, ix.d), GUARD, dtype=np.float32)
    cl = np.full(ids.size, 9, dtype=np.uint64); st = np.full(ids.size, 5, dtype=np.uint8)
    counts = np.full(2, 11, dtype=np.uint64)
    rc = capi.lib().vers_ivf_fetch(ix._h, _ptr(ids), ids.size, _ptr(rows), 4 * ix.d, _ptr(cl), _ptr(st), counts.ctypes.data_as(C.POINTER(C.c_uint64)))
    assert rc == status, (rc, status)
    assert (rows == GUARD).all() and (cl == 9).all() and (st == 5).all() and (counts == 11).all()
    with pytest.raises(capi.VersError) as e:
        fetch_dev(ix, ids)
    assert e.value.status == status
    r, c, s = fetch_dev.last
    assert (r == GUARD).all() and (c == 9).all() and (s == 5).all()


@pytest.mark.parametrize("case_id", ["n333_d33_k5_l2", "n1500_d130_k10_cos"])
def test_refusals_leave_the_outputs_untouched_and_the_index_searchable(case_id):
    case, ix = build(case_id)
    mutate(case, ix)
    n = len(ix.assignments)
    phases = capi.fetch_phases(reset=True)
    some = np.arange(0, n, 3, dtype=np.uint64)
    for bad in (n, n + 1, 1 << 40, (1 << 64) - 1):
        ids = some.copy()
        ids[ids.size // 2] = bad          # in the middle of the batch: the ids in front of it are not answered either
        refused(ix, ids, capi.ERR_INVALID)
        refused(ix, np.asarray([bad], dtype=np.uint64), capi.ERR_INVALID)
    assert all(v == 0.0 for v in capi.fetch_phases().values()), "a refused call counts nowhere"
    check_state(ix)
    check_search(ix, mm.fixed_queries(case), top_ks=(1, 10), exhaustive=False)
    check_ids(ix, some, "after the refusals")
    # a streamed upload in progress: no index until upload_end
    t = IVFFlatIndex(ix.d, metric=ix.metric)
    lens = np.bincount(ix.assignments.astype(np.int64), minlength=ix.num_centroids).astype(np.uint64)
    t.upload_begin(ix.centroids, lens, n)
    refused(t, some, capi.ERR_EMPTY)
    t.close()
    # an empty handle
    t = IVFFlatIndex(ix.d, metric=ix.metric)
    refused(t, np.zeros(1, dtype=np.uint64), capi.ERR_EMPTY)
    t.close()
    # a handle sharded by cluster
    t = IVFFlatIndex(ix.d, metric=ix.metric)
    t.set_shard(0, 2)
    t.num_centroids, t.values, t.centroids, t.assignments = ix.num_centroids, ix.values.copy(), ix.centroids.copy(), ix.assignments.copy()
    t._upload()
    refused(t, some, capi.ERR_INVALID)
    t.close()
    ix.close()


def test_the_staleness_protocol():
    case, ix = build("n1500_d130_k10_l2")
    mutate(case, ix)
    n = len(ix.assignments)
    every = lambda: np.arange(len(ix.assignments), dtype=np.uint64)
    capi.fetch_phases(reset=True)
    check_ids(ix, every(), "first")
    assert capi.fetch_phases(reset=True)["map_ms"] > 0.0          # the map was built
    check_ids(ix, every(), "second")
    ph = capi.fetch_phases(reset=True)
    assert ph["map_ms"] == 0.0 and ph["calls"] == 2.0 and ph["ids"] == 2.0 * n, ph     # ... and was valid as it was
    # an update in which every row stays changes values, not places: still no refresh, the new values come back
    live = live_ids(ix)
    pick = live[:20]
    _, st = ix.update_batch(pick, (ix.values[pick] * np.float32(1.0001)).astype(np.float32))
    if (st == 0).all():
        check_ids(ix, every(), "after an update in place")
        assert capi.fetch_phases(reset=True)["map_ms"] == 0.0
    # rows added into slack: the new ids are found
    _, vids = ix.add_batch((ix.values[live[:5]] * np.float32(0.99)).astype(np.float32))
    rows, cl, st = ix.fetch(vids)
    assert (st == 0).all() and np.array_equal(bits(rows), bits(ix.values[vids.astype(np.int64)]))
    check_ids(ix, every(), "after add_batch")
    # removed ids are not
    gone = np.concatenate([vids[:2], live[5:9].astype(np.uint64)])
    assert ix.remove_batch(gone) == gone.size
    rows, cl, st = ix.fetch(gone)
    assert (st == 2).all() and (cl == capi.NO_CLUSTER).all() and not rows.any()
    check_ids(ix, every(), "after remove_batch")
    # compact and recluster move everything
    ix.compact()
    check_ids(ix, every(), "after compact")
    ix.recluster(case.k + 1, 1, 2, init_indices=np.arange(case.k + 1))
    check_ids(ix, every(), "after recluster")
    check_state(ix)
    ix.close()
