"""vers_flat_range_search / vers_ivf_range_search_exhaustive (+ _dev): EVERY row -- of the flat corpus, of the index's lists as they are now --
whose distance to the query is <= its radius.  The expected result is the oracle's search_exhaustive over all rows (for the index: stably
filtered to the ids still in a list), cut at dist <= r: ids, order and distance BITS are compared with np.array_equal -- no tolerance.  Every
case checks both orders: the sorted one is the oracle's leading entries, the walk order is ascending vec id (flat) or the lists (get_list) one
after the other (index)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import c_oracle as co
from tests import datagen as dg
from tests.golden import make_golden as mg
from vers_amd import capi
from vers_amd.index import IVFFlatIndex

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = np.float32(np.inf)
L2, COS = capi.METRIC_L2SQ, capi.METRIC_COSDIST


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


class Ref:
    """The oracle's view of (rows, queries, metric), computed ONCE and shared by every radius / order / call shape: per query the full
    exhaustive result over the live rows, ascending (distance, vec id).  live: the ids still in a list (None: every row); lists: the
    walk order as a list of id arrays (None: ascending vec id)."""

    def __init__(self, rows, Q, metric=L2, live=None, lists=None):
        self.Q = np.atleast_2d(Q)
        n = rows.shape[0]
        self.full = []
        for q in self.Q:
            if n == 0:
                oi, od = np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.float32)
            else:
                oi, od = co.search_exhaustive(rows, q, n, metric)
            if live is not None:
                keep = np.isin(oi, live)   # (a boolean mask keeps the order: a stable filter)
                oi, od = oi[keep], od[keep]
            self.full.append((oi, od))
        self.order = (np.sort(np.asarray(live, dtype=np.uint64)) if live is not None else np.arange(n, dtype=np.uint64)) if lists is None \
            else (np.concatenate([np.asarray(l, dtype=np.uint64) for l in lists]) if lists else np.zeros(0, dtype=np.uint64))

    def mth(self, q, m):
        od = self.full[q][1]
        return od[min(m, len(od)) - 1] if len(od) else np.float32(0)

    def sorted(self, q, r):
        oi, od = self.full[q]
        m = int(np.count_nonzero(od <= np.float32(r)))
        assert not np.any(od[m:] <= np.float32(r))   # the result is the LEADING entries
        return oi[:m], od[:m]

    def walk(self, q, r):
        oi, od = self.full[q]
        dist_of = np.full(int(max(self.order.max(initial=0), oi.max(initial=0))) + 1, np.nan, dtype=np.float32)
        dist_of[oi.astype(np.int64)] = od
        dd = dist_of[self.order.astype(np.int64)]
        keep = dd <= np.float32(r)
        return self.order[keep], dd[keep]


def check_result(ref, qs, radii, got_sorted, got_walk, flat_walk):
    for name, got in (("sorted", got_sorted), ("walk", got_walk)):
        lims = got[0]
        assert lims[0] == 0 and lims[-1] == got[1].size == got[2].size and np.all(np.diff(lims.astype(np.int64)) >= 0), name
    for i, q in enumerate(qs):
        r = radii[i]
        si, sd = (a[int(got_sorted[0][i]):int(got_sorted[0][i + 1])] for a in got_sorted[1:])
        wi, wd = (a[int(got_walk[0][i]):int(got_walk[0][i + 1])] for a in got_walk[1:])
        ei, ed = ref.sorted(q, r)
        assert np.array_equal(si, ei) and np.array_equal(bits(sd), bits(ed)), ("sorted", q, float(r), si.size, ei.size)
        xi, xd = ref.walk(q, r)
        assert np.array_equal(wi, xi) and np.array_equal(bits(wd), bits(xd)), ("walk", q, float(r), wi.size, xi.size)
        if flat_walk:   # ascending vec id: a stable sort by distance is the (distance, vec id) order
            o = np.argsort(wd, kind="stable")
            assert np.array_equal(wi[o], si) and np.array_equal(bits(wd[o]), bits(sd)), ("walk re-sorted", q)
        else:
            assert np.array_equal(np.sort(wi), np.sort(si))


def check_range(call, ref, radii, singles=True, flat_walk=True):
    """call(Q, radii, walk_order) -> (lims, ids, dist)"""
    Q = ref.Q
    b = Q.shape[0]
    radii = np.broadcast_to(np.asarray(radii, dtype=np.float32), (b,)).copy()
    got = [call(Q, radii, w) for w in (False, True)]
    check_result(ref, range(b), radii, got[0], got[1], flat_walk)
    if singles:
        for q in sorted({0, b - 1}):
            one = [call(Q[q], radii[q], w) for w in (False, True)]
            check_result(ref, [q], radii[q:q + 1], one[0], one[1], flat_walk)
    return got[0]


def radii_mth(ref, m):
    return np.asarray([ref.mth(q, m) for q in range(ref.Q.shape[0])], dtype=np.float32)


def flat_call(fc, metric=L2):
    return lambda Q, r, w: fc.range_search(Q, r, metric=metric, walk_order=w)


def index_call(ix, metric=L2):
    return lambda Q, r, w: ix.range_search_exhaustive(Q, r, metric=metric, walk_order=w)


def index_ref(ix, Q, metric=L2):
    lists = [ix.get_list(c)[1] for c in range(ix.num_centroids)]
    for c, l in enumerate(lists):
        assert np.array_equal(l, np.asarray(ix.ids[c], dtype=np.uint64)), c
    live = np.concatenate(lists) if lists else np.zeros(0, dtype=np.uint64)
    return Ref(np.asarray(ix.values, dtype=np.float32), Q, metric, live=live, lists=lists)


def make_index(n, d, k, metric=L2, seed=0x7A10, iters=4, X=None):
    if X is None:
        X = dg.dist_c(seed, n, d, 2 * k, dg.default_sigma(d))
    init = mg.init_draws(seed + 1, 1, k, n)
    return IVFFlatIndex.build_index(k, 1, iters, X, init_indices=init, metric=metric)


# ---- 1. / 2. flat: query-group widths, boundary radii, one-tile and multi-tile segments ------------------------------------------------------
@pytest.fixture(scope="module")
def flat_main():
    """n = 3000: 47 segments of 64 rows when "seg_rows" = 64, the last holding 56; n = 1500 with "seg_rows" = 256: five full segments
    and one of 220 rows = 3 tiles + 28 rows.  One reference per (n, b), shared."""
    d = 96
    X = dg.dist_c(0x7B00, 3000, d, 24, dg.default_sigma(d))
    out = {}
    for n in (3000, 1500):
        fc = capi.FlatCorpus(d); fc.upload(X[:n])
        out[n] = (fc, {b: Ref(X[:n], dg.dist_c(0x7B07 + b, b, d, 24, dg.default_sigma(d))) for b in (1, 5, 8, 19)})
    yield out
    for fc, _ in out.values():
        fc.close()


@pytest.mark.parametrize("n,seg_rows", [(3000, 64), (1500, 256)])
@pytest.mark.parametrize("b", [1, 5, 8, 19])
def test_flat_widths_segments_and_boundary_radii(flat_main, b, n, seg_rows):
    fc, refs = flat_main[n]
    ref = refs[b]
    try:
        capi.set_option("seg_rows", seg_rows)
        for m in (1, 10, 300):   # r = the exact distance of the m-th nearest row: <= includes the boundary row
            lims, _, _ = check_range(flat_call(fc), ref, radii_mth(ref, m))
            assert np.all(np.diff(lims.astype(np.int64)) >= m)
        lims, _, _ = check_range(flat_call(fc), ref, -1.0, singles=False)
        assert lims[-1] == 0
        lims, _, _ = check_range(flat_call(fc), ref, INF, singles=False)
        assert np.all(np.diff(lims.astype(np.int64)) == n)
        mixed = np.asarray([(-1.0, INF, ref.mth(q, 10), ref.mth(q, 300))[q % 4] for q in range(b)], dtype=np.float32)
        check_range(flat_call(fc), ref, mixed)
    finally:
        capi.set_option("seg_rows", 0)


# ---- 3. dimensions and tiny corpora ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,n", [(7, 700), (300, 700), (1536, 700), (96, 0), (96, 5), (96, 64), (96, 65)])
def test_flat_dimensions_and_tiny_corpora(d, n):
    X = dg.dist_c(0x7C00 + d + n, max(n, 1), d, 6, dg.default_sigma(d))[:n]
    fc = capi.FlatCorpus(d); fc.upload(X)
    for b in (1, 9):
        ref = Ref(X, dg.dist_c(0x7C07 + d + n + b, b, d, 6, dg.default_sigma(d)))
        for m in (1, 10, 300):
            lims, _, _ = check_range(flat_call(fc), ref, radii_mth(ref, m), singles=m == 10)
            assert np.all(np.diff(lims.astype(np.int64)) >= min(m, n))
        lims, _, _ = check_range(flat_call(fc), ref, INF, singles=False)
        assert np.all(lims == np.arange(b + 1, dtype=np.uint64) * np.uint64(n))
    fc.close()


# ---- 4. ties ---------------------------------------------------------------------------------------------------------------------------------
def test_equal_distances_come_out_in_ascending_vec_id():
    d, m = 24, 400
    h = dg.mix64(np.arange(m * d, dtype=np.uint64) + np.uint64(0x7D00)).reshape(m, d)
    base = (h % np.uint64(7)).astype(np.float32) - np.float32(3.0)   # small integers: every distance is exact
    assert np.unique(base, axis=0).shape[0] == m
    X = np.tile(base, (3, 1))   # ids i, i + 400, i + 800 are the same vector
    Q = np.stack([base[5], base[17] + np.float32(1.0), np.zeros(d, dtype=np.float32)])
    fc = capi.FlatCorpus(d); fc.upload(X)
    ref = Ref(X, Q)
    radii = radii_mth(ref, 31)   # a distance three rows share at least
    _, od = ref.full[0]
    assert np.count_nonzero(bits(od)[1:] == bits(od)[:-1]) >= 2 * m
    lims, ids, dist = check_range(flat_call(fc), ref, radii)
    for q in range(3):
        i, dd = ids[int(lims[q]):int(lims[q + 1])], dist[int(lims[q]):int(lims[q + 1])]
        assert i.size >= 31 and i.size % 3 == 0   # the radius is a tied distance: all three copies of the boundary row are in
        same = bits(dd)[1:] == bits(dd)[:-1]
        assert np.all(i[1:][same] > i[:-1][same])
    check_range(flat_call(fc), ref, INF, singles=False)
    ix = IVFFlatIndex.build_index(4, 1, 3, X, init_indices=np.asarray([0, 100, 200, 300], dtype=np.uint64))
    check_range(index_call(ix), index_ref(ix, Q), radii, flat_walk=False)
    ix.close()
    fc.close()


# ---- 5. cosine distance, both handles --------------------------------------------------------------------------------------------------------
def test_cosine_distance_both_handles():
    n, d, k = 3000, 96, 8
    X = dg.dist_c(0x7E00, n, d, 2 * k, dg.default_sigma(d))   # (rows and queries are normalised)
    fc = capi.FlatCorpus(d); fc.upload(X)
    ix = make_index(n, d, k, metric=COS, seed=0x7E00, X=X)
    for b in (1, 9):
        Q = dg.dist_c(0x7E07 + b, b, d, 2 * k, dg.default_sigma(d))
        ref = Ref(X, Q, COS)
        iref = index_ref(ix, Q, COS)
        for m in (1, 10, 300):
            check_range(flat_call(fc, COS), ref, radii_mth(ref, m))
            check_range(index_call(ix, COS), iref, radii_mth(iref, m), flat_walk=False)
    ix.close()
    fc.close()


# ---- 6. the index, mutated -------------------------------------------------------------------------------------------------------------------
def test_index_mutated():
    n, d, k, b = 6000, 96, 12, 8
    ix = make_index(n, d, k)
    Q = dg.dist_c(0x7F07, b, d, 2 * k, dg.default_sigma(d))

    def check_now(seg_rows=0):
        ref = index_ref(ix, Q)
        try:
            capi.set_option("seg_rows", seg_rows)
            for radii in (radii_mth(ref, 10), radii_mth(ref, 300)):
                lims, ids, _ = check_range(index_call(ix), ref, radii, flat_walk=False)
                al, ai, _ = ix.range_search(Q, radii, k)   # every list probed: the same SET
                for q in range(b):
                    assert np.array_equal(np.sort(ids[int(lims[q]):int(lims[q + 1])]), np.sort(ai[int(al[q]):int(al[q + 1])])), q
            mixed = np.asarray([(INF, -1.0)[q % 2] for q in range(b)], dtype=np.float32)
            lims, _, _ = check_range(index_call(ix), ref, mixed, singles=False, flat_walk=False)
            assert np.all(np.diff(lims.astype(np.int64))[0::2] == ix.live_count()) and np.all(np.diff(lims.astype(np.int64))[1::2] == 0)
        finally:
            capi.set_option("seg_rows", 0)

    check_now()
    check_now(seg_rows=64)
    ix.add_batch(dg.dist_c(0x7F20, 500, d, 2 * k, dg.default_sigma(d)))
    check_now()
    lens = [len(l) for l in ix.ids]
    c = int(np.argmin(lens))
    assert 0 < lens[c] < 1000
    whole = set(int(v) for v in ix.ids[c])
    others = [v for v in range(0, n, 5) if v not in whole][:1000 - len(whole)]
    ix.remove_batch(sorted(whole | set(others)))
    assert len(ix.ids[c]) == 0 and ix.live_count() == n + 500 - 1000
    check_now()
    check_now(seg_rows=256)
    before, after = ix.compact()
    assert after <= before
    check_now()
    ix.close()


# ---- 7. the protocol -------------------------------------------------------------------------------------------------------------------------
def raw_call(fn, h, d, Q, radii, metric, flags, cap, ids=None, dist=None):
    Q = np.ascontiguousarray(np.atleast_2d(Q), dtype=np.float32)
    b = Q.shape[0]
    r = np.ascontiguousarray(np.broadcast_to(np.asarray(radii, dtype=np.float32), (b,)))
    lims = np.full(b + 1, 0xABABABABABABABAB, dtype=np.uint64)
    total = C.c_uint64(12345)
    rc = fn(h, capi._ptr(Q), 4 * d, b, capi._ptr(r), metric, flags, capi._ptr(lims), capi._ptr(ids) if ids is not None else None,
            capi._ptr(dist) if dist is not None else None, cap, C.byref(total))
    return rc, lims, int(total.value)


@pytest.fixture(scope="module")
def proto():
    n, d, k = 3000, 96, 8
    X = dg.dist_c(0x8000, n, d, 2 * k, dg.default_sigma(d))
    fc = capi.FlatCorpus(d); fc.upload(X)
    ix = make_index(n, d, k, seed=0x8000, X=X)
    yield X, fc, ix
    ix.close()
    fc.close()


@pytest.mark.parametrize("which", ["flat", "ivf"])
def test_capacity_protocol_and_errors(proto, which):
    X, fc, ix = proto
    d = X.shape[1]
    L = capi.lib()
    fn, fn_dev, h = (L.vers_flat_range_search, L.vers_flat_range_search_dev, fc._h) if which == "flat" else \
        (L.vers_ivf_range_search_exhaustive, L.vers_ivf_range_search_exhaustive_dev, ix._h)
    Q = dg.dist_c(0x8007, 8, d, 16, dg.default_sigma(d))
    ref = Ref(X, Q) if which == "flat" else index_ref(ix, Q)
    radii = radii_mth(ref, 10)
    want = check_range(flat_call(fc) if which == "flat" else index_call(ix), ref, radii, singles=False, flat_walk=which == "flat")
    total = int(want[0][-1])
    assert total >= 80
    call = lambda Qx, rx, metric, flags, cap, ids=None, dist=None: raw_call(fn, h, d, Qx, rx, metric, flags, cap, ids, dist)
    # the size query: cap == 0 with NULL arrays
    rc, lims, got = call(Q, radii, L2, 0, 0)
    assert rc == capi.OK and got == total and np.array_equal(lims, want[0])
    # one short: VERS_OK, the total, complete limits, ids / distances untouched
    ids = np.full(total, 0xCDCDCDCDCDCDCDCD, dtype=np.uint64); dist = np.full(total, -7.25, dtype=np.float32)
    rc, lims, got = call(Q, radii, L2, 0, total - 1, ids, dist)
    assert rc == capi.OK and got == total and np.array_equal(lims, want[0])
    assert np.all(ids == 0xCDCDCDCDCDCDCDCD) and np.all(dist == np.float32(-7.25))
    # exactly enough
    rc, lims, got = call(Q, radii, L2, 0, total, ids, dist)
    assert rc == capi.OK and got == total and np.array_equal(ids, want[1]) and np.array_equal(bits(dist), bits(want[2]))
    # b == 0: *out_total = 0
    t = C.c_uint64(99)
    assert fn(h, None, 4 * d, 0, None, L2, 0, None, None, None, 0, C.byref(t)) == capi.OK and t.value == 0
    t = C.c_uint64(99)
    assert fn_dev(h, None, d, 0, None, L2, 0, None, None, None, 0, C.byref(t), None) == capi.OK and t.value == 0
    # argument errors
    bad = radii.copy(); bad[3] = np.nan
    assert call(Q, bad, L2, 0, 0)[0] == capi.ERR_INVALID
    assert call(Q, radii, L2, 2, 0)[0] == capi.ERR_INVALID     # an unknown flag bit
    assert call(Q, radii, 2, 0, 0)[0] == capi.ERR_INVALID      # an unknown metric
    assert call(Q, radii, L2, 0, 5)[0] == capi.ERR_INVALID     # a capacity without arrays
    # a NaN query: VERS_ERR_NAN, outputs untouched, and the next call succeeds
    Qn = Q.copy(); Qn[2, 5] = np.nan
    ids[:] = 0xCDCDCDCDCDCDCDCD; dist[:] = -7.25
    rc, _, _ = call(Qn, INF, L2, 0, total, ids, dist)
    assert rc == capi.ERR_NAN and np.all(ids == 0xCDCDCDCDCDCDCDCD) and np.all(dist == np.float32(-7.25))
    rc, lims, got = call(Q, radii, L2, 0, total, ids, dist)
    assert rc == capi.OK and got == total and np.array_equal(lims, want[0]) and np.array_equal(ids, want[1])
    # a NaN radius in device memory is found there
    import torch
    dev = torch.device("cuda", 0)
    qd = torch.from_numpy(Q).to(dev); rd = torch.from_numpy(bad).to(dev)
    ld = torch.zeros(9, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    t = C.c_uint64(0)
    assert fn_dev(h, C.c_void_p(qd.data_ptr()), d, 8, C.c_void_p(rd.data_ptr()), L2, 0, C.c_void_p(ld.data_ptr()), None, None, 0, C.byref(t), None) == capi.ERR_INVALID


def test_empty_and_sharded_handles(proto):
    X, _, ix = proto
    d = X.shape[1]
    L = capi.lib()
    Q = dg.dist_c(0x8017, 3, d, 16, dg.default_sigma(d))
    # an empty flat corpus, an index without centroids: OK, total 0, every limit 0
    fe = capi.FlatCorpus(d); fe.upload(X[:0])
    rc, lims, got = raw_call(L.vers_flat_range_search, fe._h, d, Q, INF, L2, 0, 0)
    assert rc == capi.OK and got == 0 and np.all(lims == 0)
    fe.close()
    empty = IVFFlatIndex(d)
    rc, lims, got = raw_call(L.vers_ivf_range_search_exhaustive, empty._h, d, Q, INF, L2, 0, 0)
    assert rc == capi.OK and got == 0 and np.all(lims == 0)
    empty.close()
    # a handle sharded by cluster
    half = IVFFlatIndex(d)
    half.set_shard(0, 2)   # (before the upload: this handle stores the lists of rank 0 of 2)
    half.num_centroids, half.values, half.centroids, half.assignments = ix.num_centroids, ix.values, ix.centroids, ix.assignments
    half._upload()
    assert raw_call(L.vers_ivf_range_search_exhaustive, half._h, d, Q, INF, L2, 0, 0)[0] == capi.ERR_INVALID
    half.close()


# ---- 8. the neighbours are unchanged ---------------------------------------------------------------------------------------------------------
def test_neighbours_unchanged_around_an_exhaustive_range_call(proto):
    X, fc, ix = proto
    d = X.shape[1]
    Q = dg.dist_c(0x8027, 9, d, 16, dg.default_sigma(d))
    ref = Ref(X, Q)
    radii = radii_mth(ref, 10)

    def neighbours():
        out = [fc.search(Q, 10), fc.search(Q[0], 100), ix.search_exhaustive(Q, 10), ix.search_exhaustive(Q[0], 100)]
        flat = [a for (i, dd, c) in out for a in (i, bits(dd), c)]
        for w in (False, True):
            l, i, dd = ix.range_search(Q, radii, 4, walk_order=w)
            flat += [l, i, bits(dd)]
        return flat

    before = neighbours()
    check_range(flat_call(fc), ref, radii)
    check_range(index_call(ix), index_ref(ix, Q), radii, flat_walk=False)
    after = neighbours()
    assert len(before) == len(after) and all(np.array_equal(x, y) for x, y in zip(before, after))


# ---- 9. device pointers, two streams ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["flat", "ivf"])
def test_device_pointer_call_on_two_streams(proto, which):
    import torch
    X, fc, ix = proto
    d, b = X.shape[1], 8
    Q = dg.dist_c(0x8037, b, d, 16, dg.default_sigma(d))
    ref = Ref(X, Q)
    radii = radii_mth(ref, 10)
    host = flat_call(fc) if which == "flat" else index_call(ix)
    call_dev = fc.range_search_dev if which == "flat" else ix.range_search_exhaustive_dev
    want = [host(Q, radii, w) for w in (False, True)]
    total = int(want[0][0][-1])
    dev = torch.device("cuda", 0)
    qd = torch.from_numpy(Q).to(dev)
    rd = torch.from_numpy(radii).to(dev)
    streams = (torch.cuda.Stream(dev), torch.cuda.Stream(dev))
    outs = []
    torch.cuda.synchronize(dev)
    for w, flags in ((0, 0), (1, capi.RANGE_WALK_ORDER)):   # back to back, alternating streams
        for stream in streams:
            lims = torch.zeros(b + 1, dtype=torch.int64, device=dev)
            ids = torch.full((total,), -1, dtype=torch.int64, device=dev)
            dist = torch.full((total,), -7.25, dtype=torch.float32, device=dev)
            torch.cuda.synchronize(dev)
            assert call_dev(qd.data_ptr(), d, b, rd.data_ptr(), L2, flags, lims.data_ptr(), 0, 0, 0, stream.cuda_stream) == total
            assert call_dev(qd.data_ptr(), d, b, rd.data_ptr(), L2, flags, lims.data_ptr(), ids.data_ptr(), dist.data_ptr(), total - 1,
                            stream.cuda_stream) == total
            assert bool((ids == -1).all()) and bool((dist == -7.25).all())
            assert call_dev(qd.data_ptr(), d, b, rd.data_ptr(), L2, flags, lims.data_ptr(), ids.data_ptr(), dist.data_ptr(), total,
                            stream.cuda_stream) == total
            outs.append((w, lims, ids, dist))
    for w, lims, ids, dist in outs:
        assert np.array_equal(lims.cpu().numpy().astype(np.uint64), want[w][0])
        assert np.array_equal(ids.cpu().numpy().astype(np.uint64), want[w][1])
        assert np.array_equal(bits(dist.cpu().numpy()), bits(want[w][2]))


# ---- 10. the phases hook ---------------------------------------------------------------------------------------------------------------------
def test_phases_hook_counts_the_exhaustive_calls(proto):
    X, fc, ix = proto
    d = X.shape[1]
    Q = dg.dist_c(0x8047, 8, d, 16, dg.default_sigma(d))
    ref = Ref(X, Q)
    radii = radii_mth(ref, 10)
    fc.range_search(Q, radii); ix.range_search_exhaustive(Q, radii)   # (sizes the bindings' capacity: the next calls are ONE call each)
    capi.range_phases(reset=True)
    assert all(v == 0 for v in capi.range_phases().values())
    l0, _, _ = fc.range_search(Q, radii)
    ph = capi.range_phases()
    assert (ph["calls"], ph["queries"], ph["results"]) == (1, 8, int(l0[-1]))
    assert ph["count_ms"] > 0 and ph["fill_ms"] > 0 and ph["sort_ms"] > 0 and ph["plan_ms"] > 0 and ph["scan_ms"] > 0
    l1, _, _ = ix.range_search_exhaustive(Q[:3], radii[:3], walk_order=True)
    ph = capi.range_phases(reset=True)
    assert (ph["calls"], ph["queries"], ph["results"]) == (2, 11, int(l0[-1]) + int(l1[-1]))
    assert all(v == 0 for v in capi.range_phases().values())


# ---- 11. the C++ mirror ----------------------------------------------------------------------------------------------------------------------
def test_cpp_host_mirror_range_search_exhaustive(tmp_path):
    """vers_amd/host/ivfflat.hpp's range_search_exhaustive() from compiled code (tests/cpp/range_exhaustive_demo.cpp) against the Python
    mirror's result"""
    lib = capi.LIB_PATH
    exe = str(tmp_path / "range_exhaustive_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + ROOT, "-o", exe, os.path.join(ROOT, "tests", "cpp", "range_exhaustive_demo.cpp"),
                           "-L" + os.path.dirname(lib), "-lvers_hip", "-Wl,-rpath," + os.path.dirname(lib)])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.rstrip().endswith("DONE"), out.stdout[-2000:] + out.stderr
    i, j = np.meshgrid(np.arange(900), np.arange(40), indexing="ij")
    X = (((i * 7 + j * 13) % 31).astype(np.float32) * np.float32(0.25) + (i % 6).astype(np.float32)).astype(np.float32)
    ix = IVFFlatIndex.build_index(6, 1, 5, X, init_indices=np.asarray([3, 90, 200, 333, 480, 899], dtype=np.uint64))
    got = {}
    for line in out.stdout.splitlines()[:-1]:
        q, w, vid, db = (int(t) for t in line.split())
        got.setdefault((q, w), []).append((vid, db))
    n_rows = 0
    for q in range(6):
        for w in (0, 1):
            lims, ids, dist = ix.range_search_exhaustive(X[q * 31], (0.0, 150.0, 400.0)[q % 3], walk_order=bool(w))
            assert got.get((q, w), []) == list(zip(ids.tolist(), bits(dist).tolist())), (q, w)
            n_rows += ids.size
    assert n_rows > 12   # (the radii select something: every query is a stored row)
    ix.close()
