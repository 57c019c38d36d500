"""vers_ivf_range_search_filtered / vers_ivf_range_search_exhaustive_filtered (+ _dev): every ALLOWED vector within a radius.  A filter is a
VIRTUAL REMOVAL, so the expected values come from the oracle as it stands --
  probed             co.search_nprobe over ids_f[c] = [v for v in ix.ids[c] if allowed[v]] with top_k = every allowed row, cut at dist <= r;
  exhaustive         co.search_exhaustive over the allowed live rows in ascending id, mapped back, cut at r;
  probed walk order  the probed lists (get_list) in probe-rank order, ascending position, kept iff allowed and within r;
  exhaustive walk    get_list(0), (1), ... concatenated and kept the same way
-- and every comparison is np.array_equal on the limits, the ids and the distances' u32 BITS: no tolerance.  The oracle's full order is
computed once per (index, queries, filter, nprobe / metric) and cut to each radius."""
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
L2, COS = capi.METRIC_L2SQ, capi.METRIC_COSDIST
INF = np.float32(np.inf)
WALK = capi.RANGE_WALK_ORDER


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def make(n, d, k, metric=L2, seed=0xFA70, iters=4):
    X = dg.dist_c(seed, n, d, 2 * k, dg.default_sigma(d))
    init = mg.init_draws(seed + 1, 1, k, n)
    return IVFFlatIndex.build_index(k, 1, iters, X, init_indices=init, metric=metric)


def queries(ix, seed, b):
    d, k = ix.d, ix.num_centroids
    return dg.dist_c(seed, b, d, 2 * k, dg.default_sigma(d))


def clone(ix):
    """a second device handle uploaded from the same fields"""
    c = IVFFlatIndex(ix.d, ix.device, ix.metric)
    c.num_centroids, c.values, c.centroids, c.assignments = ix.num_centroids, ix.values.copy(), ix.centroids, ix.assignments
    c.ids = [list(l) for l in ix.ids]
    c._upload()
    return c


def allowed_set(n, allowed, n_bits=None):
    """The defined semantics, restated: bool [n], entry v = vec id v is allowed.  allowed: a bool array or an id array; n_bits as
    IVFFlatIndex.range_search_filtered defaults it."""
    a = np.asarray(allowed)
    if n_bits is None:
        n_bits = a.size if a.dtype == np.bool_ else (int(a.max()) + 1 if a.size else 0)
    ids = np.flatnonzero(a) if a.dtype == np.bool_ else a.astype(np.int64)
    out = np.zeros(n, dtype=bool)
    ids = ids[(ids < n_bits) & (ids < n)]
    out[ids] = True
    return out


def random_filter(n, sel, seed):
    return np.random.default_rng(seed).random(n) < sel


class Ref:
    """The oracle's view of (index, queries, filter), computed once and shared by every radius / order / call shape: the full filtered order
    per query (per nprobe, exhaustive per metric) and the device's lists."""

    def __init__(self, ix, Q, sem):
        self.ix, self.Q = ix, np.atleast_2d(Q)
        self.sem = np.zeros(max(len(sem), ix.values.shape[0]), dtype=bool)
        self.sem[:len(sem)] = np.asarray(sem, dtype=bool)
        self.ids_f = [[v for v in l if self.sem[v]] for l in ix.ids]
        self.rows = np.asarray(sorted(v for l in self.ids_f for v in l), dtype=np.int64)
        self._p, self._x, self._rank, self._lists = {}, {}, {}, {}

    def probed(self, q, nprobe):
        if (q, nprobe) not in self._p:
            ix = self.ix
            if self.rows.size == 0:
                self._p[(q, nprobe)] = (np.zeros(0, np.uint64), np.zeros(0, np.float32))
            else:
                oi, od = co.search_nprobe(ix.values, ix.centroids, self.ids_f, self.Q[q], self.rows.size, nprobe, ix.metric)
                self._p[(q, nprobe)] = (np.asarray(oi, dtype=np.uint64), np.asarray(od, dtype=np.float32))
        return self._p[(q, nprobe)]

    def exhaustive(self, q, metric):
        if (q, metric) not in self._x:
            if self.rows.size == 0:
                self._x[(q, metric)] = (np.zeros(0, np.uint64), np.zeros(0, np.float32))
            else:
                oi, od = co.search_exhaustive(self.ix.values[self.rows], self.Q[q], self.rows.size, metric)
                self._x[(q, metric)] = (self.rows[oi.astype(np.int64)].astype(np.uint64), np.asarray(od, dtype=np.float32))
        return self._x[(q, metric)]

    def probes(self, q, nprobe):
        if q not in self._rank:
            k = self.ix.num_centroids
            self._rank[q] = [int(c) for c in co.search_exhaustive(self.ix.centroids, self.Q[q], k, self.ix.metric)[0]]   # stable: ties by index
        return self._rank[q][:min(nprobe, self.ix.num_centroids)]

    def device_list(self, c):
        if c not in self._lists:
            self._lists[c] = self.ix.get_list(c)[1]
            assert np.array_equal(self._lists[c], np.asarray(self.ix.ids[c], dtype=np.uint64)), c
        return self._lists[c]

    def mth(self, q, nprobe, m):
        """the exact distance of query q's m-th nearest ALLOWED probed row (the last one when fewer are allowed)"""
        od = self.probed(q, nprobe)[1]
        return od[min(m, len(od)) - 1] if len(od) else np.float32(0)

    @staticmethod
    def _head(full, r):
        oi, od = full
        m = int(np.count_nonzero(od <= np.float32(r)))
        assert not np.any(od[m:] <= np.float32(r))   # the result is the LEADING entries
        return oi[:m], od[:m]

    def _walk(self, full, lists, r):
        oi, od = full
        dist_of = dict(zip(oi.tolist(), od.tolist()))
        ids = [v for c in lists for v in self.device_list(c).tolist() if self.sem[v] and np.float32(dist_of[v]) <= np.float32(r)]
        return np.asarray(ids, dtype=np.uint64), np.asarray([dist_of[v] for v in ids], dtype=np.float32)

    def want(self, q, r, nprobe, metric, walk):
        """nprobe None: the exhaustive call under `metric`"""
        if nprobe is not None:
            full = self.probed(q, nprobe)
            return self._walk(full, self.probes(q, nprobe), r) if walk else self._head(full, r)
        full = self.exhaustive(q, metric)
        return self._walk(full, range(self.ix.num_centroids), r) if walk else self._head(full, r)


def words_of(allowed, n_bits=None):
    return IVFFlatIndex._filter_words(allowed, n_bits)


def host_call(ix, Q, radii, nprobe, metric, allowed, n_bits, walk):
    if nprobe is not None:
        return ix.range_search_filtered(Q, radii, nprobe, allowed, n_bits, walk_order=walk)
    return ix.range_search_exhaustive_filtered(Q, radii, allowed, metric, n_bits, walk_order=walk)


def dev_call(ix, Q, radii, nprobe, metric, allowed, n_bits, walk, stream=None, null_bitmap=False):
    """the _dev call through the capacity protocol: the size query, then arrays of exactly the total; sentinel-filled arrays one larger show
    that nothing is written past it"""
    import torch
    Q = np.ascontiguousarray(np.atleast_2d(Q), dtype=np.float32)
    b = Q.shape[0]
    dev = torch.device("cuda", ix.device)
    words, nb = words_of(allowed, n_bits)
    qd = torch.from_numpy(Q).to(dev)
    rd = torch.from_numpy(capi.range_radii(radii, b).copy()).to(dev)
    wd = torch.from_numpy(words.view(np.int64).copy()).to(dev)
    wp = 0 if null_bitmap else wd.data_ptr()
    lims = torch.full((b + 1,), -5, dtype=torch.int64, device=dev)
    flags = WALK if walk else 0
    s = stream.cuda_stream if stream is not None else 0
    torch.cuda.synchronize(dev)
    fn = (lambda *a: ix.range_search_filtered_dev(qd.data_ptr(), ix.d, b, rd.data_ptr(), nprobe, flags, wp, nb, *a, s)) if nprobe is not None else \
         (lambda *a: ix.range_search_exhaustive_filtered_dev(qd.data_ptr(), ix.d, b, rd.data_ptr(), metric, flags, wp, nb, *a, s))
    total = fn(lims.data_ptr(), 0, 0, 0)
    ids = torch.full((total + 1,), -3, dtype=torch.int64, device=dev)
    dist = torch.full((total + 1,), -7.25, dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)
    assert fn(lims.data_ptr(), ids.data_ptr(), dist.data_ptr(), total) == total
    assert int(ids[total]) == -3 and float(dist[total]) == -7.25
    return lims.cpu().numpy().astype(np.uint64), ids[:total].cpu().numpy().astype(np.uint64), dist[:total].cpu().numpy()


def same(got, want, what):
    lims, ids, dist = got
    assert lims[0] == 0 and lims[-1] == ids.size == dist.size and len(lims) == len(want) + 1, what
    for i, (ei, ed) in enumerate(want):
        a, e = int(lims[i]), int(lims[i + 1])
        assert e - a == ei.size, (what, i, e - a, ei.size)
        assert np.array_equal(ids[a:e], ei), (what, i, "ids")
        assert np.array_equal(bits(dist[a:e]), bits(ed)), (what, i, "distance bits")


def check(ref, qs, radii, nprobe, allowed, n_bits=None, metric=L2, call=host_call):
    """Both orders of one call shape against the oracle; the walk order re-sorted must be the sorted order.  -> the sorted result."""
    qs = list(qs)
    radii = np.broadcast_to(np.asarray(radii, dtype=np.float32), (len(qs),)).copy()
    Q = ref.Q[qs]
    got = []
    for walk in (False, True):
        g = call(ref.ix, Q, radii, nprobe, metric, allowed, n_bits, walk)
        same(g, [ref.want(q, radii[i], nprobe, metric, walk) for i, q in enumerate(qs)], (nprobe, metric, walk, call.__name__))
        got.append(g)
    (sl, si, sd), (wl, wi, wd) = got
    assert np.array_equal(sl, wl)
    for i in range(len(qs)):
        a, e = int(sl[i]), int(sl[i + 1])
        # probed: a stable sort by distance (ties stay in probe rank, list position); exhaustive: ties go to the lower vec id
        o = np.argsort(wd[a:e], kind="stable") if nprobe is not None else np.lexsort((wi[a:e], wd[a:e]))
        assert np.array_equal(wi[a:e][o], si[a:e]) and np.array_equal(bits(wd[a:e][o]), bits(sd[a:e])), ("walk re-sorted", nprobe, i)
    return got[0]


KINDS = 5   # query q of a mixed batch: kind q % 5


def mixed_radii(ref, qs, nprobe):
    """per query the 1st / 10th / 100th-nearest ALLOWED probed distance, +inf, -1: queries without a result between queries with many"""
    out = []
    for q in qs:
        kind = q % KINDS
        out.append(ref.mth(q, nprobe, (1, 10, 100)[kind]) if kind < 3 else (INF if kind == 3 else np.float32(-1)))
    return np.asarray(out, dtype=np.float32)


@pytest.fixture(scope="module")
def main_ix():
    ix = make(6000, 96, 12)
    yield ix
    ix.close()


@pytest.fixture(scope="module")
def main_ref(main_ix):
    """40 queries and a random filter at selectivity 0.5, shared by the cases that need no other"""
    Q = queries(main_ix, 0xFA71, 40)
    allowed = random_filter(6000, 0.5, 0xFA72)
    return Ref(main_ix, Q, allowed), allowed


# ---- 1. group widths, segments, both passes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seg_rows", [0, 64])
@pytest.mark.parametrize("b", [1, 3, 8, 9, 17, 40])
def test_group_widths_segments_and_both_passes(main_ref, b, seg_rows):
    ref, allowed = main_ref
    batches = [[j] for j in range(KINDS)] if b == 1 else [list(range(b))]   # (a single query: one call per kind of radius)
    capi.set_option("seg_rows", seg_rows)
    try:
        for qs in batches:
            for nprobe in (1, 4, 12):
                radii = mixed_radii(ref, qs, nprobe)
                for call in (host_call, dev_call):
                    lims, _, _ = check(ref, qs, radii, nprobe, allowed, call=call)
                    for i, q in enumerate(qs):
                        n = int(lims[i + 1]) - int(lims[i])
                        if q % KINDS == 1:
                            assert n >= 10, (q, n)     # the 10th-nearest radius
                        if q % KINDS == 4:
                            assert n == 0, (q, n)      # radius -1
                if nprobe == 4:   # the exhaustive call at the same radii
                    for call in (host_call, dev_call):
                        check(ref, qs, radii, None, allowed, call=call)
    finally:
        capi.set_option("seg_rows", 0)


def test_the_filter_removes_results_the_unfiltered_call_returns(main_ref):
    """so that no test above passes vacuously: the reference alone, and the device, return strictly more without the filter"""
    ref, allowed = main_ref
    ix = ref.ix
    qs = list(range(40))
    radii = np.asarray([ref.mth(q, 4, 10) for q in qs], dtype=np.float32)
    live = sum(len(l) for l in ix.ids)
    want_f = sum(ref.want(q, radii[q], 4, L2, False)[0].size for q in qs)
    want_u = 0
    for q in qs:
        od = co.search_nprobe(ix.values, ix.centroids, ix.ids, ref.Q[q], live, 4, ix.metric)[1]
        want_u += int(np.count_nonzero(np.asarray(od, dtype=np.float32) <= radii[q]))
    assert want_u > want_f >= 10 * len(qs)
    lims_f, _, _ = ix.range_search_filtered(ref.Q, radii, 4, allowed)
    lims_u, _, _ = ix.range_search(ref.Q, radii, 4)
    assert int(lims_f[-1]) == want_f and int(lims_u[-1]) == want_u
    assert np.all(np.diff(lims_f.astype(np.int64)) >= 10)


# ---- 2. selectivities -----------------------------------------------------------------------------------------------------------------
def test_selectivities(main_ix):
    ix = main_ix
    Q = queries(ix, 0xFA73, 9)
    n = 6000
    for allowed in (np.ones(n, dtype=bool), random_filter(n, 0.1, 0xFA74), random_filter(n, 0.01, 0xFA75), np.asarray([int(ix.ids[3][5])], dtype=np.uint64)):
        ref = Ref(ix, Q, allowed_set(n, allowed))
        for qs in (list(range(9)), [4]):
            for nprobe in (1, 4, 12):
                check(ref, qs, mixed_radii(ref, qs, nprobe), nprobe, allowed)
                check(ref, qs, INF, nprobe, allowed)
            check(ref, qs, mixed_radii(ref, qs, 12), None, allowed)
            check(ref, qs, INF, None, allowed)


def test_selectivity_one_is_the_unfiltered_range_search(main_ix):
    ix = main_ix
    Q = queries(ix, 0xFA76, 17)
    everything = np.ones(6000, dtype=bool)
    ref = Ref(ix, Q, everything)
    for qs in (list(range(17)), [0]):
        for nprobe in (1, 4, 12):
            radii = mixed_radii(ref, qs, nprobe)
            for w in (False, True):
                l0, i0, d0 = ix.range_search(Q[qs], radii, nprobe, walk_order=w)
                l1, i1, d1 = ix.range_search_filtered(Q[qs], radii, nprobe, everything, walk_order=w)
                assert np.array_equal(l0, l1) and np.array_equal(i0, i1) and np.array_equal(bits(d0), bits(d1)), (nprobe, w)
                assert l0[-1] > 0
                l0, i0, d0 = ix.range_search_exhaustive(Q[qs], radii, walk_order=w)
                l1, i1, d1 = ix.range_search_exhaustive_filtered(Q[qs], radii, everything, walk_order=w)
                assert np.array_equal(l0, l1) and np.array_equal(i0, i1) and np.array_equal(bits(d0), bits(d1)), ("exhaustive", w)


def test_empty_filter_total_zero_and_writes_nothing(main_ix):
    import torch
    ix = main_ix
    b = 9
    Q = queries(ix, 0xFA77, b)
    for allowed, n_bits in ((np.zeros(6000, dtype=bool), None), (np.ones(6000, dtype=bool), 0), (np.zeros(0, dtype=np.uint64), 0)):
        for Qs in (Q, Q[2]):
            for w in (False, True):
                for got in (ix.range_search_filtered(Qs, INF, 4, allowed, n_bits, walk_order=w), ix.range_search_exhaustive_filtered(Qs, INF, allowed, L2, n_bits, walk_order=w)):
                    assert not got[0].any() and got[1].size == 0 and got[2].size == 0
    # the three spellings through the raw device-pointer calls -- all-zero bitmap, n_bits == 0, NULL with 0 --: sentinel-filled arrays stay
    dev = torch.device("cuda", ix.device)
    qd = torch.from_numpy(Q).to(dev)
    rd = torch.full((b,), float("inf"), dtype=torch.float32, device=dev)
    zero_words = torch.zeros(6000 // 64 + 1, dtype=torch.int64, device=dev)
    ones_words = torch.full((6000 // 64 + 1,), -1, dtype=torch.int64, device=dev)
    for bits_ptr, n_bits in ((zero_words.data_ptr(), 6000), (ones_words.data_ptr(), 0), (0, 0)):
        for probed in (True, False):
            lims = torch.full((b + 1,), -5, dtype=torch.int64, device=dev)
            ids = torch.full((50,), -3, dtype=torch.int64, device=dev)
            dist = torch.full((50,), -7.25, dtype=torch.float32, device=dev)
            torch.cuda.synchronize(dev)
            if probed:
                total = ix.range_search_filtered_dev(qd.data_ptr(), ix.d, b, rd.data_ptr(), 4, 0, bits_ptr, n_bits, lims.data_ptr(), ids.data_ptr(), dist.data_ptr(), 50)
            else:
                total = ix.range_search_exhaustive_filtered_dev(qd.data_ptr(), ix.d, b, rd.data_ptr(), L2, 0, bits_ptr, n_bits, lims.data_ptr(), ids.data_ptr(),
                                                                dist.data_ptr(), 50)
            assert total == 0 and not lims.cpu().numpy().any() and bool((ids == -3).all()) and bool((dist == -7.25).all()), (probed, n_bits)
    # NULL with 0 through the host-pointer call
    r = np.full(b, np.inf, dtype=np.float32)
    lims = np.full(b + 1, 7, dtype=np.uint64); t = C.c_uint64(99)
    assert capi.lib().vers_ivf_range_search_filtered(ix._h, capi._ptr(Q), 4 * ix.d, b, capi._ptr(r), 4, 0, None, 0, capi._ptr(lims), None, None, 0, C.byref(t)) == capi.OK
    assert t.value == 0 and not lims.any()


# ---- 3. tile edges ----------------------------------------------------------------------------------------------------------------------
def test_tile_edges(main_ix):
    ix = main_ix
    n, k = 6000, ix.num_centroids
    Q = queries(ix, 0xFA78, 9)
    lists = [ix.get_list(c)[1].astype(np.int64) for c in range(k)]
    rank = [[int(c) for c in co.search_exhaustive(ix.centroids, q, k, ix.metric)[0]] for q in Q]
    nprobe = 4
    edge = np.concatenate([l[[p for p in (0, 63, 64, 127, len(l) - 1) if p < len(l)]] for l in lists if len(l)])
    whole = lists[rank[0][0]]                       # one whole probed list and nothing else: the nearest list of query 0
    but_one = np.setdiff1d(np.arange(n), whole)     # everything but that list
    for allowed in (edge, whole, but_one):
        ref = Ref(ix, Q, allowed_set(n, allowed, n))
        for qs in (list(range(9)), [0]):
            check(ref, qs, INF, nprobe, allowed, n)
            check(ref, qs, mixed_radii(ref, qs, nprobe), nprobe, allowed, n)
            check(ref, qs, mixed_radii(ref, qs, nprobe), nprobe, allowed, n, call=dev_call)
            check(ref, qs, INF, None, allowed, n)
    # only rows of a list query 0 does not probe: count 0 for it
    far = lists[rank[0][-1]]
    ref = Ref(ix, Q, allowed_set(n, far, n))
    got = check(ref, range(9), INF, nprobe, far, n)
    assert got[0][1] == 0
    assert check(ref, [0], INF, nprobe, far, n)[0][-1] == 0


# ---- 4. bitmap edges -------------------------------------------------------------------------------------------------------------------
def test_bitmap_edges(main_ix):
    ix = main_ix
    n = 6000
    Q = queries(ix, 0xFA79, 8)
    base = random_filter(n + 1000, 0.6, 0xFA7A)
    base[[n - 2, n - 1]] = True   # (the last ids of the index are allowed whenever n_bits reaches them)
    for n_bits in (n - 1, n, n + 1, n + 1000, 64 * ((n + 63) // 64) - 1, n // 2):
        ref = Ref(ix, Q, allowed_set(n, base, n_bits))   # ids >= n_bits are not allowed; bits of ids >= n select nothing
        radii = mixed_radii(ref, range(8), 4)
        check(ref, range(8), radii, 4, base, n_bits)
        check(ref, range(8), INF, None, base, n_bits)
        check(ref, [3], INF, 4, base, n_bits)
        # garbage in the last word beyond n_bits: every bit set
        words = capi.allowed_bitmap(base, n_bits)
        if n_bits % 64:
            words[-1] |= np.uint64(0xFFFFFFFFFFFFFFFF) << np.uint64(n_bits % 64)
        check(ref, range(8), INF, 4, (words, n_bits))
        check(ref, range(8), radii, None, (words, n_bits))
        check(ref, range(8), INF, 4, (words, n_bits), call=dev_call)
    # all ones everywhere, n_bits = n - 1: the last id alone is out
    words = np.full((n + 63) // 64, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    sem = np.ones(n, dtype=bool); sem[n - 1] = False
    ref = Ref(ix, Q, sem)
    check(ref, range(8), INF, None, (words, n - 1))
    check(ref, range(8), INF, 12, (words, n - 1))


# ---- 5. items of more than 64 tiles ----------------------------------------------------------------------------------------------------------
def test_items_of_more_than_64_tiles():
    ix = make(12000, 32, 2, seed=0xFA80)
    try:
        n = 12000
        lists = [ix.get_list(c)[1].astype(np.int64) for c in range(2)]
        assert max(len(l) for l in lists) > 4096 + 64   # the longer list reaches into a second window of 64 tiles (k-means decides the split)
        Q = queries(ix, 0xFA81, 9)
        second = np.concatenate([l[4096:] for l in lists])                      # live tiles in the second window only (a shorter list: none)
        first = np.concatenate([l[:4096:7] for l in lists])                     # ... in the first only
        both = np.concatenate([np.concatenate([l[100:130], l[4090:4100], l[-3:]]) for l in lists])
        one_late = lists[0][-1:]                                                # a single row, in the last tile
        capi.set_option("seg_rows", 8192)
        for allowed in (second, first, both, one_late):
            ref = Ref(ix, Q, allowed_set(n, allowed, n))
            for qs in (list(range(9)), [0]):
                for nprobe in (1, 2):
                    check(ref, qs, INF, nprobe, allowed, n)
                check(ref, qs, mixed_radii(ref, qs, 2), 2, allowed, n)
                check(ref, qs, INF, None, allowed, n)
                check(ref, qs, mixed_radii(ref, qs, 2), None, allowed, n)
    finally:
        capi.set_option("seg_rows", 0)
        ix.close()


# ---- 6. more than 64 probes ------------------------------------------------------------------------------------------------------------
def test_more_than_64_probes():
    ix = make(4000, 16, 80, seed=0xFA90)
    try:
        Q = queries(ix, 0xFA91, 9)
        allowed = random_filter(4000, 0.3, 0xFA92)
        ref = Ref(ix, Q, allowed)
        for qs in (list(range(9)), [5]):
            check(ref, qs, mixed_radii(ref, qs, 70), 70, allowed)
            check(ref, qs, INF, 70, allowed)
    finally:
        ix.close()


# ---- 7. dimensions and the cosine metric ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 100, 320])
def test_dimensions(d):
    ix = make(1500, d, 6, seed=0xFAA0 + d)
    try:
        Q = queries(ix, 0xFAA1, 9)
        allowed = random_filter(1500, 0.4, 0xFAA2)
        ref = Ref(ix, Q, allowed)
        for qs in (list(range(9)), [1]):
            check(ref, qs, mixed_radii(ref, qs, 3), 3, allowed)
            check(ref, qs, INF, 6, allowed)
            check(ref, qs, mixed_radii(ref, qs, 3), None, allowed)
    finally:
        ix.close()


def test_cosine_metric():
    ix = make(1500, 48, 6, metric=COS, seed=0xFAB0)
    try:
        Q = queries(ix, 0xFAB1, 9)
        allowed = random_filter(1500, 0.4, 0xFAB2)
        ref = Ref(ix, Q, allowed)
        for qs in (list(range(9)), [1]):
            check(ref, qs, mixed_radii(ref, qs, 3), 3, allowed)
            check(ref, qs, INF, 6, allowed)
            for metric in (L2, COS):
                radii = np.asarray([ref.exhaustive(q, metric)[1][(0, 9, 99, -1, 0)[q % KINDS]] if q % KINDS != 4 else -1 for q in qs], dtype=np.float32)
                check(ref, qs, radii, None, allowed, metric=metric)
    finally:
        ix.close()


# ---- 8. virtual removal, GPU against GPU ----------------------------------------------------------------------------------------------------
def test_filter_equals_removal_on_a_second_index(main_ix):
    ix = main_ix
    n = 6000
    Q = queries(ix, 0xFAC0, 17)
    allowed = random_filter(n, 0.3, 0xFAC1)
    ref = Ref(ix, Q, allowed)
    other = clone(ix)
    try:
        other.remove_batch(np.flatnonzero(~allowed).astype(np.uint64))
        for qs in (list(range(17)), [0]):
            for nprobe in (1, 4, 12):
                radii = mixed_radii(ref, qs, nprobe)
                for w in (False, True):
                    l0, i0, d0 = other.range_search(Q[qs], radii, nprobe, walk_order=w)
                    l1, i1, d1 = ix.range_search_filtered(Q[qs], radii, nprobe, allowed, walk_order=w)
                    assert np.array_equal(l0, l1) and np.array_equal(i0, i1) and np.array_equal(bits(d0), bits(d1)), (nprobe, w)
                    assert l0[-1] > 0
            radii = mixed_radii(ref, qs, 12)
            for w in (False, True):
                l0, i0, d0 = other.range_search_exhaustive(Q[qs], radii, walk_order=w)
                l1, i1, d1 = ix.range_search_exhaustive_filtered(Q[qs], radii, allowed, walk_order=w)
                assert np.array_equal(l0, l1) and np.array_equal(i0, i1) and np.array_equal(bits(d0), bits(d1)), ("exhaustive", w)
    finally:
        other.close()


# ---- 9. a mutated index ----------------------------------------------------------------------------------------------------------------------
def test_mutated_index():
    ix = make(3000, 64, 8, seed=0xFAD0)
    try:
        Q = queries(ix, 0xFAD1, 9)
        new_rows = dg.dist_c(0xFAD2, 500, 64, 16, dg.default_sigma(64))
        ix.add_batch(new_rows)
        n = 3500
        allowed = random_filter(n, 0.5, 0xFAD3)
        allowed[3000:3100] = True   # new ids among the allowed
        ref = Ref(ix, Q, allowed)
        assert ref.sem[3000:].sum() >= 100

        def run(ref):
            return [check(ref, range(9), mixed_radii(ref, range(9), 4), 4, allowed), check(ref, range(9), INF, 8, allowed),
                    check(ref, range(9), mixed_radii(ref, range(9), 8), None, allowed), check(ref, [2], INF, 4, allowed)]
        got = run(ref)
        assert np.any(got[1][1] >= 3000)   # added ids are among the results
        gone = np.flatnonzero(allowed)[::3].astype(np.uint64)   # removed ids stay in the filter: they select nothing
        ix.remove_batch(gone)
        ref = Ref(ix, Q, allowed)
        assert ref.rows.size == int(allowed.sum()) - gone.size
        before = run(ref)
        assert not np.isin(before[1][1], gone).any()
        ix.compact()
        after = run(ref)
        for (l0, i0, d0), (l1, i1, d1) in zip(before, after):
            assert np.array_equal(l0, l1) and np.array_equal(i0, i1) and np.array_equal(bits(d0), bits(d1))
    finally:
        ix.close()


# ---- 10. NaN -----------------------------------------------------------------------------------------------------------------------------
def raw(ix, Q, radii, arg, flags, words, n_bits, cap=0, ids=None, dist=None, probed=True):
    Q = np.ascontiguousarray(np.atleast_2d(Q), dtype=np.float32)
    b = Q.shape[0]
    r = np.ascontiguousarray(np.broadcast_to(np.asarray(radii, dtype=np.float32), (b,)))
    lims = np.full(b + 1, 0xABABABABABABABAB, dtype=np.uint64)
    total = C.c_uint64(12345)
    fn = capi.lib().vers_ivf_range_search_filtered if probed else capi.lib().vers_ivf_range_search_exhaustive_filtered
    rc = fn(ix._h, capi._ptr(Q), 4 * ix.d, b, capi._ptr(r), arg, flags, capi._ptr(words) if words is not None else None, n_bits, capi._ptr(lims),
            capi._ptr(ids) if ids is not None else None, capi._ptr(dist) if dist is not None else None, cap, C.byref(total))
    return rc, lims, int(total.value)


def test_nan_row_outside_the_filter_is_not_scanned():
    src = make(1500, 48, 6, seed=0xFAE0)
    ix = IVFFlatIndex(48)
    try:
        bad = int(src.ids[2][70])   # a row in the second tile of list 2
        ix.num_centroids, ix.centroids, ix.assignments, ix.ids = src.num_centroids, src.centroids, src.assignments, [list(l) for l in src.ids]
        ix.values = src.values.copy()
        ix.values[bad, 7] = np.nan
        ix._upload()
        Q = queries(src, 0xFAE1, 9)
        allowed = random_filter(1500, 0.5, 0xFAE2)
        allowed[[int(v) for v in src.ids[2][64:128]]] = True   # the rest of its tile is allowed: the tile IS loaded
        allowed[bad] = False
        ref = Ref(ix, Q, allowed)
        for qs in (list(range(9)), [0]):
            check(ref, qs, INF, 6, allowed)
            check(ref, qs, mixed_radii(ref, qs, 6), 6, allowed)
            check(ref, qs, INF, None, allowed)
        allowed[bad] = True
        words = capi.allowed_bitmap(allowed, 1500)
        for Qs in (Q, Q[:1]):
            for probed in (True, False):
                ids = np.full(3000 * 9, 0xCDCDCDCDCDCDCDCD, dtype=np.uint64); dist = np.full(3000 * 9, -7.25, dtype=np.float32)
                rc, lims, _ = raw(ix, Qs, INF, 6 if probed else L2, 0, words, 1500, ids.size, ids, dist, probed=probed)
                assert rc == capi.ERR_NAN, (probed, Qs.shape)
                assert np.all(ids == 0xCDCDCDCDCDCDCDCD) and np.all(dist == np.float32(-7.25)) and np.all(lims == 0xABABABABABABABAB)
        allowed[bad] = False   # and the handle is still usable
        check(ref, range(9), INF, 6, allowed)
        # a NaN radius is an argument error, on the host-pointer call and on the device
        words = capi.allowed_bitmap(allowed, 1500)
        rad = np.full(9, 1.0, dtype=np.float32); rad[3] = np.nan
        assert raw(ix, Q, rad, 6, 0, words, 1500)[0] == capi.ERR_INVALID
        assert raw(ix, Q, rad, L2, 0, words, 1500, probed=False)[0] == capi.ERR_INVALID
        with pytest.raises(capi.VersError) as e:
            dev_call(ix, Q, rad, 6, L2, allowed, None, False)
        assert e.value.status == capi.ERR_INVALID
        with pytest.raises(capi.VersError) as e:
            dev_call(ix, Q, rad, None, L2, allowed, None, False)
        assert e.value.status == capi.ERR_INVALID
        check(ref, range(9), INF, 6, allowed)
    finally:
        ix.close()
        src.close()


# ---- 11. protocol and errors ---------------------------------------------------------------------------------------------------------------
def test_protocol_and_errors(main_ref):
    ref, allowed = main_ref
    ix = ref.ix
    qs = list(range(8))
    Q = ref.Q[qs]
    words = capi.allowed_bitmap(allowed, 6000)
    L = capi.lib()
    for probed in (True, False):
        arg = 4 if probed else L2
        radii = np.asarray([ref.mth(q, 4, 10) for q in qs], dtype=np.float32)
        want = check(ref, qs, radii, 4 if probed else None, allowed)
        total = int(want[0][-1])
        assert total >= 80
        # the size query: cap == 0 with NULL arrays
        rc, lims, got = raw(ix, Q, radii, arg, 0, words, 6000, probed=probed)
        assert rc == capi.OK and got == total and np.array_equal(lims, want[0])
        # one short: VERS_OK, the total, complete limits, ids / distances untouched
        ids = np.full(total, 0xCDCDCDCDCDCDCDCD, dtype=np.uint64); dist = np.full(total, -7.25, dtype=np.float32)
        rc, lims, got = raw(ix, Q, radii, arg, 0, words, 6000, total - 1, ids, dist, probed=probed)
        assert rc == capi.OK and got == total and np.array_equal(lims, want[0])
        assert np.all(ids == 0xCDCDCDCDCDCDCDCD) and np.all(dist == np.float32(-7.25))
        # exactly enough
        rc, lims, got = raw(ix, Q, radii, arg, 0, words, 6000, total, ids, dist, probed=probed)
        assert rc == capi.OK and got == total and np.array_equal(ids, want[1]) and np.array_equal(bits(dist), bits(want[2]))
        # argument errors
        assert raw(ix, Q, radii, arg, 2, words, 6000, probed=probed)[0] == capi.ERR_INVALID        # unknown flag bits
        assert raw(ix, Q, radii, arg, 0, None, 6000, probed=probed)[0] == capi.ERR_INVALID         # n_bits > 0 with a NULL bitmap
        assert raw(ix, Q, radii, arg, 0, words, 6000, 5, probed=probed)[0] == capi.ERR_INVALID     # a capacity without arrays
    assert raw(ix, Q, 1.0, 0, 0, words, 6000)[0] == capi.ERR_INVALID                               # nprobe == 0
    assert raw(ix, Q, 1.0, 2, 0, words, 6000, probed=False)[0] == capi.ERR_INVALID                 # metric > VERS_METRIC_COSDIST
    # the same through the device-pointer calls
    import torch
    dev = torch.device("cuda", ix.device)
    qd = torch.from_numpy(Q).to(dev); wd = torch.from_numpy(words.view(np.int64).copy()).to(dev)
    rd = torch.ones(8, dtype=torch.float32, device=dev); lims = torch.zeros(9, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    for nprobe, flags, ptr in ((0, 0, wd.data_ptr()), (4, 2, wd.data_ptr()), (4, 0, 0)):
        with pytest.raises(capi.VersError) as e:
            ix.range_search_filtered_dev(qd.data_ptr(), ix.d, 8, rd.data_ptr(), nprobe, flags, ptr, 6000, lims.data_ptr(), 0, 0, 0)
        assert e.value.status == capi.ERR_INVALID
    for metric, flags, ptr in ((2, 0, wd.data_ptr()), (L2, 2, wd.data_ptr()), (L2, 0, 0)):
        with pytest.raises(capi.VersError) as e:
            ix.range_search_exhaustive_filtered_dev(qd.data_ptr(), ix.d, 8, rd.data_ptr(), metric, flags, ptr, 6000, lims.data_ptr(), 0, 0, 0)
        assert e.value.status == capi.ERR_INVALID
    # b == 0: a no-op, *out_total = 0
    t = C.c_uint64(99)
    assert L.vers_ivf_range_search_filtered(ix._h, None, 4 * ix.d, 0, None, 4, 0, capi._ptr(words), 6000, None, None, None, 0, C.byref(t)) == capi.OK and t.value == 0
    t = C.c_uint64(99)
    assert L.vers_ivf_range_search_exhaustive_filtered(ix._h, None, 4 * ix.d, 0, None, L2, 0, capi._ptr(words), 6000, None, None, None, 0, C.byref(t)) == capi.OK and t.value == 0
    t = C.c_uint64(99)
    assert L.vers_ivf_range_search_filtered_dev(ix._h, None, ix.d, 0, None, 4, 0, None, 0, None, None, None, 0, C.byref(t), None) == capi.OK and t.value == 0
    t = C.c_uint64(99)
    assert L.vers_ivf_range_search_exhaustive_filtered_dev(ix._h, None, ix.d, 0, None, L2, 0, None, 0, None, None, None, 0, C.byref(t), None) == capi.OK and t.value == 0
    # an index without centroids: the probed call has nothing to rank, the exhaustive call finds nothing
    empty = IVFFlatIndex(ix.d)
    assert raw(empty, Q, INF, 4, 0, words, 6000)[0] == capi.ERR_INSUFFICIENT
    rc, lims, got = raw(empty, Q, INF, L2, 0, words, 6000, probed=False)
    assert rc == capi.OK and got == 0 and not lims.any()
    empty.close()
    # a streamed upload in progress is seen as an empty index
    sh = make(600, 32, 4, seed=0xFAF1)
    Qs = queries(sh, 0xFAF2, 3)
    w600 = capi.allowed_bitmap(np.ones(600, dtype=bool), 600)
    up = IVFFlatIndex(sh.d)
    up.upload_begin(sh.centroids, [len(l) for l in sh.ids], 600)
    assert raw(up, Qs, INF, 2, 0, w600, 600)[0] == capi.ERR_INSUFFICIENT
    rc, lims, got = raw(up, Qs, INF, L2, 0, w600, 600, probed=False)
    assert rc == capi.OK and got == 0 and not lims.any()
    up.close()
    # a handle sharded by cluster: out of scope
    half = IVFFlatIndex(sh.d)
    half.set_shard(0, 2)
    half.num_centroids, half.values, half.centroids, half.assignments = sh.num_centroids, sh.values, sh.centroids, sh.assignments
    half._upload()
    rc, _, got = raw(sh, Qs, INF, 2, 0, w600, 600)
    assert rc == capi.OK and got > 0
    assert half.info()[1] == 4 and raw(half, Qs, INF, 2, 0, w600, 600)[0] == capi.ERR_INVALID
    assert "out of scope" in capi.lib().vers_last_error().decode("utf-8", "replace")
    assert raw(half, Qs, INF, L2, 0, w600, 600, probed=False)[0] == capi.ERR_INVALID
    half.close()
    sh.close()


# ---- 12. _dev calls on two streams ------------------------------------------------------------------------------------------------------------
def test_device_pointer_calls_on_two_streams(main_ref):
    import torch
    ref, allowed = main_ref
    ix = ref.ix
    qs = list(range(17))
    radii = mixed_radii(ref, qs, 4)
    dev = torch.device("cuda", ix.device)
    outs = []
    for stream in (torch.cuda.Stream(dev), torch.cuda.Stream(dev)):
        for nprobe in (4, None):
            for walk in (False, True):
                got = dev_call(ix, ref.Q[qs], radii, nprobe, L2, allowed, None, walk, stream=stream)
                same(got, [ref.want(q, radii[i], nprobe, L2, walk) for i, q in enumerate(qs)], (nprobe, walk))
                outs.append(got)
    half = len(outs) // 2
    for (l0, i0, d0), (l1, i1, d1) in zip(outs[:half], outs[half:]):
        assert np.array_equal(l0, l1) and np.array_equal(i0, i1) and np.array_equal(bits(d0), bits(d1))


# ---- 13. the workspace lease is clean ---------------------------------------------------------------------------------------------------------
def test_other_calls_are_unchanged_around_filtered_range_calls(main_ref):
    ref, allowed = main_ref
    ix = ref.ix
    Q = ref.Q
    radii = np.asarray([ref.mth(q, 4, 10) for q in range(40)], dtype=np.float32)

    def others():
        out = [ix.search_batch(Q, top_k, nprobe) for top_k, nprobe in ((10, 4), (10, 0), (100, 4))] + [ix.search_batch(Q[0], 10, 4)]
        out += [ix.search_filtered(Q, 10, 4, allowed), ix.search_filtered(Q[0], 10, 4, allowed)]
        rng = [ix.range_search(Q, radii, 4), ix.range_search(Q[0], radii[0], 4, walk_order=True), ix.range_search_exhaustive(Q[:9], radii[:9])]
        return out, rng
    before = others()
    check(ref, range(40), radii, 4, allowed); check(ref, [0], INF, 12, allowed); check(ref, range(9), radii[:9], None, allowed)
    check(ref, range(17), radii[:17], 4, allowed, call=dev_call)
    after = others()
    for (i0, d0, c0), (i1, d1, c1) in zip(before[0], after[0]):
        assert np.array_equal(c0, c1)
        for q in range(len(c0)):
            assert np.array_equal(i0[q, :c0[q]], i1[q, :c0[q]]) and np.array_equal(bits(d0[q, :c0[q]]), bits(d1[q, :c0[q]]))
    for (l0, i0, d0), (l1, i1, d1) in zip(before[1], after[1]):
        assert np.array_equal(l0, l1) and np.array_equal(i0, i1) and np.array_equal(bits(d0), bits(d1)) and l0[-1] > 0


# ---- 14. the measurement hooks ------------------------------------------------------------------------------------------------------------------
def test_stats_hook(main_ix):
    ix = main_ix
    n, k = 6000, ix.num_centroids
    Q = queries(ix, 0xFB00, 1)
    rank = [int(c) for c in co.search_exhaustive(ix.centroids, Q[0], k, ix.metric)[0]]
    lists = [ix.get_list(c)[1].astype(np.int64) for c in range(k)]
    tiles = lambda c: (len(lists[c]) + 63) // 64
    nprobe = 4
    probed = rank[:nprobe]
    live = sum(len(l) for l in lists)
    planned = sum(tiles(p) for p in probed)
    capi.set_option("seg_rows", 64)   # b == 1, 64-row segments: a work item is one tile of one probed list
    try:
        t0 = ix.filter_stats()["total"]
        c = probed[0]
        pos = [0, 5, 63, 200, 201, len(lists[c]) - 1]
        held = len({p // 64 for p in pos})
        cases = ((lists[c], dict(tiles_planned=planned, tiles_loaded=tiles(c), items_skipped=planned - tiles(c), rows_allowed=len(lists[c]))),   # the nearest list, whole
                 (lists[c][pos], dict(tiles_planned=planned, tiles_loaded=held, items_skipped=planned - held, rows_allowed=len(pos))),            # a few positions of it
                 (np.arange(n), dict(tiles_planned=planned, tiles_loaded=planned, items_skipped=0, rows_allowed=live)))                            # everything
        for allowed, want in cases:
            ref = Ref(ix, Q, allowed_set(n, allowed, n))
            near = ref.mth(0, nprobe, 1)
            tiny = np.nextafter(near, np.float32(-np.inf))   # below the nearest allowed distance: the fill pass has nothing to do
            assert ix.range_search_filtered(Q, tiny, nprobe, allowed, n)[0][-1] == 0
            for r in (tiny, near, INF):     # the count pass alone feeds the counters: the same at every radius
                for walk in (False, True):
                    got = ix.range_search_filtered(Q, r, nprobe, allowed, n, walk_order=walk)
                    same(got, [ref.want(0, r, nprobe, L2, walk)], ("stats", float(r), walk))
                    st = ix.filter_stats()["last"]
                    assert st == want, (st, want, float(r))
        assert cases[0][1]["items_skipped"] > 0
        # the running totals advance by the sums (size queries: exactly one call of the C ABI each)
        t0 = ix.filter_stats()["total"]
        for allowed, _ in cases:
            rc, _, _ = raw(ix, Q, INF, nprobe, 0, capi.allowed_bitmap(allowed, n), n)
            assert rc == capi.OK
        t1 = ix.filter_stats()["total"]
        assert {key: t1[key] - t0[key] for key in t1} == {key: sum(w[key] for _, w in cases) for key in t1}
        # the exhaustive call over 64-row segments: an item is one storage tile
        everything = np.ones(n, dtype=bool)
        ref = Ref(ix, Q, everything)
        for r in (ref.mth(0, nprobe, 1), INF):
            same(ix.range_search_exhaustive_filtered(Q, r, everything), [ref.want(0, r, None, L2, False)], "stats exhaustive")
            st = ix.filter_stats()["last"]
            assert st["tiles_loaded"] == sum(tiles(p) for p in range(k)) and st["rows_allowed"] == live and st["tiles_planned"] >= st["tiles_loaded"]
            assert st["items_skipped"] == st["tiles_planned"] - st["tiles_loaded"]   # (storage slack: tiles that hold no vector at all)
    finally:
        capi.set_option("seg_rows", 0)


def test_phases_and_scan_timing_ring(main_ref):
    ref, allowed = main_ref
    ix = ref.ix
    Q = ref.Q[:8]
    radii = np.asarray([ref.mth(q, 4, 10) for q in range(8)], dtype=np.float32)
    lims, _, _ = ix.range_search_filtered(Q, radii, 4, allowed)      # (sizes the binding's capacity: the next call is ONE call of the C ABI)
    capi.range_phases(reset=True)
    lims, _, _ = ix.range_search_filtered(Q, radii, 4, allowed)
    ph = capi.range_phases(reset=True)
    assert (ph["calls"], ph["queries"], ph["results"]) == (1, 8, int(lims[-1]))
    assert ph["count_ms"] > 0 and ph["fill_ms"] > 0 and ph["sort_ms"] > 0 and ph["plan_ms"] > 0 and ph["scan_ms"] > 0
    lims, _, _ = ix.range_search_exhaustive_filtered(Q, radii, allowed)
    lims, _, _ = ix.range_search_exhaustive_filtered(Q, radii, allowed)
    ph = capi.range_phases(reset=True)
    assert ph["calls"] >= 1 and ph["results"] % int(lims[-1]) == 0 and ph["plan_ms"] > 0
    # the scan-timing ring: the mask kernel leaves its record as in every filtered call, the range passes none as in every range call
    words = capi.allowed_bitmap(allowed, 6000)
    ix.scan_times(reset=True)
    ix.range_search(Q, radii, 4)
    assert ix.scan_times(reset=True).size == 0
    for probed in (True, False):
        rc, _, total = raw(ix, Q, radii, 4 if probed else L2, 0, words, 6000, probed=probed)    # (a size query: ONE call, the count pass alone)
        assert rc == capi.OK and total > 0
        ring = ix.scan_times(reset=True)
        assert ring.size == 1 and ring[0] > 0, (probed, ring)
    ids = np.zeros(int(lims[-1]), dtype=np.uint64); dist = np.zeros(int(lims[-1]), dtype=np.float32)
    rc, _, total = raw(ix, Q, radii, L2, 0, words, 6000, ids.size, ids, dist, probed=False)    # both passes and the sort: still one record
    assert rc == capi.OK and total == ids.size
    assert ix.scan_times(reset=True).size == 1


# ---- 15. the C++ mirror --------------------------------------------------------------------------------------------------------------------
def test_cpp_host_mirror_filtered_range_search(tmp_path):
    """vers_amd/host/ivfflat.hpp's range_search_filtered() / range_search_exhaustive_filtered() from compiled code
    (tests/cpp/filtered_range_demo.cpp) against the Python mirror's result"""
    lib = capi.LIB_PATH
    exe = str(tmp_path / "filtered_range_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + ROOT, "-o", exe, os.path.join(ROOT, "tests", "cpp", "filtered_range_demo.cpp"),
                           "-L" + os.path.dirname(lib), "-lvers_hip", "-Wl,-rpath," + os.path.dirname(lib)])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.rstrip().endswith("DONE"), out.stdout[-2000:] + out.stderr
    i, j = np.meshgrid(np.arange(900), np.arange(40), indexing="ij")
    X = (((i * 7 + j * 13) % 31).astype(np.float32) * np.float32(0.25) + (i % 6).astype(np.float32)).astype(np.float32)
    ix = IVFFlatIndex.build_index(6, 1, 5, X, init_indices=np.asarray([3, 90, 200, 333, 480, 899], dtype=np.uint64))
    got = {}
    for line in out.stdout.splitlines()[:-1]:
        q, mode, vid, db = (int(t) for t in line.split())
        got.setdefault((q, mode), []).append((vid, db))
    n_rows = 0
    for q in range(6):
        allowed = np.zeros(900 - 37 * q, dtype=bool)
        allowed[::q + 2] = True
        radius = np.float32(np.inf) if q % 2 else np.float32(150.0 + 100.0 * q)
        for mode in range(4):
            walk = mode >= 2
            lims, ids, dist = ix.range_search_filtered(X[q * 31], radius, 3, allowed, walk_order=walk) if mode % 2 == 0 else \
                ix.range_search_exhaustive_filtered(X[q * 31], radius, allowed, walk_order=walk)
            assert got.get((q, mode), []) == list(zip(ids.tolist(), bits(dist).tolist())), (q, mode)
            n_rows += ids.size
    assert n_rows > 12
    ix.close()
