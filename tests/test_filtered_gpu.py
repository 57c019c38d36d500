"""vers_ivf_search_filtered / vers_ivf_search_exhaustive_filtered (+ _dev, vers_ivf_filter_stats): the top_k nearest among the vec ids a
per-call bitmap allows.  A filter is a VIRTUAL REMOVAL, so the expected values come from the oracle as it stands --
  probed      co.search_nprobe over ids_filtered[c] = [v for v in ix.ids[c] if v in A];
  exhaustive  co.search_exhaustive over the rows of the allowed live ids in ascending id, indices mapped back
-- and every comparison is np.array_equal on the ids, on the distances' u32 BITS and on out_count: no tolerance.  The oracle's full order
(top_k = every row) is computed once per (index, queries, nprobe, filter) and cut to each top_k: a stable sort's head is the top_k result."""
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


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def make(n, d, k, metric=L2, seed=0xF170, iters=4):
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
    IVFFlatIndex.search_filtered defaults it."""
    a = np.asarray(allowed)
    if n_bits is None:
        n_bits = a.size if a.dtype == np.bool_ else (int(a.max()) + 1 if a.size else 0)
    ids = np.flatnonzero(a) if a.dtype == np.bool_ else a.astype(np.int64)
    out = np.zeros(n, dtype=bool)
    ids = ids[(ids < n_bits) & (ids < n)]
    out[ids] = True
    return out


class Ref:
    """The oracle's view of (index, queries, filter): the full filtered order per query, per nprobe on demand and exhaustive per metric."""

    def __init__(self, ix, Q, sem):
        self.ix, self.Q, self.sem = ix, np.atleast_2d(Q), np.asarray(sem, dtype=bool)
        self.ids_f = [[v for v in l if self.sem[v]] for l in ix.ids]
        self.rows = np.asarray(sorted(v for l in self.ids_f for v in l), dtype=np.int64)
        self._p, self._x = {}, {}

    def probed(self, q, nprobe):
        if (q, nprobe) not in self._p:
            ix = self.ix
            self._p[(q, nprobe)] = co.search_nprobe(ix.values, ix.centroids, self.ids_f, self.Q[q], max(1, self.rows.size), nprobe, ix.metric)
        return self._p[(q, nprobe)]

    def exhaustive(self, q, metric):
        if (q, metric) not in self._x:
            if self.rows.size == 0:
                self._x[(q, metric)] = (np.zeros(0, np.uint64), np.zeros(0, np.float32))
            else:
                oi, od = co.search_exhaustive(self.ix.values[self.rows], self.Q[q], self.rows.size, metric)
                self._x[(q, metric)] = (self.rows[oi.astype(np.int64)].astype(np.uint64), od)
        return self._x[(q, metric)]


def same(got, want_fn, qs, top_k, what):
    ids, dist, cnt = got
    for i, q in enumerate(qs):
        ei, ed = want_fn(q)
        ei, ed = ei[:top_k], ed[:top_k]
        assert cnt[i] == ei.size, (what, q, int(cnt[i]), ei.size)
        assert np.array_equal(ids[i, :cnt[i]], ei), (what, q, "ids")
        assert np.array_equal(bits(dist[i, :cnt[i]]), bits(ed)), (what, q, "distance bits")


def check_probed(ref, top_k, nprobe, allowed, n_bits=None, qs=None):
    qs = list(range(ref.Q.shape[0])) if qs is None else qs
    got = ref.ix.search_filtered(ref.Q[qs], top_k, nprobe, allowed, n_bits)
    same(got, lambda q: ref.probed(q, nprobe), qs, top_k, ("probed", top_k, nprobe))
    return got


def check_exhaustive(ref, top_k, allowed, metric=L2, n_bits=None, qs=None):
    qs = list(range(ref.Q.shape[0])) if qs is None else qs
    got = ref.ix.search_exhaustive_filtered(ref.Q[qs], top_k, allowed, metric, n_bits)
    same(got, lambda q: ref.exhaustive(q, metric), qs, top_k, ("exhaustive", top_k, metric))
    return got


def random_filter(n, sel, seed):
    return np.random.default_rng(seed).random(n) < sel


@pytest.fixture(scope="module")
def main_ix():
    ix = make(6000, 96, 12)
    yield ix
    ix.close()


@pytest.fixture(scope="module")
def main_ref(main_ix):
    """40 queries and a random filter at selectivity 0.5, shared by the cases that need no other"""
    Q = queries(main_ix, 0xF171, 40)
    allowed = random_filter(6000, 0.5, 0xF172)
    return Ref(main_ix, Q, allowed), allowed


# ---- 1. query-group widths, segments and passes ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seg_rows", [0, 64])
@pytest.mark.parametrize("b", [1, 3, 8, 9, 17, 40])
def test_group_widths_segments_and_passes(main_ref, b, seg_rows):
    ref, allowed = main_ref
    qs = list(range(b))
    capi.set_option("seg_rows", seg_rows)
    try:
        for nprobe in (1, 4, 12):
            for top_k in (1, 10, 64, 65, 200):
                check_probed(ref, top_k, nprobe, allowed, qs=qs)
        for top_k in (1, 10, 64, 65, 200):
            check_exhaustive(ref, top_k, allowed, qs=qs)
    finally:
        capi.set_option("seg_rows", 0)


# ---- 2. selectivities -----------------------------------------------------------------------------------------------------------------
def test_selectivities(main_ix):
    ix = main_ix
    Q = queries(ix, 0xF173, 9)
    n = 6000
    for allowed in (np.ones(n, dtype=bool), random_filter(n, 0.1, 0xF174), random_filter(n, 0.01, 0xF175), np.asarray([int(ix.ids[3][5])], dtype=np.uint64)):
        ref = Ref(ix, Q, allowed_set(n, allowed))
        for qs in (list(range(9)), [4]):
            for nprobe in (1, 4, 12):
                check_probed(ref, 10, nprobe, allowed, qs=qs)
            check_probed(ref, 100, 12, allowed, qs=qs)
            check_exhaustive(ref, 10, allowed, qs=qs)
            check_exhaustive(ref, 100, allowed, qs=qs)


def test_selectivity_one_is_the_unfiltered_search(main_ix):
    ix = main_ix
    Q = queries(ix, 0xF176, 17)
    everything = np.ones(6000, dtype=bool)
    for Qs in (Q, Q[:1]):
        for top_k, nprobe in ((10, 4), (10, 1), (100, 12), (64, 4)):
            i0, d0, c0 = ix.search_batch(Qs, top_k, nprobe)
            i1, d1, c1 = ix.search_filtered(Qs, top_k, nprobe, everything)
            assert np.array_equal(c0, c1)
            for q in range(len(c0)):
                assert np.array_equal(i0[q, :c0[q]], i1[q, :c0[q]]) and np.array_equal(bits(d0[q, :c0[q]]), bits(d1[q, :c0[q]])), (top_k, nprobe, q)
        for top_k in (10, 100):
            i0, d0, c0 = ix.search_exhaustive(Qs, top_k)
            i1, d1, c1 = ix.search_exhaustive_filtered(Qs, top_k, everything)
            assert np.array_equal(c0, c1) and np.all(c0 == top_k)
            assert np.array_equal(i0, i1) and np.array_equal(bits(d0), bits(d1)), top_k


def test_empty_filter_counts_zero_and_writes_nothing(main_ix):
    import torch
    ix = main_ix
    b, top_k = 9, 10
    Q = queries(ix, 0xF177, b)
    for allowed, n_bits in ((np.zeros(6000, dtype=bool), None), (np.ones(6000, dtype=bool), 0), (np.zeros(0, dtype=np.uint64), 0)):
        for got in (ix.search_filtered(Q, top_k, 4, allowed, n_bits), ix.search_exhaustive_filtered(Q, top_k, allowed, L2, n_bits),
                    ix.search_filtered(Q[2], top_k, 4, allowed, n_bits)):
            assert not got[2].any()
    # a NULL bitmap with n_bits == 0, through the raw calls; device pointers: nothing beyond the counts is written
    dev = torch.device("cuda", ix.device)
    qd = torch.from_numpy(Q).to(dev)
    zero_words = torch.zeros(6000 // 64 + 1, dtype=torch.int64, device=dev)
    for bits_ptr, n_bits in ((0, 0), (zero_words.data_ptr(), 6000)):
        for call in ("probed", "exhaustive"):
            ids = torch.full((b, top_k), -3, dtype=torch.int64, device=dev)
            dist = torch.full((b, top_k), -7.25, dtype=torch.float32, device=dev)
            cnt = torch.full((b,), 77, dtype=torch.int32, device=dev)
            torch.cuda.synchronize(dev)
            if call == "probed":
                ix.search_filtered_dev(qd.data_ptr(), ix.d, b, top_k, 4, bits_ptr, n_bits, ids.data_ptr(), dist.data_ptr(), cnt.data_ptr())
            else:
                ix.search_exhaustive_filtered_dev(qd.data_ptr(), ix.d, b, top_k, L2, bits_ptr, n_bits, ids.data_ptr(), dist.data_ptr(), cnt.data_ptr())
            ix.poll()
            assert not cnt.cpu().numpy().any() and bool((ids == -3).all()) and bool((dist == -7.25).all()), (call, n_bits)
    ids = np.zeros((b, top_k), np.uint64); dist = np.zeros((b, top_k), np.float32); cnt = np.full(b, 5, np.uint32)
    assert capi.lib().vers_ivf_search_filtered(ix._h, capi._ptr(Q), 4 * ix.d, b, top_k, 4, None, 0, capi._ptr(ids), capi._ptr(dist), capi._ptr(cnt)) == capi.OK
    assert not cnt.any()


# ---- 3. tile edges ----------------------------------------------------------------------------------------------------------------------
def test_tile_edges(main_ix):
    ix = main_ix
    n, k = 6000, ix.num_centroids
    Q = queries(ix, 0xF178, 9)
    lists = [ix.get_list(c)[1].astype(np.int64) for c in range(k)]
    for c in range(k):
        assert np.array_equal(lists[c], np.asarray(ix.ids[c], dtype=np.int64))
    rank = [[int(c) for c in co.search_exhaustive(ix.centroids, q, k, ix.metric)[0]] for q in Q]
    nprobe = 4
    # exactly list positions {0, 63, 64, 127, len - 1} of every list (each query's probed lists among them)
    edge = np.concatenate([l[[p for p in (0, 63, 64, 127, len(l) - 1) if p < len(l)]] for l in lists if len(l)])
    # one whole list and nothing else: the nearest list of query 0
    whole = lists[rank[0][0]]
    # everything but one whole probed list: the nearest list of query 0 again
    but_one = np.setdiff1d(np.arange(n), whole)
    for allowed in (edge, whole, but_one):
        ref = Ref(ix, Q, allowed_set(n, allowed, n))
        for qs in (list(range(9)), [0]):
            check_probed(ref, 10, nprobe, allowed, n, qs=qs)
            check_probed(ref, 100, nprobe, allowed, n, qs=qs)
            check_exhaustive(ref, 10, allowed, L2, n, qs=qs)
    # only rows of a list query 0 does not probe: count 0 for it, and for every query that does not probe it either
    far = lists[rank[0][-1]]
    ref = Ref(ix, Q, allowed_set(n, far, n))
    got = check_probed(ref, 10, nprobe, far, n)
    assert got[2][0] == 0
    assert check_probed(ref, 10, nprobe, far, n, qs=[0])[2][0] == 0


# ---- 4. bitmap edges -------------------------------------------------------------------------------------------------------------------
def test_bitmap_edges(main_ix):
    ix = main_ix
    n = 6000
    Q = queries(ix, 0xF179, 8)
    base = random_filter(n + 1000, 0.6, 0xF17A)
    base[[n - 2, n - 1]] = True   # (the last ids of the index are allowed whenever n_bits reaches them)
    for n_bits in (n - 1, n, n + 1, n + 1000, 64 * ((n + 63) // 64) - 1, n // 2):
        ref = Ref(ix, Q, allowed_set(n, base, n_bits))   # ids >= n_bits are not allowed; bits of ids >= n select nothing
        assert ref.sem[:min(n, n_bits)].sum() == base[:min(n, n_bits)].sum() and not ref.sem[min(n, n_bits):].any()
        check_probed(ref, 10, 4, base, n_bits)
        check_exhaustive(ref, 10, base, L2, n_bits)
        check_probed(ref, 10, 4, base, n_bits, qs=[3])
        # garbage in the last word beyond n_bits: every bit set
        words = capi.allowed_bitmap(base, n_bits)
        if n_bits % 64:
            words[-1] |= np.uint64(0xFFFFFFFFFFFFFFFF) << np.uint64(n_bits % 64)
        check_probed(ref, 10, 4, (words, n_bits))
        check_exhaustive(ref, 10, (words, n_bits))
    # all ones everywhere, n_bits = n - 1: the last id alone is out
    words = np.full((n + 63) // 64, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    sem = np.ones(n, dtype=bool); sem[n - 1] = False
    ref = Ref(ix, Q, sem)
    check_exhaustive(ref, 10, (words, n - 1))
    check_probed(ref, 64, 12, (words, n - 1))


# ---- 5. more than 64 tiles per item --------------------------------------------------------------------------------------------------------
def test_items_of_more_than_64_tiles():
    ix = make(12000, 32, 2, seed=0xF180)
    try:
        n = 12000
        lists = [ix.get_list(c)[1].astype(np.int64) for c in range(2)]
        assert max(len(l) for l in lists) > 4096 + 64   # the longer list reaches into a second window of 64 tiles (k-means decides the split)
        Q = queries(ix, 0xF181, 9)
        second = np.concatenate([l[4096:] for l in lists])                      # live tiles in the second window only (a shorter list: none)
        first = np.concatenate([l[:4096:7] for l in lists])                     # ... in the first only
        both = np.concatenate([np.concatenate([l[100:130], l[4090:4100], l[-3:]]) for l in lists])
        one_late = lists[0][-1:]                                                # a single row, in the last tile
        capi.set_option("seg_rows", 8192)
        for allowed in (second, first, both, one_late):
            ref = Ref(ix, Q, allowed_set(n, allowed, n))
            for qs in (list(range(9)), [0]):
                for nprobe in (1, 2):
                    check_probed(ref, 10, nprobe, allowed, n, qs=qs)
                check_probed(ref, 100, 2, allowed, n, qs=qs)
                check_exhaustive(ref, 10, allowed, L2, n, qs=qs)
                check_exhaustive(ref, 100, allowed, L2, n, qs=qs)
    finally:
        capi.set_option("seg_rows", 0)
        ix.close()


# ---- 6. more than 64 probes ------------------------------------------------------------------------------------------------------------
def test_more_than_64_probes():
    ix = make(4000, 16, 80, seed=0xF190)
    try:
        Q = queries(ix, 0xF191, 9)
        allowed = random_filter(4000, 0.3, 0xF192)
        ref = Ref(ix, Q, allowed)
        for qs in (list(range(9)), [5]):
            for top_k in (10, 100):
                check_probed(ref, top_k, 70, allowed, qs=qs)
    finally:
        ix.close()


# ---- 7. dimensions and the cosine metric ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 100, 320])
def test_dimensions(d):
    ix = make(1500, d, 6, seed=0xF1A0 + d)
    try:
        Q = queries(ix, 0xF1A1, 9)
        allowed = random_filter(1500, 0.4, 0xF1A2)
        ref = Ref(ix, Q, allowed)
        for qs in (list(range(9)), [1]):
            check_probed(ref, 10, 3, allowed, qs=qs)
            check_probed(ref, 70, 6, allowed, qs=qs)
            check_exhaustive(ref, 10, allowed, qs=qs)
    finally:
        ix.close()


def test_cosine_metric():
    ix = make(1500, 48, 6, metric=COS, seed=0xF1B0)
    try:
        Q = queries(ix, 0xF1B1, 9)
        allowed = random_filter(1500, 0.4, 0xF1B2)
        ref = Ref(ix, Q, allowed)
        for qs in (list(range(9)), [1]):
            check_probed(ref, 10, 3, allowed, qs=qs)
            check_probed(ref, 70, 6, allowed, qs=qs)
            for metric in (L2, COS):
                check_exhaustive(ref, 10, allowed, metric, qs=qs)
    finally:
        ix.close()


# ---- 8. virtual removal, GPU against GPU ----------------------------------------------------------------------------------------------------
def test_filter_equals_removal_on_a_second_index(main_ix):
    ix = main_ix
    n = 6000
    Q = queries(ix, 0xF1C0, 17)
    allowed = random_filter(n, 0.3, 0xF1C1)
    other = clone(ix)
    try:
        other.remove_batch(np.flatnonzero(~allowed).astype(np.uint64))
        for Qs in (Q, Q[:1]):
            for nprobe in (1, 4, 12):
                for top_k in (10, 100):
                    i0, d0, c0 = other.search_batch(Qs, top_k, nprobe)
                    i1, d1, c1 = ix.search_filtered(Qs, top_k, nprobe, allowed)
                    assert np.array_equal(c0, c1), (nprobe, top_k)
                    for q in range(len(c0)):
                        assert np.array_equal(i0[q, :c0[q]], i1[q, :c0[q]]) and np.array_equal(bits(d0[q, :c0[q]]), bits(d1[q, :c0[q]])), (nprobe, top_k, q)
            for top_k in (10, 100):
                i0, d0, c0 = other.search_exhaustive(Qs, top_k)
                i1, d1, c1 = ix.search_exhaustive_filtered(Qs, top_k, allowed)
                assert np.array_equal(c0, c1) and np.array_equal(i0, i1) and np.array_equal(bits(d0), bits(d1)), top_k
    finally:
        other.close()


# ---- 9. a mutated index ----------------------------------------------------------------------------------------------------------------------
def test_mutated_index():
    ix = make(3000, 64, 8, seed=0xF1D0)
    try:
        Q = queries(ix, 0xF1D1, 9)
        new_rows = dg.dist_c(0xF1D2, 500, 64, 16, dg.default_sigma(64))
        ix.add_batch(new_rows)
        n = 3500
        allowed = random_filter(n, 0.5, 0xF1D3)
        allowed[3000:3100] = True   # new ids among the allowed
        ref = Ref(ix, Q, allowed)
        assert ref.sem[3000:].sum() >= 100
        check_probed(ref, 10, 4, allowed); check_probed(ref, 100, 8, allowed); check_exhaustive(ref, 100, allowed); check_probed(ref, 10, 4, allowed, qs=[2])
        gone = np.flatnonzero(allowed)[::3].astype(np.uint64)   # removed ids stay in the filter: they select nothing
        ix.remove_batch(gone)
        ref = Ref(ix, Q, allowed)
        assert ref.rows.size == int(allowed.sum()) - gone.size
        before = [check_probed(ref, 10, 4, allowed), check_probed(ref, 100, 8, allowed), check_exhaustive(ref, 100, allowed), check_probed(ref, 10, 4, allowed, qs=[2])]
        ix.compact()
        after = [check_probed(ref, 10, 4, allowed), check_probed(ref, 100, 8, allowed), check_exhaustive(ref, 100, allowed), check_probed(ref, 10, 4, allowed, qs=[2])]
        for (i0, d0, c0), (i1, d1, c1) in zip(before, after):
            assert np.array_equal(c0, c1)
            for q in range(len(c0)):
                assert np.array_equal(i0[q, :c0[q]], i1[q, :c0[q]]) and np.array_equal(bits(d0[q, :c0[q]]), bits(d1[q, :c0[q]]))
    finally:
        ix.close()


# ---- 10. NaN -----------------------------------------------------------------------------------------------------------------------------
def test_nan_row_outside_the_filter_is_not_scanned():
    src = make(1500, 48, 6, seed=0xF1E0)
    ix = IVFFlatIndex(48)
    try:
        bad = int(src.ids[2][70])   # a row in the second tile of list 2
        ix.num_centroids, ix.centroids, ix.assignments, ix.ids = src.num_centroids, src.centroids, src.assignments, [list(l) for l in src.ids]
        ix.values = src.values.copy()
        ix.values[bad, 7] = np.nan
        ix._upload()
        Q = queries(src, 0xF1E1, 9)
        allowed = random_filter(1500, 0.5, 0xF1E2)
        allowed[[int(v) for v in src.ids[2][64:128]]] = True   # the rest of its tile is allowed: the tile IS loaded
        allowed[bad] = False
        ref = Ref(ix, Q, allowed)
        for qs in (list(range(9)), [0]):
            check_probed(ref, 10, 6, allowed, qs=qs)
            check_exhaustive(ref, 10, allowed, qs=qs)
        allowed[bad] = True
        for Qs in (Q, Q[:1]):
            with pytest.raises(capi.VersError) as e:
                ix.search_filtered(Qs, 10, 6, allowed)
            assert e.value.status == capi.ERR_NAN
            with pytest.raises(capi.VersError) as e:
                ix.search_exhaustive_filtered(Qs, 10, allowed)
            assert e.value.status == capi.ERR_NAN
        allowed[bad] = False   # and the handle is still usable
        check_probed(ref, 10, 6, allowed)
    finally:
        ix.close()
        src.close()


# ---- 11. errors and protocol ---------------------------------------------------------------------------------------------------------------
def raw(ix, Q, top_k, nprobe_or_metric, words, n_bits, probed=True):
    Q = np.ascontiguousarray(np.atleast_2d(Q), dtype=np.float32)
    b = Q.shape[0]
    ids = np.zeros((b, max(top_k, 1)), np.uint64); dist = np.zeros((b, max(top_k, 1)), np.float32); cnt = np.full(b, 99, np.uint32)
    fn = capi.lib().vers_ivf_search_filtered if probed else capi.lib().vers_ivf_search_exhaustive_filtered
    rc = fn(ix._h, capi._ptr(Q), 4 * ix.d, b, top_k, nprobe_or_metric, capi._ptr(words) if words is not None else None, n_bits, capi._ptr(ids), capi._ptr(dist),
            capi._ptr(cnt))
    return rc, cnt


def test_errors_and_protocol(main_ix):
    import torch
    ix = main_ix
    Q = queries(ix, 0xF1F0, 8)
    words = capi.allowed_bitmap(np.ones(6000, dtype=bool), 6000)
    assert raw(ix, Q, 10, 4, words, 6000)[0] == capi.OK
    assert raw(ix, Q, 10, 0, words, 6000)[0] == capi.ERR_INVALID                 # nprobe == 0
    assert raw(ix, Q, 10, 4, None, 6000)[0] == capi.ERR_INVALID                  # n_bits > 0 with a NULL bitmap
    assert raw(ix, Q, 10, L2, None, 6000, probed=False)[0] == capi.ERR_INVALID
    assert raw(ix, Q, 10, 2, words, 6000, probed=False)[0] == capi.ERR_INVALID   # metric > VERS_METRIC_COSDIST
    dev = torch.device("cuda", ix.device)
    qd = torch.from_numpy(Q).to(dev); wd = torch.from_numpy(words.view(np.int64)).to(dev)
    oi = torch.zeros((8, 10), dtype=torch.int64, device=dev); od = torch.zeros((8, 10), dtype=torch.float32, device=dev); oc = torch.zeros(8, dtype=torch.int32, device=dev)
    for args in ((10, 0, wd.data_ptr(), 6000), (10, 4, 0, 6000)):
        with pytest.raises(capi.VersError) as e:
            ix.search_filtered_dev(qd.data_ptr(), ix.d, 8, args[0], args[1], args[2], args[3], oi.data_ptr(), od.data_ptr(), oc.data_ptr())
        assert e.value.status == capi.ERR_INVALID
    for metric, ptr in ((2, wd.data_ptr()), (L2, 0)):
        with pytest.raises(capi.VersError) as e:
            ix.search_exhaustive_filtered_dev(qd.data_ptr(), ix.d, 8, 10, metric, ptr, 6000, oi.data_ptr(), od.data_ptr(), oc.data_ptr())
        assert e.value.status == capi.ERR_INVALID
    # top_k == 0: counts 0; b == 0: a no-op
    rc, cnt = raw(ix, Q, 0, 4, words, 6000)
    assert rc == capi.OK and not cnt.any()
    rc, cnt = raw(ix, Q, 0, L2, words, 6000, probed=False)
    assert rc == capi.OK and not cnt.any()
    Lb = capi.lib()
    assert Lb.vers_ivf_search_filtered(ix._h, None, 4 * ix.d, 0, 10, 4, capi._ptr(words), 6000, None, None, None) == capi.OK
    assert Lb.vers_ivf_search_exhaustive_filtered(ix._h, None, 4 * ix.d, 0, 10, L2, capi._ptr(words), 6000, None, None, None) == capi.OK
    assert Lb.vers_ivf_search_filtered_dev(ix._h, None, ix.d, 0, 10, 4, None, 0, None, None, None, None) == capi.OK
    assert Lb.vers_ivf_search_exhaustive_filtered_dev(ix._h, None, ix.d, 0, 10, L2, None, 0, None, None, None, None) == capi.OK
    # an index without centroids: the probed call has nothing to rank, the exhaustive call counts 0
    empty = IVFFlatIndex(ix.d)
    assert raw(empty, Q, 10, 4, words, 6000)[0] == capi.ERR_INSUFFICIENT
    rc, cnt = raw(empty, Q, 10, L2, words, 6000, probed=False)
    assert rc == capi.OK and not cnt.any()
    empty.close()
    # a streamed upload in progress is seen as an empty index
    sh = make(600, 32, 4, seed=0xF1F1)
    Qs = queries(sh, 0xF1F2, 3)
    w600 = capi.allowed_bitmap(np.ones(600, dtype=bool), 600)
    up = IVFFlatIndex(sh.d)
    up.upload_begin(sh.centroids, [len(l) for l in sh.ids], 600)
    assert raw(up, Qs, 10, 2, w600, 600)[0] == capi.ERR_INSUFFICIENT
    rc, cnt = raw(up, Qs, 10, L2, w600, 600, probed=False)
    assert rc == capi.OK and not cnt.any()
    up.close()
    # a handle sharded by cluster
    half = IVFFlatIndex(sh.d)
    half.set_shard(0, 2)
    half.num_centroids, half.values, half.centroids, half.assignments = sh.num_centroids, sh.values, sh.centroids, sh.assignments
    half._upload()
    assert raw(sh, Qs, 10, 2, w600, 600)[0] == capi.OK
    assert half.info()[1] == 4 and raw(half, Qs, 10, 2, w600, 600)[0] == capi.ERR_INVALID
    assert raw(half, Qs, 10, L2, w600, 600, probed=False)[0] == capi.ERR_INVALID
    half.close()
    sh.close()


def test_device_pointer_calls_on_two_streams(main_ref):
    import torch
    ref, allowed = main_ref
    ix = ref.ix
    b = 17
    Q = ref.Q[:b]
    words = capi.allowed_bitmap(allowed, 6000)
    dev = torch.device("cuda", ix.device)
    qd = torch.from_numpy(Q).to(dev); wd = torch.from_numpy(words.view(np.int64)).to(dev)
    outs = []
    for stream in (torch.cuda.Stream(dev), torch.cuda.Stream(dev)):
        for top_k in (10, 100):
            for call in ("probed", "exhaustive"):
                ids = torch.full((b, top_k), -1, dtype=torch.int64, device=dev)
                dist = torch.full((b, top_k), -7.25, dtype=torch.float32, device=dev)
                cnt = torch.zeros(b, dtype=torch.int32, device=dev)
                torch.cuda.synchronize(dev)
                if call == "probed":
                    ix.search_filtered_dev(qd.data_ptr(), ix.d, b, top_k, 4, wd.data_ptr(), 6000, ids.data_ptr(), dist.data_ptr(), cnt.data_ptr(), stream.cuda_stream)
                else:
                    ix.search_exhaustive_filtered_dev(qd.data_ptr(), ix.d, b, top_k, L2, wd.data_ptr(), 6000, ids.data_ptr(), dist.data_ptr(), cnt.data_ptr(),
                                                      stream.cuda_stream)
                ix.poll(stream.cuda_stream)
                got = (ids.cpu().numpy().astype(np.uint64), dist.cpu().numpy(), cnt.cpu().numpy().astype(np.uint32))
                same(got, (lambda q: ref.probed(q, 4)) if call == "probed" else (lambda q: ref.exhaustive(q, L2)), list(range(b)), top_k, (call, top_k))
                outs.append(got)
    half = len(outs) // 2
    for (i0, d0, c0), (i1, d1, c1) in zip(outs[:half], outs[half:]):
        assert np.array_equal(c0, c1) and np.array_equal(i0, i1) and np.array_equal(bits(d0), bits(d1))


def test_nan_on_the_device_pointer_call_latches_for_poll(main_ref):
    import torch
    ref, allowed = main_ref
    ix = ref.ix
    Q = ref.Q[:8].copy(); Q[2, 5] = np.nan
    words = capi.allowed_bitmap(allowed, 6000)
    dev = torch.device("cuda", ix.device)
    qd = torch.from_numpy(Q).to(dev); wd = torch.from_numpy(words.view(np.int64)).to(dev)
    ids = torch.zeros((8, 10), dtype=torch.int64, device=dev); dist = torch.zeros((8, 10), dtype=torch.float32, device=dev); cnt = torch.zeros(8, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    ix.search_exhaustive_filtered_dev(qd.data_ptr(), ix.d, 8, 10, L2, wd.data_ptr(), 6000, ids.data_ptr(), dist.data_ptr(), cnt.data_ptr())
    with pytest.raises(capi.VersError) as e:
        ix.poll()
    assert e.value.status == capi.ERR_NAN
    ix.poll()   # (cleared)


def test_unfiltered_search_is_unchanged_around_a_filtered_call(main_ref):
    """the workspace lease is clean: the same top-k batch before and after filtered calls returns the same bits"""
    ref, allowed = main_ref
    ix = ref.ix
    Q = ref.Q
    shapes = ((10, 4), (10, 0), (100, 4))
    before = [ix.search_batch(Q, top_k, nprobe) for top_k, nprobe in shapes] + [ix.search_batch(Q[0], 10, 4), ix.search_exhaustive(Q[:9], 10)]
    check_probed(ref, 10, 4, allowed); check_probed(ref, 100, 12, allowed, qs=[0]); check_exhaustive(ref, 70, allowed)
    after = [ix.search_batch(Q, top_k, nprobe) for top_k, nprobe in shapes] + [ix.search_batch(Q[0], 10, 4), ix.search_exhaustive(Q[:9], 10)]
    for (i0, d0, c0), (i1, d1, c1) in zip(before, after):
        assert np.array_equal(c0, c1)
        for q in range(len(c0)):
            assert np.array_equal(i0[q, :c0[q]], i1[q, :c0[q]]) and np.array_equal(bits(d0[q, :c0[q]]), bits(d1[q, :c0[q]]))


# ---- 12. the stats hook ----------------------------------------------------------------------------------------------------------------------
def test_stats_hook(main_ix):
    ix = main_ix
    n, k = 6000, ix.num_centroids
    Q = queries(ix, 0xF200, 1)
    rank = [int(c) for c in co.search_exhaustive(ix.centroids, Q[0], k, ix.metric)[0]]
    lists = [ix.get_list(c)[1].astype(np.int64) for c in range(k)]
    tiles = lambda c: (len(lists[c]) + 63) // 64
    nprobe = 4
    probed = rank[:nprobe]
    live = sum(len(l) for l in lists)
    capi.set_option("seg_rows", 64)   # b == 1, 64-row segments: a work item is one tile of one probed list
    try:
        t0 = ix.filter_stats()["total"]
        # only one list allowed: the nearest one, whole
        c = probed[0]
        ref = Ref(ix, Q, allowed_set(n, lists[c], n))
        check_probed(ref, 10, nprobe, lists[c], n)
        st = ix.filter_stats()["last"]
        planned = sum(tiles(p) for p in probed)
        assert st == dict(tiles_planned=planned, tiles_loaded=tiles(c), items_skipped=planned - tiles(c), rows_allowed=len(lists[c])), st
        assert st["items_skipped"] > 0
        # a few positions of that list: the tiles that hold an allowed row are loaded, the others are not
        pos = [p for p in (0, 5, 63, 200, 201, len(lists[c]) - 1)]
        some = lists[c][pos]
        ref = Ref(ix, Q, allowed_set(n, some, n))
        check_probed(ref, 10, nprobe, some, n)
        st = ix.filter_stats()["last"]
        held = len({p // 64 for p in pos})
        assert st == dict(tiles_planned=planned, tiles_loaded=held, items_skipped=planned - held, rows_allowed=len(pos)), st
        # everything allowed
        everything = np.ones(n, dtype=bool)
        ref = Ref(ix, Q, everything)
        check_probed(ref, 10, nprobe, everything)
        st = ix.filter_stats()["last"]
        assert st == dict(tiles_planned=planned, tiles_loaded=planned, items_skipped=0, rows_allowed=live), st
        t1 = ix.filter_stats()["total"]
        assert t1["tiles_planned"] - t0["tiles_planned"] == 3 * planned
        assert t1["tiles_loaded"] - t0["tiles_loaded"] == tiles(c) + held + planned
        assert t1["rows_allowed"] - t0["rows_allowed"] == len(lists[c]) + len(pos) + live
        # the exhaustive call over 64-row segments: an item is one storage tile
        check_exhaustive(ref, 10, everything)
        st = ix.filter_stats()["last"]
        assert st["tiles_loaded"] == sum(tiles(p) for p in range(k)) and st["rows_allowed"] == live and st["tiles_planned"] >= st["tiles_loaded"]
        assert st["items_skipped"] == st["tiles_planned"] - st["tiles_loaded"]   # (storage slack: tiles that hold no vector at all)
    finally:
        capi.set_option("seg_rows", 0)


# ---- 13. the C++ mirror --------------------------------------------------------------------------------------------------------------------
def test_cpp_host_mirror_filtered_search(tmp_path):
    """vers_amd/host/ivfflat.hpp's search_filtered() / search_exhaustive_filtered() from compiled code (tests/cpp/filtered_demo.cpp) against the
    Python mirror's result"""
    lib = capi.LIB_PATH
    exe = str(tmp_path / "filtered_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + ROOT, "-o", exe, os.path.join(ROOT, "tests", "cpp", "filtered_demo.cpp"),
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
        top_k = 10 + 30 * q
        for mode in (0, 1):
            ids, dist, cnt = ix.search_filtered(X[q * 31], top_k, 3, allowed) if mode == 0 else ix.search_exhaustive_filtered(X[q * 31], top_k, allowed)
            assert got.get((q, mode), []) == list(zip(ids[0, :cnt[0]].tolist(), bits(dist[0, :cnt[0]]).tolist())), (q, mode)
            n_rows += int(cnt[0])
    assert n_rows > 12
    ix.close()
