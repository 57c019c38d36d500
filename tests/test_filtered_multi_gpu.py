"""vers_ivf_search_filtered_multi / vers_ivf_search_exhaustive_filtered_multi (+ _dev): one batch whose queries use different bitmaps.
Nothing new in the semantics -- row q is row q of the per-call filtered search made with bitmap filter_of[q] -- so every case is checked twice,
and every comparison is np.array_equal on the ids, on the distances' u32 BITS and on out_count, no tolerance:
  * against the oracle of tests/test_filtered_gpu.py (restated here): co.search_nprobe / co.search_exhaustive over the list ids retained by
    the query's OWN bitmap, the full order computed once per (index, queries, bitmap, nprobe) and cut to each top_k;
  * against the per-call GPU call (search_filtered / search_exhaustive_filtered), made once per distinct bitmap with the same queries.
Not covered: the exhaustive call's "batch too large" refusal, which needs 2^32 (query, segment) slots, as in the per-call suite."""
import ctypes as C

import numpy as np
import pytest

from oracle import c_oracle as co
from tests import datagen as dg
from tests.golden import make_golden as mg
from vers_amd import capi
from vers_amd.index import IVFFlatIndex

pytestmark = pytest.mark.gpu

L2, COS = capi.METRIC_L2SQ, capi.METRIC_COSDIST
ONES = np.uint64(0xFFFFFFFFFFFFFFFF)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def make(n, d, k, metric=L2, seed=0xF170, iters=4):
    X = dg.dist_c(seed, n, d, 2 * k, dg.default_sigma(d))
    init = mg.init_draws(seed + 1, 1, k, n)
    return IVFFlatIndex.build_index(k, 1, iters, X, init_indices=init, metric=metric)


def queries(ix, seed, b):
    d, k = ix.d, ix.num_centroids
    return dg.dist_c(seed, b, d, 2 * k, dg.default_sigma(d))


def allowed_set(n, allowed, n_bits):
    """The defined semantics, restated: bool [n], entry v = vec id v is allowed.  allowed: a bool array or an id array."""
    a = np.asarray(allowed)
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


class Case:
    """(index, queries, the call's bitmaps): an oracle Ref per bitmap and the per-call GPU results, each computed once.  words: the packed
    bitmaps handed to the GPU, when they are not simply capi.allowed_bitmaps(allowed, n_bits) (garbage beyond n_bits, a larger stride)."""

    def __init__(self, ix, Q, allowed, n_bits, n, words=None):
        self.ix, self.Q, self.n_bits = ix, np.atleast_2d(Q), int(n_bits)
        self.words = capi.allowed_bitmaps(allowed, n_bits) if words is None else words
        self.refs = [Ref(ix, self.Q, allowed_set(n, a, n_bits)) for a in allowed]
        self._one = {}

    def fresh(self):
        """forget the per-call GPU results (an option that changes the plan was set)"""
        self._one = {}
        return self

    def per_call(self, f, qs, top_k, arg, probed):
        key = (f, tuple(qs), top_k, arg, probed)
        if key not in self._one:
            one = (self.words[f], self.n_bits)
            self._one[key] = (self.ix.search_filtered(self.Q[qs], top_k, arg, one) if probed
                              else self.ix.search_exhaustive_filtered(self.Q[qs], top_k, one, arg))
        return self._one[key]


def same_rows(a, b, rows, what):
    (i0, d0, c0), (i1, d1, c1) = a, b
    assert np.array_equal(c0[rows], c1[rows]), (what, "counts")
    for i in rows:
        c = int(c0[i])
        assert np.array_equal(i0[i, :c], i1[i, :c]) and np.array_equal(bits(d0[i, :c]), bits(d1[i, :c])), (what, int(i))


def check(case, fo, top_k, arg, probed=True, qs=None, cross=True):
    """one multi call over queries qs with filter_of fo (one entry per entry of qs), against the oracle and against the per-call GPU call"""
    qs = list(range(case.Q.shape[0])) if qs is None else list(qs)
    fo = np.asarray(fo, dtype=np.uint32).reshape(-1)
    assert fo.size == len(qs)
    what = ("probed" if probed else "exhaustive", top_k, arg, fo.tolist())
    filters = (case.words, case.n_bits)
    got = (case.ix.search_filtered_multi(case.Q[qs], top_k, arg, filters, fo) if probed
           else case.ix.search_exhaustive_filtered_multi(case.Q[qs], top_k, filters, fo, arg))
    ids, dist, cnt = got
    for i, q in enumerate(qs):
        ref = case.refs[fo[i]]
        ei, ed = ref.probed(q, arg) if probed else ref.exhaustive(q, arg)
        ei, ed = ei[:top_k], ed[:top_k]
        assert cnt[i] == ei.size, (what, q, int(cnt[i]), ei.size)
        assert np.array_equal(ids[i, :cnt[i]], ei), (what, q, "ids")
        assert np.array_equal(bits(dist[i, :cnt[i]]), bits(ed)), (what, q, "distance bits")
    if cross:
        for f in np.unique(fo):
            same_rows(got, case.per_call(int(f), qs, top_k, arg, probed), np.flatnonzero(fo == f), what + (int(f),))
    return got


def random_filter(n, sel, seed):
    return np.random.default_rng(seed).random(n) < sel


def patterns(b, F, seed):
    """filter_of patterns over b queries and F bitmaps: all equal, alternating, every query its own (cycling in reverse beyond F), sorted
    blocks, random"""
    q = np.arange(b)
    return {"equal": np.full(b, F - 1), "alternating": q % F, "own": (F - 1) - (q % F), "blocks": (q * F) // b,
            "random": np.random.default_rng(seed).integers(0, F, b)}


N_MAIN = 6000


@pytest.fixture(scope="module")
def main_ix():
    ix = make(N_MAIN, 96, 12)
    yield ix
    ix.close()


@pytest.fixture(scope="module")
def main_case(main_ix):
    """40 queries and five random bitmaps at selectivity 0.5, shared by the cases that need no other"""
    Q = queries(main_ix, 0xF171, 40)
    allowed = [random_filter(N_MAIN, 0.5, 0xF300 + f) for f in range(5)]
    return Case(main_ix, Q, allowed, N_MAIN, N_MAIN)


# ---- 1. group widths, segments, passes and filter_of patterns ---------------------------------------------------------------------------
@pytest.mark.parametrize("seg_rows", [0, 64])
@pytest.mark.parametrize("b", [1, 3, 8, 9, 17, 40])
def test_group_widths_segments_passes_and_patterns(main_case, b, seg_rows):
    case = main_case.fresh()
    qs = list(range(b))
    capi.set_option("seg_rows", seg_rows)
    try:
        for F in (1, 2, 5):   # (the call's bitmaps are the five; filter_of uses the first F)
            for name, fo in patterns(b, F, 0xF310 + b).items():
                if F == 1 and name != "equal":
                    continue
                for nprobe in (1, 4, 12):
                    for top_k in (1, 10, 64, 65, 200):
                        check(case, fo, top_k, nprobe, qs=qs)
                for top_k in (1, 10, 64, 65, 200):
                    check(case, fo, top_k, L2, probed=False, qs=qs)
    finally:
        capi.set_option("seg_rows", 0)
        main_case.fresh()


def test_python_mirror_takes_a_list_of_filters(main_case):
    case = main_case
    allowed = [r.sem for r in case.refs[:3]]
    fo = np.arange(9) % 3
    got = case.ix.search_filtered_multi(case.Q[:9], 10, 4, allowed, fo)
    same_rows(got, check(case, fo, 10, 4, qs=range(9)), np.arange(9), "list of bool arrays")
    got = case.ix.search_exhaustive_filtered_multi(case.Q[:9], 10, [np.flatnonzero(a) for a in allowed], fo, n_bits=N_MAIN)
    same_rows(got, check(case, fo, 10, L2, probed=False, qs=range(9)), np.arange(9), "list of id arrays")


# ---- 2. disjoint tenants, an empty and an all-ones bitmap in one batch --------------------------------------------------------------------
def test_disjoint_tenants_empty_and_all_ones(main_ix):
    ix, n = main_ix, N_MAIN
    Q = queries(ix, 0xF320, 17)
    tenants = [np.arange(f * 1200, (f + 1) * 1200) for f in range(5)]   # contiguous id ranges: a tile is live for few queries of a group
    allowed = tenants + [np.zeros(0, dtype=np.int64), np.ones(n, dtype=bool)]
    case = Case(ix, Q, allowed, n, n)
    fo = np.arange(17) % 7
    for seg_rows in (0, 64):
        capi.set_option("seg_rows", seg_rows)
        case.fresh()
        try:
            for nprobe, top_k in ((4, 10), (12, 10), (12, 100), (1, 64)):
                ids, dist, cnt = check(case, fo, top_k, nprobe)
                assert not cnt[fo == 5].any() and cnt[fo == 6].all()
                # a tenant's query sees its own ids only, whatever its group's neighbours were allowed
                for i in np.flatnonzero(fo < 5):
                    got = ids[i, :cnt[i]]
                    assert ((got >= fo[i] * 1200) & (got < (fo[i] + 1) * 1200)).all()
            ids, dist, cnt = check(case, fo, 100, L2, probed=False)
            assert not cnt[fo == 5].any() and (cnt[fo != 5] == 100).all()
            check(case, fo[5:7], 10, 12, qs=[5, 6])   # the empty filter and all ones, side by side in one group
        finally:
            capi.set_option("seg_rows", 0)


# ---- 3. every bit position ------------------------------------------------------------------------------------------------------------------
def test_sixty_four_filters(main_ix):
    ix, n = main_ix, N_MAIN
    Q = queries(ix, 0xF330, 64)
    allowed = [np.arange(f, n, 64) for f in range(64)]
    case = Case(ix, Q, allowed, n, n)
    fo = np.arange(64)
    check(case, fo, 10, 4)
    check(case, fo[::-1], 70, 12)
    check(case, fo, 10, L2, probed=False)
    check(case, [63], 10, 4, qs=[7])


# ---- 4. tile and bitmap edges -----------------------------------------------------------------------------------------------------------
def test_tile_edges_split_across_two_bitmaps(main_ix):
    ix, n = main_ix, N_MAIN
    Q = queries(ix, 0xF340, 9)
    lists = [np.asarray(l, dtype=np.int64) for l in ix.ids]
    a = np.concatenate([l[[p for p in (0, 64, len(l) - 1) if p < len(l)]] for l in lists if len(l)])
    b = np.concatenate([l[[p for p in (63, 127) if p < len(l)]] for l in lists if len(l)])
    case = Case(ix, Q, [a, b], n, n)
    for fo in (np.arange(9) % 2, (np.arange(9) + 1) % 2):
        check(case, fo, 10, 4)
        check(case, fo, 100, 12)
        check(case, fo, 10, L2, probed=False)
    check(case, [1], 10, 4, qs=[3])


@pytest.mark.parametrize("n_bits", [N_MAIN - 1, N_MAIN, N_MAIN + 1, N_MAIN // 2])
def test_bitmap_edges_garbage_and_stride(main_ix, n_bits):
    ix, n = main_ix, N_MAIN
    Q = queries(ix, 0xF350, 8)
    allowed = [random_filter(n + 64, 0.6, 0xF351 + f) for f in range(3)]
    for a in allowed:
        a[[n - 2, n - 1]] = True   # the last ids of the index are allowed whenever n_bits reaches them
    need = (n_bits + 63) // 64
    fo = np.arange(8) % 3
    for stride in (need, need + 3):
        words = capi.allowed_bitmaps(allowed, n_bits, stride)
        if n_bits % 64:   # garbage in each bitmap's last word beyond n_bits: every bit set
            words[:, need - 1] |= ONES << np.uint64(n_bits % 64)
        words[:, need:] = ONES   # ... and in the padding of a larger stride
        case = Case(ix, Q, allowed, n_bits, n, words=words)
        for r, a in zip(case.refs, allowed):
            assert r.sem[:min(n, n_bits)].sum() == a[:min(n, n_bits)].sum() and not r.sem[min(n, n_bits):].any()
        check(case, fo, 10, 4)
        check(case, fo, 10, L2, probed=False)
        check(case, [2], 10, 4, qs=[3])


# ---- 5. more than 64 tiles per item ------------------------------------------------------------------------------------------------------
def test_items_of_more_than_64_tiles():
    ix = make(12000, 32, 2, seed=0xF180)
    try:
        n = 12000
        lists = [np.asarray(l, dtype=np.int64) for l in ix.ids]
        assert max(len(l) for l in lists) > 4096 + 64   # the longer list reaches into a second window of 64 tiles
        Q = queries(ix, 0xF181, 9)
        first = np.concatenate([l[:4096:7] for l in lists])    # live tiles in the first window only
        second = np.concatenate([l[4096:] for l in lists])     # ... in the second only
        case = Case(ix, Q, [first, second], n, n)
        capi.set_option("seg_rows", 8192)
        for fo in (np.arange(9) % 2, np.zeros(9, int), np.ones(9, int)):
            for nprobe in (1, 2):
                check(case, fo, 10, nprobe)
            check(case, fo, 100, 2)
            check(case, fo, 10, L2, probed=False)
            check(case, fo, 100, L2, probed=False)
        for f in (0, 1):
            check(case, [f], 10, 2, qs=[0])
            check(case, [f], 10, L2, probed=False, qs=[0])
    finally:
        capi.set_option("seg_rows", 0)
        ix.close()


# ---- 6. more than 64 probes, dimensions, the cosine metric -----------------------------------------------------------------------------------
def test_more_than_64_probes():
    ix = make(4000, 16, 80, seed=0xF190)
    try:
        Q = queries(ix, 0xF191, 9)
        case = Case(ix, Q, [random_filter(4000, 0.3, 0xF192 + f) for f in range(3)], 4000, 4000)
        for top_k in (10, 100):
            check(case, np.arange(9) % 3, top_k, 70)
            check(case, [2], top_k, 70, qs=[5])
    finally:
        ix.close()


@pytest.mark.parametrize("d", [1, 100, 320])
def test_dimensions(d):
    ix = make(1500, d, 6, seed=0xF1A0 + d)
    try:
        Q = queries(ix, 0xF1A1, 9)
        case = Case(ix, Q, [random_filter(1500, 0.4, 0xF1A2 + f) for f in range(3)], 1500, 1500)
        fo = np.arange(9) % 3
        check(case, fo, 10, 3)
        check(case, fo, 70, 6)
        check(case, fo, 10, L2, probed=False)
        check(case, [1], 10, 3, qs=[1])
    finally:
        ix.close()


def test_cosine_metric():
    ix = make(1500, 48, 6, metric=COS, seed=0xF1B0)
    try:
        Q = queries(ix, 0xF1B1, 9)
        case = Case(ix, Q, [random_filter(1500, 0.4, 0xF1B2 + f) for f in range(3)], 1500, 1500)
        fo = np.arange(9) % 3
        check(case, fo, 10, 3)
        check(case, fo, 70, 6)
        for metric in (L2, COS):
            check(case, fo, 10, metric, probed=False)
        check(case, [1], 10, 3, qs=[1])
    finally:
        ix.close()


# ---- 7. a mutated index ---------------------------------------------------------------------------------------------------------------------
def test_mutated_index():
    ix = make(3000, 64, 8, seed=0xF1D0)
    try:
        Q = queries(ix, 0xF1D1, 9)
        fo = np.arange(9) % 3
        ix.add_batch(dg.dist_c(0xF1D2, 500, 64, 16, dg.default_sigma(64)))
        n = 3500
        allowed = [random_filter(n, 0.5, 0xF1D3 + f) for f in range(3)]
        allowed[1][3000:3100] = True   # new ids among the allowed

        def all_checks():
            case = Case(ix, Q, allowed, n, n)
            return [check(case, fo, 10, 4), check(case, fo, 100, 8), check(case, fo, 100, L2, probed=False), check(case, [1], 10, 4, qs=[2])]

        all_checks()
        gone = np.flatnonzero(allowed[0] | allowed[1])[::3].astype(np.uint64)   # removed ids stay set in the bitmaps: they select nothing
        ix.remove_batch(gone)
        before = all_checks()
        ix.compact()
        after = all_checks()
        for g0, g1 in zip(before, after):
            same_rows(g0, g1, np.arange(len(g0[2])), "compact")
    finally:
        ix.close()


# ---- 8. NaN ----------------------------------------------------------------------------------------------------------------------------------
def test_nan_counts_only_for_the_queries_allowed_the_row():
    src = make(1500, 48, 6, seed=0xF1E0)
    ix = IVFFlatIndex(48)
    try:
        bad = int(src.ids[2][70])   # a row in the second tile of list 2
        ix.num_centroids, ix.centroids, ix.assignments, ix.ids = src.num_centroids, src.centroids, src.assignments, [list(l) for l in src.ids]
        ix.values = src.values.copy()
        ix.values[bad, 7] = np.nan
        ix._upload()
        Q = queries(src, 0xF1E1, 9)
        clean = random_filter(1500, 0.5, 0xF1E2)
        clean[[int(v) for v in src.ids[2][64:128]]] = True   # the rest of its tile is allowed: the tile IS loaded
        clean[bad] = False
        dirty = clean.copy()
        dirty[bad] = True
        case = Case(ix, Q, [dirty, clean], 1500, 1500)
        ones = np.ones(9, int)
        # the NaN row is allowed by bitmap 0 alone, and no query uses bitmap 0
        for qs in (list(range(9)), [0]):
            check(case, ones[:len(qs)], 10, 6, qs=qs)
            check(case, ones[:len(qs)], 10, L2, probed=False, qs=qs)
        # ... or only a query that does not probe its list (nprobe 1; no per-call cross-check: that call scans it for the other queries)
        far = next(q for q in range(9) if int(co.search_exhaustive(ix.centroids, Q[q], 6, ix.metric)[0][0]) != 2)
        fo = ones.copy(); fo[far] = 0
        check(case, fo, 10, 1, cross=False)
        # one query on bitmap 0 and probing the list: VERS_ERR_NAN, on both calls, batch and single
        for qs, f in ((list(range(9)), fo), ([far], [0])):
            for call in (lambda: ix.search_filtered_multi(Q[qs], 10, 6, (case.words, 1500), f),
                         lambda: ix.search_exhaustive_filtered_multi(Q[qs], 10, (case.words, 1500), f)):
                with pytest.raises(capi.VersError) as e:
                    call()
                assert e.value.status == capi.ERR_NAN
        check(case, ones, 10, 6)   # and the handle is still usable
    finally:
        ix.close()
        src.close()


# ---- 9. errors and protocol -------------------------------------------------------------------------------------------------------------------
def raw(ix, Q, top_k, arg, words, stride, n_filters, n_bits, fo, probed=True):
    Q = np.ascontiguousarray(np.atleast_2d(Q), dtype=np.float32)
    b = Q.shape[0]
    ids = np.zeros((b, max(top_k, 1)), np.uint64); dist = np.zeros((b, max(top_k, 1)), np.float32); cnt = np.full(b, 99, np.uint32)
    fn = capi.lib().vers_ivf_search_filtered_multi if probed else capi.lib().vers_ivf_search_exhaustive_filtered_multi
    rc = fn(ix._h, capi._ptr(Q), 4 * ix.d, b, top_k, arg, capi._ptr(words) if words is not None else None, stride, n_filters, n_bits,
            capi._ptr(fo) if fo is not None else None, capi._ptr(ids), capi._ptr(dist), capi._ptr(cnt))
    return rc, cnt


def test_errors(main_ix):
    import torch
    ix, n = main_ix, N_MAIN
    Q = queries(ix, 0xF1F0, 8)
    words = capi.allowed_bitmaps([np.ones(n, dtype=bool)] * 2, n)
    big = capi.allowed_bitmaps([np.ones(n, dtype=bool)] * 65, n)
    need = words.shape[1]
    fo = (np.arange(8) % 2).astype(np.uint32)
    INV = capi.ERR_INVALID
    for probed, arg in ((True, 4), (False, L2)):
        assert raw(ix, Q, 10, arg, words, need, 2, n, fo, probed)[0] == capi.OK
        assert raw(ix, Q, 10, arg, words, need, 0, n, fo, probed)[0] == INV            # n_filters == 0 with b > 0
        assert raw(ix, Q, 10, arg, big, need, 65, n, fo, probed)[0] == INV             # n_filters > VERS_FILTER_MAX
        assert raw(ix, Q, 10, arg, big, need, 64, n, fo, probed)[0] == capi.OK
        assert raw(ix, Q, 10, arg, None, need, 2, n, fo, probed)[0] == INV             # n_bits > 0 with NULL filters
        assert raw(ix, Q, 10, arg, words, need, 2, n, None, probed)[0] == INV          # NULL filter_of with b > 0
        assert raw(ix, Q, 10, arg, words, need - 1, 2, n, fo, probed)[0] == INV        # a stride too small
        bad = fo.copy(); bad[5] = 2
        assert raw(ix, Q, 10, arg, words, need, 2, n, bad, probed)[0] == INV           # a host filter_of entry equal to n_filters
        rc, cnt = raw(ix, Q, 10, arg, None, 0, 2, 0, fo, probed)                       # n_bits == 0: every filter empty, filters may be NULL
        assert rc == capi.OK and not cnt.any()
        rc, cnt = raw(ix, Q, 0, arg, words, need, 2, n, fo, probed)                    # top_k == 0: counts 0
        assert rc == capi.OK and not cnt.any()
    assert raw(ix, Q, 10, 0, words, need, 2, n, fo)[0] == INV                          # nprobe == 0
    assert raw(ix, Q, 10, 2, words, need, 2, n, fo, probed=False)[0] == INV            # metric > VERS_METRIC_COSDIST
    # the _dev calls refuse the same before the device is touched
    dev = torch.device("cuda", ix.device)
    qd = torch.from_numpy(Q).to(dev); wd = torch.from_numpy(words.view(np.int64)).to(dev); fd = torch.from_numpy(fo.view(np.int32)).to(dev)
    oi = torch.zeros((8, 10), dtype=torch.int64, device=dev); od = torch.zeros((8, 10), dtype=torch.float32, device=dev); oc = torch.zeros(8, dtype=torch.int32, device=dev)
    out = (oi.data_ptr(), od.data_ptr(), oc.data_ptr())
    for args in ((4, wd.data_ptr(), need, 0, n, fd.data_ptr()), (4, wd.data_ptr(), need, 65, n, fd.data_ptr()), (4, 0, need, 2, n, fd.data_ptr()),
                 (4, wd.data_ptr(), need, 2, n, 0), (4, wd.data_ptr(), need - 1, 2, n, fd.data_ptr()), (0, wd.data_ptr(), need, 2, n, fd.data_ptr())):
        with pytest.raises(capi.VersError) as e:
            ix.search_filtered_multi_dev(qd.data_ptr(), ix.d, 8, 10, *args, *out)
        assert e.value.status == INV, args
    for args in ((L2, wd.data_ptr(), need, 0, n, fd.data_ptr()), (L2, wd.data_ptr(), need, 65, n, fd.data_ptr()), (L2, 0, need, 2, n, fd.data_ptr()),
                 (L2, wd.data_ptr(), need, 2, n, 0), (L2, wd.data_ptr(), need - 1, 2, n, fd.data_ptr()), (2, wd.data_ptr(), need, 2, n, fd.data_ptr())):
        with pytest.raises(capi.VersError) as e:
            ix.search_exhaustive_filtered_multi_dev(qd.data_ptr(), ix.d, 8, 10, *args, *out)
        assert e.value.status == INV, args
    # b == 0: a no-op
    Lb = capi.lib()
    assert Lb.vers_ivf_search_filtered_multi(ix._h, None, 4 * ix.d, 0, 10, 4, capi._ptr(words), need, 2, n, None, None, None, None) == capi.OK
    assert Lb.vers_ivf_search_exhaustive_filtered_multi(ix._h, None, 4 * ix.d, 0, 10, L2, capi._ptr(words), need, 2, n, None, None, None, None) == capi.OK
    assert Lb.vers_ivf_search_filtered_multi_dev(ix._h, None, ix.d, 0, 10, 4, None, 0, 0, 0, None, None, None, None, None) == capi.OK
    assert Lb.vers_ivf_search_exhaustive_filtered_multi_dev(ix._h, None, ix.d, 0, 10, L2, None, 0, 0, 0, None, None, None, None, None) == capi.OK
    # an index without centroids: the probed call has nothing to rank, the exhaustive call counts 0
    empty = IVFFlatIndex(ix.d)
    assert raw(empty, Q, 10, 4, words, need, 2, n, fo)[0] == capi.ERR_INSUFFICIENT
    rc, cnt = raw(empty, Q, 10, L2, words, need, 2, n, fo, probed=False)
    assert rc == capi.OK and not cnt.any()
    empty.close()
    # a handle sharded by cluster
    sh = make(600, 32, 4, seed=0xF1F1)
    Qs = queries(sh, 0xF1F2, 3)
    w600 = capi.allowed_bitmaps([np.ones(600, dtype=bool)] * 2, 600)
    f3 = np.asarray([0, 1, 0], dtype=np.uint32)
    half = IVFFlatIndex(sh.d)
    half.set_shard(0, 2)
    half.num_centroids, half.values, half.centroids, half.assignments = sh.num_centroids, sh.values, sh.centroids, sh.assignments
    half._upload()
    assert raw(sh, Qs, 10, 2, w600, w600.shape[1], 2, 600, f3)[0] == capi.OK
    assert raw(half, Qs, 10, 2, w600, w600.shape[1], 2, 600, f3)[0] == INV
    assert raw(half, Qs, 10, L2, w600, w600.shape[1], 2, 600, f3, probed=False)[0] == INV
    half.close()
    sh.close()


def dev_call(ix, call, qd, b, top_k, arg, wd, stride, n_filters, n_bits, fd, stream=0):
    import torch
    dev = qd.device
    ids = torch.full((b, top_k), -1, dtype=torch.int64, device=dev)
    dist = torch.full((b, top_k), -7.25, dtype=torch.float32, device=dev)
    cnt = torch.full((b,), 77, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    fn = ix.search_filtered_multi_dev if call == "probed" else ix.search_exhaustive_filtered_multi_dev
    fn(qd.data_ptr(), ix.d, b, top_k, arg, wd.data_ptr(), stride, n_filters, n_bits, fd.data_ptr(), ids.data_ptr(), dist.data_ptr(), cnt.data_ptr(), stream)
    ix.poll(stream)
    return ids.cpu().numpy().astype(np.uint64), dist.cpu().numpy(), cnt.cpu().numpy().astype(np.uint32)


def test_dev_call_out_of_range_filter_of_selects_the_empty_filter(main_case):
    import torch
    case = main_case
    ix, b = case.ix, 17
    dev = torch.device("cuda", ix.device)
    qd = torch.from_numpy(case.Q[:b]).to(dev); wd = torch.from_numpy(case.words.view(np.int64)).to(dev)
    fo = (np.arange(b) % 3).astype(np.uint32)
    want = {c: check(case, fo, 10, a, probed=c == "probed", qs=range(b)) for c, a in (("probed", 4), ("exhaustive", L2))}
    out = [2, 9, 16]
    bad = fo.copy(); bad[out] = [3, 64, 0xFFFFFFFF]   # n_filters = 3: equal to it, the first bit position beyond a word, the largest value
    fd = torch.from_numpy(bad.view(np.int32)).to(dev)
    rest = np.setdiff1d(np.arange(b), out)
    for call, arg in (("probed", 4), ("exhaustive", L2)):
        got = dev_call(ix, call, qd, b, 10, arg, wd, case.words.shape[1], 3, N_MAIN, fd)
        assert not got[2][out].any() and got[2][rest].all(), call
        same_rows(got, want[call], rest, call)
    # a single query on an out-of-range entry
    fd1 = torch.from_numpy(np.asarray([7], dtype=np.int32)).to(dev)
    for call, arg in (("probed", 4), ("exhaustive", L2)):
        assert dev_call(ix, call, qd, 1, 10, arg, wd, case.words.shape[1], 3, N_MAIN, fd1)[2][0] == 0


def test_device_pointer_calls_on_two_streams(main_case):
    import torch
    case = main_case
    ix, b = case.ix, 17
    fo = (np.arange(b) % 5).astype(np.uint32)
    dev = torch.device("cuda", ix.device)
    qd = torch.from_numpy(case.Q[:b]).to(dev); wd = torch.from_numpy(case.words.view(np.int64)).to(dev); fd = torch.from_numpy(fo.view(np.int32)).to(dev)
    want = {(c, k): check(case, fo, k, a, probed=c == "probed", qs=range(b)) for c, a in (("probed", 4), ("exhaustive", L2)) for k in (10, 100)}
    streams = (torch.cuda.Stream(dev), torch.cuda.Stream(dev))
    # both streams in flight: every call enqueued before the first poll
    bufs = []
    for stream in streams:
        for (call, top_k) in want:
            ids = torch.full((b, top_k), -1, dtype=torch.int64, device=dev); dist = torch.zeros((b, top_k), dtype=torch.float32, device=dev)
            cnt = torch.zeros(b, dtype=torch.int32, device=dev)
            bufs.append((stream, call, top_k, ids, dist, cnt))
    torch.cuda.synchronize(dev)
    for stream, call, top_k, ids, dist, cnt in bufs:
        fn = ix.search_filtered_multi_dev if call == "probed" else ix.search_exhaustive_filtered_multi_dev
        fn(qd.data_ptr(), ix.d, b, top_k, 4 if call == "probed" else L2, wd.data_ptr(), case.words.shape[1], 5, N_MAIN, fd.data_ptr(), ids.data_ptr(),
           dist.data_ptr(), cnt.data_ptr(), stream.cuda_stream)
    for stream in streams:
        ix.poll(stream.cuda_stream)
    for stream, call, top_k, ids, dist, cnt in bufs:
        got = (ids.cpu().numpy().astype(np.uint64), dist.cpu().numpy(), cnt.cpu().numpy().astype(np.uint32))
        same_rows(got, want[(call, top_k)], np.arange(b), (call, top_k))


def test_nan_on_the_device_pointer_call_latches_for_poll(main_case):
    import torch
    case = main_case
    ix = case.ix
    Q = case.Q[:8].copy(); Q[2, 5] = np.nan
    fo = (np.arange(8) % 2).astype(np.uint32)
    dev = torch.device("cuda", ix.device)
    qd = torch.from_numpy(Q).to(dev); wd = torch.from_numpy(case.words.view(np.int64)).to(dev); fd = torch.from_numpy(fo.view(np.int32)).to(dev)
    ids = torch.zeros((8, 10), dtype=torch.int64, device=dev); dist = torch.zeros((8, 10), dtype=torch.float32, device=dev); cnt = torch.zeros(8, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    ix.search_exhaustive_filtered_multi_dev(qd.data_ptr(), ix.d, 8, 10, L2, wd.data_ptr(), case.words.shape[1], 5, N_MAIN, fd.data_ptr(), ids.data_ptr(),
                                            dist.data_ptr(), cnt.data_ptr())
    with pytest.raises(capi.VersError) as e:
        ix.poll()
    assert e.value.status == capi.ERR_NAN
    ix.poll()   # (cleared)


def test_other_searches_are_unchanged_around_a_multi_call(main_case):
    """the workspace lease is clean: unfiltered and per-call filtered batches before and after multi calls return the same bits"""
    case = main_case
    ix, Q = case.ix, case.Q
    one = (case.words[0], N_MAIN)

    def others():
        return ([ix.search_batch(Q, top_k, nprobe) for top_k, nprobe in ((10, 4), (10, 0), (100, 4))] +
                [ix.search_batch(Q[0], 10, 4), ix.search_exhaustive(Q[:9], 10), ix.search_filtered(Q, 10, 4, one), ix.search_filtered(Q[0], 100, 12, one),
                 ix.search_exhaustive_filtered(Q[:9], 70, one)])

    before = others()
    fo = np.arange(40) % 5
    check(case, fo, 10, 4); check(case, [3], 100, 12, qs=[0]); check(case, fo, 70, L2, probed=False)
    for g0, g1 in zip(before, others()):
        same_rows(g0, g1, np.arange(len(g0[2])), "around")


def test_scan_timing_ring_gets_the_mask_record_then_one_per_pass(main_case):
    case = main_case
    ix, Q = case.ix, case.Q[:9]
    fo = np.arange(9) % 5
    one, all5 = (case.words[0], N_MAIN), (case.words, N_MAIN)
    for top_k, passes in ((10, 1), (200, 4)):   # (64 result ranks per pass)
        for probed in (True, False):
            ix.scan_times(reset=True)
            ix.search_filtered(Q, top_k, 4, one) if probed else ix.search_exhaustive_filtered(Q, top_k, one)
            per_call = ix.scan_times(reset=True)
            ix.search_filtered_multi(Q, top_k, 4, all5, fo) if probed else ix.search_exhaustive_filtered_multi(Q, top_k, all5, fo)
            ring = ix.scan_times(reset=True)
            assert ring.size == per_call.size == 1 + passes and (ring > 0).all(), (top_k, probed, ring, per_call)


# ---- 10. the stats hook -------------------------------------------------------------------------------------------------------------------------
def test_stats_hook(main_ix):
    ix, n = main_ix, N_MAIN
    lists = [np.asarray(l, dtype=np.int64) for l in ix.ids]
    live = sum(len(l) for l in lists)
    Q = queries(ix, 0xF200, 9)
    selective = np.arange(1000, 1400)
    everything = np.ones(n, dtype=bool)
    nothing = np.zeros(0, dtype=np.int64)
    some = random_filter(n, 0.2, 0xF201)
    case = Case(ix, Q, [selective, everything, nothing, some], n, n)
    pops = [int(r.sem.sum()) for r in case.refs]
    assert live == n and pops[1] == n and pops[2] == 0
    head = ("tiles_planned", "tiles_loaded", "items_skipped")
    for seg_rows in (0, 64):
        capi.set_option("seg_rows", seg_rows)
        case.fresh()
        try:
            for qs in (list(range(9)), [4]):
                b = len(qs)
                for probed, arg in ((True, 4), (False, L2)):
                    # every filter_of equal: planned, loaded and skipped are the per-call call's with that bitmap; an unused all-ones bitmap
                    # (and two more) cost no loads
                    for f in (0, 3, 1, 2):
                        t0 = ix.filter_stats()["total"]
                        case.per_call(f, qs, 10, arg, probed)
                        one = ix.filter_stats()["last"]
                        assert one["rows_allowed"] == pops[f]
                        check(case, np.full(b, f), 10, arg, probed=probed, qs=qs, cross=False)
                        st = ix.filter_stats()
                        multi = st["last"]
                        assert [multi[k] for k in head] == [one[k] for k in head], (seg_rows, b, probed, f, multi, one)
                        assert multi["rows_allowed"] == sum(pops)   # allowed (bitmap, storage row) pairs over the call's bitmaps
                        for k in head:
                            assert st["total"][k] - t0[k] == 2 * one[k]
                        assert st["total"]["rows_allowed"] - t0["rows_allowed"] == pops[f] + sum(pops)
                        if f == 0:   # the selective range with all ones beside it, unused: the loads are the selective range's
                            assert multi["tiles_loaded"] < multi["tiles_planned"] and (probed or multi["tiles_loaded"] > 0)
                        if f == 2:   # all queries on an empty bitmap: nothing loaded, every item counted skipped
                            assert multi["tiles_loaded"] == 0 and multi["items_skipped"] > 0
                            if seg_rows == 64 and b == 1 and probed:   # a work item is one tile of one probed list
                                assert multi["items_skipped"] == multi["tiles_planned"]
                # mixed: a tile is loaded when some live query of the item is allowed a row of it -- no fewer loads than the most selective
                # bitmap alone, no more than everything
                check(case, np.arange(b) % 4, 10, 4, qs=qs)
                mixed = ix.filter_stats()["last"]
                assert mixed["tiles_loaded"] <= mixed["tiles_planned"] and mixed["rows_allowed"] == sum(pops)
        finally:
            capi.set_option("seg_rows", 0)
