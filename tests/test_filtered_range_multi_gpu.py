"""vers_ivf_range_search_filtered_multi / vers_ivf_range_search_exhaustive_filtered_multi (+ _dev): one range batch whose queries use
different bitmaps.  Nothing new in the semantics -- query q's CSR segment is query q's segment of the per-call filtered range search made with
bitmap filter_of[q] -- so every case is checked twice, and every comparison is np.array_equal on the limits, the ids and the distances' u32
BITS, no tolerance:
  * against the oracle of tests/test_filtered_range_gpu.py (its Ref, restated here): co.search_nprobe / co.search_exhaustive over the list
    ids retained by the query's OWN bitmap, the leading entries <= r for the default order, the list walk for VERS_RANGE_WALK_ORDER;
  * against the per-call GPU call (range_search_filtered / range_search_exhaustive_filtered), made once per distinct bitmap with the same
    queries, radii, nprobe / metric and flags, compared segment by segment.
Both orders every time; the walk order re-sorted must equal the sorted order.  The oracle's full order is computed once per (index, queries,
bitmap, nprobe / metric) and cut to each radius.  Not covered: the refusals that need 2^32 results or slots, as in the per-call suite."""
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
INF = np.float32(np.inf)
WALK = capi.RANGE_WALK_ORDER
ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
SENT = 0xCDCDCDCDCDCDCDCD


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def make(n, d, k, metric=L2, seed=0xFB70, iters=4):
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


def random_filter(n, sel, seed):
    return np.random.default_rng(seed).random(n) < sel


class Ref:
    """The oracle's view of (index, queries, ONE bitmap), computed once and shared by every radius / order / call shape: the full filtered
    order per query (per nprobe, exhaustive per metric) and the device's lists.  (tests/test_filtered_range_gpu.py's Ref; the walk is the same
    selection written with arrays.)"""

    def __init__(self, ix, Q, sem):
        self.ix, self.Q = ix, np.atleast_2d(Q)
        self.sem = np.zeros(max(len(sem), ix.values.shape[0]), dtype=bool)
        self.sem[:len(sem)] = np.asarray(sem, dtype=bool)
        self.ids_f = [[v for v in l if self.sem[v]] for l in ix.ids]
        self.rows = np.asarray(sorted(v for l in self.ids_f for v in l), dtype=np.int64)
        self._p, self._x, self._rank, self._lists, self._want = {}, {}, {}, {}, {}

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
        dist_of = np.full(self.sem.size, np.nan, dtype=np.float32)
        dist_of[oi.astype(np.int64)] = od
        lists = list(lists)
        cat = np.concatenate([self.device_list(c) for c in lists]).astype(np.int64) if lists else np.zeros(0, np.int64)
        with np.errstate(invalid="ignore"):
            keep = self.sem[cat] & (dist_of[cat] <= np.float32(r))
        return cat[keep].astype(np.uint64), dist_of[cat[keep]]

    def want(self, q, r, nprobe, metric, walk):
        """nprobe None: the exhaustive call under `metric`"""
        key = (q, int(np.float32(r).view(np.uint32)), nprobe, metric, walk)
        if key not in self._want:
            if nprobe is not None:
                full = self.probed(q, nprobe)
                self._want[key] = self._walk(full, self.probes(q, nprobe), r) if walk else self._head(full, r)
            else:
                full = self.exhaustive(q, metric)
                self._want[key] = self._walk(full, range(self.ix.num_centroids), r) if walk else self._head(full, r)
        return self._want[key]


class Case:
    """(index, queries, the call's bitmaps): an oracle Ref per bitmap and the per-call GPU results, each computed once.  words: the packed
    bitmaps handed to the GPU, when they are not simply capi.allowed_bitmaps(allowed, n_bits) (garbage beyond n_bits, a larger stride)."""

    def __init__(self, ix, Q, allowed, n_bits, n, words=None):
        self.ix, self.Q, self.n_bits = ix, np.atleast_2d(Q), int(n_bits)
        self.words = capi.allowed_bitmaps(allowed, n_bits) if words is None else words
        self.need = max(1, (self.n_bits + 63) // 64)
        self.refs = [Ref(ix, self.Q, allowed_set(n, a, n_bits)) for a in allowed]
        self._one = {}

    def fresh(self):
        """forget the per-call GPU results (an option that changes the plan was set)"""
        self._one = {}
        return self

    def per_call(self, f, qs, radii, nprobe, metric, walk):
        key = (f, tuple(qs), radii.tobytes(), nprobe, metric, walk)
        if key not in self._one:
            one = (np.ascontiguousarray(self.words[f, :self.need]), self.n_bits)
            self._one[key] = (self.ix.range_search_filtered(self.Q[qs], radii, nprobe, one, walk_order=walk) if nprobe is not None
                              else self.ix.range_search_exhaustive_filtered(self.Q[qs], radii, one, metric, walk_order=walk))
        return self._one[key]


def host_call(case, Q, radii, nprobe, metric, fo, walk):
    filters = (case.words, case.n_bits)
    if nprobe is not None:
        return case.ix.range_search_filtered_multi(Q, radii, nprobe, filters, fo, walk_order=walk)
    return case.ix.range_search_exhaustive_filtered_multi(Q, radii, filters, fo, metric, walk_order=walk)


def dev_call(case, Q, radii, nprobe, metric, fo, walk, stream=None, n_filters=None, null_filters=False):
    """the _dev call through the capacity protocol: the size query, then arrays one entry larger than the total, whose sentinels stay"""
    import torch
    ix = case.ix
    Q = np.ascontiguousarray(np.atleast_2d(Q), dtype=np.float32)
    b = Q.shape[0]
    dev = torch.device("cuda", ix.device)
    qd = torch.from_numpy(Q).to(dev)
    rd = torch.from_numpy(capi.range_radii(radii, b).copy()).to(dev)
    wd = torch.from_numpy(np.ascontiguousarray(case.words).view(np.int64).copy()).to(dev)
    fd = torch.from_numpy(np.ascontiguousarray(fo, dtype=np.uint32).view(np.int32).copy()).to(dev)
    wp = 0 if null_filters else wd.data_ptr()
    stride = 0 if null_filters else case.words.shape[1]
    nf = case.words.shape[0] if n_filters is None else n_filters
    lims = torch.full((b + 1,), -5, dtype=torch.int64, device=dev)
    flags = WALK if walk else 0
    s = stream.cuda_stream if stream is not None else 0
    torch.cuda.synchronize(dev)
    fn = (lambda *a: ix.range_search_filtered_multi_dev(qd.data_ptr(), ix.d, b, rd.data_ptr(), nprobe, flags, wp, stride, nf, case.n_bits, fd.data_ptr(), *a, s)) \
        if nprobe is not None else \
         (lambda *a: ix.range_search_exhaustive_filtered_multi_dev(qd.data_ptr(), ix.d, b, rd.data_ptr(), metric, flags, wp, stride, nf, case.n_bits, fd.data_ptr(), *a, s))
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


def same_segments(got, one, rows, what):
    """the segments `rows` of two CSR results"""
    (l0, i0, d0), (l1, i1, d1) = got, one
    for i in rows:
        a0, e0, a1, e1 = int(l0[i]), int(l0[i + 1]), int(l1[i]), int(l1[i + 1])
        assert e0 - a0 == e1 - a1, (what, int(i), "count")
        assert np.array_equal(i0[a0:e0], i1[a1:e1]) and np.array_equal(bits(d0[a0:e0]), bits(d1[a1:e1])), (what, int(i))


def check(case, qs, fo, radii, nprobe, metric=L2, calls=(host_call,), cross=True):
    """One multi call shape over queries qs with filter_of fo (one entry per entry of qs), in both orders: against the oracle, against the
    per-call GPU call of every distinct bitmap, and the walk order re-sorted against the sorted order.  -> the sorted result."""
    qs = list(qs)
    fo = np.asarray(fo, dtype=np.uint32).reshape(-1)
    assert fo.size == len(qs)
    radii = np.broadcast_to(np.asarray(radii, dtype=np.float32), (len(qs),)).copy()
    Q = case.Q[qs]
    first = None
    for call in calls:
        got = []
        for walk in (False, True):
            what = (nprobe, metric, walk, call.__name__, fo.tolist())
            g = call(case, Q, radii, nprobe, metric, fo, walk)
            same(g, [case.refs[fo[i]].want(q, radii[i], nprobe, metric, walk) for i, q in enumerate(qs)], what)
            if cross:
                for f in np.unique(fo):
                    same_segments(g, case.per_call(int(f), qs, radii, nprobe, metric, walk), np.flatnonzero(fo == f), what + (int(f),))
            got.append(g)
        (sl, si, sd), (wl, wi, wd) = got
        assert np.array_equal(sl, wl)
        for i in range(len(qs)):
            a, e = int(sl[i]), int(sl[i + 1])
            # probed: a stable sort by distance (ties stay in probe rank, list position); exhaustive: ties go to the lower vec id
            o = np.argsort(wd[a:e], kind="stable") if nprobe is not None else np.lexsort((wi[a:e], wd[a:e]))
            assert np.array_equal(wi[a:e][o], si[a:e]) and np.array_equal(bits(wd[a:e][o]), bits(sd[a:e])), ("walk re-sorted", nprobe, i)
        first = first or got[0]
    return first


KINDS = 5   # query q of a mixed batch: kind q % 5


def mixed_radii(case, qs, fo, nprobe):
    """per query the 1st / 10th / 100th-nearest ALLOWED probed distance of the query's OWN bitmap, +inf, -1"""
    out = []
    for i, q in enumerate(qs):
        kind = q % KINDS
        out.append(case.refs[fo[i]].mth(q, nprobe, (1, 10, 100)[kind]) if kind < 3 else (INF if kind == 3 else np.float32(-1)))
    return np.asarray(out, dtype=np.float32)


def patterns(b, F, seed):
    """filter_of patterns over b queries and F bitmaps (the top-k multi suite's): all equal, alternating, every query its own (cycling in
    reverse beyond F), sorted blocks, random"""
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
    Q = queries(main_ix, 0xFB71, 40)
    allowed = [random_filter(N_MAIN, 0.5, 0xFB80 + f) for f in range(5)]
    return Case(main_ix, Q, allowed, N_MAIN, N_MAIN)


# ---- 1. group widths, segments, both passes, filter_of patterns -------------------------------------------------------------------------
@pytest.mark.parametrize("seg_rows", [0, 64])
@pytest.mark.parametrize("b", [1, 3, 8, 9, 17, 40])
def test_group_widths_segments_passes_and_patterns(main_case, b, seg_rows):
    case = main_case
    batches = [[j] for j in range(KINDS)] if b == 1 else [list(range(b))]   # (a single query: one call per kind of radius)
    capi.set_option("seg_rows", seg_rows)
    case.fresh()
    try:
        for qs in batches:
            for F in (1, 2, 5):
                seen = set()
                for name, fo in patterns(len(qs), F, 0xFB90 + b).items():
                    fo = np.asarray(fo, dtype=np.uint32)
                    if fo.tobytes() in seen:    # (the same filter_of is the same call)
                        continue
                    seen.add(fo.tobytes())
                    for nprobe in (1, 4, 12):
                        radii = mixed_radii(case, qs, fo, nprobe)
                        lims, _, _ = check(case, qs, fo, radii, nprobe, calls=(host_call, dev_call))
                        for i, q in enumerate(qs):
                            n = int(lims[i + 1]) - int(lims[i])
                            if q % KINDS == 1:
                                assert n >= 10, (q, n)     # the 10th-nearest radius
                            if q % KINDS == 4:
                                assert n == 0, (q, n)      # radius -1
                        if nprobe == 4:   # the exhaustive call at the same radii
                            check(case, qs, fo, radii, None, calls=(host_call, dev_call))
    finally:
        capi.set_option("seg_rows", 0)


def test_python_mirror_takes_a_list_of_filters(main_case):
    case = main_case
    allowed = [np.flatnonzero(r.sem[:N_MAIN]) if f % 2 else r.sem[:N_MAIN] for f, r in enumerate(case.refs)]   # id arrays and bool arrays
    fo = np.arange(9) % 5
    radii = mixed_radii(case, range(9), fo, 4)
    a = case.ix.range_search_filtered_multi(case.Q[:9], radii, 4, allowed, fo, n_bits=N_MAIN)
    b = case.ix.range_search_filtered_multi(case.Q[:9], radii, 4, (case.words, N_MAIN), fo)
    assert a[0][-1] > 0 and all(np.array_equal(x, y) for x, y in zip(a, b))
    a = case.ix.range_search_exhaustive_filtered_multi(case.Q[:9], radii, allowed, fo, n_bits=N_MAIN)
    b = case.ix.range_search_exhaustive_filtered_multi(case.Q[:9], radii, (case.words, N_MAIN), fo)
    assert a[0][-1] > 0 and all(np.array_equal(x, y) for x, y in zip(a, b))


# ---- 2. disjoint tenants, an empty and an all-ones bitmap in one batch --------------------------------------------------------------------
def test_disjoint_tenants_empty_and_all_ones(main_ix):
    ix, n = main_ix, N_MAIN
    Q = queries(ix, 0xFBA0, 17)
    tenants = [np.arange(f * 1200, (f + 1) * 1200) for f in range(5)]   # contiguous id ranges: a tile is live for few queries of a group
    allowed = tenants + [np.zeros(0, dtype=np.int64), np.ones(n, dtype=bool)]
    case = Case(ix, Q, allowed, n, n)
    qs = list(range(17))
    fo = np.arange(17) % 7
    for seg_rows in (0, 64):
        capi.set_option("seg_rows", seg_rows)
        case.fresh()
        try:
            for nprobe in (4, 12, None):
                for radii in (INF, mixed_radii(case, qs, fo, 12)):
                    lims, ids, _ = check(case, qs, fo, radii, nprobe)
                    cnt = np.diff(lims.astype(np.int64))
                    assert not cnt[fo == 5].any()          # empty segments ...
                    if np.ndim(radii) == 0:
                        assert cnt[fo != 5].all()           # ... between non-empty ones
                    for i in np.flatnonzero(fo < 5):        # a tenant's query sees its own ids only, whatever its group's neighbours were allowed
                        got = ids[int(lims[i]):int(lims[i + 1])]
                        assert ((got >= fo[i] * 1200) & (got < (fo[i] + 1) * 1200)).all()
            check(case, [5, 6], fo[5:7], INF, 12)   # the empty filter and all ones, side by side in one group
        finally:
            capi.set_option("seg_rows", 0)


# ---- 3. tile edges ------------------------------------------------------------------------------------------------------------------------
def test_tile_edges(main_ix):
    ix, n = main_ix, N_MAIN
    Q = queries(ix, 0xFBB0, 9)
    lists = [np.asarray(l, dtype=np.int64) for l in ix.ids]
    near = [int(co.search_exhaustive(ix.centroids, Q[q], ix.num_centroids, ix.metric)[0][0]) for q in range(9)]
    c0 = near[0]
    edges = np.concatenate([l[[p for p in (0, 63, 64, 127, len(l) - 1) if p < len(l)]] for l in lists if len(l)])
    whole = lists[c0]                               # one whole probed list (probed by query 0, at least)
    rest = np.ones(n, dtype=bool); rest[whole] = False   # everything but that list
    case = Case(ix, Q, [edges, whole, rest], n, n)
    qs = list(range(9))
    for fo in (np.arange(9) % 3, (np.arange(9) + 1) % 3, (np.arange(9) + 2) % 3):
        for nprobe in (1, 4, 12, None):
            lims, _, _ = check(case, qs, fo, INF, nprobe)
            check(case, qs, fo, mixed_radii(case, qs, fo, 12), nprobe)
            if nprobe == 1:   # only a list the query does not probe: the segment is empty
                cnt = np.diff(lims.astype(np.int64))
                for i in qs:
                    if fo[i] == 1:
                        assert (cnt[i] == 0) == (near[i] != c0), i
                    if fo[i] == 2:
                        assert (cnt[i] == 0) == (near[i] == c0), i
    assert any(c != c0 for c in near)
    far = next(q for q in qs if near[q] != c0)
    check(case, [far, 0], [1, 1], INF, 1)
    check(case, [far], [1], INF, 1)


# ---- 4. bitmap edges ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_bits", [N_MAIN - 1, N_MAIN, N_MAIN + 1, N_MAIN + 1000, 64 * ((N_MAIN + 63) // 64) - 1, N_MAIN // 2])
def test_bitmap_edges_garbage_and_stride(main_ix, n_bits):
    ix, n = main_ix, N_MAIN
    Q = queries(ix, 0xFBC0, 8)
    allowed = [random_filter(n + 1064, 0.6, 0xFBC1 + f) for f in range(3)]
    for a in allowed:
        a[[n - 2, n - 1]] = True   # the last ids of the index are allowed whenever n_bits reaches them
    need = (n_bits + 63) // 64
    qs = list(range(8))
    fo = np.arange(8) % 3
    for stride in (need, need + 3):
        words = capi.allowed_bitmaps(allowed, n_bits, stride)
        if n_bits % 64:   # garbage in each bitmap's last word beyond n_bits: every bit set
            words[:, need - 1] |= ONES << np.uint64(n_bits % 64)
        words[:, need:] = ONES   # ... and in the padding of a larger stride
        case = Case(ix, Q, allowed, n_bits, n, words=words)
        for r, a in zip(case.refs, allowed):
            assert r.sem[:min(n, n_bits)].sum() == a[:min(n, n_bits)].sum() and not r.sem[min(n, n_bits):].any()
        for calls in ((host_call,), (dev_call,)):
            check(case, qs, fo, mixed_radii(case, qs, fo, 4), 4, calls=calls)
            check(case, qs, fo, INF, None, calls=calls)
        check(case, [3], [2], INF, 4)


def test_n_bits_zero_with_null_filters(main_ix):
    ix, n = main_ix, N_MAIN
    Q = queries(ix, 0xFBC8, 9)
    fo = (np.arange(9) % 3).astype(np.uint32)
    case = Case(ix, Q, [np.ones(n, dtype=bool)] * 3, 0, n)   # n_bits == 0: every filter is empty
    for probed in (True, False):
        rc, lims, total = raw(ix, Q, INF, 4 if probed else L2, 0, None, 0, 3, 0, fo, probed=probed)
        assert rc == capi.OK and total == 0 and not lims.any()
        got = dev_call(case, Q, INF, 4 if probed else None, L2, fo, False, null_filters=True)
        assert not got[0].any() and got[1].size == 0


# ---- 5. items of more than 64 tiles -----------------------------------------------------------------------------------------------------------
def test_items_of_more_than_64_tiles():
    ix = make(12000, 32, 2, seed=0xFB72)
    try:
        n = 12000
        lists = [np.asarray(l, dtype=np.int64) for l in ix.ids]
        longest = max(lists, key=len)
        assert len(longest) > 4096 + 64   # the longer list reaches into a second window of 64 tiles
        Q = queries(ix, 0xFB73, 9)
        second = np.concatenate([l[4096:] for l in lists])     # live tiles in the second window only
        first = np.concatenate([l[:4096:7] for l in lists])    # ... in the first only
        both = np.concatenate([l[::5] for l in lists])         # ... in both
        last = longest[-1:]                                     # a single row, in the last tile
        case = Case(ix, Q, [second, first, both, last], n, n)
        qs = list(range(9))
        capi.set_option("seg_rows", 8192)
        for fo in (np.arange(9) % 4, (np.arange(9) + 2) % 4, np.zeros(9, int), np.full(9, 3)):
            for nprobe in (1, 2, None):
                lims, _, _ = check(case, qs, fo, INF, nprobe)
                check(case, qs, fo, mixed_radii(case, qs, fo, 2), nprobe)
                if nprobe != 1:
                    assert (np.diff(lims.astype(np.int64))[fo == 3] == 1).all()
        for f in range(4):
            check(case, [0], [f], INF, 2)
            check(case, [0], [f], INF, None)
    finally:
        capi.set_option("seg_rows", 0)
        ix.close()


# ---- 6. more than 64 probes -----------------------------------------------------------------------------------------------------------------
def test_more_than_64_probes():
    ix = make(4000, 16, 80, seed=0xFB74)
    try:
        Q = queries(ix, 0xFB75, 9)
        case = Case(ix, Q, [random_filter(4000, 0.3, 0xFB76 + f) for f in range(3)], 4000, 4000)
        qs = list(range(9))
        fo = np.arange(9) % 3
        check(case, qs, fo, mixed_radii(case, qs, fo, 70), 70)
        check(case, qs, fo, INF, 70)
        check(case, [5], [2], INF, 70)
    finally:
        ix.close()


# ---- 7. dimensions and the cosine metric ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 100, 320])
def test_dimensions(d):
    ix = make(1500, d, 6, seed=0xFC00 + d)
    try:
        Q = queries(ix, 0xFC01, 9)
        case = Case(ix, Q, [random_filter(1500, 0.4, 0xFC02 + f) for f in range(3)], 1500, 1500)
        qs = list(range(9))
        fo = np.arange(9) % 3
        for nprobe in (3, 6, None):
            check(case, qs, fo, mixed_radii(case, qs, fo, 3), nprobe)
            check(case, qs, fo, INF, nprobe)
        check(case, [1], [1], INF, 3)
    finally:
        ix.close()


def test_cosine_metric():
    ix = make(1500, 48, 6, metric=COS, seed=0xFC10)
    try:
        Q = queries(ix, 0xFC11, 9)
        case = Case(ix, Q, [random_filter(1500, 0.4, 0xFC12 + f) for f in range(3)], 1500, 1500)
        qs = list(range(9))
        fo = np.arange(9) % 3
        radii = mixed_radii(case, qs, fo, 3)
        check(case, qs, fo, radii, 3)
        check(case, qs, fo, INF, 6)
        for metric in (L2, COS):
            check(case, qs, fo, radii, None, metric=metric)
            check(case, qs, fo, INF, None, metric=metric)
        check(case, [1], [1], INF, 3)
    finally:
        ix.close()


# ---- 8. a mutated index -------------------------------------------------------------------------------------------------------------------
def test_mutated_index():
    ix = make(3000, 64, 8, seed=0xFC20)
    try:
        Q = queries(ix, 0xFC21, 9)
        qs = list(range(9))
        fo = np.arange(9) % 3
        n = 3500
        allowed = [random_filter(n, 0.5, 0xFC23 + f) for f in range(3)]
        allowed[1][3000:3100] = True   # new ids among the allowed

        def all_checks():
            case = Case(ix, Q, allowed, n, n)
            radii = mixed_radii(case, qs, fo, 4)
            return [check(case, qs, fo, radii, 4), check(case, qs, fo, INF, 8), check(case, qs, fo, radii, None), check(case, [2], [1], INF, 4)]

        ix.add_batch(dg.dist_c(0xFC22, 500, 64, 16, dg.default_sigma(64)))
        all_checks()
        gone = np.flatnonzero(allowed[0] | allowed[1])[::3].astype(np.uint64)   # removed ids stay set in the bitmaps: they select nothing
        ix.remove_batch(gone)
        before = all_checks()
        ix.compact()
        after = all_checks()
        assert before[1][0][-1] > 0
        for g0, g1 in zip(before[1:2] + before[3:], after[1:2] + after[3:]):   # (the radius-free calls: the same result after compact)
            same_segments(g0, g1, range(len(g0[0]) - 1), "compact")
    finally:
        ix.close()


# ---- 9. NaN ---------------------------------------------------------------------------------------------------------------------------------
def raw(ix, Q, radii, arg, flags, words, stride, n_filters, n_bits, fo, cap=0, ids=None, dist=None, probed=True):
    """one call of the C ABI (host pointers) -> (rc, limits, total); limits start as a sentinel"""
    Q = np.ascontiguousarray(np.atleast_2d(Q), dtype=np.float32)
    b = Q.shape[0]
    r = capi.range_radii(radii, b)
    lims = np.full(b + 1, 0xABABABABABABABAB, dtype=np.uint64)
    total = C.c_uint64(77)
    fn = capi.lib().vers_ivf_range_search_filtered_multi if probed else capi.lib().vers_ivf_range_search_exhaustive_filtered_multi
    rc = fn(ix._h, capi._ptr(Q), 4 * ix.d, b, capi._ptr(r), arg, flags, capi._ptr(words) if words is not None else None, stride, n_filters, n_bits,
            capi._ptr(fo) if fo is not None else None, capi._ptr(lims), capi._ptr(ids) if ids is not None else None,
            capi._ptr(dist) if dist is not None else None, cap, C.byref(total))
    return rc, lims, int(total.value)


def test_nan_counts_only_for_the_queries_allowed_the_row():
    src = make(1500, 48, 6, seed=0xFC30)
    ix = IVFFlatIndex(48)
    try:
        bad = int(src.ids[2][70])   # a row in the second tile of list 2
        ix.num_centroids, ix.centroids, ix.assignments, ix.ids = src.num_centroids, src.centroids, src.assignments, [list(l) for l in src.ids]
        ix.values = src.values.copy()
        ix.values[bad, 7] = np.nan
        ix._upload()
        Q = queries(src, 0xFC31, 9)
        clean = random_filter(1500, 0.5, 0xFC32)
        clean[[int(v) for v in src.ids[2][64:128]]] = True   # the rest of its tile is allowed: the tile IS loaded
        clean[bad] = False
        dirty = clean.copy()
        dirty[bad] = True
        case = Case(ix, Q, [dirty, clean], 1500, 1500)
        ones = np.ones(9, dtype=np.uint32)
        # the NaN row is allowed by bitmap 0 alone, and no query uses bitmap 0: VERS_OK
        for qs in (list(range(9)), [0]):
            check(case, qs, ones[:len(qs)], INF, 6)
            check(case, qs, ones[:len(qs)], INF, None)
        # ... or only a query that does not probe its list (nprobe 1; no per-call cross-check: that call scans it for the other queries)
        far = next(q for q in range(9) if int(co.search_exhaustive(ix.centroids, Q[q], 6, ix.metric)[0][0]) != 2)
        fo = ones.copy(); fo[far] = 0
        check(case, range(9), fo, INF, 1, cross=False)
        # one query on bitmap 0 and scanning the row: VERS_ERR_NAN on both calls, batch and single, outputs untouched
        for qs, f in ((list(range(9)), fo), ([far], np.zeros(1, dtype=np.uint32))):
            for probed in (True, False):
                ids = np.full(1500 * 9, SENT, dtype=np.uint64); dist = np.full(1500 * 9, -7.25, dtype=np.float32)
                rc, lims, _ = raw(ix, Q[qs], INF, 6 if probed else L2, 0, case.words, case.words.shape[1], 2, 1500, f, ids.size, ids, dist, probed=probed)
                assert rc == capi.ERR_NAN, (probed, qs)
                assert np.all(ids == SENT) and np.all(dist == np.float32(-7.25)) and np.all(lims == 0xABABABABABABABAB)
        check(case, range(9), ones, INF, 6)   # and the handle is still usable
    finally:
        ix.close()
        src.close()


# ---- 10. protocol and errors ------------------------------------------------------------------------------------------------------------------
def test_protocol_and_errors(main_case):
    import torch
    case = main_case
    ix, n = case.ix, N_MAIN
    qs = list(range(8))
    Q = case.Q[qs]
    words = case.words
    need = words.shape[1]
    fo = (np.arange(8) % 5).astype(np.uint32)
    big = capi.allowed_bitmaps([np.ones(n, dtype=bool)] * 65, n)
    INV = capi.ERR_INVALID
    for probed in (True, False):
        arg = 4 if probed else L2
        radii = np.asarray([case.refs[fo[i]].mth(q, 4, 10) for i, q in enumerate(qs)], dtype=np.float32)
        want = check(case, qs, fo, radii, 4 if probed else None)
        total = int(want[0][-1])
        assert total >= 80
        # the size query: cap == 0 with NULL arrays
        rc, lims, got = raw(ix, Q, radii, arg, 0, words, need, 5, n, fo, probed=probed)
        assert rc == capi.OK and got == total and np.array_equal(lims, want[0])
        # one short: VERS_OK, the total, complete limits, ids / distances untouched
        ids = np.full(total, SENT, dtype=np.uint64); dist = np.full(total, -7.25, dtype=np.float32)
        rc, lims, got = raw(ix, Q, radii, arg, 0, words, need, 5, n, fo, total - 1, ids, dist, probed=probed)
        assert rc == capi.OK and got == total and np.array_equal(lims, want[0])
        assert np.all(ids == SENT) and np.all(dist == np.float32(-7.25))
        # exactly enough
        rc, lims, got = raw(ix, Q, radii, arg, 0, words, need, 5, n, fo, total, ids, dist, probed=probed)
        assert rc == capi.OK and got == total and np.array_equal(ids, want[1]) and np.array_equal(bits(dist), bits(want[2]))
        # argument errors: the range calls' ...
        assert raw(ix, Q, radii, arg, 2, words, need, 5, n, fo, probed=probed)[0] == INV          # unknown flag bits
        assert raw(ix, Q, radii, arg, 0, words, need, 5, n, fo, 5, probed=probed)[0] == INV       # a capacity without arrays
        nan_r = radii.copy(); nan_r[3] = np.nan
        assert raw(ix, Q, nan_r, arg, 0, words, need, 5, n, fo, probed=probed)[0] == INV          # a NaN radius
        # ... and the _multi calls'
        assert raw(ix, Q, radii, arg, 0, words, need, 0, n, fo, probed=probed)[0] == INV          # n_filters == 0 with b > 0
        assert raw(ix, Q, radii, arg, 0, big, need, 65, n, fo, probed=probed)[0] == INV           # n_filters > VERS_FILTER_MAX
        assert raw(ix, Q, radii, arg, 0, big, need, 64, n, fo, probed=probed)[0] == capi.OK
        assert raw(ix, Q, radii, arg, 0, None, need, 5, n, fo, probed=probed)[0] == INV           # n_bits > 0 with NULL filters
        assert raw(ix, Q, radii, arg, 0, words, need, 5, n, None, probed=probed)[0] == INV        # NULL filter_of with b > 0
        assert raw(ix, Q, radii, arg, 0, words, need - 1, 5, n, fo, probed=probed)[0] == INV      # a stride too small
        bad = fo.copy(); bad[5] = 5
        assert raw(ix, Q, radii, arg, 0, words, need, 5, n, bad, probed=probed)[0] == INV         # a host filter_of entry equal to n_filters
    assert raw(ix, Q, 1.0, 0, 0, words, need, 5, n, fo)[0] == INV                                 # nprobe == 0
    assert raw(ix, Q, 1.0, 2, 0, words, need, 5, n, fo, probed=False)[0] == INV                   # metric > VERS_METRIC_COSDIST
    # the _dev calls refuse the same before the device is touched
    dev = torch.device("cuda", ix.device)
    qd = torch.from_numpy(Q).to(dev); wd = torch.from_numpy(words.view(np.int64).copy()).to(dev); fd = torch.from_numpy(fo.view(np.int32).copy()).to(dev)
    rd = torch.ones(8, dtype=torch.float32, device=dev); ld = torch.zeros(9, dtype=torch.int64, device=dev)
    nan_d = torch.full((8,), float("nan"), dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)
    w, f_ = wd.data_ptr(), fd.data_ptr()
    #        radius         arg(p) arg(x) flags filters stride n_filters n_bits filter_of
    rows = ((rd.data_ptr(), 0, 2, 0, w, need, 5, n, f_), (rd.data_ptr(), 4, L2, 2, w, need, 5, n, f_), (rd.data_ptr(), 4, L2, 0, w, need, 0, n, f_),
            (rd.data_ptr(), 4, L2, 0, w, need, 65, n, f_), (rd.data_ptr(), 4, L2, 0, 0, need, 5, n, f_), (rd.data_ptr(), 4, L2, 0, w, need, 5, n, 0),
            (rd.data_ptr(), 4, L2, 0, w, need - 1, 5, n, f_), (nan_d.data_ptr(), 4, L2, 0, w, need, 5, n, f_))
    for r, ap, ax, flags, *rest in rows:
        with pytest.raises(capi.VersError) as e:
            ix.range_search_filtered_multi_dev(qd.data_ptr(), ix.d, 8, r, ap, flags, *rest, ld.data_ptr(), 0, 0, 0)
        assert e.value.status == INV, (ap, flags, rest)
        with pytest.raises(capi.VersError) as e:
            ix.range_search_exhaustive_filtered_multi_dev(qd.data_ptr(), ix.d, 8, r, ax, flags, *rest, ld.data_ptr(), 0, 0, 0)
        assert e.value.status == INV, (ax, flags, rest)
    # b == 0: a no-op, *out_total = 0
    Lb = capi.lib()
    for fn, arg in ((Lb.vers_ivf_range_search_filtered_multi, 4), (Lb.vers_ivf_range_search_exhaustive_filtered_multi, L2)):
        t = C.c_uint64(99)
        assert fn(ix._h, None, 4 * ix.d, 0, None, arg, 0, capi._ptr(words), need, 5, n, None, None, None, None, 0, C.byref(t)) == capi.OK and t.value == 0
    for fn, arg in ((Lb.vers_ivf_range_search_filtered_multi_dev, 4), (Lb.vers_ivf_range_search_exhaustive_filtered_multi_dev, L2)):
        t = C.c_uint64(99)
        assert fn(ix._h, None, ix.d, 0, None, arg, 0, None, 0, 0, 0, None, None, None, None, 0, C.byref(t), None) == capi.OK and t.value == 0
    # an index without centroids: the probed call has nothing to rank, the exhaustive call finds nothing
    empty = IVFFlatIndex(ix.d)
    assert raw(empty, Q, INF, 4, 0, words, need, 5, n, fo)[0] == capi.ERR_INSUFFICIENT
    rc, lims, got = raw(empty, Q, INF, L2, 0, words, need, 5, n, fo, probed=False)
    assert rc == capi.OK and got == 0 and not lims.any()
    empty.close()
    # a handle sharded by cluster is refused
    sh = make(600, 32, 4, seed=0xFC41)
    Qs = queries(sh, 0xFC42, 3)
    w600 = capi.allowed_bitmaps([np.ones(600, dtype=bool)] * 2, 600)
    f3 = np.asarray([0, 1, 0], dtype=np.uint32)
    half = IVFFlatIndex(sh.d)
    half.set_shard(0, 2)
    half.num_centroids, half.values, half.centroids, half.assignments = sh.num_centroids, sh.values, sh.centroids, sh.assignments
    half._upload()
    rc, _, got = raw(sh, Qs, INF, 2, 0, w600, w600.shape[1], 2, 600, f3)
    assert rc == capi.OK and got > 0
    assert half.info()[1] == 4 and raw(half, Qs, INF, 2, 0, w600, w600.shape[1], 2, 600, f3)[0] == INV
    assert "out of scope" in capi.lib().vers_last_error().decode("utf-8", "replace")
    assert raw(half, Qs, INF, L2, 0, w600, w600.shape[1], 2, 600, f3, probed=False)[0] == INV
    half.close()
    sh.close()


def test_dev_call_out_of_range_filter_of_selects_the_empty_filter(main_case):
    case = main_case
    b = 17
    qs = list(range(b))
    fo = (np.arange(b) % 3).astype(np.uint32)
    out = [2, 9, 16]
    bad = fo.copy(); bad[out] = [3, 64, 0xFFFFFFFF]   # n_filters = 3: equal to it, the first bit position beyond a word, the largest value
    rest = np.setdiff1d(np.arange(b), out)
    for nprobe in (4, None):
        want = check(case, qs, fo, INF, nprobe)
        for walk in (False, True):
            got = dev_call(case, case.Q[:b], INF, nprobe, L2, bad, walk, n_filters=3)
            cnt = np.diff(got[0].astype(np.int64))
            assert not cnt[out].any() and cnt[rest].all(), nprobe
            if not walk:
                same_segments(got, want, rest, ("out of range", nprobe))
        # a single query on an out-of-range entry
        got = dev_call(case, case.Q[:1], INF, nprobe, L2, np.asarray([7], dtype=np.uint32), False, n_filters=3)
        assert not got[0].any() and got[1].size == 0


# ---- 11. _dev calls on two streams --------------------------------------------------------------------------------------------------------------
def test_device_pointer_calls_on_two_streams(main_case):
    import torch
    case = main_case
    ix = case.ix
    qs = list(range(17))
    dev = torch.device("cuda", ix.device)
    streams = (torch.cuda.Stream(dev), torch.cuda.Stream(dev))
    fos = ((np.arange(17) % 5).astype(np.uint32), (4 - np.arange(17) % 5).astype(np.uint32))   # a filter_of per stream
    radii = [mixed_radii(case, qs, fo, 4) for fo in fos]
    for nprobe in (4, None):
        for walk in (False, True):
            for rnd in range(2):       # interleaved: stream 0, stream 1, stream 0, stream 1
                for s in (0, 1):
                    got = dev_call(case, case.Q[qs], radii[s], nprobe, L2, fos[s], walk, stream=streams[s])
                    same(got, [case.refs[fos[s][i]].want(q, radii[s][i], nprobe, L2, walk) for i, q in enumerate(qs)], (nprobe, walk, s, rnd))


# ---- 12. the workspace lease is clean -----------------------------------------------------------------------------------------------------------
def test_other_calls_are_unchanged_around_the_new_calls(main_case):
    case = main_case
    ix, Q = case.ix, case.Q
    one = (np.ascontiguousarray(case.words[0]), N_MAIN)
    all5 = (case.words, N_MAIN)
    fo = np.arange(40) % 5
    radii = mixed_radii(case, range(40), fo, 4)

    def others():
        topk = [ix.search_batch(Q, top_k, nprobe) for top_k, nprobe in ((10, 4), (10, 0), (100, 4))] + [ix.search_batch(Q[0], 10, 4)]
        topk += [ix.search_filtered(Q, 10, 4, one), ix.search_exhaustive_filtered(Q[:9], 70, one)]
        topk += [ix.search_filtered_multi(Q, 10, 4, all5, fo), ix.search_exhaustive_filtered_multi(Q[:9], 70, all5, fo[:9])]
        rng = [ix.range_search(Q, radii, 4), ix.range_search(Q[0], radii[0], 4, walk_order=True), ix.range_search_exhaustive(Q[:9], radii[:9]),
               ix.range_search_filtered(Q, radii, 4, one), ix.range_search_exhaustive_filtered(Q[:9], radii[:9], one, walk_order=True)]
        return topk, rng

    def the_same(x, y):
        for (i0, d0, c0), (i1, d1, c1) in zip(x[0], y[0]):
            assert np.array_equal(c0, c1)
            for q in range(len(c0)):
                assert np.array_equal(i0[q, :c0[q]], i1[q, :c0[q]]) and np.array_equal(bits(d0[q, :c0[q]]), bits(d1[q, :c0[q]]))
        for (l0, i0, d0), (l1, i1, d1) in zip(x[1], y[1]):
            assert np.array_equal(l0, l1) and np.array_equal(i0, i1) and np.array_equal(bits(d0), bits(d1)) and l0[-1] > 0

    before = others()
    check(case, range(40), fo, radii, 4); check(case, [0], [3], INF, 12)
    between = others()
    check(case, range(9), fo[:9], radii[:9], None); check(case, range(17), fo[:17], radii[:17], 4, calls=(dev_call,))
    after = others()
    the_same(before, between)
    the_same(before, after)


# ---- 13. the measurement hooks ------------------------------------------------------------------------------------------------------------------
def test_stats_hook(main_ix):
    ix, n = main_ix, N_MAIN
    lists = [np.asarray(l, dtype=np.int64) for l in ix.ids]
    live = np.concatenate(lists)
    Q = queries(ix, 0xFC50, 9)
    selective = np.arange(1000, 1400)
    everything = np.ones(n, dtype=bool)
    nothing = np.zeros(0, dtype=np.int64)
    some = random_filter(n, 0.2, 0xFC51)
    case = Case(ix, Q, [selective, everything, nothing, some], n, n)
    # [3]: the allowed (bitmap, storage row) pairs, from the bitmaps and the lists
    sems = [allowed_set(n, a, n) for a in (selective, everything, nothing, some)]
    pairs = sum(int(s[live].sum()) for s in sems)
    assert live.size == n and pairs == 400 + n + 0 + int(some.sum())
    head = ("tiles_planned", "tiles_loaded", "items_skipped")
    for seg_rows in (0, 64):
        capi.set_option("seg_rows", seg_rows)
        case.fresh()
        try:
            for qs in (list(range(9)), [4]):
                b = len(qs)
                for nprobe in (4, None):
                    fo = np.arange(b) % 4
                    t0 = ix.filter_stats()["total"]
                    stats = []
                    for radii in (mixed_radii(case, qs, fo, 4), np.full(b, INF)):   # two radii: the count pass alone feeds [0..2]
                        rc, _, total = raw(ix, Q[qs], radii, 4 if nprobe else L2, 0, case.words, case.words.shape[1], 4, n, fo.astype(np.uint32), probed=nprobe is not None)
                        assert rc == capi.OK
                        stats.append(ix.filter_stats()["last"])
                    a, c = stats
                    assert a == c, (a, c)
                    assert a["tiles_loaded"] <= a["tiles_planned"] and a["tiles_planned"] > 0 and a["rows_allowed"] == pairs
                    t1 = ix.filter_stats()["total"]
                    assert {k: t1[k] - t0[k] for k in t1} == {k: 2 * a[k] for k in a}
                    # every query on the all-ones bitmap: every planned tile of a probed list is loaded
                    ones = np.ones(b, dtype=np.uint32)
                    rc, _, total = raw(ix, Q[qs], INF, 4 if nprobe else L2, 0, case.words, case.words.shape[1], 4, n, ones, probed=nprobe is not None)
                    assert rc == capi.OK and total > 0
                    st = ix.filter_stats()["last"]
                    if nprobe is not None:
                        assert st["tiles_loaded"] == st["tiles_planned"] > 0 and st["items_skipped"] == 0, st
                    else:   # every group of queries walks every tile that holds a vector once (storage slack: planned and never loaded)
                        held = sum((len(l) + 63) // 64 for l in lists)
                        assert st["tiles_loaded"] >= held and st["tiles_loaded"] % held == 0 and st["tiles_planned"] >= st["tiles_loaded"], st
                        assert b > 1 or st["tiles_loaded"] == held, st
                    # ... equal filter_of: planned, loaded and skipped are the per-call call's with that bitmap
                    for f in (0, 2, 3):
                        case.per_call(f, qs, np.full(b, INF), nprobe, L2, False)
                        case.fresh()
                        one = ix.filter_stats()["last"]
                        check(case, qs, np.full(b, f), INF, nprobe, cross=False)
                        multi = ix.filter_stats()["last"]
                        assert [multi[k] for k in head] == [one[k] for k in head], (seg_rows, b, nprobe, f, multi, one)
                        assert one["rows_allowed"] == int(sems[f][live].sum()) and multi["rows_allowed"] == pairs
                        if f == 2:   # all queries on an empty bitmap: nothing loaded, every item counted skipped
                            assert multi["tiles_loaded"] == 0 and multi["items_skipped"] > 0
                        if f == 0:
                            assert multi["tiles_loaded"] < multi["tiles_planned"]
        finally:
            capi.set_option("seg_rows", 0)


def test_a_failed_call_leaves_the_stats_where_they_were():
    src = make(1500, 48, 6, seed=0xFC60)
    ix = IVFFlatIndex(48)
    try:
        ix.num_centroids, ix.centroids, ix.assignments, ix.ids = src.num_centroids, src.centroids, src.assignments, [list(l) for l in src.ids]
        ix.values = src.values.copy()
        ix.values[int(src.ids[2][70]), 7] = np.nan
        ix._upload()
        Q = queries(src, 0xFC61, 3)
        ok = np.ones(1500, dtype=bool); ok[int(src.ids[2][70])] = False
        words = capi.allowed_bitmaps([ok, np.ones(1500, dtype=bool)], 1500)
        fo = np.zeros(3, dtype=np.uint32)
        assert raw(ix, Q, INF, 6, 0, words, words.shape[1], 2, 1500, fo)[0] == capi.OK
        tot = ix.filter_stats()["total"]
        assert tot["tiles_planned"] > 0
        assert raw(ix, Q, INF, 6, 0, words, words.shape[1], 2, 1500, fo + 1)[0] == capi.ERR_NAN
        assert ix.filter_stats()["total"] == tot   # (the call's counters are folded into the handle's only when it succeeds)
    finally:
        ix.close()
        src.close()


def test_phases_and_scan_timing_ring(main_case):
    case = main_case
    ix = case.ix
    Q = case.Q[:8]
    fo = (np.arange(8) % 5).astype(np.uint32)
    radii = np.asarray([case.refs[fo[q]].mth(q, 4, 10) for q in range(8)], dtype=np.float32)
    words, need = case.words, case.words.shape[1]
    ix.scan_times(reset=True)
    for probed in (True, False):
        arg = 4 if probed else L2
        # a size query: ONE call of the C ABI, the count pass alone
        capi.range_phases(reset=True)
        rc, lims, total = raw(ix, Q, radii, arg, 0, words, need, 5, N_MAIN, fo, probed=probed)
        assert rc == capi.OK and total >= 80
        ph = capi.range_phases(reset=True)
        assert (ph["calls"], ph["queries"], ph["results"]) == (1, 8, total)
        assert ph["count_ms"] > 0 and ph["plan_ms"] > 0
        ring = ix.scan_times(reset=True)
        assert ring.size == 1 and ring[0] > 0, (probed, ring)    # the mask kernel's record, none for the range passes
        # both passes and the sort: the phases grow by the call's values again, still one record
        ids = np.zeros(total, dtype=np.uint64); dist = np.zeros(total, dtype=np.float32)
        rc, _, got = raw(ix, Q, radii, arg, 0, words, need, 5, N_MAIN, fo, total, ids, dist, probed=probed)
        assert rc == capi.OK and got == total
        ph = capi.range_phases(reset=True)
        assert (ph["calls"], ph["queries"], ph["results"]) == (1, 8, total)
        assert ph["count_ms"] > 0 and ph["fill_ms"] > 0 and ph["sort_ms"] > 0 and ph["plan_ms"] > 0 and ph["scan_ms"] > 0
        assert ix.scan_times(reset=True).size == 1
