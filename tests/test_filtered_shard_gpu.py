"""Filtered search on handles sharded by cluster, emulated on ONE GPU the way tests/test_range_shard_gpu.py emulates the sharded range search:
`world` handles each keep only their lists.  Every shard's partial -- vers_ivf_search_filtered_partial_dev and its exhaustive and range twins
-- is laid out the way the all-gather lays it out and merged with vers_topk_merge_dev / vers_range_merge_dev UNCHANGED.  The result must
equal, in np.array_equal, what the EXISTING filtered call returns on the unsharded handle (ids, distance bits, counts / limits), and for
three queries what the oracle returns on the index with the disallowed ids removed.  The adaptive depth needs every list's allowed count:
the shards' vers_ivf_filter_allowed_len_dev arrays add up to the unsharded handle's, and the partials planned from the sum give the
unsharded adaptive call's results and out_nprobe."""
import ctypes as C

import numpy as np
import pytest

from oracle import c_oracle as co
from tests.test_range_shard_gpu import B, INF, WALK, Case, bits, dev_i64, reshard
from vers_amd import capi
from vers_amd.index import IVFFlatIndex

pytestmark = pytest.mark.gpu

N, D, K = 3000, 40, 24   # (d = 40: the row length is padded; two extra adds make n = 3002)
TOP_KS = (1, 10, 70)     # (70: past 64 ranks, two passes)
NPROBES = (1, 5, 24)     # (24: every list)
AD_MIN, AD_MAX, AD_ALLOWED = 2, 24, 10


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        return dev_i64(a)
    if a.dtype == np.uint32:
        return torch.from_numpy(a.view(np.int32)).cuda()
    return torch.from_numpy(a).cuda()


class Filt:
    """Bitmaps on the device in the _multi form + what they mean on the host.  filter_of None: one bitmap for the batch (the per-call kernels)."""

    def __init__(self, name, sets, n_bits, n, filter_of=None):
        self.name, self.n_bits = name, int(n_bits)
        sets = [np.asarray(s, dtype=bool) for s in sets]
        self.words = capi.allowed_bitmaps([s[:n_bits] for s in sets], self.n_bits) if self.n_bits else np.zeros((len(sets), 0), np.uint64)
        self.n_filters, self.stride = len(sets), (self.words.shape[1] if self.words.size else 0)
        self.wd = dev(self.words) if self.words.size else None
        self.filter_of = None if filter_of is None else np.asarray(filter_of, dtype=np.uint32)
        self.fod = None if filter_of is None else dev(self.filter_of)
        self.sem = []   # per bitmap: allowed[v] over the n vec ids, ids at or beyond n_bits not allowed
        for s in sets:
            a = np.zeros(n, dtype=bool)
            m = min(n, self.n_bits, s.size)
            a[:m] = s[:m]
            self.sem.append(a)

    @property
    def t(self):
        return (self.wd.data_ptr() if self.wd is not None else 0, self.stride, self.n_filters, self.n_bits, self.fod.data_ptr() if self.fod is not None else 0)

    def sem_of(self, q):
        """allowed[v] for query q (the empty filter for an entry of filter_of at or beyond n_filters)"""
        f = 0 if self.filter_of is None else int(self.filter_of[q])
        return self.sem[f] if f < self.n_filters else np.zeros_like(self.sem[0])


def make_filters(n):
    rng = np.random.default_rng(0xF17)
    ones = np.ones(n, bool)
    r30 = rng.random(n) < 0.30
    r02 = rng.random(n) < 0.02
    span = np.zeros(n, bool); span[700:1900] = True
    half = rng.random(n) < 0.5
    per_call = [Filt("ones", [ones], n, n), Filt("empty", [ones], 0, n), Filt("r30", [r30], n, n), Filt("r02", [r02], n, n), Filt("span", [span], n, n),
                Filt("short", [half], 2000, n)]
    fo3 = np.arange(B, dtype=np.uint32) % 3; fo3[11] = 7        # one entry at or beyond n_filters: the empty filter
    f3 = Filt("F3", [r02, r30, span], n, n, fo3)
    fo64 = np.arange(B, dtype=np.uint32) % 64; fo64[20] = 64
    f64 = Filt("F64", [rng.random(n) < (0.01 + 0.015 * f) for f in range(64)], n, n, fo64)
    return per_call, f3, f64


class Env:
    def __init__(self, world, per_rank):
        self.case = Case(N, D, K, world, 0x51, built_per_rank=per_rank)
        self.n = self.case.whole.values.shape[0]
        self.per_call, self.f3, self.f64 = make_filters(self.n)

    def close(self):
        self.case.close()


@pytest.fixture(scope="module", params=[(2, True), (3, True), (1, False), (5, False), (30, False)], ids=lambda p: f"w{p[0]}{'b' if p[1] else 'r'}")
def env(request):
    e = Env(*request.param)
    yield e
    e.close()


@pytest.fixture(scope="module")
def env2():
    e = Env(2, True)
    yield e
    e.close()


# ---- the unsharded handle's EXISTING filtered calls (device pointers: filter_of entries beyond n_filters included) ----
def whole_topk(case, top_k, nprobe, f, metric=None, adaptive=False):
    import torch
    ix, Qd = case.whole, case.Qd
    ids = torch.zeros(B, top_k, dtype=torch.int64, device="cuda"); dist = torch.zeros(B, top_k, device="cuda")
    cnt = torch.zeros(B, dtype=torch.int32, device="cuda"); npr = torch.zeros(B, dtype=torch.int32, device="cuda")
    wp = f.wd.data_ptr() if f.wd is not None else 0
    if f.filter_of is None:
        if adaptive:
            ix.search_filtered_adaptive_dev(Qd.data_ptr(), case.d, B, top_k, AD_MIN, nprobe, AD_ALLOWED, wp, f.n_bits, ids.data_ptr(), dist.data_ptr(), cnt.data_ptr(), npr.data_ptr())
        elif metric is None:
            ix.search_filtered_dev(Qd.data_ptr(), case.d, B, top_k, nprobe, wp, f.n_bits, ids.data_ptr(), dist.data_ptr(), cnt.data_ptr())
        else:
            ix.search_exhaustive_filtered_dev(Qd.data_ptr(), case.d, B, top_k, metric, wp, f.n_bits, ids.data_ptr(), dist.data_ptr(), cnt.data_ptr())
    else:
        fo = f.fod.data_ptr()
        if adaptive:
            ix.search_filtered_multi_adaptive_dev(Qd.data_ptr(), case.d, B, top_k, AD_MIN, nprobe, AD_ALLOWED, wp, f.stride, f.n_filters, f.n_bits, fo, ids.data_ptr(),
                                                  dist.data_ptr(), cnt.data_ptr(), npr.data_ptr())
        elif metric is None:
            ix.search_filtered_multi_dev(Qd.data_ptr(), case.d, B, top_k, nprobe, wp, f.stride, f.n_filters, f.n_bits, fo, ids.data_ptr(), dist.data_ptr(), cnt.data_ptr())
        else:
            ix.search_exhaustive_filtered_multi_dev(Qd.data_ptr(), case.d, B, top_k, metric, wp, f.stride, f.n_filters, f.n_bits, fo, ids.data_ptr(), dist.data_ptr(),
                                                    cnt.data_ptr())
    torch.cuda.synchronize()
    ix.poll()
    return ids.cpu().numpy().view(np.uint64), dist.cpu().numpy(), cnt.cpu().numpy().view(np.uint32), npr.cpu().numpy().view(np.uint32)


def whole_range(case, radii, nprobe, flags, f, metric=None):
    import torch
    ix, Qd = case.whole, case.Qd
    rd = dev(np.ascontiguousarray(radii, dtype=np.float32))
    wp = f.wd.data_ptr() if f.wd is not None else 0

    def call(lims, ids, dist, cap):
        a = (Qd.data_ptr(), case.d, B, rd.data_ptr(), nprobe if metric is None else metric, flags)
        z = (lims.data_ptr(), ids.data_ptr() if ids is not None else 0, dist.data_ptr() if dist is not None else 0, cap)
        if f.filter_of is None:
            fn = ix.range_search_filtered_dev if metric is None else ix.range_search_exhaustive_filtered_dev
            return fn(*a, wp, f.n_bits, *z)
        fn = ix.range_search_filtered_multi_dev if metric is None else ix.range_search_exhaustive_filtered_multi_dev
        return fn(*a, wp, f.stride, f.n_filters, f.n_bits, f.fod.data_ptr(), *z)

    lims = torch.zeros(B + 1, dtype=torch.int64, device="cuda")
    total = call(lims, None, None, 0)
    ids = torch.zeros(max(total, 1), dtype=torch.int64, device="cuda"); dist = torch.zeros(max(total, 1), device="cuda")
    assert call(lims, ids, dist, total) == total
    return lims.cpu().numpy().view(np.uint64), ids.cpu().numpy().view(np.uint64)[:total], dist.cpu().numpy()[:total]


# ---- the shards' partials, merged ----
def allowed_counts(case, f):
    """every shard's vers_ivf_filter_allowed_len_dev -> [world][n_filters * k] i32 on the device"""
    import torch
    out = torch.full((case.world, f.n_filters * case.k), -1, dtype=torch.int32, device="cuda")
    for r, ix in enumerate(case.shards):
        ix.filter_allowed_len_dev(f.wd.data_ptr() if f.wd is not None else 0, f.stride, f.n_filters, f.n_bits, out[r].data_ptr())
    torch.cuda.synchronize()
    return out


def sharded_topk(case, top_k, nprobe, f, metric=None, adaptive=False):
    import torch
    world = case.world
    buf = torch.full((world, 2, B, top_k), -9, dtype=torch.int64, device="cuda")
    nps = torch.full((world, B), -1, dtype=torch.int32, device="cuda")
    total = allowed_counts(case, f).sum(0, dtype=torch.int32).contiguous() if adaptive else None
    for r, ix in enumerate(case.shards):
        if metric is None:
            ad = (AD_MIN, AD_ALLOWED, total.data_ptr(), nps[r].data_ptr()) if adaptive else None
            ix.search_filtered_partial_dev(case.Qd.data_ptr(), case.d, B, top_k, nprobe, f.t, buf[r, 0].data_ptr(), buf[r, 1].data_ptr(), adaptive=ad)
        else:
            ix.search_exhaustive_filtered_partial_dev(case.Qd.data_ptr(), case.d, B, top_k, metric, f.t, buf[r, 0].data_ptr(), buf[r, 1].data_ptr())
    ids = torch.full((B, top_k), -5, dtype=torch.int64, device="cuda"); dist = torch.full((B, top_k), -7.25, device="cuda")
    cnt = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    IVFFlatIndex.merge_partials_dev(buf.data_ptr(), buf[0, 1].data_ptr(), 2 * B * top_k, world, B, top_k, 1, ids.data_ptr(), dist.data_ptr(), cnt.data_ptr())
    torch.cuda.synchronize()
    for ix in case.shards:
        ix.poll()
    return ids.cpu().numpy().view(np.uint64), dist.cpu().numpy(), cnt.cpu().numpy().view(np.uint32), nps.cpu().numpy().view(np.uint32)


def same_topk(got, want, what):
    assert np.array_equal(got[2], want[2]), (what, "counts", got[2], want[2])
    live = np.arange(got[0].shape[1])[None, :] < want[2][:, None]
    assert np.array_equal(got[0][live], want[0][live]), (what, "ids")
    assert np.array_equal(bits(got[1])[live], bits(want[1])[live]), (what, "distance bits")


def sharded_range(case, radii, nprobe, flags, f, metric=None):
    import torch
    world = case.world
    rd = dev(np.ascontiguousarray(radii, dtype=np.float32))
    lims = torch.zeros(world, B + 1, dtype=torch.int64, device="cuda")
    totals = [ix.range_search_filtered_partial_dev(case.Qd.data_ptr(), case.d, B, rd.data_ptr(), nprobe, flags, f.t, lims[r].data_ptr(), 0, 0, 0,
                                                   exhaustive_metric=metric) for r, ix in enumerate(case.shards)]   # the size query
    t_max = max(totals)
    buf = torch.full((world, 2, max(t_max, 1)), -1, dtype=torch.int64, device="cuda")
    for r, ix in enumerate(case.shards):
        l2 = torch.zeros(B + 1, dtype=torch.int64, device="cuda")
        got = ix.range_search_filtered_partial_dev(case.Qd.data_ptr(), case.d, B, rd.data_ptr(), nprobe, flags, f.t, l2.data_ptr(), buf[r, 0].data_ptr(),
                                                   buf[r, 1].data_ptr(), totals[r], exhaustive_metric=metric)
        assert got == totals[r] and torch.equal(l2, lims[r]) and int(l2[B]) == got
    total = int(lims[:, B].sum())
    o_lims = torch.full((B + 1,), -3, dtype=torch.int64, device="cuda")
    o_ids = torch.full((total + 8,), -5, dtype=torch.int64, device="cuda"); o_dist = torch.full((total + 8,), -7.25, device="cuda")
    IVFFlatIndex.merge_range_partials_dev(buf.data_ptr(), buf[0, 1].data_ptr(), 2 * max(t_max, 1), lims.data_ptr(), world, B, flags, o_lims.data_ptr(),
                                          o_ids.data_ptr(), o_dist.data_ptr())
    torch.cuda.synchronize()
    assert bool((o_ids[total:] == -5).all()) and bool((o_dist[total:] == -7.25).all())
    return o_lims.cpu().numpy().view(np.uint64), o_ids.cpu().numpy().view(np.uint64)[:total], o_dist.cpu().numpy()[:total]


def same_range(got, want, what):
    assert np.array_equal(got[0], want[0]), (what, "lims")
    assert np.array_equal(got[1], want[1]), (what, "ids")
    assert np.array_equal(bits(got[2]), bits(want[2])), (what, "distance bits")


def grid(env):
    """the whole cross product on the worlds built rank by rank; on the resharded ones (1, 5, 30 ranks) every value of every axis once"""
    if env.case.world in (2, 3):
        return [(t, p) for t in TOP_KS for p in NPROBES]
    return [(1, 24), (10, 5), (70, 1), (70, 24)]


# ---- top-k ----
def test_probed_partials_merge_to_the_unsharded_result(env):
    case = env.case
    if case.world == 30:
        assert len({int(o) for o in case.owners}) < 30   # some ranks own no list
    for f in env.per_call + [env.f3, env.f64]:
        for top_k, nprobe in grid(env):
            want = whole_topk(case, top_k, nprobe, f)
            same_topk(sharded_topk(case, top_k, nprobe, f), want, (case.world, f.name, top_k, nprobe))
            # the 2 % filter allows ~60 rows, ~2.5 per list: top_k = 70 is short everywhere, top_k = 10 in most queries' nearest list
            if f.name == "r02" and (top_k == 70 or (top_k == 10 and nprobe == 1)):
                assert int((want[2] < top_k).sum()) > B // 2
    assert np.array_equal(whole_topk(case, 10, 5, env.per_call[1])[2], np.zeros(B, np.uint32))   # n_bits == 0: nothing is allowed


def test_exhaustive_partials_merge_to_the_unsharded_result(env):
    case = env.case
    for metric in (capi.METRIC_L2SQ, capi.METRIC_COSDIST):
        for f in env.per_call + [env.f3, env.f64]:
            for top_k in (TOP_KS if case.world in (2, 3) else (10, 70)):
                want = whole_topk(case, top_k, 0, f, metric=metric)
                same_topk(sharded_topk(case, top_k, 0, f, metric=metric), want, (case.world, f.name, top_k, "exhaustive", metric))


def test_three_queries_against_the_oracle(env2):
    """the virtual removal itself: the oracle on the index with the disallowed ids removed"""
    case, whole = env2.case, env2.case.whole
    for f in (env2.per_call[2], env2.per_call[5], env2.f3):
        got = sharded_topk(case, 10, 5, f)
        gx = sharded_topk(case, 10, 0, f, metric=capi.METRIC_L2SQ)
        for q in (0, 3, 36):
            sem = f.sem_of(q)
            ids_f = [[v for v in l if sem[v]] for l in whole.ids]
            rows = np.asarray(sorted(v for l in ids_f for v in l), dtype=np.int64)
            oi, od = co.search_nprobe(whole.values, whole.centroids, ids_f, case.Q[q], max(1, rows.size), 5)
            c = min(10, oi.size)
            assert got[2][q] == c and np.array_equal(got[0][q, :c], oi[:c]) and np.array_equal(bits(got[1][q, :c]), bits(od[:c])), (f.name, q)
            xi, xd = co.search_exhaustive(whole.values[rows], case.Q[q], rows.size, 0)
            c = min(10, rows.size)
            assert gx[2][q] == c and np.array_equal(gx[0][q, :c], rows[xi.astype(np.int64)][:c].astype(np.uint64)) and np.array_equal(bits(gx[1][q, :c]), bits(xd[:c]))


# ---- adaptive depth ----
def test_allowed_counts_add_up_and_adaptive_partials_match(env):
    import torch
    case = env.case
    one = Case.__new__(Case)
    one.whole, one.shards, one.world, one.d, one.k = case.whole, [case.whole], 1, case.d, case.k
    for f in (env.per_call[3], env.f3):
        local = allowed_counts(case, f)
        want_counts = allowed_counts(one, f)[0]
        assert torch.equal(local.sum(0, dtype=torch.int32), want_counts), f.name   # every list has one owner
        owners = np.repeat(case.owners[None, :].astype(np.int64), f.n_filters, 0).reshape(-1)
        lc = local.cpu().numpy()
        for r in range(case.world):
            assert not lc[r][owners != r].any()   # a list of another rank's is written as 0
        sem_counts = np.array([[int(f.sem[s][np.asarray(l, dtype=np.int64)].sum()) if len(l) else 0 for l in case.whole.ids] for s in range(f.n_filters)])
        assert np.array_equal(want_counts.cpu().numpy().reshape(f.n_filters, case.k), sem_counts)
        for top_k in (10, 70):
            want = whole_topk(case, top_k, AD_MAX, f, adaptive=True)
            got = sharded_topk(case, top_k, AD_MAX, f, adaptive=True)
            same_topk(got, want, (case.world, f.name, top_k, "adaptive"))
            for r in range(case.world):
                assert np.array_equal(got[3][r], want[3]), (f.name, r, "out_nprobe")
        # a plan that ignores the counts cannot pass: the depths differ between queries and some sit strictly between the bounds
        npr = want[3]
        assert len(set(npr.tolist())) >= 3 and bool(((npr > AD_MIN) & (npr < AD_MAX)).any()), npr


# ---- range ----
def test_range_partials_merge_to_the_unsharded_result(env):
    case = env.case
    full_grid = case.world in (2, 3)
    for f in env.per_call + [env.f3, env.f64]:
        for nprobe in (NPROBES if full_grid else (5,)):
            full = whole_range(case, np.full(B, INF, np.float32), nprobe, 0, f)
            for m in ((1, 10, 200) if full_grid and f.name in ("r30", "F3") else (10,)):
                radii = case.radii(full, m)   # radii EXACTLY on stored distances, one negative, one +inf
                for walk in (0, WALK):
                    want = whole_range(case, radii, nprobe, walk, f)
                    same_range(sharded_range(case, radii, nprobe, walk, f), want, (case.world, f.name, nprobe, m, walk))
                    assert want[0][6] == want[0][5] and want[0][8] - want[0][7] == full[0][8] - full[0][7]
        for metric in ((capi.METRIC_L2SQ, capi.METRIC_COSDIST) if full_grid else (capi.METRIC_L2SQ,)):
            full = whole_range(case, np.full(B, INF, np.float32), 0, 0, f, metric=metric)
            radii = case.radii(full, 10)
            if metric == capi.METRIC_COSDIST:
                radii[5] = np.float32(-5.0)
            same_range(sharded_range(case, radii, 0, 0, f, metric=metric), whole_range(case, radii, 0, 0, f, metric=metric), (case.world, f.name, "exhaustive", metric))


def test_range_against_the_oracle(env2):
    case, whole = env2.case, env2.case.whole
    f = env2.f3
    full = whole_range(case, np.full(B, INF, np.float32), 5, 0, f)
    radii = case.radii(full, 10)
    got = sharded_range(case, radii, 5, 0, f)
    for q in (0, 3, 36):
        sem = f.sem_of(q)
        ids_f = [[v for v in l if sem[v]] for l in whole.ids]
        oi, od = co.search_nprobe(whole.values, whole.centroids, ids_f, case.Q[q], max(1, int(sem.sum())), 5)
        keep = int(np.count_nonzero(od <= radii[q]))
        lo, hi = int(got[0][q]), int(got[0][q + 1])
        assert hi - lo == keep and np.array_equal(got[1][lo:hi], oi[:keep]) and np.array_equal(bits(got[2][lo:hi]), bits(od[:keep])), q


def test_cap_protocol_of_the_range_partial(env2):
    """the local total exceeds cap: VERS_OK, the limits complete, keys and ids untouched"""
    import torch
    case = env2.case
    rd = torch.full((B,), float("inf"), device="cuda")
    for f in (env2.per_call[2], env2.f3):
        for metric in (None, capi.METRIC_L2SQ):
            ix = case.shards[0]
            lims0 = torch.zeros(B + 1, dtype=torch.int64, device="cuda")
            total = ix.range_search_filtered_partial_dev(case.Qd.data_ptr(), case.d, B, rd.data_ptr(), 5, 0, f.t, lims0.data_ptr(), 0, 0, 0, exhaustive_metric=metric)
            assert total > 1
            keys = torch.full((total,), -11, dtype=torch.int64, device="cuda"); ids = torch.full((total,), -13, dtype=torch.int64, device="cuda")
            lims = torch.full((B + 1,), -3, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            got = ix.range_search_filtered_partial_dev(case.Qd.data_ptr(), case.d, B, rd.data_ptr(), 5, 0, f.t, lims.data_ptr(), keys.data_ptr(), ids.data_ptr(),
                                                       total - 1, exhaustive_metric=metric)
            assert got == total and torch.equal(lims, lims0) and int(lims[B]) == total and int(lims[0]) == 0
            assert bool((keys == -11).all()) and bool((ids == -13).all())


# ---- NULL g / comm on an unsharded handle: the existing filtered call ----
def test_sharded_calls_without_an_exchange_equal_the_existing_calls(env2):
    import torch
    case, ix = env2.case, env2.case.whole
    for f in (env2.per_call[2], env2.f3):
        for metric, adaptive in ((None, False), (None, True), (capi.METRIC_L2SQ, False)):
            ids = torch.full((B, 10), -5, dtype=torch.int64, device="cuda"); dist = torch.zeros(B, 10, device="cuda")
            cnt = torch.zeros(B, dtype=torch.int32, device="cuda"); npr = torch.zeros(B, dtype=torch.int32, device="cuda")
            if metric is None:
                ix.search_filtered_sharded_dev(None, case.Qd.data_ptr(), case.d, B, 10, AD_MAX if adaptive else 5, f.t, ids.data_ptr(), dist.data_ptr(), cnt.data_ptr(),
                                               adaptive=(AD_MIN, AD_ALLOWED, 0, npr.data_ptr()) if adaptive else None)
            else:
                ix.search_exhaustive_filtered_sharded_dev(None, case.Qd.data_ptr(), case.d, B, 10, metric, f.t, ids.data_ptr(), dist.data_ptr(), cnt.data_ptr())
            torch.cuda.synchronize(); ix.poll()
            want = whole_topk(case, 10, AD_MAX if adaptive else 5, f, metric=metric, adaptive=adaptive)
            same_topk((ids.cpu().numpy().view(np.uint64), dist.cpu().numpy(), cnt.cpu().numpy().view(np.uint32)), want, (f.name, metric, adaptive))
            if adaptive:
                assert np.array_equal(npr.cpu().numpy().view(np.uint32), want[3])
        for metric in (None, capi.METRIC_L2SQ):
            full = whole_range(case, np.full(B, INF, np.float32), 5, 0, f, metric=metric)
            radii = case.radii(full, 10)
            want = whole_range(case, radii, 5, 0, f, metric=metric)
            rd = dev(radii)
            total = int(want[0][B])
            lims = torch.zeros(B + 1, dtype=torch.int64, device="cuda"); ids = torch.zeros(total + 1, dtype=torch.int64, device="cuda")
            dist = torch.zeros(total + 1, device="cuda")
            got = ix.range_search_filtered_sharded_dev(None, case.Qd.data_ptr(), case.d, B, rd.data_ptr(), 5, 0, f.t, lims.data_ptr(), ids.data_ptr(), dist.data_ptr(),
                                                       total, exhaustive_metric=metric)
            assert got == total
            same_range((lims.cpu().numpy().view(np.uint64), ids.cpu().numpy().view(np.uint64)[:total], dist.cpu().numpy()[:total]), want, (f.name, metric))


# ---- the index changes under the shards ----
def test_after_remove_and_compact():
    """remove_batch on the unsharded index replayed on every shard through the stand-in communicator of tests/test_range_shard_gpu.py (the
    removal's one exchange is answered from the unsharded index's own lengths); then compact on some ranks"""
    import torch
    from vers_amd.dist import _AG, VersComm, _Mem
    env = Env(3, True)
    try:
        case = env.case
        whole, world, k = case.whole, case.world, case.k
        rng = np.random.default_rng(0x77)
        gone = np.unique(rng.integers(0, whole.values.shape[0], 700)).astype(np.uint64)
        before = whole.list_lengths().astype(np.int64)
        removed = whole.remove_batch(gone)
        per_list = before - whole.list_lengths().astype(np.int64)
        table = np.zeros((world, k), dtype=np.uint32)
        for c in range(k):
            table[int(case.owners[c]), c] = per_list[c]

        def all_gather(_ctx, send_ptr, recv_ptr, nbytes):
            try:
                if nbytes != 4 * k:
                    return 1
                torch.as_tensor(_Mem(recv_ptr, nbytes * world), device="cuda").copy_(torch.from_numpy(table.reshape(-1).view(np.uint8)))
                torch.cuda.synchronize()
                return 0
            except Exception:   # never unwind through the C frame
                return 1

        cb = _AG(all_gather)
        gd = dev_i64(gone)
        for r, ix in enumerate(case.shards):
            comm = VersComm(None, r, world, cb)
            n_removed = C.c_uint64(0)
            capi.check(capi.lib().vers_ivf_remove_batch_dev(ix._h, capi._vp(gd.data_ptr()), gone.size, C.byref(comm), C.byref(n_removed)))
            assert n_removed.value == removed

        def round_():
            for f in (env.per_call[2], env.per_call[3], env.f3):
                for top_k, nprobe in ((10, 5), (70, 24)):
                    same_topk(sharded_topk(case, top_k, nprobe, f), whole_topk(case, top_k, nprobe, f), ("removed", f.name, top_k, nprobe))
                same_topk(sharded_topk(case, 10, 0, f, metric=capi.METRIC_L2SQ), whole_topk(case, 10, 0, f, metric=capi.METRIC_L2SQ), ("removed", f.name, "exhaustive"))
                want = whole_topk(case, 10, AD_MAX, f, adaptive=True)
                got = sharded_topk(case, 10, AD_MAX, f, adaptive=True)
                same_topk(got, want, ("removed", f.name, "adaptive"))
                assert all(np.array_equal(got[3][r], want[3]) for r in range(world))
                full = whole_range(case, np.full(B, INF, np.float32), 5, 0, f)
                radii = case.radii(full, 10)
                for walk in (0, WALK):
                    same_range(sharded_range(case, radii, 5, walk, f), whole_range(case, radii, 5, walk, f), ("removed", f.name, walk))
                same_range(sharded_range(case, radii, 0, 0, f, metric=capi.METRIC_L2SQ), whole_range(case, radii, 0, 0, f, metric=capi.METRIC_L2SQ), ("removed", f.name))

        round_()
        whole.compact()
        for ix in case.shards[::2]:   # compaction is local: some ranks do, some do not
            ix.compact()
        round_()
    finally:
        env.close()


# ---- NaN rows ----
def test_a_nan_row_is_an_error_on_its_owner_only_and_only_when_allowed():
    import torch
    env = Env(3, False)
    try:
        case, whole = env.case, env.case.whole
        vid = 1234
        whole.values[vid, 7] = np.nan   # the row keeps its list; the shards are made again from the host's fields
        whole._upload()
        for ix in case.shards:
            ix.close()
        case.shards = reshard(whole, 3)
        owner = int(case.shards[0].owners()[int(whole.assignments[vid])])
        n = whole.values.shape[0]
        allow = np.ones(n, bool)
        deny = allow.copy(); deny[vid] = False
        fa, fd = Filt("nan-allowed", [allow], n, n), Filt("nan-denied", [deny], n, n)
        fo = np.zeros(B, np.uint32)
        fa3, fd3 = Filt("nan-allowed-multi", [allow, deny], n, n, fo), Filt("nan-denied-multi", [deny, allow], n, n, fo)
        buf = torch.zeros(2, B, 10, dtype=torch.int64, device="cuda")
        rd = torch.full((B,), float("inf"), device="cuda"); lims = torch.zeros(B + 1, dtype=torch.int64, device="cuda")
        for f, allowed in ((fa, True), (fd, False), (fa3, True), (fd3, False)):
            for r, ix in enumerate(case.shards):
                hit = allowed and r == owner
                ix.search_filtered_partial_dev(case.Qd.data_ptr(), case.d, B, 10, K, f.t, buf[0].data_ptr(), buf[1].data_ptr())
                torch.cuda.synchronize()
                if hit:
                    with pytest.raises(capi.VersError) as e:
                        ix.poll()
                    assert e.value.status == capi.ERR_NAN
                else:
                    ix.poll()
                ix.search_exhaustive_filtered_partial_dev(case.Qd.data_ptr(), case.d, B, 10, capi.METRIC_L2SQ, f.t, buf[0].data_ptr(), buf[1].data_ptr())
                torch.cuda.synchronize()
                if hit:
                    with pytest.raises(capi.VersError) as e:
                        ix.poll()
                    assert e.value.status == capi.ERR_NAN
                else:
                    ix.poll()
                for metric in (None, capi.METRIC_L2SQ):
                    if hit:
                        with pytest.raises(capi.VersError) as e:
                            ix.range_search_filtered_partial_dev(case.Qd.data_ptr(), case.d, B, rd.data_ptr(), K, 0, f.t, lims.data_ptr(), 0, 0, 0, exhaustive_metric=metric)
                        assert e.value.status == capi.ERR_NAN
                    else:
                        ix.range_search_filtered_partial_dev(case.Qd.data_ptr(), case.d, B, rd.data_ptr(), K, 0, f.t, lims.data_ptr(), 0, 0, 0, exhaustive_metric=metric)
    finally:
        env.close()


# ---- refusals ----
def refused(fn, *a, status=capi.ERR_INVALID, **kw):
    with pytest.raises(capi.VersError) as e:
        fn(*a, **kw)
    assert e.value.status == status, (e.value.status, str(e.value))
    return str(e.value)


def test_errors(env2):
    import torch
    from vers_amd.dist import VersComm, VersGather, _AG, _GA
    case = env2.case
    ix, whole = case.shards[0], case.whole
    Q, d = case.Qd.data_ptr(), case.d
    f, f3 = env2.per_call[2], env2.f3
    wp, n = f.wd.data_ptr(), f.n_bits
    buf = torch.full((2, B, 10), -9, dtype=torch.int64, device="cuda")
    dist = torch.zeros(B, 10, device="cuda"); cnt = torch.zeros(B, dtype=torch.int32, device="cuda")
    rd = torch.full((B,), 1.0, device="cuda"); lims = torch.full((B + 1,), -3, dtype=torch.int64, device="cuda")
    alen = torch.zeros(3 * K, dtype=torch.int32, device="cuda")
    k0, k1 = buf[0].data_ptr(), buf[1].data_ptr()
    bad_filters = [(wp, f.stride, 0, n, 0),                      # n_filters == 0 with b > 0
                   (wp, f.stride, capi.FILTER_MAX + 1, n, f3.fod.data_ptr()),   # more than VERS_FILTER_MAX
                   (f3.wd.data_ptr(), f3.stride, 3, n, 0),       # a NULL filter_of with n_filters != 1
                   (wp, f.stride - 1, 1, n, 0),                  # the stride
                   (0, f.stride, 1, n, 0)]                       # NULL bitmaps with n_bits > 0
    calls = 0

    def gather(*_a):
        nonlocal calls
        calls += 1
        return 1

    ga, ag = _GA(gather), _AG(gather)
    g_ok = VersGather(None, 0, 2, ga); g_rank = VersGather(None, 1, 2, ga); g_world = VersGather(None, 0, 3, ga)
    c_ok = VersComm(None, 0, 2, ag); c_rank = VersComm(None, 1, 2, ag); c_world = VersComm(None, 0, 3, ag)
    gp = lambda g: C.cast(C.byref(g), C.c_void_p)

    class CommPtr:
        def __init__(self, c):
            self.c = c

        def ptr(self):
            return C.byref(self.c)

    for t in bad_filters:
        refused(ix.search_filtered_partial_dev, Q, d, B, 10, 5, t, k0, k1)
        refused(ix.search_exhaustive_filtered_partial_dev, Q, d, B, 10, 0, t, k0, k1)
        refused(ix.search_filtered_sharded_dev, gp(g_ok), Q, d, B, 10, 5, t, k0, dist.data_ptr(), cnt.data_ptr())
        refused(ix.search_exhaustive_filtered_sharded_dev, gp(g_ok), Q, d, B, 10, 0, t, k0, dist.data_ptr(), cnt.data_ptr())
        for metric in (None, 0):
            refused(ix.range_search_filtered_partial_dev, Q, d, B, rd.data_ptr(), 5, 0, t, lims.data_ptr(), 0, 0, 0, exhaustive_metric=metric)
            refused(ix.range_search_filtered_sharded_dev, CommPtr(c_ok), Q, d, B, rd.data_ptr(), 5, 0, t, lims.data_ptr(), 0, 0, 0, exhaustive_metric=metric)
    for t in bad_filters[1:]:
        if t[4] == 0 and t[2] != 3:
            refused(ix.filter_allowed_len_dev, t[0], t[1], t[2], t[3], alen.data_ptr())
    refused(ix.filter_allowed_len_dev, wp, f.stride, 0, n, alen.data_ptr())
    # nprobe == 0 stays out of scope
    assert "out of scope" in refused(ix.search_filtered_partial_dev, Q, d, B, 10, 0, f.t, k0, k1)
    refused(ix.search_filtered_sharded_dev, gp(g_ok), Q, d, B, 10, 0, f.t, k0, dist.data_ptr(), cnt.data_ptr())
    refused(ix.range_search_filtered_partial_dev, Q, d, B, rd.data_ptr(), 0, 0, f.t, lims.data_ptr(), 0, 0, 0)
    refused(ix.range_search_filtered_sharded_dev, CommPtr(c_ok), Q, d, B, rd.data_ptr(), 0, 0, f.t, lims.data_ptr(), 0, 0, 0)
    # top_k == 0, unknown metric, unknown flag bits
    refused(ix.search_filtered_partial_dev, Q, d, B, 0, 5, f.t, k0, k1)
    refused(ix.search_exhaustive_filtered_partial_dev, Q, d, B, 10, 2, f.t, k0, k1)
    refused(ix.range_search_filtered_partial_dev, Q, d, B, rd.data_ptr(), 5, 2, f.t, lims.data_ptr(), 0, 0, 0)
    # the walk order has no key across ranks on the exhaustive calls
    refused(ix.range_search_exhaustive_filtered_partial_dev, Q, d, B, rd.data_ptr(), 0, WALK, f.t, lims.data_ptr(), 0, 0, 0)
    refused(ix.range_search_exhaustive_filtered_sharded_dev, CommPtr(c_ok), Q, d, B, rd.data_ptr(), 0, WALK, f.t, lims.data_ptr(), 0, 0, 0)
    # a g / comm whose rank or world disagree with the handle
    for g in (g_rank, g_world):
        refused(ix.search_filtered_sharded_dev, gp(g), Q, d, B, 10, 5, f.t, k0, dist.data_ptr(), cnt.data_ptr())
        refused(ix.search_exhaustive_filtered_sharded_dev, gp(g), Q, d, B, 10, 0, f.t, k0, dist.data_ptr(), cnt.data_ptr())
    refused(ix.search_filtered_sharded_dev, None, Q, d, B, 10, 5, f.t, k0, dist.data_ptr(), cnt.data_ptr())   # a sharded handle without an exchange
    for c in (c_rank, c_world):
        refused(ix.range_search_filtered_sharded_dev, CommPtr(c), Q, d, B, rd.data_ptr(), 5, 0, f.t, lims.data_ptr(), 0, 0, 0)
        refused(ix.range_search_exhaustive_filtered_sharded_dev, CommPtr(c), Q, d, B, rd.data_ptr(), 0, 0, f.t, lims.data_ptr(), 0, 0, 0)
    # adaptive
    refused(ix.search_filtered_partial_dev, Q, d, B, 10, 5, f.t, k0, k1, adaptive=(0, 10, alen.data_ptr(), 0))     # nprobe_min == 0
    refused(ix.search_filtered_partial_dev, Q, d, B, 10, 5, f.t, k0, k1, adaptive=(6, 10, alen.data_ptr(), 0))     # nprobe < nprobe_min
    refused(ix.search_filtered_partial_dev, Q, d, B, 10, 5, f.t, k0, k1, adaptive=(2, 10, 0, 0))                   # no global counts
    refused(ix.search_filtered_sharded_dev, gp(g_ok), Q, d, B, 10, 5, f.t, k0, dist.data_ptr(), cnt.data_ptr(), adaptive=(2, 10, alen.data_ptr(), 0))
    refused(ix.search_filtered_sharded_dev, gp(g_ok), Q, d, B, 10, 5, f.t, k0, dist.data_ptr(), cnt.data_ptr(), adaptive=(0, 10, 0, 0))
    # no centroids on the probed calls
    empty = IVFFlatIndex(d)
    try:
        refused(empty.search_filtered_partial_dev, Q, d, B, 10, 5, f.t, k0, k1, status=capi.ERR_INSUFFICIENT)
        refused(empty.search_filtered_sharded_dev, None, Q, d, B, 10, 5, f.t, k0, dist.data_ptr(), cnt.data_ptr(), status=capi.ERR_INSUFFICIENT)
        refused(empty.range_search_filtered_partial_dev, Q, d, B, rd.data_ptr(), 5, 0, f.t, lims.data_ptr(), 0, 0, 0, status=capi.ERR_INSUFFICIENT)
        refused(empty.range_search_filtered_sharded_dev, None, Q, d, B, rd.data_ptr(), 5, 0, f.t, lims.data_ptr(), 0, 0, 0, status=capi.ERR_INSUFFICIENT)
    finally:
        empty.close()
    torch.cuda.synchronize()
    assert calls == 0                                            # refused from the arguments: nothing was exchanged
    assert bool((buf == -9).all()) and bool((lims == -3).all())  # and nothing was written


def test_the_existing_filtered_calls_still_refuse_the_shards(env2):
    import torch
    case = env2.case
    ix = case.shards[1]
    f, f3 = env2.per_call[2], env2.f3
    Q, d = case.Qd.data_ptr(), case.d
    ids = torch.zeros(B, 10, dtype=torch.int64, device="cuda"); dist = torch.zeros(B, 10, device="cuda"); cnt = torch.zeros(B, dtype=torch.int32, device="cuda")
    rd = torch.full((B,), 1.0, device="cuda"); lims = torch.zeros(B + 1, dtype=torch.int64, device="cuda")
    i, x, c, w = ids.data_ptr(), dist.data_ptr(), cnt.data_ptr(), f.wd.data_ptr()
    w3, fo = f3.wd.data_ptr(), f3.fod.data_ptr()
    msgs = [refused(ix.search_filtered, case.Q, 10, 5, (f.words[0], f.n_bits)),
            refused(ix.search_exhaustive_filtered, case.Q, 10, (f.words[0], f.n_bits)),
            refused(ix.search_filtered_dev, Q, d, B, 10, 5, w, f.n_bits, i, x, c),
            refused(ix.search_exhaustive_filtered_dev, Q, d, B, 10, 0, w, f.n_bits, i, x, c),
            refused(ix.search_filtered_multi, case.Q, 10, 5, (f3.words, f3.n_bits), f3.filter_of % 3),
            refused(ix.search_exhaustive_filtered_multi, case.Q, 10, (f3.words, f3.n_bits), f3.filter_of % 3),
            refused(ix.search_filtered_multi_dev, Q, d, B, 10, 5, w3, f3.stride, 3, f3.n_bits, fo, i, x, c),
            refused(ix.search_exhaustive_filtered_multi_dev, Q, d, B, 10, 0, w3, f3.stride, 3, f3.n_bits, fo, i, x, c),
            refused(ix.search_filtered_adaptive, case.Q, 10, 2, 24, 10, (f.words[0], f.n_bits)),
            refused(ix.search_filtered_adaptive_dev, Q, d, B, 10, 2, 24, 10, w, f.n_bits, i, x, c, 0),
            refused(ix.search_filtered_multi_adaptive, case.Q, 10, 2, 24, 10, (f3.words, f3.n_bits), f3.filter_of % 3),
            refused(ix.search_filtered_multi_adaptive_dev, Q, d, B, 10, 2, 24, 10, w3, f3.stride, 3, f3.n_bits, fo, i, x, c, 0),
            refused(ix.range_search_filtered, case.Q, 1.0, 5, (f.words[0], f.n_bits)),
            refused(ix.range_search_exhaustive_filtered, case.Q, 1.0, (f.words[0], f.n_bits)),
            refused(ix.range_search_filtered_dev, Q, d, B, rd.data_ptr(), 5, 0, w, f.n_bits, lims.data_ptr(), 0, 0, 0),
            refused(ix.range_search_exhaustive_filtered_dev, Q, d, B, rd.data_ptr(), 0, 0, w, f.n_bits, lims.data_ptr(), 0, 0, 0),
            refused(ix.range_search_filtered_multi, case.Q, 1.0, 5, (f3.words, f3.n_bits), f3.filter_of % 3),
            refused(ix.range_search_exhaustive_filtered_multi, case.Q, 1.0, (f3.words, f3.n_bits), f3.filter_of % 3),
            refused(ix.range_search_filtered_multi_dev, Q, d, B, rd.data_ptr(), 5, 0, w3, f3.stride, 3, f3.n_bits, fo, lims.data_ptr(), 0, 0, 0),
            refused(ix.range_search_exhaustive_filtered_multi_dev, Q, d, B, rd.data_ptr(), 0, 0, w3, f3.stride, 3, f3.n_bits, fo, lims.data_ptr(), 0, 0, 0)]
    assert all("out of scope" in m and "sharded" in m for m in msgs), msgs


def test_filter_stats_cover_the_local_part(env2):
    case = env2.case
    f = env2.per_call[2]
    sharded_topk(case, 10, 5, f)
    rows = sum(ix.filter_stats()["last"]["rows_allowed"] for ix in case.shards)
    whole_topk(case, 10, 5, f)
    assert rows == case.whole.filter_stats()["last"]["rows_allowed"] == int(f.sem[0][np.concatenate([np.asarray(l, dtype=np.int64) for l in case.whole.ids])].sum())
