"""Prepared filters (vers_ivf_filter_prepare and the four _prepared_dev searches): masks kept across calls, refreshed when rows move.

The prepared calls have no semantics of their own, so every comparison here is np.array_equal of a prepared call against the EXISTING
vers_ivf_*_filtered_sharded_dev call (g / comm NULL) on the same handle, in the same state, with the same bitmaps: ids, distance bits,
counts or limits + total, out_nprobe and the slots of vers_ivf_filter_stats (same_stats: all four wherever the existing call reproduces
them itself).  For three queries per configuration the result is also
checked against the oracle on the index with the disallowed ids removed.  What is the object's own -- how often it rebuilt, tail-refreshed
or served a search with no mask work -- is read from vers_ivf_filter_info and the scan-timing ring.

Shape: N = 3000, d = 40, k = 24 (tests/test_filtered_shard_gpu.py): lists of ~125 rows = two storage tiles, a padded row length."""
import numpy as np
import pytest

from oracle import c_oracle as co
from tests import datagen as dg
from tests.golden import make_golden as mg
from tests.test_filtered_shard_gpu import AD_ALLOWED, AD_MAX, AD_MIN, Filt, dev
from tests.test_range_shard_gpu import bits
from vers_amd import capi
from vers_amd.index import IVFFlatIndex

pytestmark = pytest.mark.gpu

N, D, K = 3000, 40, 24
B = 40
TOP_KS = (1, 10, 70)     # (70: past 64 ranks, two passes)
NPROBES = (1, 5, 24)     # (24: every list)
BS = (1, 5, 40)
ROOM = 200               # ids beyond n that the "long" bitmaps cover: rows not yet added


def make_index():
    X = dg.dist_c(0x51, N, D, 30, dg.default_sigma(D))
    return IVFFlatIndex.build_index(K, 1, 4, X, init_indices=mg.init_draws(9, 1, K, N))


def make_filters(n):
    """-> {name: Filt}.  Per-call (filter_of None): everything allowed, random 30 % and 2 %, a contiguous id span, the empty filter
    (n_bits == 0), n_bits < n, n_bits > n with set bits for ids not yet added.  Per-query: 3 and 64 bitmaps whose filter_of has an entry at or
    beyond n_filters, one bitmap reached through a filter_of, and 3 bitmaps with n_bits > n."""
    rng = np.random.default_rng(0xF18)
    m = n + ROOM
    ones = np.ones(m, bool)
    r30 = rng.random(m) < 0.30
    r02 = rng.random(m) < 0.02
    span = np.zeros(m, bool); span[700:1900] = True
    half = rng.random(m) < 0.5
    fo3 = np.arange(B, dtype=np.uint32) % 3; fo3[11] = 7
    fo64 = np.arange(B, dtype=np.uint32) % 64; fo64[20] = 64
    fo1 = np.zeros(B, dtype=np.uint32); fo1[4] = 1
    fs = [Filt("ones", [ones[:n]], n, n), Filt("r30", [r30[:n]], n, n), Filt("r02", [r02[:n]], n, n), Filt("span", [span[:n]], n, n),
          Filt("empty", [ones[:n]], 0, n), Filt("short", [half[:n]], 2000, n), Filt("long", [r30], m, m), Filt("longones", [ones], m, m),
          Filt("F3", [r02[:n], r30[:n], span[:n]], n, n, fo3),
          Filt("F64", [rng.random(n) < (0.01 + 0.015 * f) for f in range(64)], n, n, fo64),
          Filt("F1fo", [r30[:n]], n, n, fo1), Filt("F3long", [r02, r30, half], m, m, fo3)]
    return {f.name: f for f in fs}


def prepare(ix, f):
    return ix.prepare_filter_dev(f.wd.data_ptr() if f.wd is not None else 0, f.stride, f.n_filters, f.n_bits)


class Ctx:
    def __init__(self):
        import torch
        self.ix = make_index()
        self.n = self.ix.values.shape[0]
        self.Q = dg.dist_c(0x52, B, D, 30, dg.default_sigma(D))
        self.Qd = torch.from_numpy(self.Q).cuda()
        self.f = make_filters(self.n)

    def close(self):
        self.ix.close()


@pytest.fixture(scope="module")
def fresh():
    c = Ctx()
    yield c
    c.close()


@pytest.fixture()
def ctx():
    c = Ctx()
    yield c
    c.close()


def stats(ix):
    return tuple(ix.filter_stats()["last"].values())


def topk(c, f, pf, b, top_k, nprobe, metric=None, adaptive=False, stream=0, wait=True):
    """pf None: the existing _filtered_sharded_dev call without an exchange; else the prepared call.  -> (ids, distance bits, counts,
    out_nprobe, filter stats), or the device tensors when the caller synchronises itself"""
    import torch
    ix = c.ix
    ids = torch.full((b, top_k), -5, dtype=torch.int64, device="cuda"); dist = torch.full((b, top_k), -7.25, device="cuda")
    cnt = torch.full((b,), -1, dtype=torch.int32, device="cuda"); npr = torch.full((b,), -1, dtype=torch.int32, device="cuda")
    ad = (AD_MIN, AD_ALLOWED, 0, npr.data_ptr()) if adaptive else None
    fo = f.fod.data_ptr() if f.fod is not None else 0
    if stream:
        torch.cuda.synchronize()   # (the outputs were filled on torch's stream)
    if pf is None and metric is None:
        ix.search_filtered_sharded_dev(None, c.Qd.data_ptr(), D, b, top_k, nprobe, f.t, ids.data_ptr(), dist.data_ptr(), cnt.data_ptr(), adaptive=ad, stream=stream)
    elif pf is None:
        ix.search_exhaustive_filtered_sharded_dev(None, c.Qd.data_ptr(), D, b, top_k, metric, f.t, ids.data_ptr(), dist.data_ptr(), cnt.data_ptr(), stream=stream)
    elif metric is None:
        ix.search_prepared_dev(c.Qd.data_ptr(), D, b, top_k, nprobe, pf, fo, ids.data_ptr(), dist.data_ptr(), cnt.data_ptr(), adaptive=ad, stream=stream)
    else:
        ix.search_exhaustive_prepared_dev(c.Qd.data_ptr(), D, b, top_k, metric, pf, fo, ids.data_ptr(), dist.data_ptr(), cnt.data_ptr(), stream=stream)
    if not wait:
        return ids, dist, cnt, npr
    torch.cuda.synchronize()
    ix.poll(stream)
    return host_topk(ids, dist, cnt, npr) + (stats(ix),)


def host_topk(ids, dist, cnt, npr):
    return ids.cpu().numpy().view(np.uint64), bits(dist.cpu().numpy()), cnt.cpu().numpy().view(np.uint32), npr.cpu().numpy().view(np.uint32)


def same_stats(got, want, f, b, metric, what):
    """All four slots -- except tiles_loaded and items_skipped of a PROBED batch with a filter per query.  There a work item is a group of up
    to 16 queries that probe one list, and the plan deals a list's queries into its groups in the order of an atomic counter
    (group_scatter_kernel): which queries share an item, hence the union of their filters that decides which tiles the item loads, differs
    between two runs of the SAME call (results do not).  Single bitmaps, b == 1 (an item per query) and the exhaustive calls (groups of
    consecutive queries) are reproducible and compared whole."""
    if f.filter_of is None or b == 1 or metric is not None:
        assert got == want, (what, "filter stats", got, want)
    else:
        assert (got[0], got[3]) == (want[0], want[3]) and got[1] <= got[0] and got[1] + got[2] > 0, (what, "filter stats", got, want)


def same_topk(got, want, what):
    assert np.array_equal(got[2], want[2]), (what, "counts", got[2], want[2])
    live = np.arange(got[0].shape[1])[None, :] < want[2][:, None]   # (entries past a query's count are unspecified)
    assert np.array_equal(got[0][live], want[0][live]), (what, "ids")
    assert np.array_equal(got[1][live], want[1][live]), (what, "distance bits")
    assert np.array_equal(got[3], want[3]), (what, "out_nprobe")


def both_topk(c, f, pf, b, top_k, nprobe, metric=None, adaptive=False):
    want = topk(c, f, None, b, top_k, nprobe, metric, adaptive)
    got = topk(c, f, pf, b, top_k, nprobe, metric, adaptive)
    same_topk(got, want, (f.name, b, top_k, nprobe, metric, adaptive))
    same_stats(got[4], want[4], f, b, metric, (f.name, b, top_k, nprobe, metric, adaptive))
    return got


def rng_call(c, f, pf, b, rd, nprobe, flags, metric, lims, ids, dist, cap):
    a = (c.Qd.data_ptr(), D, b, rd.data_ptr(), nprobe if metric is None else metric, flags)
    z = (lims.data_ptr(), ids.data_ptr() if ids is not None else 0, dist.data_ptr() if dist is not None else 0, cap)
    if pf is None:
        return c.ix.range_search_filtered_sharded_dev(None, *a, f.t, *z, exhaustive_metric=metric)
    return c.ix.range_search_prepared_dev(*a, pf, f.fod.data_ptr() if f.fod is not None else 0, *z, exhaustive_metric=metric)


def rng(c, f, pf, b, radius, nprobe, flags=0, metric=None):
    """the size query, then the fill -> (lims, ids, distance bits, total, filter stats)"""
    import torch
    rd = torch.full((b,), float(radius), device="cuda")
    lims = torch.full((b + 1,), -3, dtype=torch.int64, device="cuda")
    total = rng_call(c, f, pf, b, rd, nprobe, flags, metric, lims, None, None, 0)
    ids = torch.full((total + 8,), -5, dtype=torch.int64, device="cuda"); dist = torch.full((total + 8,), -7.25, device="cuda")
    assert rng_call(c, f, pf, b, rd, nprobe, flags, metric, lims, ids, dist, total) == total
    assert bool((ids[total:] == -5).all()) and bool((dist[total:] == -7.25).all())
    return lims.cpu().numpy().view(np.uint64), ids.cpu().numpy().view(np.uint64)[:total], bits(dist.cpu().numpy()[:total]), total, stats(c.ix)


def both_rng(c, f, pf, b, radius, nprobe, flags=0, metric=None):
    want = rng(c, f, None, b, radius, nprobe, flags, metric)
    got = rng(c, f, pf, b, radius, nprobe, flags, metric)
    for i, name in enumerate(("lims", "ids", "distance bits", "total")):
        assert np.array_equal(got[i], want[i]), (f.name, b, radius, nprobe, flags, metric, name)
    same_stats(got[4], want[4], f, b, metric, (f.name, b, radius, nprobe, flags, metric))
    return got


def radii(c):
    """two radii from the data: the 2 % and the 30 % quantile of the distances the queries see"""
    full = rng(c, c.f["ones"], None, B, np.inf, 24)
    d = np.sort(full[2].view(np.float32))
    return float(d[d.size // 50]), float(d[(3 * d.size) // 10])


# ---- 1. a fresh object ----
def test_fresh_object_equals_the_per_call_path(fresh):
    c, ix = fresh, fresh.ix
    r_small, r_big = radii(c)
    for name in ("ones", "r30", "r02", "span", "empty", "short", "long", "F3", "F64", "F1fo"):
        f = c.f[name]
        pf = prepare(ix, f)
        i0 = pf.info()
        assert (i0["n_filters"], i0["n_bits"], i0["builds"], i0["tail_refreshes"], i0["hits"], i0["fresh"]) == (f.n_filters, f.n_bits, 1, 0, 0, 1)
        assert i0["device_bytes"] > 0
        calls = 0
        for b in BS:
            for top_k, nprobe in ([(t, p) for t in TOP_KS for p in NPROBES] if b == B else [(10, 5), (70, 24), (1, 1)]):
                both_topk(c, f, pf, b, top_k, nprobe); calls += 1
            for metric in (capi.METRIC_L2SQ, capi.METRIC_COSDIST):
                for top_k in (TOP_KS if b == B else (10,)):
                    both_topk(c, f, pf, b, top_k, 0, metric=metric); calls += 1
            got = both_topk(c, f, pf, b, 10, AD_MAX, adaptive=True); calls += 1
            if b == B and name in ("r02", "F3"):   # the depths differ between queries: the object's counts are in use
                assert len(set(got[3].tolist())) >= 3, got[3]
            for radius in (r_small, r_big):
                for nprobe in (NPROBES if b == B else (5,)):
                    both_rng(c, f, pf, b, radius, nprobe); calls += 2   # (the size query and the fill)
                for metric in ((capi.METRIC_L2SQ, capi.METRIC_COSDIST) if b == B else (capi.METRIC_L2SQ,)):
                    both_rng(c, f, pf, b, radius, 0, metric=metric); calls += 2
            both_rng(c, f, pf, b, r_big, 5, flags=capi.RANGE_WALK_ORDER); calls += 2
        i1 = pf.info()
        # one build: prepare's, in the form the searches asked for (F1fo: one bitmap behind a filter_of -- the per-query form at first need)
        assert (i1["builds"], i1["tail_refreshes"], i1["hits"], i1["fresh"]) == (2 if name == "F1fo" else 1, 0, calls - (1 if name == "F1fo" else 0), 1), (name, i1)
        pf.close()


def test_fresh_object_leaves_no_mask_record(fresh):
    c, ix = fresh, fresh.ix
    for name in ("r30", "F3"):
        f = c.f[name]
        pf = prepare(ix, f)
        for adaptive in (False, True):
            ix.scan_times(reset=True)
            topk(c, f, None, B, 10, AD_MAX if adaptive else 5, adaptive=adaptive)
            per_call = len(ix.scan_times(reset=True))
            topk(c, f, pf, B, 10, AD_MAX if adaptive else 5, adaptive=adaptive)
            prepared = len(ix.scan_times(reset=True))
            assert per_call - prepared == (2 if adaptive else 1), (name, adaptive, per_call, prepared)   # the mask record (and the count record)
        pf.close()


def test_three_queries_against_the_oracle(fresh):
    c, ix = fresh, fresh.ix
    for name in ("r30", "short", "F3"):
        f = c.f[name]
        pf = prepare(ix, f)
        got = topk(c, f, pf, B, 10, 5)
        gx = topk(c, f, pf, B, 10, 0, metric=capi.METRIC_L2SQ)
        for q in (0, 3, 36):
            sem = f.sem_of(q)
            ids_f = [[v for v in l if sem[v]] for l in ix.ids]
            rows = np.asarray(sorted(v for l in ids_f for v in l), dtype=np.int64)
            oi, od = co.search_nprobe(ix.values, ix.centroids, ids_f, c.Q[q], max(1, rows.size), 5)
            n = min(10, oi.size)
            assert got[2][q] == n and np.array_equal(got[0][q, :n], oi[:n]) and np.array_equal(got[1][q, :n], bits(od[:n])), (name, q)
            xi, xd = co.search_exhaustive(ix.values[rows], c.Q[q], rows.size, 0)
            n = min(10, rows.size)
            assert gx[2][q] == n and np.array_equal(gx[0][q, :n], rows[xi.astype(np.int64)][:n].astype(np.uint64)) and np.array_equal(gx[1][q, :n], bits(xd[:n]))
        pf.close()


def test_range_capacity_protocol(fresh):
    """cap too small: VERS_OK, the limits and the total complete, ids and distances untouched -- as the per-call path does it"""
    import torch
    c, ix = fresh, fresh.ix
    rd = torch.full((B,), float("inf"), device="cuda")
    for name in ("r30", "F3"):
        f = c.f[name]
        pf = prepare(ix, f)
        for metric in (None, capi.METRIC_L2SQ):
            out = []
            for p in (None, pf):
                lims = torch.full((B + 1,), -3, dtype=torch.int64, device="cuda")
                total = rng_call(c, f, p, B, rd, 5, 0, metric, lims, None, None, 0)
                assert total > 1
                ids = torch.full((total,), -13, dtype=torch.int64, device="cuda"); dist = torch.full((total,), -7.25, device="cuda")
                lims2 = torch.full((B + 1,), -3, dtype=torch.int64, device="cuda")
                assert rng_call(c, f, p, B, rd, 5, 0, metric, lims2, ids, dist, total - 1) == total
                assert torch.equal(lims, lims2) and int(lims[B]) == total and bool((ids == -13).all()) and bool((dist == -7.25).all())
                out.append((lims.cpu().numpy(), total))
            assert np.array_equal(out[0][0], out[1][0]) and out[0][1] == out[1][1]
        pf.close()


# ---- 2. tail refresh ----
def storage_cap(length):
    """the storage rule of a build (vers_amd/csrc/ivf_build.hip, plan_capacities): what a list may grow to before storage is re-laid-out"""
    return -(-(length + max(8, length // 16)) // 64) * 64


def near(c, L, seed):
    """a row that lands in list L: its centroid plus tiny noise"""
    x = c.ix.centroids[L] + np.float32(1e-4) * dg.dist_u(seed, 1, D)[0]
    return np.ascontiguousarray(x, dtype=np.float32)


def add_to(c, L, count, seed):
    for i in range(count):
        cl, _ = c.ix.add(near(c, L, seed + i))
        assert cl == L


def compare_all(c, objs):
    """the per-call and the per-query form and the adaptive call, probed, exhaustive and range, against the per-call path"""
    for f, pf in objs:
        both_topk(c, f, pf, B, 10, 5)
        both_topk(c, f, pf, 5, 70, 24)
        both_topk(c, f, pf, B, 10, 0, metric=capi.METRIC_L2SQ)
        both_topk(c, f, pf, B, 10, AD_MAX, adaptive=True)   # (allowed_len has followed: the depths are the per-call path's)
        both_rng(c, f, pf, B, 0.5, 5)


@pytest.mark.parametrize("covered", [True, False], ids=["n_bits_covers_new_ids", "n_bits_is_n"])
def test_tail_refresh_after_appends_in_place(ctx, covered):
    c, ix = ctx, ctx.ix
    names = ("long", "longones", "F3long") if covered else ("r30", "F3")
    objs = [(c.f[n], prepare(ix, c.f[n])) for n in names]
    both = Filt("both", [c.f["long" if covered else "r30"].sem[0]], c.n + ROOM if covered else c.n, c.n + ROOM if covered else c.n,
                np.zeros(B, dtype=np.uint32))   # one bitmap, used with and without a filter_of: the object holds both forms
    pb = prepare(ix, both)
    both_topk(c, both, pb, B, 10, 5)
    both_nofo = c.f["long" if covered else "r30"]
    objs += [(both, pb), (both_nofo, pb)]
    lens = ix.list_lengths().astype(np.int64)
    # an emptied-then-rebuilt list with two tiles of storage, and a list that grows within its last tile
    E = int(np.argmax(lens))
    assert storage_cap(int(lens[E])) >= 128
    G = next(int(L) for L in np.argsort(-lens) if L != E and lens[L] % 64 <= 60 and storage_cap(int(lens[L])) - lens[L] >= 2)
    ix.remove_batch(np.asarray(ix.ids[E], dtype=np.uint64))
    compare_all(c, objs)   # (the removal: a full rebuild, once per object)
    base = [pf.info() for _, pf in objs[:-1]]
    assert all(i["fresh"] == 1 for i in base)
    first_new = ix.values.shape[0]
    # 0 -> 1, 1 -> 3 (within a tile), 3 -> 64 (exactly to a multiple of 64), 64 -> 65 (across the tile boundary), 65 -> 70; then G + 2
    steps = [(E, 1), (E, 2), (E, 61), (E, 1), (E, 5), (G, 2)]
    seed = 1000
    for n_step, (L, count) in enumerate(steps, 1):
        add_to(c, L, count, seed); seed += count
        assert all(pf.info()["fresh"] == 0 for _, pf in objs[:-1])
        before = [pf.info() for _, pf in objs[:-1]]
        compare_all(c, objs)
        for (f, pf), i0, ib in zip(objs[:-1], base, before):
            i1 = pf.info()
            assert i1["builds"] == i0["builds"], (f.name, n_step, "an append in place must not rebuild")
            assert i1["fresh"] == 1
            if covered:
                assert i1["tail_refreshes"] == n_step, (f.name, n_step, i1)
            else:   # every new id is at or beyond n_bits: no kernel, the snapshot is taken and the call is a hit
                assert i1["tail_refreshes"] == 0 and i1["hits"] > ib["hits"], (f.name, n_step, i1)
    assert int(ix.list_lengths()[E]) == 70
    if covered:   # the new rows are found where they are allowed: everything is, in "longones"
        f, pf = objs[1]
        import torch
        q = torch.from_numpy(np.ascontiguousarray(np.repeat(ix.centroids[E][None], B, 0))).cuda()
        keep, c.Qd = c.Qd, q
        got = both_topk(c, f, pf, 1, 70, 1)
        c.Qd = keep
        assert got[2][0] == 70 and set(got[0][0].tolist()) == set(range(first_new, first_new + 70))
    for _, pf in objs[:-1]:
        pf.close()


@pytest.mark.parametrize("adaptive_first", [False, True], ids=["plain_first", "adaptive_first"])
def test_second_form_built_after_appends_the_object_has_not_seen(ctx, adaptive_first):
    """One bitmap, prepared (the per-call form), then in-place adds below n_bits, then the FIRST search with a filter_of: the per-query form
    is built from rows the object's counts do not cover yet.  out_nprobe and rows_allowed must be the per-call path's at once and after."""
    c, ix = ctx, ctx.ix
    m = c.n + ROOM
    lens = ix.list_lengths().astype(np.int64)
    G = next(int(L) for L in np.argsort(-lens) if storage_cap(int(lens[L])) - lens[L] >= 24)
    for name in ("longones", "long"):
        nofo = c.f[name]
        fo = Filt(name + "fo", [nofo.sem[0]], m, m, np.zeros(B, dtype=np.uint32))
        pf = prepare(ix, nofo)
        add_to(c, G, 6, 5000 + (100 if name == "long" else 0))
        i0 = pf.info()
        assert (i0["builds"], i0["tail_refreshes"], i0["fresh"]) == (1, 0, 0)
        first = both_topk(c, fo, pf, B, 10, AD_MAX if adaptive_first else 5, adaptive=adaptive_first)   # (rows_allowed: same_stats)
        assert first[4][3] == int(sum(nofo.sem[0][v] for l in ix.ids for v in l))
        i1 = pf.info()
        assert (i1["builds"], i1["fresh"]) == (2, 1), i1
        for f in (fo, nofo):
            both_topk(c, f, pf, B, 10, AD_MAX, adaptive=True)
            both_topk(c, f, pf, B, 10, 5)
            both_rng(c, f, pf, B, 0.5, 5)
        add_to(c, G, 6, 5050 + (100 if name == "long" else 0))   # both forms held now: a tail refresh
        for f in (fo, nofo):
            got = both_topk(c, f, pf, B, 10, AD_MAX, adaptive=True)
            assert got[4][3] == int(sum(nofo.sem[0][v] for l in ix.ids for v in l))
            both_topk(c, f, pf, B, 10, 5)
        i2 = pf.info()
        assert (i2["builds"], i2["tail_refreshes"], i2["fresh"]) == (2, 1, 1), i2
        pf.close()


def test_a_new_form_on_another_stream_waits_for_the_rebuild(ctx):
    """after a removal: a search without filter_of on stream A rebuilds masks, counts and total; at once an adaptive search WITH a filter_of on
    stream B builds the per-query form for the first time -- it reads the counts and the total A is still writing unless it waits"""
    import torch
    c, ix = ctx, ctx.ix
    nofo = c.f["r30"]
    fo = Filt("r30fo", [nofo.sem[0]], c.n, c.n, np.zeros(B, dtype=np.uint32))
    pf = prepare(ix, nofo)
    ix.remove_batch(np.arange(0, 1500, 2, dtype=np.uint64))
    sa, sb, sc = torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Stream()
    a = topk(c, nofo, pf, B, 10, 5, stream=sa.cuda_stream, wait=False)
    b = topk(c, fo, pf, B, 10, AD_MAX, adaptive=True, stream=sb.cuda_stream, wait=False)
    cc = topk(c, nofo, pf, B, 10, AD_MAX, adaptive=True, stream=sc.cuda_stream, wait=False)
    torch.cuda.synchronize()
    for s in (sa, sb, sc):
        ix.poll(s.cuda_stream)
    same_topk(host_topk(*a), topk(c, nofo, None, B, 10, 5)[:4], "stream A")
    same_topk(host_topk(*b), topk(c, fo, None, B, 10, AD_MAX, adaptive=True)[:4], "stream B")
    same_topk(host_topk(*cc), topk(c, nofo, None, B, 10, AD_MAX, adaptive=True)[:4], "stream C")
    i = pf.info()
    assert (i["builds"], i["hits"]) == (3, 1), i
    both_topk(c, fo, pf, B, 10, AD_MAX, adaptive=True)   # (rows_allowed too)
    pf.close()


# ---- 3. full rebuild ----
def test_full_rebuild_when_rows_moved(ctx):
    c, ix = ctx, ctx.ix
    objs = [(c.f["long"], prepare(ix, c.f["long"])), (c.f["F3long"], prepare(ix, c.f["F3long"]))]

    def rebuilt_once(what):
        for f, pf in objs:
            i0 = pf.info()
            assert i0["fresh"] == 0, (what, f.name)
            both_topk(c, f, pf, B, 10, 5)
            i1 = pf.info()
            assert (i1["builds"], i1["hits"], i1["tail_refreshes"], i1["fresh"]) == (i0["builds"] + 1, i0["hits"], i0["tail_refreshes"], 1), (what, f.name, i0, i1)
            both_topk(c, f, pf, B, 10, AD_MAX, adaptive=True)
            both_rng(c, f, pf, B, 0.5, 5)
            both_topk(c, f, pf, 5, 10, 0, metric=capi.METRIC_L2SQ)
            i2 = pf.info()
            assert (i2["builds"], i2["hits"]) == (i1["builds"], i1["hits"] + 4), (what, f.name, i2)   # (the range call: size query and fill)

    rng_ = np.random.default_rng(5)
    assert ix.remove_batch(rng_.choice(c.n, 300, replace=False).astype(np.uint64)) == 300
    rebuilt_once("remove_batch")
    ix.compact()
    rebuilt_once("compact")
    lens = ix.list_lengths().astype(np.int64)
    L = int(np.argmax(lens))
    more = 200   # more than any list's slack: storage is re-laid-out
    ix.add_batch(np.stack([near(c, L, 3000 + i) for i in range(more)]))
    assert int(ix.list_lengths()[L]) == lens[L] + more
    rebuilt_once("add_batch with a re-layout")
    ix._upload()   # (every position is back in its list: the host mirror follows)
    ix.ids = [np.flatnonzero(ix.assignments == cl).tolist() for cl in range(K)]
    rebuilt_once("upload")
    # a refresh ahead of the search moves the rebuild out of it
    ix.remove_batch(np.arange(100, 140, dtype=np.uint64))
    for f, pf in objs:
        i0 = pf.info()
        pf.refresh()
        i1 = pf.info()
        assert (i1["builds"], i1["hits"], i1["fresh"]) == (i0["builds"] + 1, i0["hits"], 1)
        ix.scan_times(reset=True)
        topk(c, f, None, B, 10, 5)
        per_call = len(ix.scan_times(reset=True))
        both_topk(c, f, pf, B, 10, 5)
        assert per_call - (len(ix.scan_times(reset=True)) - per_call) == 1   # (both_topk ran the per-call path too)
        i2 = pf.info()
        assert (i2["builds"], i2["hits"]) == (i1["builds"], i1["hits"] + 1)
    # ... and a search that rebuilds leaves the rebuild's record where the mask kernel's was
    ix.remove_batch(np.arange(200, 210, dtype=np.uint64))
    f, pf = objs[0]
    ix.scan_times(reset=True)
    topk(c, f, None, B, 10, 5)
    per_call = len(ix.scan_times(reset=True))
    topk(c, f, pf, B, 10, 5)
    assert len(ix.scan_times(reset=True)) == per_call
    for _, pf in objs:
        pf.close()


# ---- 4. two streams, one thread ----
def test_two_streams_share_one_rebuild(ctx):
    import torch
    c, ix = ctx, ctx.ix
    for name in ("r30", "F3"):
        f = c.f[name]
        pf = prepare(ix, f)
        ix.remove_batch(np.arange(0, 900, 3, dtype=np.uint64) + (0 if name == "r30" else 1))
        sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
        i0 = pf.info()
        a = topk(c, f, pf, B, 10, 5, stream=sa.cuda_stream, wait=False)
        b = topk(c, f, pf, B, 10, 5, stream=sb.cuda_stream, wait=False)   # at once: A's rebuild may still be running
        torch.cuda.synchronize()
        ix.poll(sa.cuda_stream); ix.poll(sb.cuda_stream)
        i1 = pf.info()
        assert (i1["builds"], i1["hits"]) == (i0["builds"] + 1, i0["hits"] + 1)
        want = topk(c, f, None, B, 10, 5)
        same_topk(host_topk(*a), want[:4], (name, "stream A"))
        same_topk(host_topk(*b), want[:4], (name, "stream B"))
        pf.close()


# ---- 5. refusals ----
def test_refusals_leave_outputs_and_object_alone(fresh):
    import torch
    c, ix = fresh, fresh.ix
    f1, f3 = c.f["r30"], c.f["F3"]
    p1, p3 = prepare(ix, f1), prepare(ix, f3)
    other = IVFFlatIndex(D)
    sharded = IVFFlatIndex(D); sharded.set_shard(0, 2)
    ps = prepare(sharded, f1)   # (no index: empty masks)
    assert ps.info()["builds"] == 1
    ids = torch.full((B, 10), -5, dtype=torch.int64, device="cuda"); dist = torch.full((B, 10), -7.25, device="cuda")
    cnt = torch.full((B,), -1, dtype=torch.int32, device="cuda"); lims = torch.full((B + 1,), -3, dtype=torch.int64, device="cuda")
    rd = torch.full((B,), 1.0, device="cuda"); alen = torch.zeros(3 * K, dtype=torch.int32, device="cuda")
    out = (ids.data_ptr(), dist.data_ptr(), cnt.data_ptr())
    q = (c.Qd.data_ptr(), D, B)

    def refused(call):
        with pytest.raises(capi.VersError) as e:
            call()
        assert e.value.status == capi.ERR_INVALID, e.value
        torch.cuda.synchronize()
        assert bool((ids == -5).all()) and bool((dist == -7.25).all()) and bool((cnt == -1).all()) and bool((lims == -3).all())

    # an object used with another handle; a NULL object
    refused(lambda: other.search_prepared_dev(*q, 10, 5, p1, 0, *out))
    refused(lambda: other.search_exhaustive_prepared_dev(*q, 10, capi.METRIC_L2SQ, p1, 0, *out))
    refused(lambda: other.range_search_prepared_dev(*q, rd.data_ptr(), 5, 0, p1, 0, lims.data_ptr(), ids.data_ptr(), dist.data_ptr(), 10))
    refused(lambda: other.range_search_exhaustive_prepared_dev(*q, rd.data_ptr(), capi.METRIC_L2SQ, 0, p1, 0, lims.data_ptr(), ids.data_ptr(), dist.data_ptr(), 10))
    refused(lambda: ix.search_prepared_dev(*q, 10, 5, 0, 0, *out))
    with pytest.raises(capi.VersError):
        capi.check(capi.lib().vers_ivf_filter_refresh(other._h, p1.ptr, None))
    with pytest.raises(capi.VersError):
        capi.check(capi.lib().vers_ivf_filter_destroy(other._h, p1.ptr))
    # filter_of NULL with three bitmaps; a caller's allowed counts; nprobe == 0
    refused(lambda: ix.search_prepared_dev(*q, 10, 5, p3, 0, *out))
    refused(lambda: ix.range_search_prepared_dev(*q, rd.data_ptr(), 5, 0, p3, 0, lims.data_ptr(), ids.data_ptr(), dist.data_ptr(), 10))
    refused(lambda: ix.search_prepared_dev(*q, 10, AD_MAX, p3, f3.fod.data_ptr(), *out, adaptive=(AD_MIN, AD_ALLOWED, alen.data_ptr(), 0)))
    refused(lambda: ix.search_prepared_dev(*q, 10, 0, p1, 0, *out))
    refused(lambda: ix.range_search_prepared_dev(*q, rd.data_ptr(), 0, 0, p1, 0, lims.data_ptr(), ids.data_ptr(), dist.data_ptr(), 10))
    # a handle sharded by cluster
    refused(lambda: sharded.search_prepared_dev(*q, 10, 5, ps, 0, *out))
    refused(lambda: sharded.search_exhaustive_prepared_dev(*q, 10, capi.METRIC_L2SQ, ps, 0, *out))
    refused(lambda: sharded.range_search_exhaustive_prepared_dev(*q, rd.data_ptr(), capi.METRIC_L2SQ, 0, ps, 0, lims.data_ptr(), ids.data_ptr(), dist.data_ptr(), 10))
    # prepare: no bitmap, too many, a stride below one bitmap's words
    words = f3.wd.data_ptr()
    for n_filters, stride in ((0, f3.stride), (65, f3.stride), (3, f3.stride - 1)):
        with pytest.raises(capi.VersError) as e:
            ix.prepare_filter_dev(words, stride, n_filters, f3.n_bits)
        assert e.value.status == capi.ERR_INVALID
    # the objects are still usable
    both_topk(c, f1, p1, B, 10, 5)
    both_topk(c, f3, p3, B, 10, 5)
    assert p1.info()["builds"] == 1 and p3.info()["builds"] == 1
    for p in (p1, p3, ps):
        p.close()
    other.close(); sharded.close()


# ---- 6. lifetime ----
def test_the_object_owns_its_bits_and_gives_its_memory_back(fresh):
    import torch
    c, ix = fresh, fresh.ix
    f = c.f["F3"]
    want = topk(c, f, None, B, 10, 5)   # (and the workspace's scratch is as large as these calls make it)
    torch.cuda.synchronize()
    mem0 = capi.mem_stats()[0]
    mine = f.wd.clone()
    pf = ix.prepare_filter_dev(mine.data_ptr(), f.stride, f.n_filters, f.n_bits)
    info = pf.info()
    assert capi.mem_stats()[0] - mem0 == info["device_bytes"] > 0
    mine.zero_()   # the caller's bitmaps change: the object has its own
    torch.cuda.synchronize()
    same_topk(topk(c, f, pf, B, 10, 5), want, "bitmaps zeroed after prepare")
    host = ix.prepare_filter(f.words, f.n_bits)   # the host-pointer twin
    same_topk(topk(c, f, host, B, 10, 5), want, "prepared from host bitmaps")
    host.close(); pf.close()
    assert capi.mem_stats()[0] == mem0
    # vers_ivf_destroy with a live object frees it
    small = IVFFlatIndex(D)
    torch.cuda.synchronize()
    mem1 = capi.mem_stats()[0]
    alive = prepare(small, c.f["r30"])
    assert capi.mem_stats()[0] > mem1
    small.close()
    assert capi.mem_stats()[0] <= mem1
    alive.ptr = 0
