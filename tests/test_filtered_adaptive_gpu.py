"""vers_ivf_search_filtered_adaptive / _multi_adaptive (+ _dev): every query of a batch probes lists until min_allowed rows its bitmap allows
are in reach, between nprobe_min and nprobe_max lists.  The calls have no semantics of their own, so the expected values come from the oracle
as it stands:
  list order of query q   co.search_exhaustive(ix.centroids, Q[q], k, ix.metric)
  a_j                     the ids of ix.ids[L_j] the allowed set holds
  P_q                     the smallest P in [min(nprobe_min, k), min(nprobe_max, k)] with a_0 + ... + a_{P-1} >= min_allowed, else the upper end
  rows                    co.search_nprobe over the filtered ids at nprobe = P_q
and every comparison is np.array_equal on the ids, on the distances' u32 BITS, on out_count and on out_nprobe: no tolerance."""
import os
import subprocess

import numpy as np
import pytest

from oracle import c_oracle as co
from tests import datagen as dg
from tests.test_filtered_gpu import Ref, allowed_set, bits, make, queries, random_filter
from vers_amd import capi
from vers_amd.index import IVFFlatIndex

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L2, COS = capi.METRIC_L2SQ, capi.METRIC_COSDIST
N, D, K, B = 6000, 24, 200, 37
# (filter seed, selectivity) of the main batches: chosen so that the oracle's depths span the plan kernel's 64-rank chunks (asserted below)
MAIN_FILTERS = ((0xADA1, 0.02), (0xADA2, 0.005), (0xADA3, 0.003))


class ARef(Ref):
    """Ref + the oracle's list order per query and the allowed rows per list: the depth rule restated."""

    def __init__(self, ix, Q, sem, order=None):
        super().__init__(ix, Q, sem)
        k = ix.num_centroids
        self.k = k
        self.order = order if order is not None else [co.search_exhaustive(ix.centroids, self.Q[q], k, ix.metric)[0].astype(np.int64) for q in range(self.Q.shape[0])]
        self.alen = np.asarray([len(l) for l in self.ids_f], dtype=np.int64)

    def depth(self, q, nprobe_min, nprobe_max, min_allowed):
        lo, hi = min(nprobe_min, self.k), min(nprobe_max, self.k)
        before = np.concatenate([[0], np.cumsum(self.alen[self.order[q]])])
        for p in range(lo, hi + 1):
            if before[p] >= min_allowed:
                return p
        return hi

    def depths(self, nprobe_min, nprobe_max, min_allowed, qs=None):
        qs = range(self.Q.shape[0]) if qs is None else qs
        return np.asarray([self.depth(q, nprobe_min, nprobe_max, min_allowed) for q in qs], dtype=np.uint32)


def same_rows(got, ar, qs, top_k, want_np, what):
    ids, dist, cnt = got[:3]
    for i, q in enumerate(qs):
        ei, ed = ar.probed(q, int(want_np[i]))
        ei, ed = ei[:top_k], ed[:top_k]
        assert cnt[i] == ei.size, (what, q, int(cnt[i]), ei.size)
        assert np.array_equal(ids[i, :cnt[i]], ei), (what, q, "ids")
        assert np.array_equal(bits(dist[i, :cnt[i]]), bits(ed)), (what, q, "distance bits")


def check(ar, top_k, nprobe_min, nprobe_max, min_allowed, allowed, n_bits=None, qs=None):
    qs = list(range(ar.Q.shape[0])) if qs is None else qs
    want_np = ar.depths(nprobe_min, nprobe_max, min_allowed, qs)
    got = ar.ix.search_filtered_adaptive(ar.Q[qs], top_k, nprobe_min, nprobe_max, min_allowed, allowed, n_bits)
    what = ("adaptive", top_k, nprobe_min, nprobe_max, min_allowed)
    assert np.array_equal(got[3], want_np), (what, got[3].tolist(), want_np.tolist())
    same_rows(got, ar, qs, top_k, want_np, what)
    return got, want_np


@pytest.fixture(scope="module")
def main_ix():
    ix = make(N, D, K)
    yield ix
    ix.close()


@pytest.fixture(scope="module")
def main_q(main_ix):
    return queries(main_ix, 0xADA0, B)


@pytest.fixture(scope="module")
def main_refs(main_ix, main_q):
    out = []
    for seed, sel in MAIN_FILTERS:
        allowed = random_filter(N, sel, seed)
        out.append((ARef(main_ix, main_q, allowed), allowed))
    return out


# ---- 1. depths across the chunk boundaries of the plan's 64-rank walk; agreement with the plain call ------------------------------------------
def test_depths_across_chunk_boundaries(main_refs):
    top_k, lo, hi, m = 10, 4, 150, 10
    assert any(len(l) == 0 for l in main_refs[0][0].ix.ids), "the k = 200 build is expected to have empty lists"
    want = np.concatenate([ar.depths(lo, hi, m) for ar, _ in main_refs])
    stopped = [q for ar, _ in main_refs for q in range(B) if ar.depth(q, lo, hi, m) == hi and ar.alen[ar.order[q][:hi]].sum() < m]
    assert (want < 64).any() and ((want >= 65) & (want <= 128)).any() and (want > 128).any(), sorted(set(want.tolist()))
    assert stopped, "no query is stopped at nprobe_max short of min_allowed"
    assert len(set(want.tolist())) >= 10, sorted(set(want.tolist()))
    for ar, allowed in main_refs:
        (ids, dist, cnt, npr), want_np = check(ar, top_k, lo, hi, m, allowed)
        # agreement with the existing call, GPU against GPU: the rows of every distinct depth P equal search_filtered at nprobe = P
        for P in sorted(set(want_np.tolist())):
            rows = np.flatnonzero(want_np == P)
            i1, d1, c1 = ar.ix.search_filtered(ar.Q[rows], top_k, int(P), allowed)
            assert np.array_equal(cnt[rows], c1), P
            for i, q in enumerate(rows):
                assert np.array_equal(ids[q, :c1[i]], i1[i, :c1[i]]) and np.array_equal(bits(dist[q, :c1[i]]), bits(d1[i, :c1[i]])), (P, q)


# ---- 2. edges of the rule ---------------------------------------------------------------------------------------------------------------------
def test_edges_of_the_rule(main_refs, main_ix, main_q):
    ar, allowed = main_refs[0]
    n_allowed = int(ar.alen.sum())
    (_, _, _, npr), _ = check(ar, 10, 4, 150, 0, allowed)              # min_allowed = 0: every depth is P_min
    assert (npr == 4).all()
    check(ar, 10, 1, 150, 1, allowed)                                  # min_allowed = 1
    (_, _, cnt, npr), _ = check(ar, 10, 4, 150, n_allowed + 1, allowed)  # more than the filter allows at all: every depth is P_max
    assert (npr == 150).all()
    (_, _, _, npr), _ = check(ar, 10, 4, 1000, n_allowed + 1, allowed)  # nprobe_max above k
    assert (npr == K).all()
    (_, _, _, npr), _ = check(ar, 10, 300, 1000, 1, allowed)           # nprobe_min above k too
    assert (npr == K).all()
    (i0, d0, c0, npr), _ = check(ar, 10, 7, 7, 10, allowed)            # nprobe_min == nprobe_max: the plain call
    i1, d1, c1 = ar.ix.search_filtered(ar.Q, 10, 7, allowed)
    assert (npr == 7).all() and np.array_equal(c0, c1)
    for q in range(B):
        assert np.array_equal(i0[q, :c0[q]], i1[q, :c1[q]]) and np.array_equal(bits(d0[q, :c0[q]]), bits(d1[q, :c1[q]]))
    # the empty filter: n_bits == 0 with a NULL bitmap
    empty = ARef(main_ix, main_q, np.zeros(N, dtype=bool))
    (_, _, cnt, npr), _ = check(empty, 10, 4, 150, 10, (np.zeros(0, dtype=np.uint64), 0))
    assert (npr == 150).all() and not cnt.any()
    rc, cnt, npr = raw(main_ix, main_q, 10, 4, 150, 10, None, 0)
    assert rc == capi.OK and (npr == 150).all() and not cnt.any()
    # a filter of ones
    ones = np.ones(N, dtype=bool)
    full = ARef(main_ix, main_q, ones)
    (_, _, cnt, npr), _ = check(full, 10, 1, 150, 10, ones)
    assert (cnt == 10).all() and npr.max() < 150
    # n_bits below n and above n
    for n_bits in (N - 1777, N + 500):
        sem = allowed_set(N, ones if n_bits > N else allowed, n_bits)
        check(ARef(main_ix, main_q, sem), 10, 2, 150, 10, np.ones(n_bits, dtype=bool) if n_bits > N else allowed, n_bits)


# ---- 3. batch and result widths -----------------------------------------------------------------------------------------------------------------
def test_batch_and_result_widths(main_refs, main_ix):
    ar, allowed = main_refs[1]
    check(ar, 10, 4, 150, 10, allowed, qs=[5])                         # b = 1
    Q = queries(main_ix, 0xADB0, 130)                                  # b = 130
    check(ARef(main_ix, Q, allowed), 10, 4, 150, 10, allowed)
    ar2, allowed2 = main_refs[0]
    check(ar2, 70, 2, 150, 70, allowed2)                               # top_k = 70: two result passes
    check(ar2, 70, 2, 150, 70, allowed2, qs=[3])


def test_cosine_metric():
    ix = make(1500, 48, 70, metric=COS, seed=0xADC0)
    try:
        Q = queries(ix, 0xADC1, 9)
        allowed = random_filter(1500, 0.02, 0xADC2)
        ar = ARef(ix, Q, allowed)
        (_, _, _, npr), _ = check(ar, 10, 1, 70, 10, allowed)
        assert len(set(npr.tolist())) > 1
        check(ar, 10, 1, 70, 10, allowed, qs=[4])
    finally:
        ix.close()


# ---- 4. a mutated index ------------------------------------------------------------------------------------------------------------------------
def test_mutated_index():
    ix = make(3000, 32, 40, seed=0xADD0)
    try:
        Q = queries(ix, 0xADD1, 9)
        ix.add_batch(dg.dist_c(0xADD2, 500, 32, 80, dg.default_sigma(32)))
        n = 3500
        allowed = random_filter(n, 0.05, 0xADD3)
        allowed[3000:3040] = True   # new ids among the allowed
        ar = ARef(ix, Q, allowed)
        check(ar, 10, 1, 40, 10, allowed); check(ar, 10, 1, 40, 25, allowed, qs=[2])
        gone = np.concatenate([np.flatnonzero(allowed)[::3], np.flatnonzero(~allowed)[::5]]).astype(np.uint64)   # allowed and disallowed ids
        ix.remove_batch(gone)
        ar = ARef(ix, Q, allowed)   # (removed ids stay in the bitmap: they select nothing)
        assert int(ar.alen.sum()) == int(allowed.sum()) - len(np.flatnonzero(allowed)[::3])
        before = [check(ar, 10, 1, 40, 10, allowed)[0], check(ar, 10, 1, 40, 25, allowed, qs=[2])[0]]
        ix.compact()
        after = [check(ar, 10, 1, 40, 10, allowed)[0], check(ar, 10, 1, 40, 25, allowed, qs=[2])[0]]
        for (i0, d0, c0, p0), (i1, d1, c1, p1) in zip(before, after):
            assert np.array_equal(c0, c1) and np.array_equal(p0, p1)
            for q in range(len(c0)):
                assert np.array_equal(i0[q, :c0[q]], i1[q, :c0[q]]) and np.array_equal(bits(d0[q, :c0[q]]), bits(d1[q, :c0[q]]))
    finally:
        ix.close()


# ---- 5. a filter per query ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [1, 3, 64])
def test_multi(main_ix, main_q, F):
    import torch
    ix, Q = main_ix, main_q
    sels = [0.003, 0.02, 0.3, 0.005, 1.0, 0.0]
    filters = [random_filter(N, sels[f % len(sels)], 0xADE0 + f) for f in range(F)]
    filter_of = (np.arange(B) % F).astype(np.uint32)
    top_k, lo, hi, m = 10, 2, 150, 10
    ids, dist, cnt, npr = ix.search_filtered_multi_adaptive(Q, top_k, lo, hi, m, filters, filter_of)
    order = ARef(ix, Q, filters[0]).order   # (the ranking does not depend on the filter: computed once)
    for f in range(F):
        rows = np.flatnonzero(filter_of == f)
        ar = ARef(ix, Q, filters[f], order)
        want_np = ar.depths(lo, hi, m, rows)
        assert np.array_equal(npr[rows], want_np), (f, npr[rows].tolist(), want_np.tolist())
        same_rows((ids[rows], dist[rows], cnt[rows]), ar, rows, top_k, want_np, ("multi", F, f))
        # row q equals the per-call adaptive call with bitmap filter_of[q]
        i1, d1, c1, p1 = ix.search_filtered_adaptive(Q[rows], top_k, lo, hi, m, filters[f])
        assert np.array_equal(cnt[rows], c1) and np.array_equal(npr[rows], p1)
        for i, q in enumerate(rows):
            assert np.array_equal(ids[q, :c1[i]], i1[i, :c1[i]]) and np.array_equal(bits(dist[q, :c1[i]]), bits(d1[i, :c1[i]])), (f, q)
    # an out-of-range filter_of entry: VERS_ERR_INVALID on the host call; on _dev the empty filter -- depth P_max, count 0
    bad_of = filter_of.copy(); bad_of[[1, B - 1]] = [F, 0xFFFFFFFF]
    with pytest.raises(capi.VersError) as e:
        ix.search_filtered_multi_adaptive(Q, top_k, lo, hi, m, filters, bad_of)
    assert e.value.status == capi.ERR_INVALID
    words = capi.allowed_bitmaps(filters, N)
    dev = torch.device("cuda", ix.device)
    qd = torch.from_numpy(Q).to(dev); wd = torch.from_numpy(words.view(np.int64)).to(dev); fd = torch.from_numpy(bad_of.view(np.int32)).to(dev)
    oi = torch.zeros((B, top_k), dtype=torch.int64, device=dev); od = torch.zeros((B, top_k), dtype=torch.float32, device=dev)
    oc = torch.full((B,), 77, dtype=torch.int32, device=dev); on = torch.full((B,), 77, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    ix.search_filtered_multi_adaptive_dev(qd.data_ptr(), ix.d, B, top_k, lo, hi, m, wd.data_ptr(), words.shape[1], F, N, fd.data_ptr(), oi.data_ptr(), od.data_ptr(),
                                          oc.data_ptr(), on.data_ptr())
    ix.poll()
    c2, p2 = oc.cpu().numpy().astype(np.uint32), on.cpu().numpy().astype(np.uint32)
    assert p2[1] == hi and p2[B - 1] == hi and c2[1] == 0 and c2[B - 1] == 0
    keep = np.ones(B, dtype=bool); keep[[1, B - 1]] = False
    assert np.array_equal(c2[keep], cnt[keep]) and np.array_equal(p2[keep], npr[keep])
    i2, d2 = oi.cpu().numpy().astype(np.uint64), od.cpu().numpy()
    for q in np.flatnonzero(keep):
        assert np.array_equal(i2[q, :cnt[q]], ids[q, :cnt[q]]) and np.array_equal(bits(d2[q, :cnt[q]]), bits(dist[q, :cnt[q]])), q


# ---- 6. device pointers on a stream of the caller's ---------------------------------------------------------------------------------------------
def test_device_pointer_call_on_a_stream(main_refs):
    import torch
    ar, allowed = main_refs[1]
    ix = ar.ix
    top_k, lo, hi, m = 10, 4, 150, 10
    want_np = ar.depths(lo, hi, m)
    words = capi.allowed_bitmap(allowed, N)
    dev = torch.device("cuda", ix.device)
    qd = torch.from_numpy(ar.Q).to(dev); wd = torch.from_numpy(words.view(np.int64)).to(dev)
    stream = torch.cuda.Stream(dev)
    for with_np in (True, False):   # (out_nprobe is nullable)
        ids = torch.full((B, top_k), -1, dtype=torch.int64, device=dev); dist = torch.full((B, top_k), -7.25, dtype=torch.float32, device=dev)
        cnt = torch.zeros(B, dtype=torch.int32, device=dev); npr = torch.full((B,), 77, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        ix.search_filtered_adaptive_dev(qd.data_ptr(), ix.d, B, top_k, lo, hi, m, wd.data_ptr(), N, ids.data_ptr(), dist.data_ptr(), cnt.data_ptr(),
                                        npr.data_ptr() if with_np else 0, stream.cuda_stream)
        ix.poll(stream.cuda_stream)
        got = (ids.cpu().numpy().astype(np.uint64), dist.cpu().numpy(), cnt.cpu().numpy().astype(np.uint32))
        same_rows(got, ar, list(range(B)), top_k, want_np, ("dev", with_np))
        assert np.array_equal(npr.cpu().numpy().astype(np.uint32), want_np if with_np else np.full(B, 77, np.uint32))


# ---- 7. NaN --------------------------------------------------------------------------------------------------------------------------------------
def test_nan_row_beyond_the_depth_is_not_an_error():
    src = make(1500, 48, 6, seed=0xADF0)
    ix = IVFFlatIndex(48)
    try:
        c = 2
        bad = int(src.ids[c][70])
        ix.num_centroids, ix.centroids, ix.assignments, ix.ids = src.num_centroids, src.centroids, src.assignments, [list(l) for l in src.ids]
        ix.values = src.values.copy()
        ix.values[bad, 7] = np.nan
        ix._upload()
        Q = queries(src, 0xADF1, 24)
        allowed = random_filter(1500, 0.5, 0xADF2)
        allowed[bad] = True   # the NaN row IS allowed
        ar = ARef(ix, Q, allowed)
        m = 5
        # the queries whose depth stops before list c's rank: the NaN row is allowed for them but lies beyond their P_q lists
        qs = [q for q in range(24) if ar.depth(q, 1, 6, m) <= int(np.flatnonzero(ar.order[q] == c)[0])]
        assert len(qs) >= 3
        for sub in (qs, qs[:1]):
            check(ar, 10, 1, 6, m, allowed, qs=sub)
        for sub in (qs, qs[:1]):   # the same row inside a probed list
            with pytest.raises(capi.VersError) as e:
                ix.search_filtered_adaptive(Q[sub], 10, 6, 6, m, allowed)
            assert e.value.status == capi.ERR_NAN
        check(ar, 10, 1, 6, m, allowed, qs=qs)   # and the handle is still usable
    finally:
        ix.close()
        src.close()


# ---- 8. errors -----------------------------------------------------------------------------------------------------------------------------------
def raw(ix, Q, top_k, nprobe_min, nprobe_max, min_allowed, words, n_bits):
    Q = np.ascontiguousarray(np.atleast_2d(Q), dtype=np.float32)
    b = Q.shape[0]
    ids = np.zeros((b, max(top_k, 1)), np.uint64); dist = np.zeros((b, max(top_k, 1)), np.float32); cnt = np.full(b, 99, np.uint32); npr = np.full(b, 99, np.uint32)
    rc = capi.lib().vers_ivf_search_filtered_adaptive(ix._h, capi._ptr(Q), 4 * ix.d, b, top_k, nprobe_min, nprobe_max, min_allowed,
                                                      capi._ptr(words) if words is not None else None, n_bits, capi._ptr(ids), capi._ptr(dist), capi._ptr(cnt),
                                                      capi._ptr(npr))
    return rc, cnt, npr


def test_errors_and_protocol(main_ix, main_q):
    import torch
    ix, Q = main_ix, main_q[:8]
    words = capi.allowed_bitmap(np.ones(N, dtype=bool), N)
    assert raw(ix, Q, 10, 1, 4, 10, words, N)[0] == capi.OK
    assert raw(ix, Q, 10, 0, 4, 10, words, N)[0] == capi.ERR_INVALID     # nprobe_min == 0
    assert raw(ix, Q, 10, 0, 0, 10, words, N)[0] == capi.ERR_INVALID
    assert raw(ix, Q, 10, 5, 4, 10, words, N)[0] == capi.ERR_INVALID     # nprobe_max < nprobe_min
    assert raw(ix, Q, 10, 1, 4, 10, None, N)[0] == capi.ERR_INVALID      # n_bits > 0 with a NULL bitmap
    fo = np.zeros(8, dtype=np.uint32)
    ids = np.zeros((8, 10), np.uint64); dist = np.zeros((8, 10), np.float32); cnt = np.zeros(8, np.uint32); npr = np.zeros(8, np.uint32)
    Lb = capi.lib()
    for lo, hi, nf in ((0, 4, 1), (5, 4, 1), (1, 4, 0), (1, 4, capi.FILTER_MAX + 1)):
        assert Lb.vers_ivf_search_filtered_multi_adaptive(ix._h, capi._ptr(Q), 4 * ix.d, 8, 10, lo, hi, 10, capi._ptr(words), len(words), nf, N, capi._ptr(fo),
                                                          capi._ptr(ids), capi._ptr(dist), capi._ptr(cnt), capi._ptr(npr)) == capi.ERR_INVALID
    dev = torch.device("cuda", ix.device)
    qd = torch.from_numpy(Q).to(dev); wd = torch.from_numpy(words.view(np.int64)).to(dev)
    oi = torch.zeros((8, 10), dtype=torch.int64, device=dev); od = torch.zeros((8, 10), dtype=torch.float32, device=dev)
    oc = torch.zeros(8, dtype=torch.int32, device=dev); on = torch.zeros(8, dtype=torch.int32, device=dev)
    for lo, hi in ((0, 4), (5, 4)):
        with pytest.raises(capi.VersError) as e:
            ix.search_filtered_adaptive_dev(qd.data_ptr(), ix.d, 8, 10, lo, hi, 10, wd.data_ptr(), N, oi.data_ptr(), od.data_ptr(), oc.data_ptr(), on.data_ptr())
        assert e.value.status == capi.ERR_INVALID
    # top_k == 0: counts 0; b == 0: a no-op
    rc, cnt, npr = raw(ix, Q, 0, 1, 4, 10, words, N)
    assert rc == capi.OK and not cnt.any()
    assert Lb.vers_ivf_search_filtered_adaptive(ix._h, None, 4 * ix.d, 0, 10, 1, 4, 10, capi._ptr(words), N, None, None, None, None) == capi.OK
    assert Lb.vers_ivf_search_filtered_adaptive_dev(ix._h, None, ix.d, 0, 10, 1, 4, 10, None, 0, None, None, None, None, None) == capi.OK
    # an index without centroids
    empty = IVFFlatIndex(ix.d)
    assert raw(empty, Q, 10, 1, 4, 10, words, N)[0] == capi.ERR_INSUFFICIENT
    empty.close()
    # a handle sharded by cluster
    sh = make(600, 32, 4, seed=0xAE00)
    Qs = queries(sh, 0xAE01, 3)
    w600 = capi.allowed_bitmap(np.ones(600, dtype=bool), 600)
    half = IVFFlatIndex(sh.d)
    half.set_shard(0, 2)
    half.num_centroids, half.values, half.centroids, half.assignments = sh.num_centroids, sh.values, sh.centroids, sh.assignments
    half._upload()
    assert raw(sh, Qs, 10, 1, 2, 10, w600, 600)[0] == capi.OK
    assert half.info()[1] == 4 and raw(half, Qs, 10, 1, 2, 10, w600, 600)[0] == capi.ERR_INVALID
    half.close()
    sh.close()


# ---- 9. the C++ mirror ---------------------------------------------------------------------------------------------------------------------------
def test_cpp_host_mirror(tmp_path):
    """vers_amd/host/ivfflat.hpp's search_filtered_adaptive() from compiled code (tests/cpp/filtered_adaptive_demo.cpp) against the Python mirror"""
    lib = capi.LIB_PATH
    exe = str(tmp_path / "filtered_adaptive_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + ROOT, "-o", exe, os.path.join(ROOT, "tests", "cpp", "filtered_adaptive_demo.cpp"),
                           "-L" + os.path.dirname(lib), "-lvers_hip", "-Wl,-rpath," + os.path.dirname(lib)])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.rstrip().endswith("DONE"), out.stdout[-2000:] + out.stderr
    i, j = np.meshgrid(np.arange(900), np.arange(40), indexing="ij")
    X = (((i * 7 + j * 13) % 31).astype(np.float32) * np.float32(0.25) + (i % 6).astype(np.float32)).astype(np.float32)
    ix = IVFFlatIndex.build_index(6, 1, 5, X, init_indices=np.asarray([3, 90, 200, 333, 480, 899], dtype=np.uint64))
    rows, depth = {}, {}
    for line in out.stdout.splitlines()[:-1]:
        t = line.split()
        if t[1] == "D":
            depth[int(t[0])] = int(t[2])
        else:
            rows.setdefault(int(t[0]), []).append((int(t[2]), int(t[3])))
    for q in range(6):
        allowed = np.zeros(900 - 37 * q, dtype=bool)
        allowed[::13 + 7 * q] = True
        ids, dist, cnt, npr = ix.search_filtered_adaptive(X[q * 31], 12, 1, 5, 6 + 3 * q, allowed)
        assert depth[q] == int(npr[0]), q
        assert rows.get(q, []) == list(zip(ids[0, :cnt[0]].tolist(), bits(dist[0, :cnt[0]]).tolist())), q
    assert len(set(depth.values())) > 1 and sum(len(r) for r in rows.values()) > 12
    ix.close()


# ---- 10. the existing calls around adaptive calls ----------------------------------------------------------------------------------------------
def test_existing_calls_are_unchanged_around_adaptive_calls(main_refs):
    ar, allowed = main_refs[0]
    ix, Q = ar.ix, ar.Q

    def snapshot():
        out = [ix.search_filtered(Q, 10, 8, allowed)]
        stats = ix.filter_stats()["last"]
        out += [ix.search_batch(Q, 10, 4), ix.search_batch(Q, 10, 0), ix.search_batch(Q[0], 10, 4)]
        return out, stats

    before, st0 = snapshot()
    check(ar, 10, 4, 150, 10, allowed); check(ar, 70, 2, 150, 70, allowed, qs=[3])
    assert ix.filter_stats()["last"] != st0   # (the hook covers the adaptive call: another plan, other counts)
    after, st1 = snapshot()
    assert st0 == st1
    for (i0, d0, c0), (i1, d1, c1) in zip(before, after):
        assert np.array_equal(c0, c1)
        for q in range(len(c0)):
            assert np.array_equal(i0[q, :c0[q]], i1[q, :c0[q]]) and np.array_equal(bits(d0[q, :c0[q]]), bits(d1[q, :c0[q]]))


def test_scan_timing_ring_and_stats(main_refs):
    """the ring gets the mask record, the allowed-count record and one record per scan pass; the stats hook counts the plan the depths imply"""
    ar, allowed = main_refs[0]
    ix = ar.ix
    capi.set_option("scan_events", 1)
    try:
        lo, hi, m = 4, 150, 10
        ix.scan_times(reset=True)
        check(ar, 70, lo, hi, m, allowed)
        assert len(ix.scan_times(reset=True)) == 4   # ... + two passes
        (_, _, _, npr), _ = check(ar, 10, lo, hi, m, allowed)
        assert len(ix.scan_times(reset=True)) == 3   # the mask kernel, the allowed-count kernel, one filtered pass
        st = ix.filter_stats()["last"]
        assert st["rows_allowed"] == int(ar.alen.sum())
        # tiles planned (one pass): a visited list's whole tiles once per group of the queries that visit it -- at least once per visited list, at
        # most once per (query, visited rank); nothing of a rank beyond a query's depth
        t_list = (np.asarray([len(l) for l in ix.ids]) + 63) // 64
        union = np.unique(np.concatenate([ar.order[q][:npr[q]] for q in range(B)]))
        per_pair = sum(int(t_list[ar.order[q][:npr[q]]].sum()) for q in range(B))
        assert int(t_list[union].sum()) <= st["tiles_planned"] <= per_pair and st["tiles_loaded"] <= st["tiles_planned"]
        assert per_pair < sum(int(t_list[ar.order[q][:hi]].sum()) for q in range(B))   # (the depths do stop short of nprobe_max here)
    finally:
        capi.set_option("scan_events", 2)
