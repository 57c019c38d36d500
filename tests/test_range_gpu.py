"""vers_ivf_range_search / vers_ivf_range_search_dev: every row of the min(nprobe, k) nearest lists whose distance to the query is <= its
radius.  The expected result is the oracle's nprobe search with top_k = every live row, cut at dist <= r: ids, order and distance BITS are
compared with np.array_equal -- no tolerance.  Every case checks both orders, the batch and (for its first and last query) the single-query
call, that the walk order stably re-sorted by distance is the sorted order, and that the walk order is the probed lists (get_list) in
probe-rank order with ascending list position inside a list."""
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


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def make(n, d, k, metric=capi.METRIC_L2SQ, seed=0x5A10, iters=4, X=None):
    if X is None:
        X = dg.dist_c(seed, n, d, 2 * k, dg.default_sigma(d))
    init = mg.init_draws(seed + 1, 1, k, n)
    return IVFFlatIndex.build_index(k, 1, iters, X, init_indices=init, metric=metric)


def queries(ix, seed, b):
    d, k = ix.d, ix.num_centroids
    return dg.dist_c(seed, b, d, 2 * k, dg.default_sigma(d))


class Ref:
    """The oracle's view of (index, queries, nprobe), computed ONCE and shared by every radius / order / call shape: per query the full
    nprobe result over every live row (ascending (distance, probe rank, list position)) and the probed lists in probe-rank order."""

    def __init__(self, ix, Q, nprobe):
        self.ix, self.Q, self.nprobe = ix, np.atleast_2d(Q), nprobe
        k = ix.num_centroids
        live = sum(len(l) for l in ix.ids)
        self.full, self.probes = [], []
        for q in self.Q:
            self.full.append(co.search_nprobe(ix.values, ix.centroids, ix.ids, q, max(live, 1), nprobe, ix.metric))
            rank, _ = co.search_exhaustive(ix.centroids, q, k, ix.metric)   # stable: first minimum, ties by index
            self.probes.append([int(c) for c in rank[:min(nprobe, k)]])
        self.lists = {}   # the device's lists, read back once

    def device_list(self, c):
        if c not in self.lists:
            self.lists[c] = self.ix.get_list(c)[1]
            assert np.array_equal(self.lists[c], np.asarray(self.ix.ids[c], dtype=np.uint64)), c
        return self.lists[c]

    def mth(self, q, m):
        """the exact distance of query q's m-th nearest probed row (the last one when fewer are probed)"""
        od = self.full[q][1]
        return od[min(m, len(od)) - 1] if len(od) else np.float32(0)

    def sorted(self, q, r):
        oi, od = self.full[q]
        m = int(np.count_nonzero(od <= np.float32(r)))
        assert not np.any(od[m:] <= np.float32(r))   # the result is the LEADING entries
        return oi[:m], od[:m]

    def walk(self, q, r):
        oi, od = self.full[q]
        dist_of = dict(zip(oi.tolist(), od.tolist()))
        ids = [v for c in self.probes[q] for v in self.device_list(c).tolist() if np.float32(dist_of[v]) <= np.float32(r)]
        return np.asarray(ids, dtype=np.uint64), np.asarray([dist_of[v] for v in ids], dtype=np.float32)


def check_result(ref, qs, radii, got_sorted, got_walk):
    """qs: the reference's query numbers the two results (lims, ids, dist) were computed for, in order"""
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
        o = np.argsort(wd, kind="stable")
        assert np.array_equal(wi[o], si) and np.array_equal(bits(wd[o]), bits(sd)), ("walk re-sorted", q)


def check_range(ref, radii, singles=True):
    ix, Q, nprobe = ref.ix, ref.Q, ref.nprobe
    b = Q.shape[0]
    radii = np.broadcast_to(np.asarray(radii, dtype=np.float32), (b,)).copy()
    got = [ix.range_search(Q, radii, nprobe, walk_order=w) for w in (False, True)]
    check_result(ref, range(b), radii, got[0], got[1])
    if singles:
        for q in sorted({0, b - 1}):
            one = [ix.range_search(Q[q], radii[q], nprobe, walk_order=w) for w in (False, True)]
            check_result(ref, [q], radii[q:q + 1], one[0], one[1])
    return got[0]


def radii_mth(ref, m):
    return np.asarray([ref.mth(q, m) for q in range(ref.Q.shape[0])], dtype=np.float32)


# ---- 1. query-group widths and segmenting ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def main_ix():
    ix = make(6000, 96, 12)
    yield ix
    ix.close()


@pytest.fixture(scope="module")
def main_refs(main_ix):
    """(queries, nprobe = 4) references per batch size: by plan_search's rule b = 1, 5 -> one query per item, 8 -> groups of 8,
    40 -> groups of 16 with some lists walked by several groups"""
    return {b: Ref(main_ix, queries(main_ix, 0x5A17 + b, b), 4) for b in (1, 5, 8, 40)}


@pytest.mark.parametrize("seg_rows", [0, 64])
@pytest.mark.parametrize("b", [1, 5, 8, 40])
def test_query_group_widths_segments_and_boundary_radii(main_refs, b, seg_rows):
    ref = main_refs[b]
    if b == 40:
        per_list = np.bincount([c for p in ref.probes for c in p], minlength=12)
        assert per_list.max() > 16   # a list probed by more queries than one group holds
    try:
        capi.set_option("seg_rows", seg_rows)   # 64: lists of ~500 rows span many one-tile segments
        for m in (1, 10, 300):   # r = the exact distance of the m-th nearest probed row: <= includes the boundary row
            lims, _, _ = check_range(ref, radii_mth(ref, m))
            assert np.all(np.diff(lims.astype(np.int64)) >= min(m, 1))
    finally:
        capi.set_option("seg_rows", 0)


# ---- 2. ties inside a list and across lists; radii -1, 0, +inf mixed in one batch -----------------------------------------------------------
def test_equal_distances_and_mixed_radii():
    n, d, k, b = 3000, 96, 8, 16
    X = dg.dist_c(0x5B20, n, d, 2 * k, dg.default_sigma(d)).copy()
    X[:, 0] *= 8.0                       # coordinate 0 decides the cluster ...
    X[50::50] = X[49:n - 1:50]           # every 50th row is a copy of its predecessor: equal distances inside a list
    X[75::50] = X[74:n - 1:50]
    X[75::50, 0] *= -1.0                 # ... and a mirror image in coordinate 0: equal distances across lists for queries with q[0] = 0
    ix = make(n, d, k, seed=0x5B20, X=X)
    A = ix.assignments.astype(np.int64)
    assert np.all(A[50::50] == A[49:n - 1:50]) and np.any(A[75::50] != A[74:n - 1:50])
    Q = queries(ix, 0x5B27, b).copy()
    Q[:, 0] = 0.0
    Q[3] = X[99]; Q[3, 0] = 0.0
    ref = Ref(ix, Q, k)
    od = ref.full[0][1]
    assert np.count_nonzero(bits(od)[1:] == bits(od)[:-1]) >= 2 * (n // 50) - 2   # the ties are there, in lists and across them
    check_range(ref, INF)
    check_range(ref, radii_mth(ref, 101))
    mixed = np.asarray([(-1.0, 0.0, INF, ref.mth(q, 10))[q % 4] for q in range(b)], dtype=np.float32)
    lims, _, _ = check_range(ref, mixed)
    cnt = np.diff(lims.astype(np.int64))
    assert np.all(cnt[0::4] == 0) and np.all(cnt[2::4] == n) and np.all(cnt[3::4] >= 10)
    Q0 = np.stack([X[49], X[74]])        # radius 0 on a stored row: the row and its copy
    ref0 = Ref(ix, Q0, k)
    lims, ids, _ = check_range(ref0, 0.0)
    assert sorted(ids[:int(lims[1])].tolist()) == [49, 50]
    ix.close()


# ---- 3. every list; more than 64 probes ----------------------------------------------------------------------------------------------------
def test_every_list_probed(main_ix):
    ref = Ref(main_ix, queries(main_ix, 0x5C31, 8), main_ix.num_centroids)
    check_range(ref, radii_mth(ref, 300))
    lims, _, _ = check_range(ref, INF, singles=False)
    assert np.all(np.diff(lims.astype(np.int64)) == 6000)


def test_more_than_64_probes():
    ix = make(4000, 96, 80, seed=0x5C40)
    ref = Ref(ix, queries(ix, 0x5C47, 3), 80)
    check_range(ref, radii_mth(ref, 10))
    lims, _, _ = check_range(ref, INF)
    assert np.all(np.diff(lims.astype(np.int64)) == 4000)
    ix.close()


# ---- 4. dimensions and metrics ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,n,k", [(7, 1500, 6), (300, 1500, 6), (1536, 1500, 6), (2816, 600, 4)])
def test_dimensions(d, n, k):
    """d = 2816: a block of 16 queries no longer fits LDS, the planner drops to groups of 8"""
    ix = make(n, d, k, seed=0x5D00 + d)
    ref = Ref(ix, queries(ix, 0x5D07 + d, 40), 3)
    for m in (1, 10, 300):
        check_range(ref, radii_mth(ref, m), singles=m == 10)
    ix.close()


def test_cosine_distance():
    ix = make(6000, 96, 12, metric=capi.METRIC_COSDIST, seed=0x5D60)
    for b in (5, 40):
        ref = Ref(ix, queries(ix, 0x5D67 + b, b), 4)
        for m in (1, 10, 300):
            check_range(ref, radii_mth(ref, m))
    ix.close()


# ---- 5. a mutated index -------------------------------------------------------------------------------------------------------------------
def test_mutated_index():
    n, d, k, b = 2600, 64, 12, 8
    ix = make(n, d, k, seed=0x5E10)
    Q = queries(ix, 0x5E17, b)

    def check_now():
        assert np.array_equal(ix.list_lengths(), np.asarray([len(l) for l in ix.ids], dtype=np.uint64))
        ref = Ref(ix, Q, k)   # every list probed: the empty one, the 64- and the 65-row one too
        check_range(ref, radii_mth(ref, 10))
        mixed = np.asarray([(INF, ref.mth(q, 100))[q % 2] for q in range(b)], dtype=np.float32)
        lims, _, _ = check_range(ref, mixed, singles=False)
        assert np.all(np.diff(lims.astype(np.int64))[0::2] == ix.live_count())

    lens = [len(l) for l in ix.ids]
    order = np.argsort(lens)[::-1]
    c_tile, c_empty, c64, c65 = (int(order[i]) for i in range(4))
    assert lens[c_tile] >= 128 and lens[c65] >= 110
    gone = set(range(0, n, 3)) | set(ix.ids[c_tile][64:128])   # every third id + one whole tile of a list
    ix.remove_batch(sorted(gone))
    check_now()
    ix.remove_batch(list(ix.ids[c_empty]) + list(ix.ids[c64][64:]) + list(ix.ids[c65][65:]))
    assert (len(ix.ids[c_empty]), len(ix.ids[c64]), len(ix.ids[c65])) == (0, 64, 65)
    check_now()
    capi.add_batch_phases(reset=True)
    ix.add_batch(dg.dist_c(0x5E20, 40, d, 2 * k, dg.default_sigma(d)))        # into the freed slack
    assert capi.add_batch_phases()["relayouts"] == 0
    check_now()
    ix.add_batch(dg.dist_c(0x5E21, 2500, d, 2 * k, dg.default_sigma(d)))      # beyond every list's capacity: a re-layout
    assert capi.add_batch_phases()["relayouts"] >= 1
    check_now()
    before, after = ix.compact()
    assert after <= before
    check_now()
    ix.close()


# ---- 6. the protocol ----------------------------------------------------------------------------------------------------------------------
def raw_call(ix, Q, radii, nprobe, flags, cap, ids=None, dist=None):
    Q = np.ascontiguousarray(np.atleast_2d(Q), dtype=np.float32)
    b = Q.shape[0]
    r = np.ascontiguousarray(np.broadcast_to(np.asarray(radii, dtype=np.float32), (b,)))
    lims = np.full(b + 1, 0xABABABABABABABAB, dtype=np.uint64)
    total = C.c_uint64(12345)
    rc = capi.lib().vers_ivf_range_search(ix._h, capi._ptr(Q), 4 * ix.d, b, capi._ptr(r), nprobe, flags, capi._ptr(lims),
                                          capi._ptr(ids) if ids is not None else None, capi._ptr(dist) if dist is not None else None, cap,
                                          C.byref(total))
    return rc, lims, int(total.value)


def test_capacity_protocol_and_errors(main_ix):
    ix = main_ix
    Q = queries(ix, 0x5F10, 8)
    ref = Ref(ix, Q, 4)
    radii = radii_mth(ref, 10)
    want = check_range(ref, radii, singles=False)
    total = int(want[0][-1])
    assert total >= 80
    L = capi.lib()
    # the size query: cap == 0 with NULL arrays
    rc, lims, got = raw_call(ix, Q, radii, 4, 0, 0)
    assert rc == capi.OK and got == total and np.array_equal(lims, want[0])
    # one short: VERS_OK, the total, complete limits, ids / distances untouched
    ids = np.full(total, 0xCDCDCDCDCDCDCDCD, dtype=np.uint64); dist = np.full(total, -7.25, dtype=np.float32)
    rc, lims, got = raw_call(ix, Q, radii, 4, 0, total - 1, ids, dist)
    assert rc == capi.OK and got == total > total - 1 and np.array_equal(lims, want[0])
    assert np.all(ids == 0xCDCDCDCDCDCDCDCD) and np.all(dist == np.float32(-7.25))
    # exactly enough
    rc, lims, got = raw_call(ix, Q, radii, 4, 0, total, ids, dist)
    assert rc == capi.OK and got == total and np.array_equal(ids, want[1]) and np.array_equal(bits(dist), bits(want[2]))
    # b == 0: a no-op, *out_total = 0
    t = C.c_uint64(99)
    assert L.vers_ivf_range_search(ix._h, None, 4 * ix.d, 0, None, 4, 0, None, None, None, 0, C.byref(t)) == capi.OK and t.value == 0
    assert L.vers_ivf_range_search_dev(ix._h, None, ix.d, 0, None, 4, 0, None, None, None, 0, C.byref(t), None) == capi.OK and t.value == 0
    # argument errors
    bad = radii.copy(); bad[3] = np.nan
    assert raw_call(ix, Q, bad, 4, 0, 0)[0] == capi.ERR_INVALID
    assert raw_call(ix, Q, radii, 0, 0, 0)[0] == capi.ERR_INVALID
    assert raw_call(ix, Q, radii, 4, 2, 0)[0] == capi.ERR_INVALID
    assert raw_call(ix, Q, radii, 4, 0, 5)[0] == capi.ERR_INVALID           # a capacity without arrays
    # a NaN query: VERS_ERR_NAN, and the handle is still usable
    Qn = Q.copy(); Qn[2, 5] = np.nan
    rc, _, _ = raw_call(ix, Qn, INF, 4, 0, 0)
    assert rc == capi.ERR_NAN
    rc, lims, got = raw_call(ix, Q, radii, 4, 0, 0)
    assert rc == capi.OK and got == total and np.array_equal(lims, want[0])
    # an empty handle; a handle sharded by cluster
    empty = IVFFlatIndex(ix.d)
    assert raw_call(empty, Q, radii, 4, 0, 0)[0] == capi.ERR_INSUFFICIENT
    empty.close()
    sh = make(600, 32, 4, seed=0x5F40)
    Qs = queries(sh, 0x5F47, 3)
    assert raw_call(sh, Qs, INF, 2, 0, 0)[0] == capi.OK
    half = IVFFlatIndex(sh.d)
    half.set_shard(0, 2)   # (before the upload: this handle stores the lists of rank 0 of 2)
    half.num_centroids, half.values, half.centroids, half.assignments = sh.num_centroids, sh.values, sh.centroids, sh.assignments
    half._upload()
    assert half.info()[1] == 4 and raw_call(half, Qs, INF, 2, 0, 0)[0] == capi.ERR_INVALID
    half.close()
    sh.close()


def test_top_k_search_is_unchanged_around_a_range_call(main_ix):
    """the workspace lease is clean: the same top-k batch before and after a range call returns the same bits"""
    ix = main_ix
    Q = queries(ix, 0x5F60, 40)
    before = [ix.search_batch(Q, top_k, nprobe) for top_k, nprobe in ((10, 4), (10, 0), (100, 4))] + [ix.search_batch(Q[0], 10, 4)]
    ref = Ref(ix, Q, 4)
    check_range(ref, radii_mth(ref, 10), singles=True)
    after = [ix.search_batch(Q, top_k, nprobe) for top_k, nprobe in ((10, 4), (10, 0), (100, 4))] + [ix.search_batch(Q[0], 10, 4)]
    for (i0, d0, c0), (i1, d1, c1) in zip(before, after):
        assert np.array_equal(c0, c1)
        for q in range(len(c0)):
            assert np.array_equal(i0[q, :c0[q]], i1[q, :c0[q]]) and np.array_equal(bits(d0[q, :c0[q]]), bits(d1[q, :c0[q]]))


def test_device_pointer_call_on_two_streams(main_ix):
    import torch
    ix = main_ix
    b = 8
    Q = queries(ix, 0x5F80, b)
    ref = Ref(ix, Q, 4)
    radii = radii_mth(ref, 10)
    want = [ix.range_search(Q, radii, 4, walk_order=w) for w in (False, True)]
    total = int(want[0][0][-1])
    dev = torch.device("cuda", ix.device)
    qd = torch.from_numpy(Q).to(dev)
    rd = torch.from_numpy(radii).to(dev)
    for stream in (torch.cuda.Stream(dev), torch.cuda.Stream(dev)):
        for w, flags in ((0, 0), (1, capi.RANGE_WALK_ORDER)):
            lims = torch.zeros(b + 1, dtype=torch.int64, device=dev)
            ids = torch.full((total,), -1, dtype=torch.int64, device=dev)
            dist = torch.full((total,), -7.25, dtype=torch.float32, device=dev)
            torch.cuda.synchronize(dev)
            # the size query, one short (untouched), then the full call
            assert ix.range_search_dev(qd.data_ptr(), ix.d, b, rd.data_ptr(), 4, flags, lims.data_ptr(), 0, 0, 0, stream.cuda_stream) == total
            assert ix.range_search_dev(qd.data_ptr(), ix.d, b, rd.data_ptr(), 4, flags, lims.data_ptr(), ids.data_ptr(), dist.data_ptr(), total - 1,
                                       stream.cuda_stream) == total
            assert bool((ids == -1).all()) and bool((dist == -7.25).all())
            assert ix.range_search_dev(qd.data_ptr(), ix.d, b, rd.data_ptr(), 4, flags, lims.data_ptr(), ids.data_ptr(), dist.data_ptr(), total,
                                       stream.cuda_stream) == total
            assert np.array_equal(lims.cpu().numpy().astype(np.uint64), want[w][0])
            assert np.array_equal(ids.cpu().numpy().astype(np.uint64), want[w][1])
            assert np.array_equal(bits(dist.cpu().numpy()), bits(want[w][2]))
    # a NaN radius on the device is an argument error there too
    bad = rd.clone(); bad[1] = float("nan")
    lims = torch.zeros(b + 1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    with pytest.raises(capi.VersError) as e:
        ix.range_search_dev(qd.data_ptr(), ix.d, b, bad.data_ptr(), 4, 0, lims.data_ptr(), 0, 0, 0, 0)
    assert e.value.status == capi.ERR_INVALID


# ---- 7. the phases hook -------------------------------------------------------------------------------------------------------------------
def test_phases_hook(main_ix):
    ix = main_ix
    Q = queries(ix, 0x5FA0, 8)
    ref = Ref(ix, Q, 4)
    radii = radii_mth(ref, 10)
    lims, _, _ = ix.range_search(Q, radii, 4)      # (sizes the binding's capacity: the next call is ONE call of the C ABI)
    capi.range_phases(reset=True)
    assert all(v == 0 for v in capi.range_phases().values())
    lims, _, _ = ix.range_search(Q, radii, 4)
    ph = capi.range_phases(reset=True)
    assert (ph["calls"], ph["queries"], ph["results"]) == (1, 8, int(lims[-1]))
    assert ph["count_ms"] > 0 and ph["fill_ms"] > 0 and ph["sort_ms"] > 0 and ph["plan_ms"] > 0 and ph["scan_ms"] > 0
    assert all(v == 0 for v in capi.range_phases().values())


# ---- 8. the C++ mirror --------------------------------------------------------------------------------------------------------------------
def test_cpp_host_mirror_range_search(tmp_path):
    """vers_amd/host/ivfflat.hpp's range_search() from compiled code (tests/cpp/range_demo.cpp) against the Python mirror's result"""
    lib = capi.LIB_PATH
    exe = str(tmp_path / "range_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + ROOT, "-o", exe, os.path.join(ROOT, "tests", "cpp", "range_demo.cpp"),
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
            lims, ids, dist = ix.range_search(X[q * 31], (0.0, 150.0, 400.0)[q % 3], 3, walk_order=bool(w))
            assert got.get((q, w), []) == list(zip(ids.tolist(), bits(dist).tolist())), (q, w)
            n_rows += ids.size
    assert n_rows > 12   # (the radii select something: every query is a stored row)
    ix.close()
