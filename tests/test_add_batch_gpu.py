"""vers_ivf_add_batch / vers_ivf_add_batch_dev: n vectors in one call leave exactly what n calls of vers_ivf_add leave behind.
Every case grows a TWIN -- the same build (injected init draws), grown with single adds -- and compares clusters, vec ids,
info, list lengths, every list's stored bits and ids, and search results bit for bit (batches of >= 32 queries: the fp16-shadow
list scan; single queries: the single-query path), plus the oracle on a sample."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import c_oracle as co
from tests import datagen as dg
from tests.golden import make_golden as mg
from vers_amd import build as vbuild
from vers_amd import capi
from vers_amd.index import IVFFlatIndex

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def pair(n, d, k, metric=capi.METRIC_L2SQ, seed=0xADD0, iters=4, X=None):
    if X is None:
        X = dg.dist_c(seed, n, d, 2 * k, dg.default_sigma(d))
    init = mg.init_draws(seed + 1, 1, k, X.shape[0])
    a = IVFFlatIndex.build_index(k, 1, iters, X, init_indices=init, metric=metric)
    b = IVFFlatIndex.build_index(k, 1, iters, X, init_indices=init, metric=metric)
    assert np.array_equal(a.assignments, b.assignments)
    return a, b


def grow_twin(twin, rows):
    out = [twin.add(x) for x in rows]
    return (np.array([c for c, _ in out], dtype=np.uint64), np.array([v for _, v in out], dtype=np.uint64))


def same_state(a, b):
    assert a.info() == b.info()
    assert np.array_equal(a.list_lengths(), b.list_lengths())
    assert np.array_equal(a.assignments, b.assignments)
    assert a.ids == b.ids
    assert np.array_equal(bits(a.values), bits(b.values))
    for c in range(a.info()[1]):
        ra, ia = a.get_list(c)
        rb, ib = b.get_list(c)
        assert np.array_equal(ia, ib), c
        assert np.array_equal(bits(ra), bits(rb)), c
        assert np.array_equal(ia, np.asarray(a.ids[c], dtype=np.uint64)), c   # ... and the host mirror's list order
        assert np.array_equal(bits(ra), bits(a.values[ia.astype(np.int64)])), c


def same_search(a, b, Q, nprobes=None, top_ks=(1, 10, 64, 200), oracle_rows=(0,)):
    k = a.info()[1]
    nprobes = nprobes or (0, 1, 5, k)
    for nprobe in nprobes:
        for top_k in top_ks:
            if nprobe == 0 and top_k > a.info()[0]:
                continue
            for qs in (Q, Q[:1], Q[-1:]):   # a batch (matrix-core scan on the shadow) and single queries
                ia, da, ca = a.search_batch(qs, top_k, nprobe)
                ib, db, cb = b.search_batch(qs, top_k, nprobe)
                assert np.array_equal(ca, cb), (nprobe, top_k)
                for q in range(qs.shape[0]):
                    c = int(ca[q])
                    assert np.array_equal(ia[q, :c], ib[q, :c]) and np.array_equal(bits(da[q, :c]), bits(db[q, :c])), (nprobe, top_k, q)
            ia, da, ca = a.search_batch(Q, top_k, nprobe)
            for q in oracle_rows:
                oi, od = (co.search_approximate(a.values, a.centroids, a.ids, Q[q], top_k, a.metric) if nprobe == 0 else
                          co.search_nprobe(a.values, a.centroids, a.ids, Q[q], top_k, nprobe, a.metric))
                assert np.array_equal(ia[q, :len(oi)], oi) and np.array_equal(bits(da[q, :len(oi)]), bits(od)), (nprobe, top_k, q)


@pytest.fixture
def small_chunks():
    """Batches streamed in chunks of 64 rows: every chunk is a batch add of its own."""
    capi.set_option("add_batch_rows", 64)
    yield
    capi.set_option("add_batch_rows", 131072)


@pytest.mark.parametrize("metric", [capi.METRIC_L2SQ, capi.METRIC_COSDIST])
@pytest.mark.parametrize("d", [16, 300, 768])
def test_batches_equal_single_adds(metric, d):
    n, k = 2000, 24
    a, b = pair(n, d, k, metric, seed=0xADD0 + d)
    sigma = dg.default_sigma(d)
    Q = dg.dist_c(0xADD7 + d, 40, d, 2 * k, sigma, seed_c=0xADD0 + d)
    seq = [1, "single", 63, "search", 64, 65, "single", 300, "search"]
    s = 0
    for step in seq:
        if step == "search":
            same_state(a, b)
            same_search(a, b, Q)
            continue
        if step == "single":
            x = dg.dist_u(0xADD9 + s, 1, d)[0]
            assert a.add(x) == b.add(x)
            s += 1
            continue
        rows = dg.dist_c(0xADD1 + s, step, d, 2 * k, sigma, seed_c=0xADD0 + d)
        rows[::7] *= np.float32(3.0)   # some rows far from every mode
        n0 = a.info()[0]
        cl, vids = a.add_batch(rows)
        tc, tv = grow_twin(b, rows)
        assert np.array_equal(cl, tc) and np.array_equal(vids, tv)
        assert np.array_equal(vids, np.arange(n0, n0 + step, dtype=np.uint64))
        for i in range(0, step, 29):   # the oracle's first-minimum centroid
            assert cl[i] == co.add_cluster(a.centroids, rows[i], metric)
        s += 1
    a.close(); b.close()


def test_chunked_host_batch_equals_single_adds(small_chunks):
    d, k = 40, 16
    a, b = pair(1500, d, k, seed=0xC40)
    rows = dg.dist_c(0xC41, 333, d, 2 * k, dg.default_sigma(d), seed_c=0xC40)
    cl, vids = a.add_batch(rows)
    tc, tv = grow_twin(b, rows)
    assert np.array_equal(cl, tc) and np.array_equal(vids, tv)
    same_state(a, b)
    same_search(a, b, dg.dist_c(0xC42, 33, d, 2 * k, dg.default_sigma(d), seed_c=0xC40), nprobes=(0, 3), top_ks=(10,))


def test_relayout_one_list_doubled_and_batch_larger_than_index():
    d, k = 64, 12
    a, b = pair(1200, d, k, seed=0x4E1)
    sizes = a.list_lengths()
    c = int(np.argmax(sizes))
    rng = np.random.default_rng(5)
    around = (a.centroids[c][None, :] + rng.normal(0, 1e-3, (2 * int(sizes[c]) + 70, d))).astype(np.float32)
    lb0 = a.layout_bytes()["rows"]
    cl, _ = a.add_batch(around)
    grow_twin(b, around)
    assert a.list_lengths()[c] > 2 * sizes[c]
    assert a.layout_bytes()["rows"] > lb0 and capi.add_batch_phases()["relayouts"] >= 1
    same_state(a, b)
    big = dg.dist_c(0x4E2, 1500, d, 2 * k, dg.default_sigma(d), seed_c=0x4E1)   # more rows than the whole index
    a.add_batch(big)
    grow_twin(b, big)
    same_state(a, b)
    same_search(a, b, dg.dist_c(0x4E3, 36, d, 2 * k, dg.default_sigma(d), seed_c=0x4E1), top_ks=(10, 64))


def test_certificate_inputs_follow_the_batch():
    """Rows 10^3 x the corpus norm and rows whose fp16 residual beats every stored row's: the norm and residual maxima the
    certificates of the batched and single-query scans read must include them."""
    d, k = 128, 16
    a, b = pair(3000, d, k, seed=0xCE0)
    assert a.shadow_state()["active"]
    base = dg.dist_c(0xCE1, 40, d, 2 * k, dg.default_sigma(d), seed_c=0xCE0)
    huge = base[:20] * np.float32(1000.0)
    coarse = (base[20:] + np.float32(1000.3)).astype(np.float32)   # fp16 spacing 0.5 at 1000: residuals up to 0.25 per element
    rows = np.concatenate([huge, coarse])
    a.add_batch(rows)
    grow_twin(b, rows)
    assert a.shadow_state()["active"], "the batch left the fp16 shadow behind"
    same_state(a, b)
    rng = np.random.default_rng(9)
    Q = (rows + rng.normal(0, 1e-2, rows.shape)).astype(np.float32)   # their true neighbours are the added rows
    for nprobe in (0, 1, k):
        for top_k in (1, 10):
            ia, da, ca = a.search_batch(Q, top_k, nprobe)
            for q in range(Q.shape[0]):
                oi, od = (co.search_approximate(a.values, a.centroids, a.ids, Q[q], top_k) if nprobe == 0 else
                          co.search_nprobe(a.values, a.centroids, a.ids, Q[q], top_k, nprobe))
                assert np.array_equal(ia[q, :len(oi)], oi) and np.array_equal(bits(da[q, :len(oi)]), bits(od)), (nprobe, top_k, q)
            for q in (0, 25):
                i1, d1, c1 = a.search_batch(Q[q], top_k, nprobe)
                assert np.array_equal(i1[0, :c1[0]], ia[q, :ca[q]]) and np.array_equal(bits(d1[0, :c1[0]]), bits(da[q, :ca[q]]))
    same_search(a, b, Q, nprobes=(0, 5), top_ks=(10,))


def test_matrix_core_assignment():
    """d = 768, k = 4096 and n k d >= 1e11: the chunk's assignment runs the matrix-core cascade (km_use_mfma)."""
    d, k, n0, n = 768, 4096, 8192, 32768
    assert n * k * d >= 1e11
    X = dg.dist_c(0x3F0, n0, d, k, dg.default_sigma(d))
    ix = IVFFlatIndex.build_index(k, 1, 2, X, init_indices=mg.init_draws(0x3F1, 1, k, n0))
    rows = dg.dist_c(0x3F2, n, d, k, dg.default_sigma(d), seed_c=0x3F0)
    lens0 = ix.list_lengths().copy()
    before = {c: ix.get_list(c) for c in range(0, k, 97)}
    capi.assign_stats(reset=True)
    cl, vids = ix.add_batch(rows)
    assert capi.assign_stats()[0] >= n, "the batch did not go through the matrix-core assign pass"
    ref = capi.kmeans_assign(rows, ix.centroids)
    assert np.array_equal(cl, ref)
    for i in range(0, n, 1031):
        assert cl[i] == co.add_cluster(ix.centroids, rows[i])
    assert np.array_equal(ix.list_lengths(), lens0 + np.bincount(cl.astype(np.int64), minlength=k).astype(np.uint64))
    for c, (r0, i0) in before.items():   # old rows untouched, then the new ones in ascending vec id
        r1, i1 = ix.get_list(c)
        mine = np.nonzero(cl == c)[0]
        assert np.array_equal(i1, np.concatenate([i0, vids[mine]]))
        assert np.array_equal(bits(r1), bits(np.concatenate([r0, rows[mine]])))
    ix.close()


@pytest.mark.parametrize("chunked", [False, True])
def test_nan_row_stops_where_the_loop_would(chunked):
    d, k, i = 32, 8, 37
    if chunked:
        capi.set_option("add_batch_rows", 16)
    try:
        a, b = pair(800, d, k, seed=0x7A0)
        rows = dg.dist_u(0x7A1, 100, d)
        rows[i, 3] = np.nan
        rows[i + 5, 0] = np.nan
        first = C.c_uint64(0); added = C.c_uint64(0)
        cl = np.zeros(100, np.uint64)
        rc = capi.lib().vers_ivf_add_batch(a._h, capi._ptr(rows), 100, 4 * d, capi._ptr(cl), C.byref(first), C.byref(added))
        assert rc == capi.ERR_NAN and added.value == i and first.value == 800
        tc, _ = grow_twin(b, rows[:i])
        with pytest.raises(capi.VersError) as e:
            b.add(rows[i])
        assert e.value.status == capi.ERR_NAN
        assert np.array_equal(cl[:i], tc)
        a.assignments = b.assignments; a.ids = b.ids; a.values = b.values   # (raw call above: mirror the twin's fields)
        same_state(a, b)
        # the Python mirror keeps the rows before the NaN and raises
        a2, b2 = pair(800, d, k, seed=0x7A0)
        with pytest.raises(capi.VersError) as e:
            a2.add_batch(rows)
        assert e.value.status == capi.ERR_NAN and a2.info()[0] == 800 + i
        grow_twin(b2, rows[:i])
        same_state(a2, b2)
    finally:
        capi.set_option("add_batch_rows", 131072)


def test_nan_with_one_centroid_empty_index_and_empty_batch():
    d = 24
    X = dg.dist_u(0x7B0, 300, d)
    a = IVFFlatIndex.build_index(1, 1, 3, X, init_indices=np.zeros(1, np.uint64))
    b = IVFFlatIndex.build_index(1, 1, 3, X, init_indices=np.zeros(1, np.uint64))
    rows = dg.dist_u(0x7B1, 20, d)
    rows[4, 2] = np.nan   # k == 1: nothing is compared, the row is accepted (as vers_ivf_add accepts it)
    cl, vids = a.add_batch(rows)
    grow_twin(b, rows)
    assert np.array_equal(cl, np.zeros(20, np.uint64)) and len(vids) == 20
    same_state(a, b)
    # n == 0: a no-op
    info = a.info()
    cl, vids = a.add_batch(np.zeros((0, d), np.float32))
    assert len(cl) == 0 and a.info() == info
    # k == 0: VERS_ERR_EMPTY, nothing added
    e0 = IVFFlatIndex(d)
    with pytest.raises(capi.VersError) as e:
        e0.add_batch(rows[:3])
    assert e.value.status == capi.ERR_EMPTY and e0.info()[0] == 0
    for ix in (a, b, e0):
        ix.close()


def test_dev_call_with_nan_padding_equals_host_call():
    import torch
    d, k, n = 300, 20, 700
    ld = d + 20
    a, b = pair(2500, d, k, metric=capi.METRIC_COSDIST, seed=0xDE0)
    rows = dg.dist_c(0xDE1, n, d, 2 * k, dg.default_sigma(d), seed_c=0xDE0)
    padded = np.full((n, ld), np.nan, np.float32)
    padded[:, :d] = rows
    Xd = torch.from_numpy(padded).cuda()
    out = torch.zeros(n, dtype=torch.int64, device="cuda")
    first, added = a.add_batch_dev(Xd.data_ptr(), n, ld, out.data_ptr())
    assert (first, added) == (2500, n)
    cl_dev = out.cpu().numpy().astype(np.uint64)
    a.assignments = np.concatenate([a.assignments, cl_dev]); a.values = np.concatenate([a.values, rows])
    for j, c in enumerate(cl_dev.tolist()):
        a.ids[c].append(2500 + j)
    cl, _ = b.add_batch(rows)
    assert np.array_equal(cl_dev, cl)
    same_state(a, b)
    same_search(a, b, dg.dist_c(0xDE2, 34, d, 2 * k, dg.default_sigma(d), seed_c=0xDE0), nprobes=(0, 2, k), top_ks=(10, 64))
    # NaN in the row itself (not the padding) stops the device call too
    bad = padded[:10].copy(); bad[6, 5] = np.nan
    Bd = torch.from_numpy(bad).cuda()
    first = C.c_uint64(0); added = C.c_uint64(0)
    rc = capi.lib().vers_ivf_add_batch_dev(a._h, capi._vp(Bd.data_ptr()), 10, ld, None, C.byref(first), C.byref(added))
    assert rc == capi.ERR_NAN and added.value == 6


@pytest.mark.parametrize("opt", [("memory", 1, 0), ("shadow", 0, 1)])
def test_layout_options(opt):
    name, value, default = opt
    d, k = 96, 16
    rows = dg.dist_c(0x0B1, 400, d, 2 * k, dg.default_sigma(d), seed_c=0x0B0)
    ref, _ = pair(2000, d, k, seed=0x0B0)
    ref.add_batch(rows)
    capi.set_option(name, value)
    try:
        a, b = pair(2000, d, k, seed=0x0B0)
        if name == "memory":
            assert a.layout_bytes()["rowmajor"] == 0
        else:
            assert not a.shadow_state()["active"]
        a.add_batch(rows)
        grow_twin(b, rows)
        same_state(a, b)
        same_state(a, ref)   # same bits as with the default layout
        same_search(a, b, dg.dist_c(0x0B2, 33, d, 2 * k, dg.default_sigma(d), seed_c=0x0B0), nprobes=(0, 4), top_ks=(10,))
        same_search(a, ref, dg.dist_c(0x0B2, 33, d, 2 * k, dg.default_sigma(d), seed_c=0x0B0), nprobes=(0, 4), top_ks=(10,))
    finally:
        capi.set_option(name, default)


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_batch(world):
    import torch
    n, d, k = 3000, 40, 24
    X = dg.dist_c(0x5B1, n, d, 30, dg.default_sigma(d))
    init = mg.init_draws(0x5B2, 1, k, n)
    whole = IVFFlatIndex.build_index(k, 1, 4, X, init_indices=init)
    shards = []
    for r in range(world):
        ix = IVFFlatIndex(d)
        ix.set_shard(r, world)
        cent = np.zeros((k, d), np.float32); asg = np.zeros(n, np.uint64)
        cost = C.c_float(0); kept = C.c_int32(0)
        capi.check(capi.lib().vers_ivf_build(ix._h, capi._ptr(X), n, 4 * d, k, 1, 4, capi._ptr(init), capi._ptr(cent), 4 * d,
                                             capi._ptr(asg), C.byref(cost), C.byref(kept), None))
        ix.num_centroids, ix.centroids, ix.assignments = k, cent, asg
        ix.values = X.copy(); ix.ids = [list(np.nonzero(asg == c)[0]) for c in range(k)]
        shards.append(ix)
    owners = shards[0].owners()
    big = int(np.argmax(whole.list_lengths()))
    rows = np.concatenate([dg.dist_c(0x5B3, 500, d, 30, dg.default_sigma(d), seed_c=0x5B1),
                           (whole.centroids[big][None, :] + np.random.default_rng(3).normal(0, 1e-3, (400, d))).astype(np.float32)])
    tc, tv = grow_twin(whole, rows)
    for ix in shards:   # every rank adds the same rows: same clusters and vec ids, only the owner stores a list's rows
        cl, vids = ix.add_batch(rows)
        assert np.array_equal(cl, tc) and np.array_equal(vids, tv)
        assert ix.info()[0] == whole.info()[0] and np.array_equal(ix.list_lengths(), whole.list_lengths())
    stored = 0
    for r, ix in enumerate(shards):
        for c in range(k):
            if owners[c] == r:
                ri, ii = ix.get_list(c)
                wr, wi = whole.get_list(c)
                assert np.array_equal(ii, wi) and np.array_equal(bits(ri), bits(wr)), (r, c)
                stored += len(ii)
            else:
                with pytest.raises(capi.VersError):
                    ix.get_list(c)
        assert ix.layout_bytes()["rows"] < whole.layout_bytes()["rows"]
    assert stored == whole.info()[0]
    b = 37
    Q = dg.dist_c(0x5B4, b, d, 30, dg.default_sigma(d), seed_c=0x5B1); Q[3] = rows[510]
    Qd = torch.from_numpy(Q).cuda()
    for nprobe, top_k in [(0, 10), (0, 64), (5, 10), (24, 33), (1, 1)]:
        keys = torch.empty(world, b, top_k, dtype=torch.int64, device="cuda")
        ids = torch.empty(world, b, top_k, dtype=torch.int64, device="cuda")
        for r, ix in enumerate(shards):
            ix.search_partial_dev(Qd.data_ptr(), d, b, top_k, nprobe, keys[r].data_ptr(), ids[r].data_ptr())
            ix.poll()
        oi = torch.zeros(b, top_k, dtype=torch.int64, device="cuda")
        od = torch.zeros(b, top_k, dtype=torch.float32, device="cuda")
        oc = torch.zeros(b, dtype=torch.int32, device="cuda")
        IVFFlatIndex.merge_partials_dev(keys.data_ptr(), ids.data_ptr(), b * top_k, world, b, top_k, nprobe, oi.data_ptr(), od.data_ptr(),
                                        oc.data_ptr())
        torch.cuda.synchronize()
        wi, wd, wc = whole.search_batch(Q, top_k, nprobe)
        gi, gd, gc = oi.cpu().numpy().astype(np.uint64), od.cpu().numpy(), oc.cpu().numpy()
        assert np.array_equal(gc, wc)
        for q in range(b):
            c = int(wc[q])
            assert np.array_equal(gi[q, :c], wi[q, :c]) and np.array_equal(bits(gd[q, :c]), bits(wd[q, :c])), (nprobe, top_k, q)
    for ix in shards + [whole]:
        ix.close()


def test_python_mirror_save_load(tmp_path):
    d, k = 48, 10
    a, b = pair(900, d, k, seed=0x5A0)
    rows = dg.dist_c(0x5A1, 250, d, 2 * k, dg.default_sigma(d), seed_c=0x5A0)
    a.add_batch(rows[:100]); a.add(rows[100]); a.add_batch(rows[101:])
    grow_twin(b, rows)
    pa, pb = str(tmp_path / "a.idx"), str(tmp_path / "b.idx")
    a.save_index(pa); b.save_index(pb)
    assert open(pa, "rb").read() == open(pb, "rb").read()
    la = IVFFlatIndex.load_index(pa, d)
    same_state(la, b)
    same_search(la, a, dg.dist_c(0x5A2, 32, d, 2 * k, dg.default_sigma(d), seed_c=0x5A0), nprobes=(0, 3), top_ks=(10,))


def test_cpp_host_mirror_add_batch(tmp_path):
    """vers_amd/host/ivfflat.hpp's add_batch from compiled code: the same fields as add called row by row."""
    src = tmp_path / "add_batch_demo.cpp"
    src.write_text(r'''
#include <cstdio>
#include "%s"
int main() {
  constexpr size_t N = 40;
  std::vector<vers::Vector<N>> X(600), extra(150);
  for (size_t i = 0; i < X.size(); ++i) for (size_t j = 0; j < N; ++j) X[i].v[j] = (float)((i * 7 + j * 13) %% 31) * 0.25f + (float)(i %% 5);
  for (size_t i = 0; i < extra.size(); ++i) for (size_t j = 0; j < N; ++j) extra[i].v[j] = (float)((i * 11 + j * 3) %% 17) * 0.5f;
  std::vector<uint64_t> init = {3, 90, 200, 333, 480, 599};
  auto a = vers::IVFFlatIndex<N>::build_index(6, 1, 5, X, &init);
  auto b = vers::IVFFlatIndex<N>::build_index(6, 1, 5, X, &init);
  a.add_batch(extra);
  for (size_t i = 0; i < extra.size(); ++i) b.add(extra[i], 0);
  if (a.assignments != b.assignments || a.ids != b.ids || a.values.size() != b.values.size()) { std::puts("DIFFER"); return 1; }
  std::puts("SAME");
  return 0;
}
''' % os.path.join(ROOT, "vers_amd", "host", "ivfflat.hpp"))
    lib = vbuild.build()
    exe = str(tmp_path / "add_batch_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-o", exe, str(src), "-L" + os.path.dirname(lib), "-lvers_hip",
                           "-Wl,-rpath," + os.path.dirname(lib)])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "SAME" in out.stdout, out.stdout + out.stderr
