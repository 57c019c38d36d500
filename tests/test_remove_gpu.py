"""vers_ivf_remove_batch / vers_ivf_remove_batch_dev: removing vec id v is ids[assignments[v]].retain(|&x| x != v) on the reference's
fields and nothing else.  Every case keeps the host mirror (IVFFlatIndex.ids shortened by hand or by the mirror's own remove_batch) and
compares bit for bit, with no tolerance: info(), live_count(), list_lengths(), every list's stored rows and ids, and searches -- batches
of >= 32 queries (matrix-core scan on the shadow), single queries, exhaustive search -- against the oracle called with the shortened
lists."""
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


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def make(n, d, k, metric=capi.METRIC_L2SQ, seed=0x4E30, iters=4):
    X = dg.dist_c(seed, n, d, 2 * k, dg.default_sigma(d))
    init = mg.init_draws(seed + 1, 1, k, n)
    return IVFFlatIndex.build_index(k, 1, iters, X, init_indices=init, metric=metric)


def queries(ix, seed, b=40):
    d, k = ix.d, ix.num_centroids
    return dg.dist_c(seed, b, d, 2 * k, dg.default_sigma(d))


def live_ids(ix):
    return np.sort(np.concatenate([np.asarray(l, dtype=np.int64) for l in ix.ids] + [np.zeros(0, np.int64)]))


def check_state(ix):
    n, k, longest = ix.info()
    lens = [len(l) for l in ix.ids]
    assert n == len(ix.assignments) == ix.values.shape[0]
    assert k == ix.num_centroids
    assert longest == (max(lens) if lens else 0)
    assert ix.live_count() == sum(lens)
    assert np.array_equal(ix.list_lengths(), np.asarray(lens, dtype=np.uint64))
    for c in range(k):
        rows, ids = ix.get_list(c)
        assert np.array_equal(ids, np.asarray(ix.ids[c], dtype=np.uint64)), c
        assert np.array_equal(bits(rows), bits(ix.values[ids.astype(np.int64)])), c


def expect(ix, q, top_k, nprobe):
    if nprobe == 0:
        return co.search_approximate(ix.values, ix.centroids, ix.ids, q, top_k, ix.metric)
    return co.search_nprobe(ix.values, ix.centroids, ix.ids, q, top_k, nprobe, ix.metric)


def check_search(ix, Q, nprobes=None, top_ks=(1, 10, 64, 200), exhaustive=True):
    k = ix.num_centroids
    live = live_ids(ix)
    for nprobe in nprobes if nprobes is not None else (0, 1, 5, k):
        for top_k in top_ks:
            if nprobe == 0 and top_k > live.size:
                continue
            want = [expect(ix, Q[q], top_k, nprobe) for q in range(Q.shape[0])]
            ib, db, cb = ix.search_batch(Q, top_k, nprobe)   # a batch: the matrix-core scan on the shadow
            for q in range(Q.shape[0]):
                oi, od = want[q]
                assert cb[q] == len(oi), (nprobe, top_k, q, cb[q], len(oi))
                assert np.array_equal(ib[q, :len(oi)], oi) and np.array_equal(bits(db[q, :len(oi)]), bits(od)), (nprobe, top_k, q)
            for q in (0, Q.shape[0] - 1):   # single queries
                i1, d1, c1 = ix.search_batch(Q[q], top_k, nprobe)
                oi, od = want[q]
                assert c1[0] == len(oi), (nprobe, top_k, q)
                assert np.array_equal(i1[0, :len(oi)], oi) and np.array_equal(bits(d1[0, :len(oi)]), bits(od)), (nprobe, top_k, q)
    if exhaustive:
        for top_k in top_ks:
            ie, de, ce = ix.search_exhaustive(Q, top_k, ix.metric)
            for q in range(0, Q.shape[0], 7):
                if live.size == 0:
                    assert ce[q] == 0
                    continue
                oi, od = co.search_exhaustive(ix.values[live], Q[q], top_k, ix.metric)
                assert ce[q] == min(top_k, live.size) == len(oi), (top_k, q)
                assert np.array_equal(ie[q, :len(oi)], live[oi.astype(np.int64)].astype(np.uint64)), (top_k, q)
                assert np.array_equal(bits(de[q, :len(oi)]), bits(od)), (top_k, q)


def check(ix, Q, **kw):
    check_state(ix)
    check_search(ix, Q, **kw)


@pytest.mark.parametrize("metric", [capi.METRIC_L2SQ, capi.METRIC_COSDIST])
@pytest.mark.parametrize("d", [16, 300, 768])
def test_scattered_descending_repeated_and_twice(metric, d):
    n, k = 2000, 24
    ix = make(n, d, k, metric, seed=0x4E30 + d)
    Q = queries(ix, 0x4E37 + d)
    assert ix.remove_batch(np.arange(3, n, 17)) == len(range(3, n, 17))            # scattered
    check(ix, Q)
    desc = np.arange(n - 1, 0, -13)
    assert ix.remove_batch(np.concatenate([desc, desc[:40]])) > 0                  # descending, with repeats
    rng = np.random.default_rng(d)
    rnd = rng.integers(0, n, 300)
    ix.remove_batch(np.concatenate([rnd, rnd[::-1][:100]]))                        # random order, repeats, some already gone
    check(ix, Q)
    assert ix.remove_batch(rnd[:50]) == 0                                          # removed twice across calls: nothing left to remove
    assert ix.info()[0] == n
    check_state(ix)
    ix.close()


def test_tile_from_the_middle_first_last_whole_list_and_nearly_everything():
    n, d, k = 2600, 64, 12
    ix = make(n, d, k, seed=0x7110)
    Q = queries(ix, 0x7117)
    lens = [len(l) for l in ix.ids]
    c = int(np.argmax(lens))
    assert lens[c] >= 192
    mid = list(ix.ids[c][64:128])                          # a whole tile's worth from the middle of a list
    assert ix.remove_batch(mid) == 64
    check(ix, Q, top_ks=(10, 64))
    assert ix.remove_batch([ix.ids[c][0]]) == 1            # the first row
    assert ix.remove_batch([ix.ids[c][-1]]) == 1           # the last row
    other = int(np.argsort(lens)[k // 2])
    assert ix.remove_batch([ix.ids[other][-1], ix.ids[other][0]]) == 2
    check(ix, Q, top_ks=(1, 10))
    assert ix.remove_batch(list(ix.ids[c])) == lens[c] - 66   # all rows of a list: empty, skipped by every mode
    assert ix.ids[c] == [] and ix.list_lengths()[c] == 0
    check(ix, Q)
    keep = set(ix.ids[other][:3]) | set(ix.ids[(other + 1) % k][-2:])
    keep -= set(ix.ids[c])
    ix.remove_batch([v for v in range(n) if v not in keep])   # all rows of all lists but a few
    assert ix.live_count() == len(keep) <= 5
    check(ix, Q)
    for qs in (Q, Q[:1]):                                  # reference mode above the live count: the reference's panic
        with pytest.raises(capi.VersError) as e:
            ix.search_batch(qs, len(keep) + 1, 0)
        assert e.value.status == capi.ERR_INSUFFICIENT
    ix.remove_batch(sorted(keep))
    assert ix.live_count() == 0 and ix.info() == (n, k, 0)
    check_state(ix)
    ib, db, cb = ix.search_batch(Q, 5, 3)
    assert not cb.any()
    ix.close()


def test_reference_mode_batch_spills_after_a_list_is_cut_below_top_k():
    """A reference-mode batch is served as nprobe = 1 while no list is shorter than top_k (vers_ivf::len_asc_prefix): after the cut
    the queries whose nearest list is the short one must spill into the next list."""
    n, d, k, top_k = 2400, 48, 24, 10
    ix = make(n, d, k, seed=0x5B10)
    assert min(len(l) for l in ix.ids) >= top_k
    c = int(np.argmax([len(l) for l in ix.ids]))
    rng = np.random.default_rng(11)
    near = (ix.centroids[c][None, :] + rng.normal(0, 1e-3, (12, d))).astype(np.float32)
    Q = np.concatenate([near, queries(ix, 0x5B17, 28)])
    check_search(ix, Q, nprobes=(0,), top_ks=(top_k,), exhaustive=False)
    ix.remove_batch(ix.ids[c][3:])
    assert len(ix.ids[c]) == 3
    got = ix.search_batch(Q, top_k, 0)
    assert (got[2] == top_k).all()
    assert set(got[0][0, :3].tolist()) == set(ix.ids[c])    # the nearest list's three rows, then the spill
    check(ix, Q, nprobes=(0, 1), top_ks=(1, top_k, 64))
    ix.close()


def test_reference_mode_dev_call_ranks_as_deep_as_the_shortened_lists_need():
    """A reference-mode _dev call cannot retry: it ranks up front as many lists as the list LENGTHS can make the walk need.  With the
    60 lists nearest to a query emptied, the walk passes more than the 48 lists ranked by default."""
    import torch
    n, d, k, top_k = 3000, 32, 80, 10
    ix = make(n, d, k, seed=0xDE50, iters=3)
    Q = queries(ix, 0xDE57, 36)
    order = np.argsort(((ix.centroids.astype(np.float64) - Q[0].astype(np.float64)) ** 2).sum(1), kind="stable")
    gone = [v for c in order[:60] for v in ix.ids[int(c)]]
    ids_d = torch.from_numpy(np.asarray(gone, dtype=np.int64)).cuda()
    assert ix.remove_batch_dev(ids_d.data_ptr(), len(gone)) == len(gone)   # the device-pointer entry, unsharded: comm = None
    for c in order[:60]:
        ix.ids[int(c)] = []
    assert ix.live_count() == n - len(gone) >= top_k
    check_state(ix)
    Qd = torch.from_numpy(Q).cuda()
    for qs, b in ((Qd, Q.shape[0]), (Qd[:1], 1)):
        oi = torch.zeros(b, top_k, dtype=torch.int64, device="cuda")
        od = torch.zeros(b, top_k, dtype=torch.float32, device="cuda")
        oc = torch.zeros(b, dtype=torch.int32, device="cuda")
        ix.search_dev(qs.data_ptr(), d, b, top_k, 0, oi.data_ptr(), od.data_ptr(), oc.data_ptr())
        ix.poll()
        gi, gd, gc = oi.cpu().numpy().astype(np.uint64), od.cpu().numpy(), oc.cpu().numpy()
        for q in range(b):
            wi, wd = expect(ix, Q[q], top_k, 0)
            assert gc[q] == len(wi) == top_k
            assert np.array_equal(gi[q], wi) and np.array_equal(bits(gd[q]), bits(wd)), q
    check_search(ix, Q, nprobes=(0, 70), top_ks=(top_k,))
    ix.close()


def test_remove_add_remove_reuses_the_freed_slack():
    n, d, k = 2000, 96, 24
    ix = make(n, d, k, seed=0xAD10)
    Q = queries(ix, 0xAD17)
    rows_bytes = ix.layout_bytes()["rows"]
    rng = np.random.default_rng(3)
    first = rng.choice(n, 500, replace=False)
    assert ix.remove_batch(first) == 500
    check(ix, Q, top_ks=(10, 64))
    # no more rows per list than it lost: they fit the freed slack, nothing is re-laid out
    back = ix.values[first[:300]] + np.float32(1e-3)
    relayouts = capi.add_batch_phases()["relayouts"]
    cl, vids = ix.add_batch(back[:200])
    assert np.array_equal(vids, np.arange(n, n + 200, dtype=np.uint64))   # vec ids continue from n, never reused
    for x in back[200:220]:
        c, v = ix.add(x)
        assert ix.ids[c][-1] == v == len(ix.assignments) - 1
    assert ix.layout_bytes()["rows"] == rows_bytes and capi.add_batch_phases()["relayouts"] == relayouts
    check(ix, Q, top_ks=(10, 64))
    assert ix.remove_batch(np.concatenate([vids[::2].astype(np.int64), first[:10], np.arange(0, n, 9)])) > 100   # new rows, gone rows, old rows
    check(ix, Q)
    ix.add_batch(back[220:])
    assert ix.info()[0] == n + 300
    check(ix, Q, top_ks=(10,))
    ix.close()


def test_removal_after_a_relayout():
    d, k = 64, 12
    ix = make(1200, d, k, seed=0x4E10)
    sizes = ix.list_lengths()
    c = int(np.argmax(sizes))
    rng = np.random.default_rng(5)
    around = (ix.centroids[c][None, :] + rng.normal(0, 1e-3, (2 * int(sizes[c]) + 70, d))).astype(np.float32)
    lb0 = ix.layout_bytes()["rows"]
    ix.add_batch(around)
    assert ix.layout_bytes()["rows"] > lb0   # every list moved: the tile -> list table of the build is stale
    Q = queries(ix, 0x4E17)
    victims = np.concatenate([np.asarray(ix.ids[c][10::3]), np.arange(5, 1200, 11)])
    ix.remove_batch(victims)
    check(ix, Q, top_ks=(10, 64))
    last = max(range(k), key=lambda j: (len(ix.ids[j]) > 0, j))
    ix.remove_batch(ix.ids[last][:1] + ix.ids[0][-1:])
    check(ix, Q, top_ks=(10,))
    ix.close()


def test_invalid_id_removes_nothing_empty_call_and_index_without_centroids():
    n, d, k = 1500, 40, 16
    ix = make(n, d, k, seed=0x1A10)
    Q = queries(ix, 0x1A17, 33)
    ix.remove_batch([7, 8, 9])
    before = [list(l) for l in ix.ids]
    for bad in (n, n + 5, 2 ** 40):
        with pytest.raises(capi.VersError) as e:
            ix.remove_batch([1, 2, bad, 3])
        assert e.value.status == capi.ERR_INVALID
        assert ix.ids == before
    check(ix, Q, top_ks=(10,))
    assert ix.remove_batch([]) == 0 and ix.remove_batch(np.zeros(0, np.uint64)) == 0
    removed = C.c_uint64(77)
    assert capi.lib().vers_ivf_remove_batch(ix._h, None, 0, C.byref(removed)) == 0 and removed.value == 0
    check_state(ix)
    ix.add(ix.values[1])   # n grows: the id n is valid now
    assert ix.remove_batch([n]) == 1
    check_state(ix)
    # no centroids: nothing can be listed; an empty call is a no-op, any id is out of range
    e0 = IVFFlatIndex(d)
    assert e0.remove_batch([]) == 0 and e0.live_count() == 0
    with pytest.raises(capi.VersError) as e:
        e0.remove_batch([0])
    assert e.value.status == capi.ERR_INVALID
    nothing = IVFFlatIndex.build_index(4, 0, 3, ix.values[:50], init_indices=np.zeros(0, np.uint64))   # no attempt: empty assignments
    assert nothing.remove_batch([]) == 0
    with pytest.raises(capi.VersError):
        nothing.remove_batch([0])
    # a streamed upload in progress: the handle holds no index yet, as for add
    up = IVFFlatIndex(d)
    up.upload_begin(ix.centroids, np.bincount(ix.assignments.astype(np.int64), minlength=k), len(ix.assignments))
    with pytest.raises(capi.VersError) as e:
        up.remove_batch([0])
    assert e.value.status == capi.ERR_EMPTY
    for j in (ix, e0, nothing, up):
        j.close()


@pytest.mark.parametrize("opt", [("memory", 1, 0), ("shadow", 0, 1), ("prescan", 2, 1), ("coarse", 2, 0), ("remove_batch_ids", 7, 1 << 20)])
def test_layouts_forced_exact_paths_and_chunked_ids(opt):
    name, value, default = opt
    n, d, k = 2000, 96, 24
    capi.set_option(name, value)
    try:
        ix = make(n, d, k, seed=0x0B10)
        if name == "memory":
            assert ix.layout_bytes()["rowmajor"] == 0
        if name == "shadow":
            assert not ix.shadow_state()["active"]
        Q = queries(ix, 0x0B17)
        rng = np.random.default_rng(8)
        capi.remove_phases(reset=True)
        gone = rng.choice(n, 333, replace=False)
        assert ix.remove_batch(gone) == 333
        ph = capi.remove_phases()
        assert ph["calls"] == 1 and ph["ids"] == 333 and ph["removed"] == 333
        check(ix, Q, top_ks=(1, 10, 64))
        ix.add_batch(ix.values[gone[:50]])
        ix.remove_batch(ix.ids[3][::2])
        check(ix, Q, top_ks=(10, 200))
        ix.close()
    finally:
        capi.set_option(name, default)


def test_save_load_keeps_removed_vectors_out(tmp_path):
    d, k, n = 48, 10, 900
    ix = make(n, d, k, seed=0x5A10)
    ix.remove_batch(np.arange(1, n, 6))
    ix.add_batch(ix.values[:40] * np.float32(1.01))
    ix.remove_batch([n + 3, n + 4, 0])
    path = str(tmp_path / "removed.idx")
    ix.save_index(path)
    back = IVFFlatIndex.load_index(path, d)
    assert back.ids == ix.ids and back.info() == ix.info() and back.live_count() == ix.live_count()
    Q = queries(ix, 0x5A17, 32)
    check(back, Q, top_ks=(10, 64))
    for nprobe in (0, 3):
        a, b = ix.search_batch(Q, 10, nprobe), back.search_batch(Q, 10, nprobe)
        assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1])) and np.array_equal(a[2], b[2])
    # a file without removals (what the reference writes) loads as before
    whole = make(300, d, 4, seed=0x5A20)
    p2 = str(tmp_path / "whole.idx")
    whole.save_index(p2)
    w2 = IVFFlatIndex.load_index(p2, d)
    assert w2.live_count() == 300
    check_state(w2)
    for j in (ix, back, whole, w2):
        j.close()


def test_k4096_many_short_lists():
    d, k, n = 64, 4096, 20000
    X = dg.dist_c(0x4F0, n, d, k, dg.default_sigma(d))
    ix = IVFFlatIndex.build_index(k, 1, 2, X, init_indices=mg.init_draws(0x4F1, 1, k, n))
    rng = np.random.default_rng(12)
    gone = rng.choice(n, 6000, replace=False)
    assert ix.remove_batch(gone) == 6000
    Q = dg.dist_c(0x4F2, 40, d, k, dg.default_sigma(d), seed_c=0x4F0)
    check_state(ix)
    check_search(ix, Q, nprobes=(0, 1, 8), top_ks=(1, 10))
    ix.close()


def test_cpp_host_mirror_remove_batch(tmp_path):
    """vers_amd/host/ivfflat.hpp's remove_batch and load_index from compiled code."""
    src = tmp_path / "remove_batch_demo.cpp"
    src.write_text(r'''
#include <cstdio>
#include "%s"
int main(int argc, char** argv) {
  constexpr size_t N = 40;
  std::vector<vers::Vector<N>> X(600), extra(50);
  for (size_t i = 0; i < X.size(); ++i) for (size_t j = 0; j < N; ++j) X[i].v[j] = (float)((i * 7 + j * 13) %% 31) * 0.25f + (float)(i %% 5);
  for (size_t i = 0; i < extra.size(); ++i) for (size_t j = 0; j < N; ++j) extra[i].v[j] = (float)((i * 11 + j * 3) %% 17) * 0.5f;
  std::vector<uint64_t> init = {3, 90, 200, 333, 480, 599};
  auto a = vers::IVFFlatIndex<N>::build_index(6, 1, 5, X, &init);
  std::vector<size_t> gone;
  for (size_t v = 2; v < 600; v += 5) gone.push_back(v);
  gone.push_back(7); gone.push_back(7);
  const size_t expect = gone.size() - (7 %% 5 == 2 ? 2 : 1);
  if (a.remove_batch(gone) != expect) { std::puts("COUNT"); return 1; }
  if (a.live_count() != 600 - expect || a.assignments.size() != 600 || a.values.size() != 600) { std::puts("FIELDS"); return 1; }
  size_t listed = 0;
  for (auto& l : a.ids) { listed += l.size(); for (size_t x : l) if (x %% 5 == 2 || x == 7) { std::puts("STILL LISTED"); return 1; } }
  if (listed != a.live_count()) { std::puts("LISTED"); return 1; }
  a.add_batch(extra);
  if (a.ids[a.assignments[600]].back() < 600) { std::puts("ADD"); return 1; }
  bool threw = false;
  try { a.remove_batch({1, 650}); } catch (const vers::Panic& p) { threw = p.status == VERS_ERR_INVALID; }
  if (!threw || a.live_count() != 650 - expect) { std::puts("INVALID"); return 1; }
  a.save_index(argv[1]);
  auto b = vers::IVFFlatIndex<N>::load_index(argv[1]);
  if (b.live_count() != a.live_count() || b.ids != a.ids) { std::puts("LOAD"); return 1; }
  for (size_t q = 0; q < 20; ++q) {
    auto ra = a.search_approximate(X[q * 29], 10), rb = b.search_approximate(X[q * 29], 10);
    if (ra != rb) { std::puts("SEARCH"); return 1; }
    for (auto& p : ra) if (p.first < 600 && (p.first %% 5 == 2 || p.first == 7)) { std::puts("REMOVED ROW FOUND"); return 1; }
  }
  std::puts("SAME");
  return 0;
}
''' % os.path.join(ROOT, "vers_amd", "host", "ivfflat.hpp"))
    lib = capi.LIB_PATH   # the library these tests run against
    exe = str(tmp_path / "remove_batch_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-o", exe, str(src), "-L" + os.path.dirname(lib), "-lvers_hip",
                           "-Wl,-rpath," + os.path.dirname(lib)])
    out = subprocess.run([exe, str(tmp_path / "cpp.idx")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "SAME" in out.stdout, out.stdout + out.stderr
