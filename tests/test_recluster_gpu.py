"""vers_ivf_recluster: build_index over the rows that are in some list, taken in ascending vec id (L), with the vec ids kept.  Every index
goes through a scattered removal (id 0 and the last id included), the removal of a whole list, an add_batch of 65 rows and an update_batch
with movers before the call, and through NO compact: freed slack lies inside the lists.  Compared bit for bit, with no tolerance:
  1. the call's outputs with oracle.build_index(values[L], k', 2 attempts, ...) for k' = k, 1, 2 k, k / 2 and a k' above m;
  2. the handle with the IVFFlatIndex mirror (check_state / check_search of tests/test_remove_gpu.py), n, the live count, the next vec id;
  3. every search family, every list and the storage size with a TWIN: upload(values, centroids', assignments') + remove_batch(dead ids);
  4. a filter prepared before the call with the per-call filtered search at its first use afterwards;
  5. every mutator, a second recluster and save_index -> load_index afterwards;
  6. the refusals (the index unchanged, the outputs untouched), 7. the options, 8. the phase counters."""
import ctypes as C

import numpy as np
import pytest

from oracle import c_oracle as co
from tests import datagen as dg
from tests import mutation_model as mm
from tests.golden import make_golden as mg
from tests.test_remove_gpu import bits, check_search, check_state, live_ids
from vers_amd import capi
from vers_amd.index import IVFFlatIndex

pytestmark = pytest.mark.gpu

# mutation_model.SHAPES: one column | empty lists, every list inside one tile | lists one row past a tile | ld 192 | ld 320 | k above rows per tile
SHAPES = ["n50_d1_k3", "n200_d7_k40", "n333_d33_k5", "n1500_d130_k10", "n900_d300_k30", "n2500_d20_k300"]
METRICS = ["l2", "cos"]
ATTEMPTS, ITERS = 2, 3


def build(case_id):
    case = mm.CASES[case_id]
    X, init, ob, _ = mm.base(case)
    ix = IVFFlatIndex.build_index(case.k, 1, case.iters, X, init_indices=init, metric=case.metric)
    assert np.array_equal(ix.assignments, ob["assignments"])
    return case, ix


def mutate(case, ix):
    """scattered removal with id 0 and id n - 1 | one whole list | add_batch of 65 rows | update_batch with movers | NO compact"""
    n = case.n
    rng = np.random.default_rng(case.seed)
    gone = sorted(set(range(0, n, 7)) | {0, n - 1})
    assert ix.remove_batch(gone) == len(gone)
    lens = [len(l) for l in ix.ids]
    nonempty = sorted((c for c in range(len(lens)) if lens[c]), key=lambda c: lens[c])
    whole = nonempty[len(nonempty) // 2]
    assert ix.remove_batch(list(ix.ids[whole])) == lens[whole] and ix.ids[whole] == []
    rows = (ix.values[rng.integers(0, n, 65)] * np.float32(1.01)).astype(np.float32)
    _, vids = ix.add_batch(rows)
    assert vids.tolist() == list(range(n, n + 65))
    live = live_ids(ix)
    pick = rng.choice(live, min(40, live.size), replace=False)
    _, st = ix.update_batch(pick, movers_rows(ix, pick, live))
    if sum(1 for l in ix.ids if l) > 1:
        assert (st == 1).any(), "no mover"
    return live_ids(ix)


def movers_rows(ix, pick, live):
    """every second picked id gets the vector of a live row of ANOTHER list (that row's own cluster is its first minimum: the id moves), the
    others a vector of their own list"""
    rows = ix.values[pick].copy()
    for i, v in enumerate(pick.tolist()):
        other = live[ix.assignments[live] != ix.assignments[v]]
        if i % 2 == 0 and other.size:
            rows[i] = ix.values[other[(i * 31) % other.size]]
    return rows


def draws(seed, attempts, kp, m):
    return mg.init_draws(seed, attempts, kp, m)


def the_queries(case):
    return mm.fixed_queries(case)


def recluster_and_compare(ix, kp, seed, attempts=ATTEMPTS):
    """one call through the mirror, its outputs against the oracle on values[L] -> the oracle's build"""
    L = live_ids(ix)
    n, m = len(ix.assignments), L.size
    init = draws(seed, attempts, kp, m)
    want = co.build_index(ix.values[L], kp, attempts, ITERS, init, metric=ix.metric)
    cost, kept, iters = ix.recluster(kp, attempts, ITERS, init_indices=init)
    assert kept == int(want["kept"]) == 1, (kp, kept)
    assert bits(cost) == bits(want["cost"]), (kp, cost, want["cost"])
    assert np.array_equal(bits(ix.centroids), bits(want["centroids"])), kp
    assert np.array_equal(ix.assignments[L], want["assignments"]), kp
    dead = np.ones(n, dtype=bool); dead[L] = False
    assert not ix.assignments[dead].any()
    for a in range(attempts):    # the iteration count of every attempt: build_kmeans on that attempt's draws
        assert int(iters[a]) == co.build_kmeans(ix.values[L], kp, ITERS, np.asarray(init).reshape(attempts, kp)[a], ix.metric)[2], (kp, a)
    assert np.array_equal(bits(ix.get_centroids()), bits(want["centroids"]))
    assert ix.num_centroids == kp and len(ix.ids) == kp
    assert np.array_equal(live_ids(ix), L) and ix.info()[0] == n and ix.live_count() == m
    return want


def twin_of(ix):
    t = IVFFlatIndex(ix.d, metric=ix.metric)
    t.num_centroids, t.values, t.centroids, t.assignments = ix.num_centroids, ix.values.copy(), ix.centroids.copy(), ix.assignments.copy()
    t._upload()
    t.ids = [np.flatnonzero(t.assignments == c).tolist() for c in range(t.num_centroids)]
    live = np.zeros(len(ix.assignments), dtype=bool); live[live_ids(ix)] = True
    t.remove_batch(np.flatnonzero(~live))
    assert t.ids == ix.ids
    return t


def same_topk(a, b, what):
    assert np.array_equal(a[2], b[2]), what
    on = np.arange(a[0].shape[1])[None, :] < a[2][:, None]
    assert np.array_equal(a[0][on], b[0][on]) and np.array_equal(bits(a[1])[on], bits(b[1])[on]), what


def same_csr(a, b, what):
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(bits(a[2]), bits(b[2])), what


def compare_with_twin(case, ix, Q):
    t = twin_of(ix)
    kp, n = ix.num_centroids, len(ix.assignments)
    m = ix.live_count()
    rng = np.random.default_rng(case.seed ^ 0x7717)
    sem = rng.random(n) < 0.10
    three = [sem, rng.random(n) < 0.5, np.zeros(n, dtype=bool)]
    fo = (np.arange(Q.shape[0]) % 3).astype(np.uint32)
    for nprobe in sorted({1, min(5, kp), kp}):
        for top_k in sorted({1, min(10, m), min(64, m)}):
            same_topk(ix.search_batch(Q, top_k, nprobe), t.search_batch(Q, top_k, nprobe), ("search_batch", nprobe, top_k))
        same_topk(ix.search_filtered(Q, 10, nprobe, sem, n), t.search_filtered(Q, 10, nprobe, sem, n), ("search_filtered", nprobe))
        same_topk(ix.search_filtered_multi(Q, 10, nprobe, three, fo, n), t.search_filtered_multi(Q, 10, nprobe, three, fo, n), ("search_filtered_multi", nprobe))
        ref = ix.search_batch(Q, min(10, m), nprobe)
        r = np.where(ref[2] > 0, ref[1][np.arange(Q.shape[0]), np.maximum(ref[2].astype(np.int64) - 1, 0)], np.float32(-1)).astype(np.float32)
        r[::4] = np.inf
        for walk in (False, True):
            same_csr(ix.range_search(Q, r, nprobe, walk_order=walk), t.range_search(Q, r, nprobe, walk_order=walk), ("range_search", nprobe, walk))
            same_csr(ix.range_search_filtered(Q, r, nprobe, sem, n, walk_order=walk), t.range_search_filtered(Q, r, nprobe, sem, n, walk_order=walk),
                     ("range_search_filtered", nprobe, walk))
    same_topk(ix.search_batch(Q, 1, 0), t.search_batch(Q, 1, 0), ("search_batch", 0, 1))
    for c in range(kp):
        (ra, ia), (rb, ib) = ix.get_list(c), t.get_list(c)
        assert np.array_equal(ia, ib) and np.array_equal(bits(ra), bits(rb)), ("get_list", c)
    # Storage: the call leaves the plan of a fresh upload of the NEW lengths.  The twin's upload planned list 0 with the dead ids in it (their
    # assignments' is 0) and a removal gives no storage back, so the twin is compacted first -- which changes nothing observable -- and then
    # both hold the same plan: the rule of DESIGN.md section 2 summed over the lists.
    t.compact()
    assert ix.layout_bytes() == t.layout_bytes()
    assert ix.layout_bytes()["rows"] == sum(mm.capacity(len(l)) for l in ix.ids) * ((ix.d + 63) // 64 * 64) * 4
    t.close()


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("shape", SHAPES)
def test_oracle_state_and_twin(shape, metric):
    case, ix = build(f"{shape}_{metric}")
    L = mutate(case, ix)
    n, m, k = len(ix.assignments), L.size, case.k
    Q = the_queries(case)
    for i, kp in enumerate(dict.fromkeys([k, 1, 2 * k, max(1, k // 2)])):
        recluster_and_compare(ix, kp, case.seed + 17 * i)
        check_state(ix)
        check_search(ix, Q, nprobes=(0, 1, 5, kp))
        if i == 0 or kp == 2 * k:
            compare_with_twin(case, ix, Q)
    # the next add hands out id n, whatever was removed
    c, vid = ix.add(ix.values[int(L[1])])
    assert vid == n and ix.info()[0] == n + 1 and ix.live_count() == m + 1
    # a k' above m: down to three rows first
    live = live_ids(ix)
    ix.remove_batch(live[3:])
    kp = 7
    recluster_and_compare(ix, kp, case.seed + 99)
    assert sum(1 for l in ix.ids if l) <= 3
    check_state(ix)
    check_search(ix, Q, nprobes=(0, 1, 5, kp), top_ks=(1, 3, 10))
    ix.close()


def test_both_sides_of_the_matrix_core_threshold():
    """km_use_mfma: below n k d = 1e11 the exact scan assigns (every case above); option "assign" = 2 sends the same call through the matrix-core
    cascade, as tests/test_assign_mfma_gpu.py chooses its side.  Same bits, and the points are counted on the side that ran."""
    case, ix = build("n1500_d130_k10_l2")
    mutate(case, ix)
    m = ix.live_count()
    capi.assign_stats(reset=True)
    recluster_and_compare(ix, 12, 0xA551)
    assert capi.assign_stats(reset=True)[0] == 0
    try:
        capi.set_option("assign", 2)
        recluster_and_compare(ix, 12, 0xA551)
        pts, _ = capi.assign_stats(reset=True)
    finally:
        capi.set_option("assign", 0)
    assert pts >= m * ATTEMPTS * 2, (pts, m)
    check_state(ix)
    check_search(ix, the_queries(case), nprobes=(0, 5), top_ks=(10, 64))
    ix.close()


# ---- 4. a prepared filter lives through the call ---------------------------------------------------------------------------------------
def prepared_topk(ix, pf, Q, top_k, nprobe):
    import torch
    Q = np.ascontiguousarray(np.atleast_2d(Q), dtype=np.float32)
    b = Q.shape[0]
    Qd = torch.from_numpy(Q).cuda()
    ids = torch.zeros((b, top_k), dtype=torch.int64, device="cuda"); dist = torch.zeros((b, top_k), device="cuda")
    cnt = torch.zeros(b, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ix.search_prepared_dev(Qd.data_ptr(), ix.d, b, top_k, nprobe, pf, 0, ids.data_ptr(), dist.data_ptr(), cnt.data_ptr())
    torch.cuda.synchronize()
    ix.poll(0)
    return ids.cpu().numpy().view(np.uint64), dist.cpu().numpy(), cnt.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("kp_of", [lambda k: k, lambda k: 2 * k + 1], ids=["same_k", "other_k"])
def test_prepared_filter_rebuilds_in_full_at_its_first_use(kp_of, metric):
    case, ix = build(f"n1500_d130_k10_{metric}")
    mutate(case, ix)
    n = len(ix.assignments)
    Q = the_queries(case)
    sem = np.random.default_rng(0xF17).random(n + 500) < 0.3
    pf = ix.prepare_filter(capi.allowed_bitmap(sem, n + 500), n + 500)
    same_topk(prepared_topk(ix, pf, Q, 10, 5), ix.search_filtered(Q, 10, 5, sem, n + 500), "before")
    info0 = pf.info()
    kp = kp_of(case.k)
    recluster_and_compare(ix, kp, 0x9F1)
    same_topk(prepared_topk(ix, pf, Q, 10, 5), ix.search_filtered(Q, 10, 5, sem, n + 500), "first use after the call")
    info1 = pf.info()
    assert info1["builds"] == info0["builds"] + 1 and info1["tail_refreshes"] == info0["tail_refreshes"], (info0, info1)
    same_topk(prepared_topk(ix, pf, Q, 10, kp), ix.search_filtered(Q, 10, kp, sem, n + 500), "second use")
    assert pf.info()["builds"] == info1["builds"]
    pf.close()
    ix.close()


# ---- 5. life goes on ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("shape", ["n333_d33_k5", "n900_d300_k30"])
def test_life_goes_on(shape, metric, tmp_path):
    case, ix = build(f"{shape}_{metric}")
    mutate(case, ix)
    Q = the_queries(case)
    kp = case.k + 3
    recluster_and_compare(ix, kp, 0x11FE)
    rng = np.random.default_rng(0x11FE)
    n = len(ix.assignments)

    def ok(what):
        try:
            check_state(ix)
            check_search(ix, Q, nprobes=(0, 1, 5, kp), top_ks=(1, 10, 64))
        except AssertionError as e:
            raise AssertionError(f"after {what}: {e}") from e

    cl, vids = ix.add_batch((ix.values[rng.integers(0, case.n, 65)] * np.float32(0.99)).astype(np.float32))
    assert vids.tolist() == list(range(n, n + 65)) and cl.max() < kp
    ok("add_batch")
    live = live_ids(ix)
    assert ix.remove_batch(live[::5]) == live[::5].size
    ok("remove_batch")
    live = live_ids(ix)
    pick = rng.choice(live, 30, replace=False)
    _, st = ix.update_batch(pick, movers_rows(ix, pick, live))
    assert (st == 1).any() and (st == 0).any()
    ok("update_batch")
    before, after = ix.compact()
    assert after == sum(mm.capacity(len(l)) for l in ix.ids)
    ok("compact")
    recluster_and_compare(ix, case.k, 0x22FE)
    kp = case.k
    ok("a second recluster")
    path = str(tmp_path / "reclustered.idx")
    ix.save_index(path)
    ix.close()
    ix = IVFFlatIndex.load_index(path, case.d, metric=case.metric)
    ok("save_index -> load_index")
    c, vid = ix.add(Q[0])
    assert vid == n + 65
    ix.close()


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------------
def raw(ix, kp, attempts, iters, init):
    """the C call with sentinels in every output -> (status, outputs untouched)"""
    n = max(ix.info()[0], 1)
    init = np.ascontiguousarray(np.asarray(init, dtype=np.uint64).reshape(-1))
    cent = np.full((max(kp, 1), ix.d), 7.5, dtype=np.float32)
    asg = np.full(n, 9, dtype=np.uint64)
    its = np.full(max(attempts, 1), 77, dtype=np.uint64)
    cost, kept = C.c_float(-3.0), C.c_int32(-5)
    rc = capi.lib().vers_ivf_recluster(ix._h, kp, attempts, iters, capi._ptr(init) if init.size else None, capi._ptr(cent), 4 * ix.d, capi._ptr(asg),
                                       C.byref(cost), C.byref(kept), capi._ptr(its))
    untouched = bool((cent == 7.5).all() and (asg == 9).all() and (its == 77).all() and cost.value == -3.0 and kept.value == -5)
    return rc, untouched, (cost.value, kept.value, its)


def snapshot(ix, Q):
    out = [ix.info(), ix.live_count(), ix.list_lengths().tolist()]
    for c in range(ix.info()[1]):
        rows, ids = ix.get_list(c)
        out.append((bits(rows).tobytes(), ids.tobytes()))
    try:
        i, d, c = ix.search_batch(Q, 5, 3)
        on = np.arange(5)[None, :] < c[:, None]
        out.append((i[on].tobytes(), bits(d)[on].tobytes(), c.tobytes()))
    except capi.VersError as e:   # (an index that holds a NaN row: the reference's search panics, before and after alike)
        out.append(e.status)
    return out


@pytest.mark.parametrize("metric", METRICS)
def test_refusals_leave_the_index_unchanged_and_the_outputs_untouched(metric):
    case, ix = build(f"n333_d33_k5_{metric}")
    mutate(case, ix)
    Q = the_queries(case)
    m, k = ix.live_count(), case.k
    capi.recluster_phases(reset=True)
    s0 = snapshot(ix, Q)
    good = draws(1, 2, k, m)
    bad = good.copy().reshape(-1); bad[-1] = m
    for what, args, status in (("an init index == m", (k, 2, 3, bad), capi.ERR_INVALID), ("num_clusters == 0", (0, 2, 3, np.zeros(0, np.uint64)), capi.ERR_EMPTY)):
        rc, untouched, _ = raw(ix, *args)
        assert rc == status and untouched, (what, rc, untouched)
        assert snapshot(ix, Q) == s0, what
        check_state(ix)
    # num_attempts == 0: VERS_OK, nothing kept, the index unchanged (vers_ivf_build would leave an empty one)
    rc, _, (cost, kept, _) = raw(ix, k, 0, 3, np.zeros(0, np.uint64))
    assert rc == capi.OK and kept == 0 and cost == np.inf
    assert snapshot(ix, Q) == s0
    check_state(ix)
    assert ix.recluster(k, 0, 3)[1] == 0 and ix.num_centroids == k
    check_search(ix, Q, nprobes=(0, 5), top_ks=(10,))
    ph = capi.recluster_phases()
    assert ph["calls"] == 2 and ph["rows"] == 2 * m, ph      # the two calls that kept nothing ran; the refused ones count nowhere
    # an emptied index
    ix.remove_batch(live_ids(ix))
    s1 = snapshot(ix, Q)
    rc, untouched, _ = raw(ix, k, 1, 3, np.zeros(k, np.uint64))
    assert rc == capi.ERR_EMPTY and untouched and snapshot(ix, Q) == s1
    check_state(ix)
    ix.close()
    # a handle sharded by cluster
    X, _, ob, _ = mm.base(case)
    sh = IVFFlatIndex(case.d, metric=case.metric)
    sh.set_shard(0, 2)
    sh.num_centroids, sh.values, sh.centroids, sh.assignments = case.k, X.copy(), ob["centroids"].copy(), ob["assignments"].copy()
    sh._upload()
    lens0, owners = sh.list_lengths().tolist(), sh.owners()
    lists0 = [sh.get_list(c)[1].tobytes() for c in range(case.k) if owners[c] == 0]
    rc, untouched, _ = raw(sh, case.k, 1, 3, np.zeros(case.k, np.uint64))
    assert rc == capi.ERR_INVALID and untouched
    assert sh.list_lengths().tolist() == lens0 and [sh.get_list(c)[1].tobytes() for c in range(case.k) if owners[c] == 0] == lists0
    sh.close()
    # a streamed upload in progress: refused, and the upload goes on to a complete index
    up = IVFFlatIndex(case.d, metric=case.metric)
    up.values, up.centroids, up.assignments = X.copy(), ob["centroids"].copy(), ob["assignments"].copy()
    up.ids = [np.flatnonzero(up.assignments == c).tolist() for c in range(case.k)]
    up.upload_begin(up.centroids, [len(l) for l in up.ids], case.n)
    half = case.n // 2
    up.upload_chunk(X[:half], up.assignments[:half], 0)
    rc, untouched, _ = raw(up, case.k, 1, 3, np.zeros(case.k, np.uint64))
    assert rc == capi.ERR_EMPTY and untouched
    up.upload_chunk(X[half:], up.assignments[half:], half)
    up.upload_end()
    check_state(up)
    check_search(up, Q, nprobes=(0, 5), top_ks=(10,))
    up.close()
    assert capi.recluster_phases()["calls"] == 2


@pytest.mark.parametrize("metric", METRICS)
def test_a_nan_distance_is_refused(metric):
    d = 12
    X = dg.dist_c(0x4A4, 120, d, 4, dg.default_sigma(d))
    ix = IVFFlatIndex.build_index(1, 1, 2, X, init_indices=[5], metric=capi.METRIC_COSDIST if metric == "cos" else capi.METRIC_L2SQ)
    row = X[3].copy(); row[4] = np.nan
    c, vid = ix.add(row)      # k = 1 accepts it
    assert (c, vid) == (0, 120)
    Q = X[:8]
    capi.recluster_phases(reset=True)
    s0 = snapshot(ix, Q)
    rc, untouched, _ = raw(ix, 2, 2, 3, draws(3, 2, 2, 121))
    assert rc == capi.ERR_NAN and untouched
    assert snapshot(ix, Q) == s0
    check_state(ix)
    assert capi.recluster_phases()["calls"] == 0
    assert ix.remove_batch([120]) == 1     # without the row the same call goes through
    recluster_and_compare(ix, 2, 3)
    check_state(ix)
    ix.close()


# ---- 7. options ---------------------------------------------------------------------------------------------------------------------------
OPTIONS = {"memory1": ("memory", 1, 0), "f32rows": ("shadow", 0, 1), "no_rowmajor": ("rowmajor", 0, -1), "int8_head": ("pre_head", 1, 1)}


@pytest.mark.parametrize("name", list(OPTIONS))
def test_under_options(name):
    opt, value, default = OPTIONS[name]
    capi.set_option(opt, value)
    try:
        case, ix = build("n900_d300_k30_l2")     # ld 320: the smallest at which the int8 head exists (256 columns + a 64-column step)
        mutate(case, ix)
        Q = the_queries(case)
        recluster_and_compare(ix, case.k + 5, 0x0B7)
        lay = ix.layout_bytes()
        if name in ("memory1", "no_rowmajor"):
            assert lay["rowmajor"] == 0
        else:
            assert lay["rowmajor"] == lay["rows"]
        assert (lay["shadow"] == 0) == (name == "f32rows") and ix.shadow_state()["active"] == (name != "f32rows")
        assert ix.head_state()["valid"] == (name != "f32rows")     # (the head is derived from the shadow's rounding: none without it)
        check_state(ix)
        check_search(ix, Q, nprobes=(0, 1, 5), top_ks=(1, 10, 64))
        compare_with_twin(case, ix, Q)
        ix.close()
    finally:
        capi.set_option(opt, default)


# ---- 8. phases ----------------------------------------------------------------------------------------------------------------------------
def test_phases_count_calls_and_live_rows():
    case, ix = build("n333_d33_k5_l2")
    mutate(case, ix)
    m = ix.live_count()
    capi.recluster_phases(reset=True)
    assert all(v == 0.0 for v in capi.recluster_phases().values())
    recluster_and_compare(ix, 6, 1)
    recluster_and_compare(ix, 4, 2)
    rc, untouched, _ = raw(ix, 0, 1, 3, np.zeros(0, np.uint64))
    assert rc == capi.ERR_EMPTY and untouched
    ph = capi.recluster_phases(reset=True)
    assert ph["calls"] == 2 and ph["rows"] == 2 * m and ph["reserved"] == 0.0, ph
    assert all(ph[key] > 0.0 for key in ("gather_ms", "kmeans_ms", "install_ms", "derive_ms", "tables_ms")), ph
    assert capi.recluster_phases()["calls"] == 0
    ix.close()
