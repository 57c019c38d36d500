"""vers_ivf_compact: the storage of a mutated index goes back to the plan a fresh upload of the CURRENT list lengths makes, the
certificate maxima are recomputed over the rows the lists hold, and nothing observable through the reference's five fields changes.
Everything is compared bit for bit, with no tolerance, against the host mirror (IVFFlatIndex leaves its fields untouched in compact())
and the oracle called with the current lists -- the check_state / check_search of tests/test_remove_gpu.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import c_oracle as co
from tests.test_certificate_mutation_gpu import r2_ref, row_r2, row_x2, xmax2_ref
from tests.test_remove_gpu import bits, check, check_search, check_state, make, queries
from vers_amd import capi, testhooks
from vers_amd.index import IVFFlatIndex

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def round_up(x, m):
    return (x + m - 1) // m * m


def planned_rows(ix, owned=None):
    """plan_storage's rule summed over the lists this handle stores"""
    return sum(round_up(len(l) + max(8, len(l) // 16), 64) for c, l in enumerate(ix.ids) if owned is None or owned[c])


def mutate(ix, scattered=True):
    """scattered ids, a whole tile from the middle of the longest list, one whole list"""
    n = len(ix.assignments)
    lens = [len(l) for l in ix.ids]
    c = int(np.argmax(lens))
    assert lens[c] >= 192   # (callers build n >= 192 k rows, or have just grown the longest list)
    other = int(np.argsort(lens)[len(lens) // 2])
    gone = list(ix.ids[c][64:128]) + list(ix.ids[other])
    if scattered:
        gone += list(range(3, n, 17))
    assert ix.remove_batch(gone) > 64 + lens[other] - 1
    assert ix.ids[other] == []
    return c, other


def same_results(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1])) and np.array_equal(a[2], b[2])


def fallbacks_of(ix, Q, top_k=10, nprobe=5):
    """(results, matrix-core batches, queries re-scanned exactly) of one batch"""
    s0 = ix.prescan_stats()
    res = ix.search_batch(Q, top_k, nprobe)
    s1 = ix.prescan_stats()
    return res, s1["batches"] - s0["batches"], s1["fallback_queries"] - s0["fallback_queries"]


# ---- 1. state and searches, sizes and memory -------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [capi.METRIC_L2SQ, capi.METRIC_COSDIST])
@pytest.mark.parametrize("d", [16, 300, 768])
def test_state_searches_sizes_and_memory(metric, d):
    n, k = 2400, 12   # (the longest of 12 lists holds at least the mean, 200 rows: a whole tile lies in its middle)
    ix = make(n, d, k, metric, seed=0xC0A0 + d)
    Q = queries(ix, 0xC0A7 + d)
    mutate(ix)
    lb0 = ix.layout_bytes()
    now0, _ = capi.mem_stats(reset_peak=True)
    before, after = ix.compact()
    now1, peak = capi.mem_stats()
    lb1 = ix.layout_bytes()
    assert after == planned_rows(ix) and after < before, (before, after, planned_rows(ix))
    assert lb0["rows"] % before == 0 and lb1["rows"] == lb0["rows"] // before * after
    assert lb1["shadow"] == lb0["shadow"] // before * after and lb1["rowmajor"] == lb0["rowmajor"] // before * after
    assert now1 < now0, (now0, now1)
    allowed = now0 - lb0["shadow"] - lb0["rowmajor"] + lb1["rows"] + lb1["shadow"] + lb1["rowmajor"] + 8 * after + (1 << 20)
    assert peak <= allowed, (peak, allowed, now0, lb0, lb1)
    check(ix, Q)
    # slack independence, as the LAST step: whatever the rows without a vector hold, the same results and as many exact re-scans
    res0, b0, f0 = fallbacks_of(ix, Q)
    for v in (float("nan"), 1.0e30):
        testhooks.poison_slack(ix, v)
        res1, b1, f1 = fallbacks_of(ix, Q)
        assert same_results(res0, res1) and (b1, f1) == (b0, f0), (v, b0, f0, b1, f1)
    check_search(ix, Q, nprobes=(0, 5), top_ks=(10,), exhaustive=False)
    ix.close()


# ---- 2. maxima and shadow revival --------------------------------------------------------------------------------------------------
def test_maxima_are_retightened_and_a_retired_shadow_comes_back():
    n, d, k, b = 2400, 96, 12, 64
    ix = make(n, d, k, seed=0xC1A0)
    Q = queries(ix, 0xC1A7, b)
    res_f, batches_f, fb_f = fallbacks_of(ix, Q)
    assert batches_f == 1
    info = testhooks.last_vals(ix, 0, cap=32768)[3]
    x_fresh, r_fresh = info["xmax2"], info["r2"]
    assert x_fresh == xmax2_ref(ix.values) and r_fresh == r2_ref(ix.values) and info["shadow"] != 0
    big = ix.values[5] * np.float32(100.0)                     # 100 x the norm
    over = ix.values[6].copy(); over[3] = np.float32(7.0e4)    # beyond fp16: the residual is inf
    plain = (ix.values[7] * np.float32(1.001)).astype(np.float32)
    _, vids = ix.add_batch(np.stack([big, over, plain]))
    assert vids.tolist() == [n, n + 1, n + 2]
    for _ in range(6):   # no certificate holds with R = inf: after 256 queries the shadow retires itself for the handle
        ix.search_batch(Q, 10, 5)
    assert not ix.shadow_state()["active"]
    assert ix.remove_batch([n, n + 1]) == 2
    ix.search_batch(Q, 10, 5)
    assert not ix.shadow_state()["active"]                      # removing the rows cures nothing
    ix.compact()
    assert ix.shadow_state()["active"]
    res, batches, fb = fallbacks_of(ix, Q)
    print(f"fallback queries of the batch: fresh {fb_f}, after compact {fb}")
    assert batches == 1 and fb == 0, (batches, fb)
    info = testhooks.last_vals(ix, 0, cap=32768)[3]
    assert info["shadow"] != 0
    live = np.concatenate([np.arange(n), [n + 2]])
    x_want = max(x_fresh, float(row_x2(plain)[0]))
    r_want = max(r_fresh, float(row_r2(plain)[0]))
    assert x_want == xmax2_ref(ix.values[live]) and r_want == r2_ref(ix.values[live])
    assert info["xmax2"] == x_want and info["r2"] == r_want, (info, x_want, r_want, x_fresh, r_fresh)
    assert np.isfinite(info["r2"]) and info["xmax2"] < 2 * x_fresh
    check_state(ix)
    check_search(ix, Q, nprobes=(0, 5), top_ks=(10, 64))
    ix.close()


# ---- 3. fused against unfused -------------------------------------------------------------------------------------------------------
def grown_and_cut(d, seed):
    """an add_batch that forces a re-layout (more than twice the longest list's rows around its centroid), then removals"""
    ix = make(2000, d, 12, seed=seed)
    sizes = ix.list_lengths()
    c = int(np.argmax(sizes))
    rng = np.random.default_rng(seed)
    sigma = float(np.std(ix.values[np.asarray(ix.ids[c], dtype=np.int64)].astype(np.float64) - ix.centroids[c].astype(np.float64)))
    around = (ix.centroids[c][None, :] + rng.normal(0, sigma, (2 * int(sizes[c]) + 70, d))).astype(np.float32)
    rows0 = ix.layout_bytes()["rows"]
    ix.add_batch(around)
    assert ix.layout_bytes()["rows"] > rows0
    mutate(ix)
    return ix


@pytest.mark.parametrize("d", [16, 300, 768])   # one partial column pass | two passes, the second ragged | three whole passes
def test_fused_equals_unfused(d):
    b, top_k, nprobe = 40, 10, 5
    a, u = grown_and_cut(d, 0xC2A0 + d), grown_and_cut(d, 0xC2A0 + d)
    assert a.ids == u.ids
    Q = queries(a, 0xC2A7 + d, b)
    try:
        capi.set_option("compact_fused", 1)
        capi.compact_phases(reset=True)
        ra = a.compact()
        pa = capi.compact_phases(reset=True)
        capi.set_option("compact_fused", 0)
        ru = u.compact()
        pu = capi.compact_phases()
    finally:
        capi.set_option("compact_fused", 1)
    assert ra == ru and ra[1] == planned_rows(a) < ra[0]
    assert pa["calls"] == 1 and pa["rows_before"] == ra[0] and pa["rows_after"] == ra[1] and pa["derive_ms"] == 0.0
    assert pu["calls"] == 1 and pu["derive_ms"] > 0.0    # the unfused sequence ran refresh_norms
    assert a.layout_bytes() == u.layout_bytes()
    for c in range(a.num_centroids):
        (rows_a, ids_a), (rows_u, ids_u) = a.get_list(c), u.get_list(c)
        assert np.array_equal(ids_a, ids_u) and np.array_equal(bits(rows_a), bits(rows_u)), c
    res_a, ba, fa = fallbacks_of(a, Q, top_k, nprobe)
    dumps_a = [testhooks.last_vals(a, q, cap=32768) for q in range(b)]
    res_u, bu, fu = fallbacks_of(u, Q, top_k, nprobe)
    dumps_u = [testhooks.last_vals(u, q, cap=32768) for q in range(b)]
    assert same_results(res_a, res_u) and (ba, fa) == (bu, fu) and ba == 1
    for q in range(b):
        (va, xa, _, ia), (vu, xu, _, iu) = dumps_a[q], dumps_u[q]
        assert 0 < len(va) < 32768
        # Which candidates a scan KEEPS depends on when its waves saw each other's thresholds (test_certificate_mutation_gpu.same_vals):
        # the (vec id, val) pairs both scans kept are compared -- the shadow's and xnorm's bits -- and they cover the answer.
        common, ka, ku = np.intersect1d(va, vu, return_indices=True)
        assert np.array_equal(bits(xa[ka]), bits(xu[ku])), q
        assert fa + fu > 0 or np.all(np.isin(res_a[0][q, :res_a[2][q]], common)), q
        assert ia["xmax2"] == iu["xmax2"] and ia["r2"] == iu["r2"] and ia["shadow"] == iu["shadow"] != 0, (q, ia, iu)
    live = np.sort(np.concatenate([np.asarray(l, dtype=np.int64) for l in a.ids]))
    assert dumps_a[0][3]["xmax2"] == xmax2_ref(a.values[live]) and dumps_a[0][3]["r2"] == r2_ref(a.values[live])
    check_state(a)
    check_search(a, Q, nprobes=(0, nprobe), top_ks=(10, 64), exhaustive=False)
    a.close(); u.close()


# ---- 4. life cycle ------------------------------------------------------------------------------------------------------------------
def light(ix, Q):
    check_state(ix)
    check_search(ix, Q, nprobes=(0, 3), top_ks=(10,), exhaustive=False)


def test_life_cycle(tmp_path):
    n, d, k = 2400, 64, 12
    ix = make(n, d, k, seed=0xC3A0)
    Q = queries(ix, 0xC3A7)
    r0 = ix.search_batch(Q, 10, 3)
    before, after = ix.compact()                       # a fresh build: already at the plan
    assert before == after == planned_rows(ix)
    assert same_results(r0, ix.search_batch(Q, 10, 3))
    light(ix, Q)
    c, empty = mutate(ix)                              # `empty`: an empty list among full ones from here on
    before, after = ix.compact()
    assert after == planned_rows(ix) < before
    light(ix, Q)
    rows = ix.layout_bytes()["rows"]
    relayouts = capi.add_batch_phases()["relayouts"]
    ix.add(ix.centroids[c] + np.float32(1e-3))         # into the new slack: at least 8 rows per list
    ix.add_batch(ix.centroids[c][None, :] + np.linspace(2e-3, 5e-3, 4, dtype=np.float32)[:, None])
    ix.add(ix.centroids[empty])                        # the emptied list has its 64 rows
    assert ix.layout_bytes()["rows"] == rows and capi.add_batch_phases()["relayouts"] == relayouts
    light(ix, Q)
    rng = np.random.default_rng(4)
    past = (ix.centroids[c][None, :] + rng.normal(0, 0.05, (len(ix.ids[c]) // 8 + 80, d))).astype(np.float32)
    ix.add_batch(past)                                 # past the slack: a re-layout
    assert ix.layout_bytes()["rows"] > rows
    light(ix, Q)
    ix.remove_batch(np.arange(1, len(ix.assignments), 5))
    light(ix, Q)
    before, after = ix.compact()
    assert after == planned_rows(ix) < before
    light(ix, Q)
    r1 = ix.search_batch(Q, 10, 3)
    again = ix.compact()                               # twice in a row: nothing left to give back
    assert again == (after, after)
    assert same_results(r1, ix.search_batch(Q, 10, 3))
    light(ix, Q)
    path = str(tmp_path / "compacted.idx")             # save -> load
    ix.save_index(path)
    back = IVFFlatIndex.load_index(path, d)
    assert back.ids == ix.ids and back.info() == ix.info()
    # (load_index uploads every position and then removes the ones missing from the file's lists: its storage is the whole corpus' plan)
    assert back.compact()[1] == after and back.layout_bytes() == ix.layout_bytes()    # the same plan from the same lists
    assert same_results(r1, back.search_batch(Q, 10, 3))
    back.close()
    ix.remove_batch(np.arange(len(ix.assignments)))    # every row removed
    before, after = ix.compact()
    assert after == 64 * k and ix.live_count() == 0 and ix.info() == (len(ix.assignments), k, 0)
    check_state(ix)
    assert not ix.search_batch(Q, 5, 3)[2].any()
    for qs in (Q, Q[:1]):
        with pytest.raises(capi.VersError) as e:
            ix.search_batch(qs, 1, 0)
        assert e.value.status == capi.ERR_INSUFFICIENT
    ix.add(ix.values[0])                               # ... and the index lives on
    light(ix, Q[:32])
    ix.close()


# ---- 5. options -----------------------------------------------------------------------------------------------------------------------
def option_scenario():
    """one case in a process started under VERS_OPTIONS (see test_under_options)"""
    n, d, k = 2400, 96, 12
    ix = make(n, d, k, seed=0xC4A0)
    Q = queries(ix, 0xC4A7)
    if capi.env_option("memory", 0) == 1:
        assert ix.layout_bytes()["rowmajor"] == 0
    if capi.env_option("shadow", 1) == 0:
        assert not ix.shadow_state()["active"]
    mutate(ix)
    before, after = ix.compact()
    assert after == planned_rows(ix) < before
    lb = ix.layout_bytes()
    assert lb["rows"] == after * 128 * 4
    assert lb["rowmajor"] == (0 if capi.env_option("memory", 0) == 1 else lb["rows"])
    assert ix.shadow_state()["active"] == (capi.env_option("shadow", 1) != 0)
    check_state(ix)
    check_search(ix, Q, top_ks=(10, 64))
    ix.add_batch(ix.values[:30] * np.float32(1.01))
    ix.remove_batch(ix.ids[3][::2])
    ix.compact()
    check_state(ix)
    check_search(ix, Q, nprobes=(0, 5), top_ks=(10,), exhaustive=False)
    ix.close()
    print("compact scenario ok")


@pytest.mark.parametrize("options", ["memory=1", "shadow=0", "prescan=2,coarse=2", "poison_alloc=255"])
def test_under_options(options):
    env = dict(os.environ, VERS_OPTIONS=options, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", "from tests.test_compact_gpu import option_scenario; option_scenario()"], capture_output=True, text=True,
                       env=env, cwd=ROOT, timeout=600)
    assert r.returncode == 0 and "compact scenario ok" in r.stdout, r.stdout + r.stderr


def test_memory_options_are_read_as_a_build_reads_them():
    ix = make(2400, 96, 12, seed=0xC4B0)
    Q = queries(ix, 0xC4B7)
    assert ix.layout_bytes()["rowmajor"] > 0 and ix.shadow_state()["active"]
    mutate(ix)
    try:
        capi.set_option("memory", 1)
        ix.compact()
        assert ix.layout_bytes()["rowmajor"] == 0 and ix.layout_bytes()["shadow"] > 0     # compact layout: the row-major copy is dropped
        check_search(ix, Q, nprobes=(0, 5), top_ks=(10,), exhaustive=False)
        capi.set_option("memory", 0)
        capi.set_option("shadow", 0)
        assert ix.compact()[0] == ix.compact()[1]
        assert ix.layout_bytes()["rowmajor"] > 0 and ix.layout_bytes()["shadow"] == 0 and not ix.shadow_state()["active"]
        check_search(ix, Q, nprobes=(0, 5), top_ks=(10,), exhaustive=False)
    finally:
        capi.set_option("memory", 0)
        capi.set_option("shadow", 1)
    ix.compact()
    assert ix.layout_bytes()["shadow"] > 0 and ix.shadow_state()["active"]
    check(ix, Q, top_ks=(10,))
    ix.close()


# ---- 6. errors --------------------------------------------------------------------------------------------------------------------------
def test_no_centroids_upload_in_progress_and_null_outputs():
    n, d, k = 2400, 40, 12
    ix = make(n, d, k, seed=0xC5A0)
    Q = queries(ix, 0xC5A7, 33)
    L = capi.lib()
    # no centroids: nothing to do
    e0 = IVFFlatIndex(d)
    assert e0.compact() == (0, 0)
    nothing = IVFFlatIndex.build_index(4, 0, 3, ix.values[:50], init_indices=np.zeros(0, np.uint64))   # no attempt: nothing kept
    a, b = C.c_uint64(7), C.c_uint64(7)
    assert L.vers_ivf_compact(nothing._h, C.byref(a), C.byref(b)) == capi.OK and (a.value, b.value) == (0, 0)
    # null handle, null outputs
    assert L.vers_ivf_compact(None, None, None) == capi.ERR_INVALID
    mutate(ix, scattered=False)
    assert L.vers_ivf_compact(ix._h, None, None) == capi.OK
    assert ix.layout_bytes()["rows"] == planned_rows(ix) * 64 * 4
    assert L.vers_ivf_compact(ix._h, None, C.byref(b)) == capi.OK and b.value == planned_rows(ix)
    check(ix, Q, top_ks=(10,))
    # between upload_begin and upload_end: the handle holds no index yet, as for add / remove; the upload can still finish
    up = IVFFlatIndex(d)
    A = ix.assignments
    up.upload_begin(ix.centroids, np.bincount(A.astype(np.int64), minlength=k), len(A))
    a, b = C.c_uint64(7), C.c_uint64(7)
    assert L.vers_ivf_compact(up._h, C.byref(a), C.byref(b)) == capi.ERR_EMPTY and (a.value, b.value) == (0, 0)
    with pytest.raises(capi.VersError) as e:
        up.compact()
    assert e.value.status == capi.ERR_EMPTY
    up.upload_chunk(ix.values[:700], A[:700], 0)
    up.upload_chunk(ix.values[700:], A[700:], 700)
    up.upload_end()
    up.values, up.centroids, up.assignments = ix.values, ix.centroids, A
    up.ids = [np.flatnonzero(A == c).tolist() for c in range(k)]
    check(up, Q, top_ks=(10,))
    assert up.compact()[0] == up.compact()[1]
    for j in (ix, e0, nothing, up):
        j.close()


# ---- 8. the C++ mirror --------------------------------------------------------------------------------------------------------------------
def test_cpp_host_mirror_compact(tmp_path):
    """vers_amd/host/ivfflat.hpp's compact() from compiled code (tests/cpp/compact_demo.cpp): remove -> compact -> search equals before"""
    lib = capi.LIB_PATH   # the library these tests run against
    exe = str(tmp_path / "compact_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + ROOT, "-o", exe, os.path.join(ROOT, "tests", "cpp", "compact_demo.cpp"),
                           "-L" + os.path.dirname(lib), "-lvers_hip", "-Wl,-rpath," + os.path.dirname(lib)])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "SAME" in out.stdout, out.stdout + out.stderr
