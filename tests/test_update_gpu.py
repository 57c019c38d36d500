"""vers_ivf_update_batch / vers_ivf_update_batch_dev: values[v] = x under the id the vector already has; a row whose first-minimum
centroid is still its list is overwritten in place, one that changes cluster leaves its list and enters the new one at its SORTED place by
vec id.  The specification in one sentence: afterwards the handle is, bit for bit in everything observable, a handle that received
vers_ivf_upload(values', centroids, assignments') followed by remove_batch of the ids that are in no list.

Every case keeps the host mirror (IVFFlatIndex.update_batch: values, assignments, ids with bisect.insort, the device's status and clusters
asserted against the mirror's own) and compares with check_state / check_search of tests/test_remove_gpu.py: info(), live_count(),
list_lengths(), every list's stored rows and ids, and searches -- batches of >= 32 queries (matrix-core scan on the shadow), single queries,
exhaustive -- against the oracle on the mirror.  No tolerance anywhere.

The inputs need no tuning: a row replaced by values[u] of a u whose own first-minimum centroid (co.add_cluster) is list c goes to c -- it
moves when c is another list, stays when it is the row's own (a copy of itself, or of a list-mate)."""
import ctypes as C

import numpy as np
import pytest

from oracle import c_oracle as co
from tests.golden import make_golden as mg
from tests.test_certificate_gpu import corpus, d_ref
from tests.test_certificate_mutation_gpu import fresh_handle, r2_ref, row_r2, row_x2, same_vals, xmax2_ref
from tests.test_remove_gpu import bits, check, check_search, check_state, live_ids, make, queries
from vers_amd import capi, testhooks
from vers_amd.index import IVFFlatIndex

pytestmark = pytest.mark.gpu

STAYED, MOVED, SKIPPED = 0, 1, 2


def own_cluster(ix):
    """per vec id ever stored: the first-minimum centroid of its CURRENT value (the rule of add; not necessarily assignments[v], which the
    build took before the last centroid update)"""
    return np.array([co.add_cluster(ix.centroids, x, ix.metric) for x in ix.values], dtype=np.int64)


def donors_by_list(ix):
    """per list: the rows (as the index holds them NOW -- later updates do not change the donors) whose own cluster is that list"""
    cl = own_cluster(ix)
    return [ix.values[cl == c].copy() for c in range(ix.num_centroids)]


def rows_to(ix, don, targets, rng):
    """one row per target list: values[u] of a random u whose own cluster is that list"""
    out = np.zeros((len(targets), ix.d), dtype=np.float32)
    for i, t in enumerate(targets):
        assert don[t].shape[0] > 0, t
        out[i] = don[t][int(rng.integers(don[t].shape[0]))]
    return out


def update(ix, vids, rows, targets, status):
    """update_batch with the expectation spelled out: cluster targets[i] (asserted against the oracle's add rule as well) and `status`"""
    vids = np.asarray(vids, dtype=np.int64)
    for x, t in zip(rows, targets):
        assert co.add_cluster(ix.centroids, x, ix.metric) == t
    n0, live0 = ix.info()[0], ix.live_count()
    cl, st = ix.update_batch(vids, rows)
    assert np.array_equal(cl, np.asarray(targets, dtype=np.uint64))
    assert np.array_equal(st, np.broadcast_to(np.asarray(status, dtype=np.uint8), st.shape)), (st, status)
    assert ix.info()[0] == n0 and ix.live_count() == live0     # n and the live count do not change
    for l in ix.ids:
        assert l == sorted(l)                                   # every list ascending in vec id
    return cl, st


def other_list(ix, don, v, k, step=1):
    """another list than v's, `step` lists on -- the next one that has donors"""
    a = int(ix.assignments[v])
    t = (a + step) % k
    while t == a or don[t].shape[0] == 0:
        t = (t + 1) % k
    return t


def usable(ix, don, vids):
    """the ids whose own list has donors (a list all of whose rows the final centroids assign elsewhere has none: its rows cannot be told to stay)"""
    return np.asarray([v for v in np.asarray(vids).tolist() if don[int(ix.assignments[v])].shape[0]], dtype=np.int64)


def same_as_saved_and_loaded(ix, Q, tmp_path, name):
    """the specification, directly: save_index -> load_index builds the handle of upload(values', centroids, assignments') + remove_batch
    of the ids in no list -- the same rows and ids in every list, the same search results"""
    path = str(tmp_path / (name + ".idx"))
    ix.save_index(path)
    back = IVFFlatIndex.load_index(path, ix.d, metric=ix.metric)
    assert back.ids == ix.ids and back.info() == ix.info() and back.live_count() == ix.live_count()
    for c in range(ix.num_centroids):
        ra, ia = ix.get_list(c)
        rb, ib = back.get_list(c)
        assert np.array_equal(ia, ib) and np.array_equal(bits(ra), bits(rb)), (name, c)
    for nprobe, top_k in ((0, 10), (1, 1), (5, 64), (ix.num_centroids, 200)):
        for qs in (Q, Q[:1]):
            a, b = ix.search_batch(qs, top_k, nprobe), back.search_batch(qs, top_k, nprobe)
            assert np.array_equal(a[2], b[2]), (name, nprobe, top_k)
            m = np.arange(top_k)[None, :] < a[2][:, None]
            assert np.array_equal(a[0][m], b[0][m]) and np.array_equal(bits(a[1])[m], bits(b[1])[m]), (name, nprobe, top_k)
    back.close()


@pytest.mark.parametrize("metric", [capi.METRIC_L2SQ, capi.METRIC_COSDIST])
@pytest.mark.parametrize("d", [16, 300, 768])
def test_scattered_stays_scattered_moves_and_a_mix_with_repeats(metric, d, tmp_path):
    n, k = 2000, 24
    ix = make(n, d, k, metric, seed=0x19D0 + d)
    Q = queries(ix, 0x19D7 + d)
    rng = np.random.default_rng(d + metric)
    don = donors_by_list(ix)
    capi.update_phases(reset=True)
    # stays only: a list-mate's value (every third: the row's own value again)
    vids = usable(ix, don, np.arange(3, n, 17))
    targets = [int(ix.assignments[v]) for v in vids]
    rows = rows_to(ix, don, targets, rng)
    rows[::3] = ix.values[vids[::3]]
    keep = [i for i, (v, t) in enumerate(zip(vids, targets)) if co.add_cluster(ix.centroids, rows[i], metric) == t]   # (a row's own value may belong elsewhere)
    vids, rows, targets = vids[keep], rows[keep], [targets[i] for i in keep]
    assert len(keep) > 80
    update(ix, vids, rows, targets, STAYED)
    assert ix.last_update_counts == (len(keep), 0, 0, 0)
    check(ix, Q)
    # moves only
    vids = np.arange(5, n, 23)
    targets = [other_list(ix, don, v, k, 1 + i % 5) for i, v in enumerate(vids)]
    update(ix, vids, rows_to(ix, don, targets, rng), targets, MOVED)
    assert ix.last_update_counts[:3] == (0, len(vids), 0)
    check(ix, Q)
    # a mix, in random order, with ids of the two calls above and of each other
    rows_passed, rows_moved = len(keep) + len(vids), len(vids)
    for rep in range(2):
        vids = usable(ix, don, rng.choice(n, 320, replace=False))[:300]
        targets = [int(ix.assignments[v]) if i % 2 else other_list(ix, don, v, k, 1 + i % 7) for i, v in enumerate(vids)]
        update(ix, vids, rows_to(ix, don, targets, rng), targets, [STAYED if i % 2 else MOVED for i in range(vids.size)])
        rows_passed, rows_moved = rows_passed + vids.size, rows_moved + (vids.size + 1) // 2
    ph = capi.update_phases()
    assert ph["calls"] == 4 and ph["rows"] == rows_passed and ph["moved"] == rows_moved and ph["stayed"] == rows_passed - rows_moved
    check(ix, Q)
    if d == 300:
        same_as_saved_and_loaded(ix, Q, tmp_path, "mix")
    ix.close()


def test_head_tail_middle_more_than_64_movers_a_list_emptied_and_filled_again(tmp_path):
    n, d, k = 2600, 64, 12
    ix = make(n, d, k, seed=0x7110)
    Q = queries(ix, 0x7117)
    rng = np.random.default_rng(64)
    don = donors_by_list(ix)
    lens = [len(l) for l in ix.ids]
    c = max((j for j in range(k) if 0 not in ix.ids[j] and n - 1 not in ix.ids[j] and don[j].shape[0]), key=lambda j: lens[j])
    outside = [v for v in live_ids(ix).tolist() if ix.assignments[v] != c]
    # more than 64 movers into one list in one call (and the list is >= 192 rows long afterwards, whatever the build made of it)
    many = rng.choice(outside[1:-1], max(100, 200 - lens[c]), replace=False)
    update(ix, many, rows_to(ix, don, [c] * many.size, rng), [c] * many.size, MOVED)
    assert len(ix.ids[c]) >= 192
    check(ix, Q, top_ks=(10, 64))
    # to the head, to the tail and into the middle of it -- and exactly onto the tile boundary (position 64)
    lst = ix.ids[c]
    between = lambda lo, hi: next(v for v in range(lo + 1, hi) if v not in lst and any(v in l for l in ix.ids))
    head, tail = 0, n - 1
    mid = between(lst[len(lst) // 2], lst[-1])
    edge = next((v for v in range(lst[63] + 1, lst[64]) if any(v in l for l in ix.ids)), None)
    vids = [tail, mid, head] + ([edge] if edge is not None and edge != mid else [])
    update(ix, vids, rows_to(ix, don, [c] * len(vids), rng), [c] * len(vids), MOVED)
    assert ix.ids[c][0] == head and ix.ids[c][-1] == tail and 0 < ix.ids[c].index(mid) < len(ix.ids[c]) - 1
    if edge is not None and edge != mid:
        assert ix.ids[c].index(edge) == 65   # (the head moved in front of it)
    check(ix, Q, top_ks=(1, 10))
    same_as_saved_and_loaded(ix, Q, tmp_path, "head_tail_middle")
    # a list emptied by moves ...
    e = min((j for j in range(k) if j != c and ix.ids[j] and don[j].shape[0]), key=lambda j: len(ix.ids[j]))
    gone = list(ix.ids[e])
    targets = [other_list(ix, don, v, k, 1 + i % (k - 1)) for i, v in enumerate(gone)]
    update(ix, gone, rows_to(ix, don, targets, rng), targets, MOVED)
    assert ix.ids[e] == [] and ix.list_lengths()[e] == 0
    check(ix, Q, top_ks=(10, 200))
    # ... and filled again: rows into an empty list, in descending order of their ids
    back = sorted(rng.choice(live_ids(ix), 70, replace=False).tolist(), reverse=True)
    update(ix, back, rows_to(ix, don, [e] * 70, rng), [e] * 70, MOVED)
    assert ix.ids[e] == sorted(back)
    check(ix, Q)
    ix.close()


def test_movers_into_a_list_at_capacity_re_lay_out_the_storage():
    d, k = 64, 12
    ix = make(1200, d, k, seed=0x4E10)
    Q = queries(ix, 0x4E17)
    rng = np.random.default_rng(5)
    don = donors_by_list(ix)
    lens = [len(l) for l in ix.ids]
    c = int(np.argmax(lens))
    cap = (lens[c] + max(8, lens[c] // 16) + 63) // 64 * 64          # plan_storage's rule
    outside = np.array([v for v in range(1200) if ix.assignments[v] != c])
    fill = outside[:cap - lens[c]]                                    # exactly to capacity: no re-layout
    lb0 = ix.layout_bytes()["rows"]
    update(ix, fill, rows_to(ix, don, [c] * fill.size, rng), [c] * fill.size, MOVED)
    assert ix.last_update_counts == (0, fill.size, 0, 0) and ix.layout_bytes()["rows"] == lb0 and len(ix.ids[c]) == cap
    check(ix, Q, top_ks=(10,))
    more = outside[cap - lens[c]:][::3][:90]                          # one row too many would do; 90 of them, interleaved
    update(ix, more, rows_to(ix, don, [c] * more.size, rng), [c] * more.size, MOVED)
    assert ix.last_update_counts == (0, more.size, 0, 1) and ix.layout_bytes()["rows"] > lb0
    check(ix, Q, top_ks=(10, 64))
    stay = np.asarray(ix.ids[c][5::7])
    update(ix, stay, rows_to(ix, don, [c] * stay.size, rng), [c] * stay.size, STAYED)
    check(ix, Q, top_ks=(10,))
    ix.close()


def test_removed_ids_are_skipped_and_updates_mix_with_remove_compact_and_add(tmp_path):
    n, d, k = 2000, 96, 24
    ix = make(n, d, k, seed=0xAD10)
    Q = queries(ix, 0xAD17)
    rng = np.random.default_rng(3)
    don = donors_by_list(ix)
    gone = rng.choice(n, 400, replace=False)
    assert ix.remove_batch(gone) == 400
    # ids removed earlier: status 2, nothing changes for them -- among rows that stay and rows that move
    vids = np.concatenate([gone[:50], usable(ix, don, np.setdiff1d(np.arange(0, n, 9), gone))])
    rng.shuffle(vids)
    was_gone = np.isin(vids, gone)
    targets = [other_list(ix, don, v, k, 3) if i % 2 or was_gone[i] else int(ix.assignments[v]) for i, v in enumerate(vids)]
    values0 = ix.values.copy()
    update(ix, vids, rows_to(ix, don, targets, rng), targets, np.where(was_gone, SKIPPED, np.where(np.arange(vids.size) % 2, MOVED, STAYED)))
    assert np.array_equal(bits(ix.values[gone]), bits(values0[gone])) and ix.last_update_counts[2] == 50
    check(ix, Q, top_ks=(10, 64))
    same_as_saved_and_loaded(ix, Q, tmp_path, "after_remove")
    only_gone = gone[100:130]
    t0 = next(j for j in range(k) if don[j].shape[0])
    update(ix, only_gone, rows_to(ix, don, [t0] * 30, rng), [t0] * 30, SKIPPED)   # a call that changes nothing at all
    check_state(ix)
    # after compact
    ix.compact()
    vids = usable(ix, don, np.setdiff1d(np.arange(4, n, 11), gone))
    targets = [other_list(ix, don, v, k, 1 + i % 2) if i % 3 else int(ix.assignments[v]) for i, v in enumerate(vids)]
    update(ix, vids, rows_to(ix, don, targets, rng), targets, [MOVED if i % 3 else STAYED for i in range(vids.size)])
    check(ix, Q, top_ks=(10, 64))
    # add_batch after an update: the new ids land behind
    cl, new = ix.add_batch(ix.values[vids[:60]])
    for c_, v in zip(cl.tolist(), new.tolist()):
        assert ix.ids[c_][-1] >= n and v in ix.ids[c_]
    upd = np.concatenate([new[:20].astype(np.int64), vids[:30]])
    targets = [other_list(ix, don, v, k, 2) for v in upd]
    update(ix, upd, rows_to(ix, don, targets, rng), targets, MOVED)   # added rows move in front of nothing: their ids are the largest
    check(ix, Q, top_ks=(10,))
    # remove_batch of updated ids
    assert ix.remove_batch(np.concatenate([upd, vids[40:80]])) == upd.size + 40
    check(ix, Q)
    ix.close()


def snapshot(ix, Q):
    lists = [ix.get_list(c) for c in range(ix.num_centroids)]
    s = ix.search_batch(Q, 10, 5)
    return ix.info(), ix.live_count(), [(bits(r).copy(), i.copy()) for r, i in lists], s[0].copy(), bits(s[1]).copy(), s[2].copy()


def same_snapshot(a, b):
    assert a[0] == b[0] and a[1] == b[1]
    for (ra, ia), (rb, ib) in zip(a[2], b[2]):
        assert np.array_equal(ia, ib) and np.array_equal(ra, rb)
    assert np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4]) and np.array_equal(a[5], b[5])


def test_all_or_nothing():
    n, d, k = 2000, 40, 16
    ix = make(n, d, k, seed=0x1A10)
    Q = queries(ix, 0x1A17, 33)
    rng = np.random.default_rng(7)
    don = donors_by_list(ix)
    ix.remove_batch([7, 8, 9])
    vids = usable(ix, don, np.setdiff1d(np.arange(1, n, 13), [7, 8, 9]))
    targets = [other_list(ix, don, v, k, 1 + i % 3) if i % 2 else int(ix.assignments[v]) for i, v in enumerate(vids)]
    rows = rows_to(ix, don, targets, rng)
    before = snapshot(ix, Q)
    mirror = (ix.values.copy(), ix.assignments.copy(), [list(l) for l in ix.ids])
    lib = capi.lib()
    out = (np.full(vids.size + 1, 77, dtype=np.uint64), np.full(vids.size + 1, 9, dtype=np.uint8), np.full(4, 5, dtype=np.uint64))

    def refused(v, r, status):
        v = np.ascontiguousarray(v, dtype=np.uint64)
        r = np.ascontiguousarray(r, dtype=np.float32)
        rc = lib.vers_ivf_update_batch(ix._h, capi._ptr(v), capi._ptr(r), v.size, 4 * d, capi._ptr(out[0]), capi._ptr(out[1]),
                                       out[2].ctypes.data_as(C.POINTER(C.c_uint64)))
        assert rc == status, (rc, status)
        assert (out[0] == 77).all() and (out[1] == 9).all() and (out[2] == 5).all()   # the outputs are untouched
        same_snapshot(snapshot(ix, Q), before)                                          # the index is unchanged and searchable

    for bad in (n, n + 5, 2 ** 40):                                                     # an id >= n, among valid movers
        v = vids.astype(np.uint64).copy(); v[len(v) // 2] = bad
        refused(v, rows, capi.ERR_INVALID)
    v = vids.copy(); v[-1] = v[3]                                                       # the same id twice
    refused(v, rows, capi.ERR_INVALID)
    refused(np.concatenate([vids, vids[:1]]), np.concatenate([rows, rows[:1]]), capi.ERR_INVALID)
    r = rows.copy(); r[len(r) // 2, 3] = np.nan                                         # a NaN row in the middle
    refused(vids, r, capi.ERR_NAN)
    capi.set_option("add_batch_rows", 64)                                               # several chunks, the NaN in the last one
    try:
        assert vids.size > 128
        r = rows.copy(); r[-2, d - 1] = np.nan
        refused(vids, r, capi.ERR_NAN)
        # ... and the same call without the NaN goes through, chunk by chunk (every chunk staged twice)
        with pytest.raises(capi.VersError) as e:
            ix.update_batch(vids, r)
        assert e.value.status == capi.ERR_NAN
        ix.values, ix.assignments, ix.ids = mirror   # (the mirror had nothing to follow)
        update(ix, vids, rows, targets, [MOVED if i % 2 else STAYED for i in range(vids.size)])
    finally:
        capi.set_option("add_batch_rows", 131072)
    check(ix, Q, top_ks=(10, 64))
    # n == 0 is a no-op
    before = snapshot(ix, Q)
    cl, st = ix.update_batch([], np.zeros((0, d), np.float32))
    assert cl.size == 0 and st.size == 0
    assert lib.vers_ivf_update_batch(ix._h, None, None, 0, 4 * d, None, None, None) == 0
    same_snapshot(snapshot(ix, Q), before)
    # no centroids; a streamed upload in progress
    e0 = IVFFlatIndex(d)
    up = IVFFlatIndex(d)
    up.upload_begin(ix.centroids, np.bincount(ix.assignments.astype(np.int64), minlength=k), len(ix.assignments))
    for j in (e0, up):
        one_id, one_row = np.zeros(1, np.uint64), np.zeros((1, d), np.float32)
        assert lib.vers_ivf_update_batch(j._h, capi._ptr(one_id), capi._ptr(one_row), 1, 4 * d, None, None, None) == capi.ERR_EMPTY
        j.close()
    ix.close()


def test_k1_accepts_a_nan_row_as_add_does():
    d = 16
    X = corpus("dist_c", 300, d, 0x1C1)
    ix = IVFFlatIndex.build_index(1, 1, 2, X, init_indices=mg.init_draws(3, 1, 1, 300))
    r = X[:3].copy(); r[1, 2] = np.nan
    cl, st = ix.update_batch([5, 6, 299], r)
    assert cl.tolist() == [0, 0, 0] and st.tolist() == [0, 0, 0]
    rows, ids = ix.get_list(0)
    assert np.array_equal(ids, np.arange(300, dtype=np.uint64)) and np.array_equal(bits(rows), bits(ix.values))
    ix.close()


def test_device_pointer_call():
    import torch
    n, d, k = 2000, 40, 16
    ix = make(n, d, k, seed=0x1A20)
    Q = queries(ix, 0x1A27, 33)
    rng = np.random.default_rng(9)
    don = donors_by_list(ix)
    vids = usable(ix, don, np.arange(2, n, 7))
    targets = [other_list(ix, don, v, k, 2) if i % 2 else int(ix.assignments[v]) for i, v in enumerate(vids)]
    rows = rows_to(ix, don, targets, rng)
    ld = 44
    padded = np.full((vids.size, ld), np.nan, dtype=np.float32)   # padding columns are never read
    padded[:, :d] = rows
    ids_d = torch.from_numpy(vids.astype(np.int64)).cuda()
    rows_d = torch.from_numpy(padded).cuda()
    cl_d = torch.zeros(vids.size, dtype=torch.int64, device="cuda")
    st_d = torch.full((vids.size,), 9, dtype=torch.uint8, device="cuda")
    counts = ix.update_batch_dev(ids_d.data_ptr(), rows_d.data_ptr(), vids.size, ld, cl_d.data_ptr(), st_d.data_ptr())
    assert counts == ((vids.size + 1) // 2, vids.size // 2, 0, 0)
    assert np.array_equal(cl_d.cpu().numpy(), np.asarray(targets)) and np.array_equal(st_d.cpu().numpy(), np.arange(vids.size) % 2)
    # the mirror by hand, as the _dev mutators leave it to the caller
    import bisect
    ix.values = ix.values.copy()
    for v, t, x in zip(vids.tolist(), targets, rows):
        ix.values[v] = x
        if ix.assignments[v] != t:
            ix.ids[int(ix.assignments[v])].remove(v)
            ix.assignments[v] = t
            bisect.insort(ix.ids[t], v)
    check(ix, Q, top_ks=(10, 64))
    ix.close()


def test_prepared_filters_stay_valid_when_every_row_stays_and_rebuild_after_a_move():
    from tests.test_filtered_prepared_gpu import Ctx, prepare, same_topk, topk
    c = Ctx()
    ix = c.ix
    k = ix.num_centroids
    rng = np.random.default_rng(11)
    don = donors_by_list(ix)
    fs = [c.f["r30"], c.f["span"]]                         # two bitmaps
    pfs = [prepare(ix, f) for f in fs]

    def compare(what):
        for f, pf in zip(fs, pfs):
            for b, top_k, nprobe in ((40, 10, 5), (1, 70, 24)):
                want = topk(c, f, None, b, top_k, nprobe)
                got = topk(c, f, pf, b, top_k, nprobe)
                same_topk(got, want, (what, f.name, b, top_k, nprobe))

    compare("fresh")
    info0 = [pf.info() for pf in pfs]
    # a stays-only update: no storage row changed its vec id -- no rebuild, the next search does no mask work
    vids = usable(ix, don, np.arange(2, c.n, 19))
    targets = [int(ix.assignments[v]) for v in vids]
    update(ix, vids, rows_to(ix, don, targets, rng), targets, STAYED)
    for f, pf, i0 in zip(fs, pfs, info0):
        topk(c, f, pf, 40, 10, 5)
        i1 = pf.info()
        assert i1["builds"] == i0["builds"] and i1["hits"] == i0["hits"] + 1, (i0, i1)
    compare("after stays")
    info1 = [pf.info() for pf in pfs]
    # an update with a mover: one full build more, and the same results as the per-call filtered search again
    vids = usable(ix, don, np.arange(3, c.n, 29))
    targets = [other_list(ix, don, v, k, 2) if i == 4 else int(ix.assignments[v]) for i, v in enumerate(vids)]
    update(ix, vids, rows_to(ix, don, targets, rng), targets, [MOVED if i == 4 else STAYED for i in range(vids.size)])
    for f, pf, i1 in zip(fs, pfs, info1):
        topk(c, f, pf, 40, 10, 5)
        assert pf.info()["builds"] == i1["builds"] + 1, (i1, pf.info())
    compare("after a mover")
    for pf in pfs:
        pf.close()
    c.close()


# ---- derived state: |x|^2, the fp16 shadow, the two maxima -- the search oracle cannot see a wrong one, a fallback hides it ---------------
def audit(ix, Q, top_k, nprobe, qs, ever, label, tight_live=False):
    """One batched search on the matrix-core list scan with the shadow on, then for every query of `qs` what the scan dumped: every val
    inside its bound, only live rows of the probed lists, each once; the maxima between the restatement over the live rows' CURRENT values
    and the restatement over every value EVER stored (`ever`: the mirror's values plus the overwritten ones, which the mirror no longer
    holds); the results against the oracle.  tight_live (straight after compact): both maxima EQUAL the restatement over the live rows.
    -> the dict tests/test_certificate_mutation_gpu.same_vals compares"""
    metric = ix.metric
    n_ever = ix.values.shape[0]
    live = live_ids(ix)
    is_live = np.zeros(n_ever, dtype=bool); is_live[live] = True
    x_lo, x_hi = float(row_x2(ix.values[live]).max()), float(row_x2(ever).max())
    r_lo, r_hi = float(row_r2(ix.values[live]).max()), float(row_r2(ever).max())
    asg = ix.assignments.astype(np.int64)
    st0 = ix.prescan_stats()
    ids, dist, cnt = ix.search_batch(Q, top_k, nprobe)
    st1 = ix.prescan_stats()
    assert st1["batches"] > st0["batches"], "the batch did not run the matrix-core list scan"
    out = dict(fallback=st1["fallback_queries"] - st0["fallback_queries"], dumps={}, oracle={}, worst=0.0, n_vals=0, info=None)
    for qi in qs:
        vids, vals, bnd, info = testhooks.last_vals(ix, qi, cap=32768)
        assert 0 < len(vids) < 32768 and info["metric"] == metric and info["shadow"] != 0, (label, qi, info)
        v = vids.astype(np.int64)
        assert np.all(v < n_ever) and np.all(is_live[np.minimum(v, n_ever - 1)]), (label, qi, "a removed or unknown vec id was dumped")
        assert np.unique(v).size == v.size, (label, qi, "a row was dumped twice")
        cd = np.array([d_ref(c, Q[qi], metric) for c in ix.centroids], dtype=np.float32)
        assert np.all(np.isin(asg[v], np.argsort(cd, kind="stable")[:nprobe])), (label, qi, "a row of a list that was not probed")
        for vid, val, b in zip(v, vals, bnd):
            D = d_ref(ix.values[vid], Q[qi], metric)
            err = abs((1.0 + float(val) - D) if metric else (float(val) + info["qn"] - D))
            assert np.isfinite(b) and b > 0 and err <= b, (label, qi, int(vid), float(val), D, err, b)
            out["worst"] = max(out["worst"], err / b)
            out["n_vals"] += 1
        assert x_lo <= info["xmax2"] <= x_hi, (label, qi, x_lo, info["xmax2"], x_hi)
        assert r_lo <= info["r2"] <= r_hi, (label, qi, r_lo, info["r2"], r_hi)
        if tight_live:
            assert info["xmax2"] == xmax2_ref(ix.values[live]) and info["r2"] == r2_ref(ix.values[live]), (label, qi, info["xmax2"], x_lo, info["r2"], r_lo)
        oi, od = co.search_nprobe(ix.values, ix.centroids, ix.ids, Q[qi], top_k, nprobe, metric)
        assert cnt[qi] == len(oi) and np.array_equal(ids[qi, :len(oi)], oi) and np.array_equal(bits(dist[qi, :len(oi)]), bits(od)), (label, qi)
        out["dumps"][qi] = (v, bits(vals).copy())
        out["oracle"][qi] = oi.astype(np.int64)
        out["info"] = info
    print(f"metric {metric} {label:34s}: worst |val - exact| / bound = {out['worst']:.4f} over {out['n_vals']} dumped vals ({out['fallback']} of {Q.shape[0]} re-scanned)")
    assert out["n_vals"] > 0
    return out


@pytest.mark.parametrize("metric", [capi.METRIC_L2SQ, capi.METRIC_COSDIST])
def test_derived_state_after_updates(tmp_path, metric):
    n, d, k, b, nprobe, top_k = 3000, 96, 12, 64, 6, 30
    X = corpus("dist_c", n, d, 0x19C0 + metric)
    Q = corpus("dist_c", b, d, 0x19C8 + metric)
    ix = IVFFlatIndex.build_index(k, 1, 3, X, init_indices=mg.init_draws(0x19C, 1, k, n), metric=metric)
    assert ix.shadow_state()["active"]
    qs = range(0, b, 5)
    rng = np.random.default_rng(0x19C)
    ever = [ix.values.copy()]

    def twin(label, r):
        t = fresh_handle(ix, tmp_path, False)
        rt = audit(t, Q, top_k, nprobe, qs, t.values, label + " (fresh handle)")
        same_vals(r, rt, label)
        t.close()

    audit(ix, Q, top_k, nprobe, qs, np.concatenate(ever), "build")
    # stays only: new values (a list-mate's, scaled: norms and residuals change; every 7th by 3: the maxima rise), kept when the row stays
    don = donors_by_list(ix)
    cand = usable(ix, don, np.arange(1, n, 7))
    rows = rows_to(ix, don, [int(ix.assignments[v]) for v in cand], rng) * np.float32(1.03)
    rows[::7] *= np.float32(3.0)
    stay = [i for i, v in enumerate(cand) if co.add_cluster(ix.centroids, rows[i], metric) == int(ix.assignments[v])]
    assert len(stay) > 100
    cand, rows = cand[stay], rows[stay]
    update(ix, cand, rows, [int(ix.assignments[v]) for v in cand], STAYED)
    ever.append(rows.copy())
    r = audit(ix, Q, top_k, nprobe, qs, np.concatenate(ever), "stays only")
    twin("stays only", r)
    # the row that carries max |x|^2 is replaced by a small one: the maximum does not come down (an upper bound, as after a removal)
    x2 = row_x2(ix.values)
    top = np.flatnonzero(x2 == x2.max())   # (every row that attains it)
    small = (ix.values[top] * np.float32(0.25)).astype(np.float32)
    ix.update_batch(top, small)
    ever.append(small.copy())
    r = audit(ix, Q, top_k, nprobe, qs, np.concatenate(ever), "the largest row made small")
    assert r["info"]["xmax2"] == float(x2.max()) > float(row_x2(ix.values).max())
    # a mix of stays and moves
    vids = usable(ix, don, rng.choice(n, 420, replace=False))[:400]
    targets = [int(ix.assignments[v]) if i % 2 else other_list(ix, don, v, k, 1 + i % 5) for i, v in enumerate(vids)]
    rows = rows_to(ix, don, targets, rng)
    update(ix, vids, rows, targets, [STAYED if i % 2 else MOVED for i in range(vids.size)])
    ever.append(rows.copy())
    r = audit(ix, Q, top_k, nprobe, qs, np.concatenate(ever), "stays and moves")
    twin("stays and moves", r)
    check_search(ix, Q[:40], nprobes=(1, 5), top_ks=(10,))
    ix.close()


# ---- the adversarial rows of the add and compact suites, delivered by update_batch ----------------------------------------------------------
@pytest.mark.parametrize("metric", [capi.METRIC_L2SQ, capi.METRIC_COSDIST])
def test_adversarial_rows_delivered_as_stays(tmp_path, metric):
    """A row of 100 x the corpus norm and a row with an element of 7e4 (beyond fp16: its shadow residual is inf) overwrite two rows in
    place.  What the handle then does with its shadow -- retire it, or re-scan every query exactly -- is what a handle does that received
    the same two rows through add_batch; results stay the oracle's; the maxima are upper bounds until compact re-tightens them."""
    from tests.test_compact_gpu import fallbacks_of
    n, d, k, b = 3000, 96, 12, 64
    X = corpus("dist_c", n, d, 0x19E0 + metric)
    Q = corpus("dist_c", b, d, 0x19E8 + metric)
    init = mg.init_draws(0x19E, 1, k, n)
    ix = IVFFlatIndex.build_index(k, 1, 3, X, init_indices=init, metric=metric)
    by_add = IVFFlatIndex.build_index(k, 1, 3, X, init_indices=init, metric=metric)
    assert ix.shadow_state()["active"]
    _, batches, _ = fallbacks_of(ix, Q)
    assert batches == 1
    info = testhooks.last_vals(ix, 0, cap=32768)[3]
    x_fresh, r_fresh = info["xmax2"], info["r2"]
    assert x_fresh == xmax2_ref(ix.values) and r_fresh == r2_ref(ix.values)

    def stays(v, x):
        return co.add_cluster(ix.centroids, x, metric) == int(ix.assignments[v])

    def overflowing(x):
        x = x.copy(); x[3] = np.float32(7.0e4)
        return x

    home = [v for v in range(n) if stays(v, X[v])]          # (rows that can be told to stay with their ordinary value again)
    vb = next(v for v in home if stays(v, X[v] * np.float32(100.0)))
    vo = next(v for v in home if v != vb and stays(v, overflowing(X[v])))
    rows = np.stack([X[vb] * np.float32(100.0), overflowing(X[vo])]).astype(np.float32)
    targets = [int(ix.assignments[vb]), int(ix.assignments[vo])]
    update(ix, [vb, vo], rows, targets, STAYED)
    by_add.add_batch(rows)
    for _ in range(6):   # (256 queries: a shadow whose certificates fail retires itself for the handle)
        _, _, fa = fallbacks_of(ix, Q)
        _, _, ft = fallbacks_of(by_add, Q)
    assert ix.shadow_state()["active"] == by_add.shadow_state()["active"], (ix.shadow_state(), by_add.shadow_state())
    if ix.shadow_state()["active"]:
        assert fa == ft == b, (fa, ft)                       # every query re-scanned exactly
    print(f"metric {metric}: shadow active after the adversarial stays {ix.shadow_state()['active']}, re-scanned {fa} (through add: {ft}) of {b}")
    by_add.close()
    check_state(ix)
    check_search(ix, Q[:40], nprobes=(1, 5), top_ks=(10,))
    # back to ordinary values: the maxima do not come down (upper bounds)
    update(ix, [vb, vo], X[[vb, vo]], targets, STAYED)
    assert np.array_equal(bits(ix.values), bits(X))
    ix.search_batch(Q, 10, 5)
    info = testhooks.last_vals(ix, 0, cap=32768)[3]
    assert info["xmax2"] >= xmax2_ref(rows) > x_fresh, (info, x_fresh)
    if info["shadow"] != 0:   # (a scan on the f32 rows charges no residual: the hook reports 0 for it)
        assert info["r2"] >= r2_ref(rows) > r_fresh, (info, r_fresh)
    else:                     # the residual maximum stayed inf: ordinary values in every row again cure nothing, the shadow stays retired
        assert not ix.shadow_state()["active"]
    check_search(ix, Q[:40], nprobes=(5,), top_ks=(10,), exhaustive=False)
    # compact: both maxima equal the live rows', the shadow is active again, and a batch re-scans as many queries as on a fresh handle
    ix.compact()
    assert ix.shadow_state()["active"]
    _, batches, fb = fallbacks_of(ix, Q)
    info = testhooks.last_vals(ix, 0, cap=32768)[3]
    assert batches == 1 and info["shadow"] != 0
    assert info["xmax2"] == xmax2_ref(ix.values) == x_fresh and info["r2"] == r2_ref(ix.values) == r_fresh, (info, x_fresh, r_fresh)
    t = fresh_handle(ix, tmp_path, False)
    _, batches_t, fb_t = fallbacks_of(t, Q)
    assert (batches_t, fb_t) == (1, fb), (fb, fb_t)
    t.close()
    check(ix, Q[:40], nprobes=(1, 5), top_ks=(10,))
    ix.close()
