"""vers_ivf_update_batch_sharded_dev, emulated on ONE GPU: the plans of tests/mutation_model.py (stays, movers, skipped ids, a drained and
refilled list, the crowd block that forces a re-layout) applied step by step to the unsharded handle and to the shards of worlds 2, 3
and 5 -- add / add_batch through the existing calls, remove through remove_batch_dev with the answered callback, update through the new
call with the where table ([world][n + 1] u32) predicted from the Model BEFORE the step and the sent row asserted, compact on every other
shard only, reload as a re-shard from the Model's fields.  After every step: list_lengths() on every shard equal the Model's, every
owned list (get_list) is the Model's ids and row bits, out_clusters / out_status / out_counts[0..2] equal the unsharded call's, the
sharded search (partials + vers_topk_merge_dev) and fetch_sharded_dev of every id equal the unsharded handle's, and three queries equal
the oracle's.  The all-or-nothing cases -- a duplicate id, an id >= n, a NaN row with k >= 2: the same status on every rank with 0
callbacks; a poisoned status word in the answer: that status -- leave lengths, lists and a search unchanged."""
import numpy as np
import pytest

from oracle import c_oracle as co
from tests import mutation_model as mm
from tests.test_fetch_shard_gpu import NONE, Answered, bits, fetch_sharded, tables
from tests.test_fetch_gpu import fetch_dev
from vers_amd import capi
from vers_amd.index import IVFFlatIndex

pytestmark = pytest.mark.gpu

CASES = ["n333_d33_k5_l2", "n1500_d130_k10_cos", "n900_d300_k30_l2", "n2500_d20_k300_l2"]
WORLDS = (2, 3, 5)
TOP_K = 10


def round_up(x, m):
    return (x + m - 1) // m * m


def dev(a, dtype=None):
    import torch
    a = np.ascontiguousarray(a if dtype is None else np.asarray(a, dtype=dtype))
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()


def shard_from(model, case, world):
    """`world` handles over the Model's fields (vers_ivf_set_shard + vers_ivf_upload_dev) without the ids in no list"""
    import torch
    n, d, k = len(model.assignments), case.d, case.k
    ld = round_up(d, 4)   # (the _dev calls take a pitch that is a multiple of 4 floats)
    Xp = np.zeros((n, ld), dtype=np.float32); Xp[:, :d] = model.values
    Cp = np.zeros((k, ld), dtype=np.float32); Cp[:, :d] = model.centroids
    Xd, Cd, Ad = dev(Xp), dev(Cp), dev(model.assignments, np.int64)
    dead = np.asarray([v for v in range(n) if not model.in_list(v)], dtype=np.int64)
    shards = []
    for r in range(world):
        ix = IVFFlatIndex(d, 0, case.metric)
        ix.set_shard(r, world)
        ix.upload_dev(Xd.data_ptr(), n, ld, Cd.data_ptr(), k, ld, Ad.data_ptr())
        shards.append(ix)
    torch.cuda.synchronize()
    if dead.size:
        remove_on(shards, dead, np.bincount(np.asarray(model.assignments, dtype=np.int64)[dead], minlength=k), dead.size)
    return shards


def remove_on(shards, ids, per_list, removed):
    """remove_batch_dev on every shard, its one exchange (the per-list removed counts) answered"""
    world, k = len(shards), len(per_list)
    owners = shards[0].owners()
    table = np.zeros((world, k), dtype=np.uint32)
    table[owners.astype(np.int64), np.arange(k)] = per_list
    idd = dev(ids, np.int64)
    for r, ix in enumerate(shards):
        comm = Answered(r, world)
        comm.expect([table.view(np.uint8).reshape(world, -1)])
        assert ix.remove_batch_dev(idd.data_ptr(), len(ids), comm) == removed and comm.calls == 1
        assert np.array_equal(comm.sent[0].view(np.uint32), table[r])


def where_table(model, owners, world, ids):
    n = len(ids)
    t = np.full((world, n + 1), NONE, dtype=np.uint32)
    t[:, n] = 0
    for i, v in enumerate(ids):
        if model.in_list(v):
            c = model.assignments[v]
            t[int(owners[c]), i] = c
    return t


def update_on(shards, ids, rows, table, d):
    """the new call on every shard with the answered where round -> [(clusters, status, counts, callbacks)]"""
    import torch
    world, n = len(shards), len(ids)
    ld = round_up(d + 3, 4)
    p = np.full((n, ld), np.nan, dtype=np.float32)
    p[:, :d] = rows
    rd, idd = dev(p), dev(ids, np.int64)
    out = []
    for r, ix in enumerate(shards):
        comm = Answered(r, world)
        comm.expect([table.view(np.uint8).reshape(world, -1)])
        cd = torch.full((n,), 7, dtype=torch.int64, device="cuda")
        sd = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        try:
            counts = ix.update_batch_sharded_dev(comm, idd.data_ptr(), rd.data_ptr(), n, ld, cd.data_ptr(), sd.data_ptr())
            err = None
        except capi.VersError as e:
            counts, err = None, e.status
        torch.cuda.synchronize()
        out.append(dict(cl=cd.cpu().numpy().tolist(), st=sd.cpu().numpy().tolist(), counts=counts, err=err, calls=comm.calls,
                        sent=comm.sent[0].view(np.uint32) if comm.sent else None))
    return out


def sharded_search(shards, Qd, d, b, nprobe):
    import torch
    world = len(shards)
    buf = torch.full((world, 2, b * TOP_K), -1, dtype=torch.int64, device="cuda")
    for r, ix in enumerate(shards):
        ix.search_partial_dev(Qd.data_ptr(), Qd.shape[1], b, TOP_K, nprobe, buf[r, 0].data_ptr(), buf[r, 1].data_ptr())
    oi = torch.zeros(b, TOP_K, dtype=torch.int64, device="cuda"); od = torch.zeros(b, TOP_K, device="cuda")
    oc = torch.zeros(b, dtype=torch.int32, device="cuda")
    IVFFlatIndex.merge_partials_dev(buf.data_ptr(), buf[0, 1].data_ptr(), 2 * b * TOP_K, world, b, TOP_K, nprobe, oi.data_ptr(), od.data_ptr(), oc.data_ptr())
    torch.cuda.synchronize()
    for ix in shards:
        ix.poll()
    return oi.cpu().numpy().view(np.uint64), od.cpu().numpy(), oc.cpu().numpy().view(np.uint32)


class World:
    def __init__(self, case, model, world):
        self.case, self.world = case, world
        self.shards = shard_from(model, case, world)

    def close(self):
        for ix in self.shards:
            ix.close()

    def check(self, model, whole, Q, Qd, want_search, what):
        case, shards, world = self.case, self.shards, self.world
        owners = shards[0].owners()
        lens = np.asarray(model.lens(), dtype=np.uint64)
        for r, ix in enumerate(shards):
            assert np.array_equal(ix.list_lengths(), lens), (what, r, "global list lengths")
            for c in range(case.k):
                if owners[c] != r:
                    continue
                rows, ids = ix.get_list(c)
                assert ids.tolist() == model.ids[c], (what, r, c, "owned list: ids")
                assert np.array_equal(bits(rows), bits(model.values[model.ids[c]].reshape(-1, case.d))), (what, r, c, "owned list: row bits")
        nprobe = min(4, case.k)
        gi, gd, gc = sharded_search(shards, Qd, case.d, Q.shape[0], nprobe)
        wi, wd, wc = want_search
        assert np.array_equal(gc, wc), (what, "search counts")
        for q in range(Q.shape[0]):
            c = int(wc[q])
            assert np.array_equal(gi[q, :c], wi[q, :c]) and np.array_equal(bits(gd[q, :c]), bits(wd[q, :c])), (what, "search", q)
        ids = np.arange(len(model.assignments), dtype=np.uint64)
        want = fetch_dev(whole, ids)
        answers = tables(whole, owners, world, ids, 131072, True)
        for r, ix in enumerate(shards):
            comm = Answered(r, world)
            comm.expect(answers)
            got = fetch_sharded(ix, comm, ids)
            assert comm.calls == len(answers), (what, r, "fetch callbacks")
            assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]) and got[3] == want[3], (what, r, "fetch")


def follow(whole, model):
    whole.values, whole.assignments, whole.ids = model.values.copy(), np.asarray(model.assignments, dtype=np.uint64), [list(l) for l in model.ids]


@pytest.mark.parametrize("case_id", CASES)
def test_plan_on_shards(case_id):
    import torch
    case = mm.CASES[case_id]
    X, init, ob, _ = mm.base(case)
    model = mm.fresh_model(case)
    steps = mm.plan(case)
    whole = IVFFlatIndex.build_index(case.k, 1, case.iters, X, init_indices=init, metric=case.metric)
    worlds = [World(case, model, w) for w in WORLDS]
    Q = mm.fixed_queries(case)
    Qp = np.zeros((Q.shape[0], round_up(case.d, 4)), dtype=np.float32); Qp[:, :case.d] = Q
    Qd = dev(Qp)
    nprobe = min(4, case.k)
    try:
        for si, (op, a) in enumerate(steps):
            what = (case_id, si, a["kind"])
            if op in ("add", "add_batch"):
                rows = np.asarray(a["rows"], dtype=np.float32)
                wcl, wv = mm.apply(model, (op, a))
                cl, vids = whole.add_batch(rows)
                assert cl.tolist() == wcl and vids.tolist() == wv
                for w in worlds:
                    for ix in w.shards:   # every rank adds the same rows: only the owner stores them, everyone counts them
                        cd = torch.zeros(len(rows), dtype=torch.int64, device="cuda")
                        first, added = add_padded(ix, rows, case.d, cd)
                        assert (first, added) == (wv[0], len(wv)) and cd.cpu().numpy().tolist() == wcl, what
            elif op == "remove":
                before = np.asarray(model.lens(), dtype=np.int64)
                want = mm.apply(model, (op, a))
                assert whole.remove_batch(a["ids"]) == want
                per_list = before - np.asarray(model.lens(), dtype=np.int64)
                for w in worlds:
                    remove_on(w.shards, a["ids"], per_list, want)
            elif op == "update":
                for c in a["calls"]:
                    ids, rows = c["ids"], np.asarray(c["rows"], dtype=np.float32)
                    tabs = {w.world: where_table(model, w.shards[0].owners(), w.world, ids) for w in worlds}   # BEFORE the step
                    wcl, wst, wcounts = model.update(ids, rows)
                    cl, st = whole.update_batch(ids, rows)
                    assert cl.tolist() == wcl and st.tolist() == wst and tuple(whole.last_update_counts[:3]) == wcounts
                    for w in worlds:
                        for r, got in enumerate(update_on(w.shards, ids, rows, tabs[w.world], case.d)):
                            assert got["err"] is None and got["calls"] == 1, (what, w.world, r, got["err"], got["calls"])
                            assert np.array_equal(got["sent"], tabs[w.world][r]), (what, w.world, r, "the rank did not send its own row of the where table")
                            assert got["cl"] == wcl and got["st"] == wst and tuple(got["counts"][:3]) == wcounts, (what, w.world, r, "clusters / status / counts")
                            assert got["counts"][3] in (0, 1)
            elif op == "compact":
                mm.apply(model, (op, a))
                whole.compact()
                for w in worlds:
                    for ix in w.shards[::2]:   # compaction is local: every other shard only
                        ix.compact()
            else:
                assert op == "reload"
                for w in worlds:
                    w.close()
                worlds = [World(case, model, w) for w in WORLDS]
            follow(whole, model)
            want_search = whole.search_batch(Q, TOP_K, nprobe)
            want_search = (want_search[0], want_search[1], np.asarray(want_search[2], dtype=np.uint32))
            for q in (0, Q.shape[0] // 2, Q.shape[0] - 1):
                oi, od = co.search_nprobe(model.values, model.centroids, model.ids, Q[q], TOP_K, nprobe, metric=case.metric)
                assert want_search[2][q] == len(oi) and np.array_equal(want_search[0][q, :len(oi)], oi) and np.array_equal(bits(want_search[1][q, :len(oi)]), bits(od)), (what, q)
            for w in worlds:
                w.check(model, whole, Q, Qd, want_search, what + (w.world,))
    finally:
        for w in worlds:
            w.close()
        whole.close()


def add_padded(ix, rows, d, cd):
    ld = round_up(d + 3, 4)
    p = np.full((len(rows), ld), np.nan, dtype=np.float32)
    p[:, :d] = rows
    rd = dev(p)
    return ix.add_batch_dev(rd.data_ptr(), len(rows), ld, cd.data_ptr())


def test_all_or_nothing_on_shards():
    case = mm.CASES["n1500_d130_k10_l2"]
    X, init, ob, _ = mm.base(case)
    model = mm.fresh_model(case)
    whole = IVFFlatIndex.build_index(case.k, 1, case.iters, X, init_indices=init, metric=case.metric)
    gone = list(range(5, 300, 9))
    model.remove(gone)
    whole.remove_batch(gone)
    w = World(case, model, 3)
    Q = mm.fixed_queries(case)
    Qp = np.zeros((Q.shape[0], round_up(case.d, 4)), dtype=np.float32); Qp[:, :case.d] = Q
    Qd = dev(Qp)
    want_search = whole.search_batch(Q, TOP_K, 4)
    want_search = (want_search[0], want_search[1], np.asarray(want_search[2], dtype=np.uint32))
    n = len(model.assignments)
    ids = list(range(0, 120, 3))
    rows = X[np.arange(len(ids)) * 7 % n].copy()
    owners = w.shards[0].owners()
    good = where_table(model, owners, 3, ids)
    try:
        def refused(ids_, rows_, table, status, calls):
            for r, got in enumerate(update_on(w.shards, ids_, rows_, table, case.d)):
                assert got["err"] == status and got["calls"] == calls, (r, got["err"], got["calls"])
                assert got["cl"] == [7] * len(ids_) and got["st"] == [9] * len(ids_), (r, "outputs touched")
            w.check(model, whole, Q, Qd, want_search, ("after a refusal", status, calls))

        dup = list(ids); dup[9] = dup[3]
        refused(dup, rows, where_table(model, owners, 3, dup), capi.ERR_INVALID, 0)       # a duplicate id
        big = list(ids); big[11] = n
        refused(big, rows, good, capi.ERR_INVALID, 0)                                      # an id >= n
        nan = rows.copy(); nan[17, 5] = np.nan
        refused(ids, nan, good, capi.ERR_NAN, 0)                                           # a NaN row with k >= 2
        poisoned = good.copy(); poisoned[2, len(ids)] = capi.ERR_HIP
        # a poisoned status word of rank 2 in the answer: ranks 0 and 1 return that status after the one callback (rank 2's own row says 0)
        for r in (0, 1):
            got = update_on_one(w.shards[r], r, 3, ids, rows, poisoned, case.d)
            assert got["err"] == capi.ERR_HIP and got["calls"] == 1 and got["cl"] == [7] * len(ids) and got["st"] == [9] * len(ids), (r, got["err"])
        double = good.copy()
        i = int(np.nonzero(double[0, :len(ids)] != NONE)[0][0])
        double[1, i] = double[0, i]
        got = update_on_one(w.shards[2], 2, 3, ids, rows, double, case.d)
        assert got["err"] == capi.ERR_HIP and got["calls"] == 1                           # an id claimed by two ranks
        w.check(model, whole, Q, Qd, want_search, ("after the poisoned answers",))
        # and the same call goes through afterwards
        wcl, wst, wcounts = model.update(ids, rows)
        whole.update_batch(ids, rows)
        for r, got in enumerate(update_on(w.shards, ids, rows, good, case.d)):
            assert got["err"] is None and got["cl"] == wcl and got["st"] == wst and tuple(got["counts"][:3]) == wcounts, r
        follow(whole, model)
        ws = whole.search_batch(Q, TOP_K, 4)
        w.check(model, whole, Q, Qd, (ws[0], ws[1], np.asarray(ws[2], dtype=np.uint32)), ("after the update",))
    finally:
        w.close()
        whole.close()


def update_on_one(ix, r, world, ids, rows, table, d):
    """update_on for ONE rank of `world` (the answer need not hold that rank's own row)"""
    import torch
    n = len(ids)
    ld = round_up(d + 3, 4)
    p = np.full((n, ld), np.nan, dtype=np.float32)
    p[:, :d] = rows
    rd, idd = dev(p), dev(ids, np.int64)
    comm = Answered(r, world)
    comm.expect([table.view(np.uint8).reshape(world, -1)])
    cd = torch.full((n,), 7, dtype=torch.int64, device="cuda")
    sd = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    try:
        ix.update_batch_sharded_dev(comm, idd.data_ptr(), rd.data_ptr(), n, ld, cd.data_ptr(), sd.data_ptr())
        err = None
    except capi.VersError as e:
        err = e.status
    torch.cuda.synchronize()
    return dict(cl=cd.cpu().numpy().tolist(), st=sd.cpu().numpy().tolist(), err=err, calls=comm.calls)
