"""vers_ivf_update_batch_sharded_dev, vers_ivf_fetch_sharded_dev and vers_ivf_search_by_id_sharded_dev on handles sharded by cluster, with
real exchanges: two and three processes share the one GPU of the test box and exchange through gloo (vers_amd.dist.TorchComm /
TorchGather), the scaffold of tests/test_remove_dist_gpu.py: N = 5003, d = 96, k = 70, build_sharded_dev.  After one sharded removal
every rank makes two update calls (a mixed one with movers whose old and new owners differ and ids in no list; one in which every row
stays; ONE all_gather each), fetches every id (1 + chunks all_gathers) and searches by stored id at (nprobe, top_k) = (0, 10), (6, 10) and (6, 10) with VERS_BYID_EXCLUDE_SELF; an id in no
list is VERS_ERR_INVALID on every rank after exactly one all_gather.  The parent then makes the same calls on the unsharded index, once the
ranks have left the GPU, and every rank's outputs must equal them bit for bit; a third of the unsharded searches are pinned to the oracle."""
import datetime
import os

import numpy as np
import pytest
import torch.multiprocessing as mp

from tests.test_remove_dist_gpu import D, ITERS, K, N, free_port, ranges

pytestmark = pytest.mark.gpu

B = 40
CHUNK = 2048   # option "add_batch_rows" of the fetch: N ids travel in 3 chunks
BYID = [(0, 10, False), (6, 10, False), (6, 10, True)]


def gone_ids():
    return np.arange(2, N, 7, dtype=np.int64)


def update_calls(X):
    """(ids, rows) of the mixed call -- every third id below 900, removed ones among them, each with the row of a far-away id -- and of the
    call in which every row stays: the live ids of the first call with the rows they have just been given"""
    ids = np.arange(0, 900, 3, dtype=np.int64)
    rows = X[(ids * 37 + 1511) % N].copy()
    rows[::5] = X[ids[::5]] * np.float32(1.001)   # (every fifth keeps its direction: most of these stay)
    live = ~np.isin(ids, gone_ids())
    return (ids, rows), (ids[live][::-1].copy(), rows[live][::-1].copy())


def query_ids():
    live = np.setdiff1d(np.arange(N, dtype=np.int64), gone_ids())
    return np.random.default_rng(0x5B).permutation(live)[:B]


def worker(rank, world, port, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))
    from tests import datagen as dg
    from tests.golden import make_golden as mg
    from vers_amd import capi
    from vers_amd.dist import TorchComm, TorchGather
    from vers_amd.index import IVFFlatIndex
    cuts = ranges(world)
    lo, hi = cuts[rank], cuts[rank + 1]
    X = dg.dist_c(0xD7, N, D, 210, dg.default_sigma(D))
    init = mg.init_draws(0xD7, 1, K, N)
    Xl = torch.from_numpy(X[lo:hi]).cuda()
    comm = TorchComm(device=0)
    gather = TorchGather(device=0)
    ix = IVFFlatIndex(D, device=0)
    assert ix.build_sharded_dev(Xl.data_ptr(), hi - lo, D, lo, N, K, 1, ITERS, init, comm)
    gone = torch.from_numpy(gone_ids()).cuda()
    out = dict(own=ix.owners(), removed=ix.remove_batch_dev(gone.data_ptr(), gone.numel(), comm))
    out["lens"], out["upd"] = [ix.list_lengths().copy()], []
    for ids_u, rows_u in update_calls(X):
        iu, ru = torch.from_numpy(ids_u).cuda(), torch.from_numpy(rows_u).cuda()
        cu = torch.full((len(ids_u),), 7, dtype=torch.int64, device="cuda"); su = torch.full((len(ids_u),), 9, dtype=torch.uint8, device="cuda")
        g0 = comm.calls["all_gather"]
        counts = ix.update_batch_sharded_dev(comm, iu.data_ptr(), ru.data_ptr(), len(ids_u), D, cu.data_ptr(), su.data_ptr())
        torch.cuda.synchronize()
        out["upd"].append((cu.cpu().numpy().view(np.uint64), su.cpu().numpy(), counts, comm.calls["all_gather"] - g0))
        out["lens"].append(ix.list_lengths().copy())
    out["lists"] = {int(c): ix.get_list(int(c)) for c in range(K) if out["own"][c] == rank}
    # every id, rows at a pitch above d whose padding keeps its sentinel
    capi.set_option("add_batch_rows", CHUNK)
    ld = D + 4
    ids = torch.arange(N, dtype=torch.int64, device="cuda")
    rows = torch.full((N, ld), -7.0, device="cuda")
    cl = torch.full((N,), 9, dtype=torch.int64, device="cuda")
    st = torch.full((N,), 5, dtype=torch.uint8, device="cuda")
    g0 = comm.calls["all_gather"]
    out["counts"] = ix.fetch_sharded_dev(comm, ids.data_ptr(), N, rows.data_ptr(), ld, cl.data_ptr(), st.data_ptr())
    out["fetch_gathers"] = comm.calls["all_gather"] - g0
    capi.set_option("add_batch_rows", 131072)
    torch.cuda.synchronize()
    out["rows"], out["cl"], out["st"] = rows.cpu().numpy().view(np.uint32), cl.cpu().numpy().view(np.uint64), st.cpu().numpy()
    # search by stored id
    qd = torch.from_numpy(query_ids()).cuda()
    res = {}
    for nprobe, top_k, ex in BYID:
        si = torch.zeros(B, top_k, dtype=torch.int64, device="cuda"); sd = torch.zeros(B, top_k, device="cuda")
        sc = torch.zeros(B, dtype=torch.int32, device="cuda")
        ix.search_by_id_sharded_dev(comm, gather.ptr(), qd.data_ptr(), B, top_k, nprobe, si.data_ptr(), sd.data_ptr(), sc.data_ptr(), exclude_self=ex)
        ix.poll(); torch.cuda.synchronize()
        res[(nprobe, top_k, ex)] = (si.cpu().numpy().astype(np.uint64), sd.cpu().numpy().view(np.uint32), sc.cpu().numpy())
    out["res"] = res
    # an id in no list among the queries: the same verdict on every rank after exactly one all_gather, nothing written
    bad = query_ids().copy(); bad[7] = 2
    bd = torch.from_numpy(bad).cuda()
    si = torch.full((B, 10), -3, dtype=torch.int64, device="cuda"); sd = torch.full((B, 10), -2.0, device="cuda")
    sc = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    g0 = comm.calls["all_gather"]
    try:
        ix.search_by_id_sharded_dev(comm, gather.ptr(), bd.data_ptr(), B, 10, 6, si.data_ptr(), sd.data_ptr(), sc.data_ptr())
        out["missing"] = "ok"
    except capi.VersError as e:
        torch.cuda.synchronize()
        out["missing"] = (e.status, comm.calls["all_gather"] - g0, bool((si == -3).all()) and bool((sd == -2.0).all()) and bool((sc == -1).all()))
    ret[rank] = out
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_fetch_and_search_by_id_equal_the_unsharded_index(world):
    from oracle import c_oracle as co
    from tests import datagen as dg
    from tests.golden import make_golden as mg
    from vers_amd import capi
    from vers_amd.index import IVFFlatIndex
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(worker, args=(world, free_port(), ret), nprocs=world, join=True)
    X = dg.dist_c(0xD7, N, D, 210, dg.default_sigma(D))
    whole = IVFFlatIndex.build_index(K, 1, ITERS, X, init_indices=mg.init_draws(0xD7, 1, K, N))
    lens0 = whole.list_lengths().copy()
    removed = whole.remove_batch(gone_ids())
    owner = capi.shard_plan(lens0, world)
    lens, upd = [whole.list_lengths().copy()], []
    for j, (ids_u, rows_u) in enumerate(update_calls(X)):
        old = whole.assignments[ids_u].astype(np.int64)
        ucl, ust = whole.update_batch(ids_u, rows_u)
        upd.append((ucl, ust, whole.last_update_counts[:3]))
        lens.append(whole.list_lengths().copy())
        if j == 0:   # movers whose old and new owners differ, stays and ids in no list in ONE call
            mv = ust == 1
            assert (owner[old[mv]] != owner[ucl[mv].astype(np.int64)]).any() and (ust == 0).any() and (ust == 2).any()
        else:
            assert (ust == 0).all()
    rows, cl, st = whole.fetch(np.arange(N), row_stride_floats=D + 4, fill=np.float32(-7.0))
    counts = whole.last_fetch_counts
    assert counts == (N - removed, removed)
    X = whole.values   # (the queries below are the UPDATED stored vectors)
    qids = query_ids()
    want = {}
    for nprobe, top_k, ex in BYID:
        wi, wd, wc = whole.search_by_id(qids, top_k, nprobe, exclude_self=ex)
        if not ex:   # the search by id is the search with the stored vector: a third of the queries against the oracle
            for q in range(0, B, 3):
                oi, od = (co.search_approximate(X, whole.centroids, whole.ids, X[qids[q]], top_k) if nprobe == 0 else
                          co.search_nprobe(X, whole.centroids, whole.ids, X[qids[q]], top_k, nprobe))
                assert wc[q] == len(oi) and np.array_equal(wi[q, :len(oi)], oi) and np.array_equal(wd[q, :len(oi)].view(np.uint32), od.view(np.uint32))
        want[(nprobe, top_k, ex)] = (wi, wd.view(np.uint32), wc)
    chunks = (N + CHUNK - 1) // CHUNK
    for r in range(world):
        g = ret[r]
        assert np.array_equal(g["own"], owner) and g["removed"] == removed, r
        for j, (ucl, ust, ucounts) in enumerate(upd):
            gcl, gst, gcounts, gathers = g["upd"][j]
            assert np.array_equal(gcl, ucl) and np.array_equal(gst, ust) and tuple(gcounts[:3]) == tuple(ucounts), (r, j, gcounts, ucounts)
            assert gathers == 1 and gcounts[3] in (0, 1), (r, j, gathers)                 # ONE exchange per update call
        for j in range(3):
            assert np.array_equal(g["lens"][j], lens[j]), (r, j, "global lengths")
        assert set(g["lists"]) == {c for c in range(K) if owner[c] == r}
        for c, (lrows, lids) in g["lists"].items():                                      # the owned lists: ascending ids, the updated row bits
            assert np.array_equal(lids, np.asarray(whole.ids[c], dtype=np.uint64)), (r, c)
            assert np.array_equal(lrows.view(np.uint32), whole.values[lids.astype(np.int64)].view(np.uint32)), (r, c)
        assert g["counts"] == counts and g["fetch_gathers"] == 1 + chunks, (r, g["counts"], g["fetch_gathers"])
        assert np.array_equal(g["rows"], rows.view(np.uint32)), (r, "rows and their padding")
        assert np.array_equal(g["cl"], cl) and np.array_equal(g["st"], st), r
        for key, (wi, wd, wc) in want.items():
            gi, gd, gc = g["res"][key]
            assert np.array_equal(gc, wc), (r, key)
            for q in range(B):
                c = int(wc[q])
                assert np.array_equal(gi[q, :c], wi[q, :c]) and np.array_equal(gd[q, :c], wd[q, :c]), (r, key, q)
        assert g["missing"] == (capi.ERR_INVALID, 1, True), (r, g["missing"])
    whole.close()
