"""vers_ivf_remove_batch_dev on handles sharded by cluster: two and three processes share the one GPU of the test box and exchange
through gloo (vers_amd.dist.TorchComm), as tests/test_dist_build_gpu.py does.  Every rank passes the same ids; a list's owner removes
its rows; ONE all_gather of the per-list removed counts per call gives every rank the same global lengths and the same count.  The
result -- list lengths, the owned lists' bits, the sharded search -- must be the unsharded index's after the same removals, which is
the oracle's on the shortened lists."""
import os
import socket

import numpy as np
import pytest
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

N, D, K, ITERS = 5003, 96, 70, 4
SEARCHES = [(0, 10), (6, 10), (0, 64), (70, 33)]


def removals():
    rng = np.random.default_rng(0x4D)
    rnd = rng.integers(0, N, 900)
    return [np.arange(2, N, 7, dtype=np.int64),                                  # scattered
            np.concatenate([rnd, rnd[:200], np.arange(2, 300, 7)]),              # random order, repeats, ids already gone
            np.arange(1500, 100, -1, dtype=np.int64)]                            # a descending range: whole stretches of many lists


def ranges(world):
    return [int(N * r / world) for r in range(world)] + [N]


def worker(rank, world, port, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import ctypes as C
    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
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
    ix = IVFFlatIndex(D, device=0)
    assert ix.build_sharded_dev(Xl.data_ptr(), hi - lo, D, lo, N, K, 1, ITERS, init, comm)
    own = ix.owners()
    lens0 = ix.list_lengths().copy()
    out = dict(own=own, lens=[lens0], removed=[], gathers=[], errors=[])
    steps = removals()
    dev = [torch.from_numpy(s.astype(np.int64)).cuda() for s in steps]
    # a sharded handle without the communicator: an error on every rank before anything is exchanged or removed
    for call in ("dev", "host"):
        removed = C.c_uint64(5)
        if call == "dev":
            rc = capi.lib().vers_ivf_remove_batch_dev(ix._h, capi._vp(dev[0].data_ptr()), len(steps[0]), None, C.byref(removed))
        else:
            host = np.ascontiguousarray(steps[0], dtype=np.uint64)
            rc = capi.lib().vers_ivf_remove_batch(ix._h, capi._ptr(host), host.size, C.byref(removed))
        out["errors"].append((rc, int(removed.value), bool(np.array_equal(ix.list_lengths(), lens0)), ix.live_count()))
    # an id >= n among valid ones: the same verdict on every rank, nothing removed, no exchange
    bad = torch.from_numpy(np.array([5, 6, N, 7], dtype=np.int64)).cuda()
    g0 = comm.calls["all_gather"]
    try:
        ix.remove_batch_dev(bad.data_ptr(), 4, comm)
        out["bad"] = "ok"
    except capi.VersError as e:
        out["bad"] = (e.status, comm.calls["all_gather"] - g0, bool(np.array_equal(ix.list_lengths(), lens0)))
    Q = dg.dist_c(0xD8, 40, D, 210, dg.default_sigma(D))
    Qd = torch.from_numpy(Q).cuda()
    gather = TorchGather(device=0)
    res = {}
    for i, s in enumerate(steps):
        g0 = comm.calls["all_gather"]
        out["removed"].append(ix.remove_batch_dev(dev[i].data_ptr(), len(s), comm))
        out["gathers"].append(comm.calls["all_gather"] - g0)
        out["lens"].append(ix.list_lengths().copy())
        out.setdefault("live", []).append(ix.live_count())
        for nprobe, top_k in SEARCHES if i == len(steps) - 1 else SEARCHES[:2]:
            si = torch.zeros(40, top_k, dtype=torch.int64, device="cuda"); sd = torch.zeros(40, top_k, device="cuda")
            sc = torch.zeros(40, dtype=torch.int32, device="cuda")
            ix.search_sharded_dev(gather.ptr(), Qd.data_ptr(), D, 40, top_k, nprobe, si.data_ptr(), sd.data_ptr(), sc.data_ptr())
            ix.poll(); torch.cuda.synchronize()
            res[(i, nprobe, top_k)] = (si.cpu().numpy().astype(np.uint64), sd.cpu().numpy().view(np.uint32), sc.cpu().numpy())
    out["lists"] = {int(c): ix.get_list(int(c)) for c in range(K) if own[c] == rank}
    out["info"] = ix.info()
    out["res"] = res
    ret[rank] = out
    dist.barrier()
    dist.destroy_process_group()


def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_removal_equals_the_unsharded_index(world):
    from oracle import c_oracle as co
    from tests import datagen as dg
    from tests.golden import make_golden as mg
    from vers_amd import capi
    from vers_amd.index import IVFFlatIndex
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(worker, args=(world, free_port(), ret), nprocs=world, join=True)
    # the unsharded index after the same removals (built once the ranks have left the GPU), itself pinned to the oracle
    X = dg.dist_c(0xD7, N, D, 210, dg.default_sigma(D))
    whole = IVFFlatIndex.build_index(K, 1, ITERS, X, init_indices=mg.init_draws(0xD7, 1, K, N))
    Q = dg.dist_c(0xD8, 40, D, 210, dg.default_sigma(D))
    steps = removals()
    lens = [whole.list_lengths().copy()]
    counts, want = [], {}
    for i, s in enumerate(steps):
        counts.append(whole.remove_batch(s))
        lens.append(whole.list_lengths().copy())
        for nprobe, top_k in SEARCHES if i == len(steps) - 1 else SEARCHES[:2]:
            wi, wd, wc = whole.search_batch(Q, top_k, nprobe)
            for q in range(0, 40, 3):
                oi, od = (co.search_approximate(X, whole.centroids, whole.ids, Q[q], top_k) if nprobe == 0 else
                          co.search_nprobe(X, whole.centroids, whole.ids, Q[q], top_k, nprobe))
                assert wc[q] == len(oi) and np.array_equal(wi[q, :len(oi)], oi) and np.array_equal(wd[q, :len(oi)].view(np.uint32), od.view(np.uint32))
            want[(i, nprobe, top_k)] = (wi, wd.view(np.uint32), wc)
    assert counts[0] == len(steps[0]) and all(c > 0 for c in counts)
    owner = capi.shard_plan(lens[0], world)
    stored = 0
    for r in range(world):
        g = ret[r]
        assert np.array_equal(g["own"], owner), r
        for rc, removed, same, live in g["errors"]:      # comm = None / the host call on a sharded handle
            assert rc == capi.ERR_INVALID and removed == 0 and same and live == N, (r, g["errors"])
        assert g["bad"] == (capi.ERR_INVALID, 0, True), (r, g["bad"])
        assert g["removed"] == counts, (r, g["removed"], counts)      # the same count on every rank: the global one
        assert g["gathers"] == [1] * len(steps), (r, g["gathers"])    # ONE exchange per call
        for i in range(len(steps) + 1):
            assert np.array_equal(g["lens"][i], lens[i]), (r, i)      # global lengths, identical on all ranks
        assert g["live"] == [int(l.sum()) for l in lens[1:]]
        assert g["info"] == whole.info() and g["info"][0] == N
        assert set(g["lists"]) == {c for c in range(K) if owner[c] == r}
        for c, (rows, ids) in g["lists"].items():                      # the owned lists: surviving rows in their order, bit for bit
            assert np.array_equal(ids, np.asarray(whole.ids[c], dtype=np.uint64)), (r, c)
            assert np.array_equal(rows.view(np.uint32), X[ids.astype(np.int64)].view(np.uint32)), (r, c)
            stored += len(ids)
        for key, (wi, wd, wc) in want.items():
            gi, gd, gc = g["res"][key]
            assert np.array_equal(gc, wc), (r, key)
            for q in range(40):
                c = int(wc[q])
                assert np.array_equal(gi[q, :c], wi[q, :c]) and np.array_equal(gd[q, :c], wd[q, :c]), (r, key, q)
    assert stored == whole.live_count()
    whole.close()
