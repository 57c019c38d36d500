"""vers_ivf_compact on handles sharded by cluster: compaction is purely local -- the list lengths are global already -- so it takes no
communicator and every rank may call it or not.  Two and three processes share the one GPU of the test box and exchange through gloo
(vers_amd.dist.TorchComm), as tests/test_remove_dist_gpu.py does: remove, compact, and the sharded searches must equal the unsharded
compacted index's, which is pinned to the oracle."""
import os
import socket

import numpy as np
import pytest
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

N, D, K, ITERS = 3001, 96, 24, 4
SEARCHES = [(0, 10), (5, 10), (24, 33)]


def removal():
    rng = np.random.default_rng(0xC6)
    return np.unique(np.concatenate([np.arange(2, N, 5), rng.integers(0, N, 400), np.arange(900, 400, -1)])).astype(np.int64)


def round_up(x, m):
    return (x + m - 1) // m * m


def worker(rank, world, port, who, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from tests import datagen as dg
    from tests.golden import make_golden as mg
    from vers_amd.dist import TorchComm, TorchGather
    from vers_amd.index import IVFFlatIndex
    lo, hi = int(N * rank / world), int(N * (rank + 1) / world)
    X = dg.dist_c(0xC7, N, D, 3 * K, dg.default_sigma(D))
    init = mg.init_draws(0xC7, 1, K, N)
    Xl = torch.from_numpy(X[lo:hi]).cuda()
    comm = TorchComm(device=0)
    ix = IVFFlatIndex(D, device=0)
    assert ix.build_sharded_dev(Xl.data_ptr(), hi - lo, D, lo, N, K, 1, ITERS, init, comm)
    own = ix.owners()
    gone = torch.from_numpy(removal()).cuda()
    out = dict(own=own, removed=ix.remove_batch_dev(gone.data_ptr(), gone.numel(), comm))
    calls0 = dict(comm.calls)
    out["rows_before"] = ix.layout_bytes()["rows"]
    out["compact"] = ix.compact() if who == "all" or rank == 0 else None     # no communicator: local
    out["no_exchange"] = dict(comm.calls) == calls0
    out["rows_after"] = ix.layout_bytes()["rows"]
    out["lens"] = ix.list_lengths().copy()
    out["info"], out["live"] = ix.info(), ix.live_count()
    Q = dg.dist_c(0xC8, 40, D, 3 * K, dg.default_sigma(D))
    Qd = torch.from_numpy(Q).cuda()
    gather = TorchGather(device=0)
    res = {}
    for nprobe, top_k in SEARCHES:
        si = torch.zeros(40, top_k, dtype=torch.int64, device="cuda"); sd = torch.zeros(40, top_k, device="cuda")
        sc = torch.zeros(40, dtype=torch.int32, device="cuda")
        ix.search_sharded_dev(gather.ptr(), Qd.data_ptr(), D, 40, top_k, nprobe, si.data_ptr(), sd.data_ptr(), sc.data_ptr())
        ix.poll(); torch.cuda.synchronize()
        res[(nprobe, top_k)] = (si.cpu().numpy().astype(np.uint64), sd.cpu().numpy().view(np.uint32), sc.cpu().numpy())
    out["lists"] = {int(c): ix.get_list(int(c)) for c in range(K) if own[c] == rank}
    out["res"] = res
    ret[rank] = out
    dist.barrier()
    dist.destroy_process_group()


def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.parametrize("world,who", [(2, "all"), (3, "all"), (2, "rank 0 only")])
def test_sharded_compaction_equals_the_unsharded_compacted_index(world, who):
    from oracle import c_oracle as co
    from tests import datagen as dg
    from tests.golden import make_golden as mg
    from vers_amd.index import IVFFlatIndex
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(worker, args=(world, free_port(), who, ret), nprocs=world, join=True)
    # the unsharded index after the same removal and a compaction (built once the ranks have left the GPU), itself pinned to the oracle
    X = dg.dist_c(0xC7, N, D, 3 * K, dg.default_sigma(D))
    whole = IVFFlatIndex.build_index(K, 1, ITERS, X, init_indices=mg.init_draws(0xC7, 1, K, N))
    Q = dg.dist_c(0xC8, 40, D, 3 * K, dg.default_sigma(D))
    removed = whole.remove_batch(removal())
    before, after = whole.compact()
    caps = [round_up(len(l) + max(8, len(l) // 16), 64) for l in whole.ids]
    assert after == sum(caps) < before
    want = {}
    for nprobe, top_k in SEARCHES:
        wi, wd, wc = whole.search_batch(Q, top_k, nprobe)
        for q in range(0, 40, 3):
            oi, od = (co.search_approximate(X, whole.centroids, whole.ids, Q[q], top_k) if nprobe == 0 else
                      co.search_nprobe(X, whole.centroids, whole.ids, Q[q], top_k, nprobe))
            assert wc[q] == len(oi) and np.array_equal(wi[q, :len(oi)], oi) and np.array_equal(wd[q, :len(oi)].view(np.uint32), od.view(np.uint32))
        want[(nprobe, top_k)] = (wi, wd.view(np.uint32), wc)
    stored = 0
    for r in range(world):
        g = ret[r]
        assert g["removed"] == removed and g["no_exchange"], r
        assert np.array_equal(g["lens"], whole.list_lengths()) and g["info"] == whole.info() and g["live"] == whole.live_count(), r
        mine = sum(c for j, c in enumerate(caps) if g["own"][j] == r)
        if g["compact"] is not None:      # the plan rule over the lists this rank owns; another rank's list takes no storage
            assert g["compact"][1] == mine < g["compact"][0], (r, g["compact"], mine)
            assert g["rows_after"] == g["rows_before"] // g["compact"][0] * mine
        else:
            assert g["rows_after"] == g["rows_before"], r
        for c, (rows, ids) in g["lists"].items():
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
