"""vers_ivf_range_search_sharded_dev and its exhaustive twin on handles sharded by cluster: two and three processes share the one GPU of the
test box and exchange through gloo (vers_amd.dist.TorchComm), as tests/test_remove_dist_gpu.py does.  Every rank calls with the same
arguments; the results must be identical on all ranks and equal to the UNSHARDED index's bits, and the number of all_gather callbacks per
call is part of the contract: 2 for a normal call (counts + status, then keys | ids), 1 for the size query, for a batch without a hit and
for a call some rank fails locally (the agreement round), 0 for what is refused from the arguments."""
import os
import socket

import numpy as np
import pytest
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

N, D, K, ITERS = 5003, 96, 70, 4
B, NPROBE = 29, 6
NAN_ROW = 1234


def data():
    from tests import datagen as dg
    from tests.golden import make_golden as mg
    X = dg.dist_c(0xD7, N, D, 210, dg.default_sigma(D))
    Q = dg.dist_c(0xD9, B, D, 210, dg.default_sigma(D))
    return X, Q, mg.init_draws(0xD7, 1, K, N)


def worker(rank, world, port, ret, radii, radii_x, cent, asg):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import ctypes as C
    import datetime
    import torch
    import torch.distributed as dist
    # (a rank that left the protocol must fail its peers' collective, not park them: the callback then reports VERS_ERR_COMM)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))
    from vers_amd import capi
    from vers_amd.dist import TorchComm, VersComm
    from vers_amd.index import IVFFlatIndex
    X, Q, init = data()
    lo, hi = int(N * rank / world), int(N * (rank + 1) / world)
    Xl = torch.from_numpy(X[lo:hi]).cuda()
    comm = TorchComm(device=0)
    ix = IVFFlatIndex(D, device=0)
    assert ix.build_sharded_dev(Xl.data_ptr(), hi - lo, D, lo, N, K, 1, ITERS, init, comm)
    Qd = torch.from_numpy(Q).cuda()
    out = dict(res={}, gathers={})

    def gathers():
        return comm.calls["all_gather"]

    def call(name, handle, rd, flags, cap, metric=None, cm=comm, nprobe=NPROBE):
        """one end-to-end call into poisoned outputs -> (status, total, lims, ids, dist, all_gather callbacks it made)"""
        lims = torch.full((B + 1,), -3, dtype=torch.int64, device="cuda")
        ids = torch.full((max(cap, 1),), -5, dtype=torch.int64, device="cuda")
        dst = torch.full((max(cap, 1),), -7.25, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        g0 = gathers()
        status, total = capi.OK, -1
        try:
            if metric is None:
                total = handle.range_search_sharded_dev(cm, Qd.data_ptr(), D, B, rd.data_ptr(), nprobe, flags, lims.data_ptr(),
                                                        ids.data_ptr() if cap else 0, dst.data_ptr() if cap else 0, cap)
            else:
                total = handle.range_search_exhaustive_sharded_dev(cm, Qd.data_ptr(), D, B, rd.data_ptr(), metric, flags, lims.data_ptr(),
                                                                   ids.data_ptr() if cap else 0, dst.data_ptr() if cap else 0, cap)
        except capi.VersError as e:
            status = e.status
        torch.cuda.synchronize()
        out["res"][name] = (status, total, lims.cpu().numpy(), ids.cpu().numpy(), dst.cpu().numpy().view(np.uint32))
        out["gathers"][name] = gathers() - g0
        return total

    rd = torch.from_numpy(radii).cuda()
    rdx = torch.from_numpy(radii_x).cuda()
    none = torch.full((B,), -1.0, device="cuda")
    inf = torch.full((B,), float("inf"), device="cuda")
    # the size query, then the call proper
    t = call("size", ix, rd, 0, 0)
    call("sorted", ix, rd, 0, t)
    call("small_cap", ix, rd, 0, t - 1)                       # 0 < cap < total: no exchange of results either
    tx = call("x_size", ix, rdx, 0, 0, metric=capi.METRIC_L2SQ)
    call("x_sorted", ix, rdx, 0, tx, metric=capi.METRIC_L2SQ)
    call("x_walk", ix, rdx, capi.RANGE_WALK_ORDER, tx, metric=capi.METRIC_L2SQ)   # refused from the arguments
    call("no_hit", ix, none, 0, 64)
    # refused before any exchange: a communicator that disagrees with the handle, nprobe == 0
    call("no_comm", ix, rd, 0, t, cm=None)

    class Wrong:   # the right world, somebody else's rank
        struct = VersComm(None, (rank + 1) % world, world, *comm._cbs)

        def ptr(self):
            return C.byref(self.struct)

    call("wrong_rank", ix, rd, 0, t, cm=Wrong())
    call("nprobe0", ix, rd, 0, t, nprobe=0)
    # a local failure on ONE rank (the test hook): everyone leaves the agreement round with that rank's status
    if rank == world - 1:
        capi.set_option("test_fail_sharded", 1)
    call("injected", ix, rd, 0, t)
    # a NaN row stored on one rank only: a second sharded handle over the same fields with one row poisoned
    Xn = X.copy(); Xn[NAN_ROW, 7] = np.nan
    Xd = torch.from_numpy(Xn).cuda(); Cd = torch.from_numpy(cent).cuda(); Ad = torch.from_numpy(asg.astype(np.int64)).cuda()
    ixn = IVFFlatIndex(D, device=0)
    ixn.set_shard(rank, world)
    ixn.upload_dev(Xd.data_ptr(), N, D, Cd.data_ptr(), K, D, Ad.data_ptr())
    out["nan_owner"] = int(ixn.owners()[int(asg[NAN_ROW])])
    call("nan", ixn, inf, 0, N, nprobe=K)
    call("x_nan", ixn, inf, 0, N, metric=capi.METRIC_L2SQ)
    ixn.close()
    # and the ranks are still in step: the walk order on the first handle
    call("walk", ix, rd, capi.RANGE_WALK_ORDER, t)
    out["own"] = ix.owners()
    ret[rank] = out
    dist.barrier()
    dist.destroy_process_group()
    ix.close()


def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.fixture(scope="module")
def unsharded():
    """the unsharded index's answers, computed once for both worlds (and gone from the GPU before the ranks start)"""
    from vers_amd import capi
    from vers_amd.index import IVFFlatIndex
    X, Q, init = data()
    whole = IVFFlatIndex.build_index(K, 1, ITERS, X, init_indices=init)
    full = whole.range_search(Q, np.float32(np.inf), NPROBE)
    fullx = whole.range_search_exhaustive(Q, np.float32(np.inf))

    def mth(f, m):   # per query the distance of its m-th result: a radius exactly on a stored distance
        r = np.zeros(B, dtype=np.float32)
        for q in range(B):
            run = f[2][int(f[0][q]):int(f[0][q + 1])]
            r[q] = run[min(m, run.size) - 1]
        return r
    radii = mth(full, 40); radii[::3] = mth(full, 3)[::3]; radii[4] = np.float32(-1.0); radii[9] = np.float32(np.inf)
    radii_x = mth(fullx, 25); radii_x[4] = np.float32(-1.0)
    want = dict(sorted=whole.range_search(Q, radii, NPROBE), walk=whole.range_search(Q, radii, NPROBE, walk_order=True),
                x_sorted=whole.range_search_exhaustive(Q, radii_x, capi.METRIC_L2SQ))
    u = dict(radii=radii, radii_x=radii_x, want=want, cent=np.ascontiguousarray(whole.centroids), asg=whole.assignments.copy(),
             lens=whole.list_lengths().copy())
    whole.close()
    return u


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_range_search_equals_the_unsharded_index(world, unsharded):
    from vers_amd import capi
    u = unsharded
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(worker, args=(world, free_port(), ret, u["radii"], u["radii_x"], u["cent"], u["asg"]), nprocs=world, join=True)
    want = u["want"]
    owner = capi.shard_plan(u["lens"], world)
    untouched = lambda r: bool(np.all(r[2] == -3) and np.all(r[3] == -5) and np.all(r[4] == np.float32(-7.25).view(np.uint32)))
    for rank in range(world):
        g = ret[rank]
        res, gat = g["res"], g["gathers"]
        assert np.array_equal(g["own"], owner), rank
        for name in ("sorted", "walk", "x_sorted"):
            lims, ids, dist = want[name]
            status, total, gl, gi, gd = res[name]
            assert status == capi.OK and total == ids.size > 0, (rank, name)
            assert np.array_equal(gl.view(np.uint64), lims) and np.array_equal(gi.view(np.uint64), ids) and np.array_equal(gd, dist.view(np.uint32)), (rank, name)
            assert gat[name] == 2, (rank, name, gat[name])
        # the size query and a capacity that is too small: the global total, the limits complete, ids / distances untouched, ONE exchange
        for name, ref in (("size", "sorted"), ("small_cap", "sorted"), ("x_size", "x_sorted")):
            status, total, gl, gi, gd = res[name]
            assert status == capi.OK and total == want[ref][1].size and np.array_equal(gl.view(np.uint64), want[ref][0]), (rank, name)
            assert np.all(gi == -5) and np.all(gd == np.float32(-7.25).view(np.uint32)) and gat[name] == 1, (rank, name, gat[name])
        status, total, gl, gi, gd = res["no_hit"]
        assert status == capi.OK and total == 0 and np.all(gl == 0) and np.all(gi == -5) and gat["no_hit"] == 1, (rank, gat["no_hit"])
        for name in ("no_comm", "wrong_rank", "nprobe0", "x_walk"):   # refused from the arguments: no exchange, nothing written
            assert res[name][0] == capi.ERR_INVALID and untouched(res[name]) and gat[name] == 0, (rank, name, res[name][0], gat[name])
        # one rank fails locally: every rank returns ITS status after exactly one exchange, outputs untouched
        assert res["injected"][0] == capi.ERR_HIP and untouched(res["injected"]) and gat["injected"] == 1, (rank, res["injected"][0], gat["injected"])
        assert g["nan_owner"] == int(owner[int(u["asg"][NAN_ROW])])   # ONE rank stores the NaN row
        for name in ("nan", "x_nan"):
            assert res[name][0] == capi.ERR_NAN and untouched(res[name]) and gat[name] == 1, (rank, name, res[name][0], gat[name])
