"""The filtered _sharded_dev calls end to end on handles sharded by cluster: two and three processes share the one GPU of the test box and
exchange through gloo (vers_amd.dist.TorchGather behind vers_gather_t for the top-k calls, TorchComm behind vers_comm_t for the range calls),
as tests/test_range_dist_gpu.py does.  Every rank calls with the same arguments and bitmaps; the results must be identical on all ranks and
equal to the UNSHARDED index's bits -- plain and adaptive depth, one bitmap per call and F = 3, top-k and range -- and the number of gathers
per call is part of the contract: top-k 1 (adaptive: 2), range 2 (the size query and a batch without a hit: 1), refused from the arguments 0.
A rank that fails locally (the library's "test_fail_sharded" hook; nothing faults on the GPU) still joins every gather."""
import os
import socket

import numpy as np
import pytest
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

N, D, K, ITERS = 5003, 96, 70, 4
B, NPROBE, TOP_K = 29, 6, 10
AD = (2, 40, 10)   # nprobe_min, nprobe_max, min_allowed


def data():
    from tests import datagen as dg
    from tests.golden import make_golden as mg
    X = dg.dist_c(0xD7, N, D, 210, dg.default_sigma(D))
    Q = dg.dist_c(0xD9, B, D, 210, dg.default_sigma(D))
    return X, Q, mg.init_draws(0xD7, 1, K, N)


def filters():
    """(words [n_filters][stride], filter_of or None) by name: one bitmap per call (2 %), and F = 3 round-robin"""
    from vers_amd import capi
    rng = np.random.default_rng(0xF11)
    r02 = rng.random(N) < 0.02
    r30 = rng.random(N) < 0.30
    span = np.zeros(N, bool); span[1000:3000] = True
    return dict(one=(capi.allowed_bitmaps([r02], N), None), f3=(capi.allowed_bitmaps([r02, r30, span], N), (np.arange(B) % 3).astype(np.uint32)))


def worker(rank, world, port, ret, radii):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import ctypes as C
    import datetime
    import torch
    import torch.distributed as dist
    # (a rank that left the protocol must fail its peers' collective, not park them)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))
    from vers_amd import capi
    from vers_amd.dist import TorchComm, TorchGather, VersComm, VersGather
    from vers_amd.index import IVFFlatIndex
    X, Q, init = data()
    lo, hi = int(N * rank / world), int(N * (rank + 1) / world)
    Xl = torch.from_numpy(X[lo:hi]).cuda()
    comm = TorchComm(device=0)
    gather = TorchGather(device=0)
    ix = IVFFlatIndex(D, device=0)
    assert ix.build_sharded_dev(Xl.data_ptr(), hi - lo, D, lo, N, K, 1, ITERS, init, comm)
    Qd = torch.from_numpy(Q).cuda()
    dev = {}
    for name, (words, fo) in filters().items():
        wd = torch.from_numpy(words.view(np.int64)).cuda()
        fod = None if fo is None else torch.from_numpy(fo.view(np.int32)).cuda()
        dev[name] = (wd, fod, (wd.data_ptr(), words.shape[1], words.shape[0], N, fod.data_ptr() if fod is not None else 0))
    out = dict(topk={}, rng={}, gathers={})

    def topk(name, f, adaptive=False, metric=None, g=gather, nprobe=NPROBE):
        ids = torch.full((B, TOP_K), -5, dtype=torch.int64, device="cuda"); dst = torch.full((B, TOP_K), -7.25, device="cuda")
        cnt = torch.full((B,), -1, dtype=torch.int32, device="cuda"); npr = torch.full((B,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        g0 = gather.calls
        call = poll = capi.OK
        try:
            if metric is None:
                ix.search_filtered_sharded_dev(g.ptr() if g is not None else None, Qd.data_ptr(), D, B, TOP_K, AD[1] if adaptive else nprobe, dev[f][2], ids.data_ptr(),
                                               dst.data_ptr(), cnt.data_ptr(), adaptive=(AD[0], AD[2], 0, npr.data_ptr()) if adaptive else None)
            else:
                ix.search_exhaustive_filtered_sharded_dev(g.ptr() if g is not None else None, Qd.data_ptr(), D, B, TOP_K, metric, dev[f][2], ids.data_ptr(), dst.data_ptr(),
                                                          cnt.data_ptr())
        except capi.VersError as e:
            call = e.status
        torch.cuda.synchronize()
        try:
            ix.poll()
        except capi.VersError as e:
            poll = e.status
        out["topk"][name] = (call, poll, ids.cpu().numpy(), dst.cpu().numpy().view(np.uint32), cnt.cpu().numpy(), npr.cpu().numpy())
        out["gathers"][name] = gather.calls - g0

    def rng(name, f, rd, flags, cap, metric=None, cm=comm, nprobe=NPROBE):
        lims = torch.full((B + 1,), -3, dtype=torch.int64, device="cuda")
        ids = torch.full((max(cap, 1),), -5, dtype=torch.int64, device="cuda"); dst = torch.full((max(cap, 1),), -7.25, device="cuda")
        torch.cuda.synchronize()
        g0 = comm.calls["all_gather"]
        status, total = capi.OK, -1
        try:
            total = ix.range_search_filtered_sharded_dev(cm, Qd.data_ptr(), D, B, rd.data_ptr(), nprobe, flags, dev[f][2], lims.data_ptr(), ids.data_ptr() if cap else 0,
                                                         dst.data_ptr() if cap else 0, cap, exhaustive_metric=metric)
        except capi.VersError as e:
            status = e.status
        torch.cuda.synchronize()
        out["rng"][name] = (status, total, lims.cpu().numpy(), ids.cpu().numpy(), dst.cpu().numpy().view(np.uint32))
        out["gathers"][name] = comm.calls["all_gather"] - g0
        return total

    class WrongGather:   # the right world, somebody else's rank
        struct = VersGather(None, (rank + 1) % world, world, gather._cb)

        def ptr(self):
            return C.cast(C.byref(self.struct), C.c_void_p)

    class WrongComm:
        struct = VersComm(None, (rank + 1) % world, world, *comm._cbs)

        def ptr(self):
            return C.byref(self.struct)

    none = torch.full((B,), -1.0, device="cuda")
    for f in ("one", "f3"):
        topk(f + "_plain", f)
        topk(f + "_adaptive", f, adaptive=True)
        topk(f + "_x", f, metric=capi.METRIC_L2SQ)
        rd = torch.from_numpy(radii[f]).cuda()
        t = rng(f + "_size", f, rd, 0, 0)
        rng(f + "_sorted", f, rd, 0, t)
        rng(f + "_walk", f, rd, capi.RANGE_WALK_ORDER, t)
        rdx = torch.from_numpy(radii[f + "_x"]).cuda()
        tx = rng(f + "_x_size", f, rdx, 0, 0, metric=capi.METRIC_L2SQ)
        rng(f + "_x_sorted", f, rdx, 0, tx, metric=capi.METRIC_L2SQ)
    rd = torch.from_numpy(radii["one"]).cuda()
    rng("no_hit", "one", none, 0, 64)
    # refused from the arguments, before any exchange
    topk("t_wrong_rank", "one", g=WrongGather())
    topk("t_no_gather", "one", g=None)
    topk("t_nprobe0", "one", nprobe=0)
    rng("r_wrong_rank", "one", rd, 0, 64, cm=WrongComm())
    rng("r_no_comm", "one", rd, 0, 64, cm=None)
    rng("r_nprobe0", "one", rd, 0, 64, nprobe=0)
    rng("r_x_walk", "one", rd, capi.RANGE_WALK_ORDER, 64, metric=capi.METRIC_L2SQ)
    # a local failure on ONE rank (the test hook): every gather still completes
    for name, kw in (("fail_plain", {}), ("fail_adaptive", dict(adaptive=True))):
        if rank == world - 1:
            capi.set_option("test_fail_sharded", 1)
        topk(name, "f3", **kw)
    if rank == world - 1:
        capi.set_option("test_fail_sharded", 1)
    rng("fail_range", "f3", rd, 0, 64)
    # and the ranks are still in step
    topk("again", "f3", adaptive=True)
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
    """the unsharded index's answers from its EXISTING filtered calls, computed once for both worlds (and gone from the GPU before the ranks start)"""
    from vers_amd import capi
    from vers_amd.index import IVFFlatIndex
    X, Q, init = data()
    whole = IVFFlatIndex.build_index(K, 1, ITERS, X, init_indices=init)
    want, radii = {}, {}

    def mth(f, m):   # per query the distance of its m-th result: a radius exactly on a stored distance
        r = np.ones(B, dtype=np.float32)
        for q in range(B):
            run = f[2][int(f[0][q]):int(f[0][q + 1])]
            if run.size:
                r[q] = run[min(m, run.size) - 1]
        return r

    for name, (words, fo) in filters().items():
        one = fo is None
        flt = (words[0], N) if one else (words, N)
        a = () if one else (fo,)
        want[name + "_plain"] = (whole.search_filtered if one else whole.search_filtered_multi)(Q, TOP_K, NPROBE, flt, *a)
        want[name + "_adaptive"] = (whole.search_filtered_adaptive if one else whole.search_filtered_multi_adaptive)(Q, TOP_K, AD[0], AD[1], AD[2], flt, *a)
        want[name + "_x"] = (whole.search_exhaustive_filtered if one else whole.search_exhaustive_filtered_multi)(Q, TOP_K, flt, *a)
        rs = whole.range_search_filtered if one else whole.range_search_filtered_multi
        rx = whole.range_search_exhaustive_filtered if one else whole.range_search_exhaustive_filtered_multi
        r = mth(rs(Q, np.float32(np.inf), NPROBE, flt, *a), 12); r[4] = np.float32(-1.0); r[9] = np.float32(np.inf)
        x = mth(rx(Q, np.float32(np.inf), flt, *a), 25); x[4] = np.float32(-1.0)
        radii[name], radii[name + "_x"] = r, x
        want[name + "_sorted"] = rs(Q, r, NPROBE, flt, *a)
        want[name + "_walk"] = rs(Q, r, NPROBE, flt, *a, walk_order=True)
        want[name + "_x_sorted"] = rx(Q, x, flt, *a)
    whole.close()
    return dict(want=want, radii=radii)


@pytest.mark.parametrize("world", [2, 3])
def test_filtered_sharded_calls_equal_the_unsharded_index(world, unsharded):
    from vers_amd import capi
    want = unsharded["want"]
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(worker, args=(world, free_port(), ret, unsharded["radii"]), nprocs=world, join=True)   # (a hang here = a rank skipped a gather)
    f32 = lambda v: np.float32(v).view(np.uint32)
    for rank in range(world):
        tk, rg, gat = ret[rank]["topk"], ret[rank]["rng"], ret[rank]["gathers"]
        for f in ("one", "f3"):
            for kind, n_gathers in (("_plain", 1), ("_adaptive", 2), ("_x", 1)):
                name = f + kind
                w = want[name]
                call, poll, ids, dst, cnt, npr = tk[name]
                assert call == capi.OK and poll == capi.OK and gat[name] == n_gathers, (rank, name, call, poll, gat[name])
                assert np.array_equal(cnt.view(np.uint32), w[2]), (rank, name)
                live = np.arange(TOP_K)[None, :] < w[2][:, None]
                assert np.array_equal(ids.view(np.uint64)[live], w[0][live]) and np.array_equal(dst[live], w[1].view(np.uint32)[live]), (rank, name)
                if kind == "_adaptive":
                    assert np.array_equal(npr.view(np.uint32), w[3]), (rank, name)
                    assert len(set(w[3].tolist())) >= 3, w[3]   # (the depths do differ between the queries)
            for kind in ("_sorted", "_walk", "_x_sorted"):
                name = f + kind
                lims, ids, dist = want[name]
                status, total, gl, gi, gd = rg[name]
                assert status == capi.OK and total == ids.size > 0 and gat[name] == 2, (rank, name, status, total, gat[name])
                assert np.array_equal(gl.view(np.uint64), lims) and np.array_equal(gi.view(np.uint64), ids) and np.array_equal(gd, dist.view(np.uint32)), (rank, name)
            for name, ref in ((f + "_size", f + "_sorted"), (f + "_x_size", f + "_x_sorted")):
                status, total, gl, gi, gd = rg[name]
                assert status == capi.OK and total == want[ref][1].size and np.array_equal(gl.view(np.uint64), want[ref][0]) and gat[name] == 1, (rank, name, gat[name])
        status, total, gl, gi, gd = rg["no_hit"]
        assert status == capi.OK and total == 0 and np.all(gl == 0) and np.all(gi == -5) and gat["no_hit"] == 1, (rank, gat["no_hit"])
        # refused from the arguments: no exchange, nothing written, nothing latched
        for name in ("t_wrong_rank", "t_no_gather", "t_nprobe0"):
            call, poll, ids, dst, cnt, npr = tk[name]
            assert call == capi.ERR_INVALID and poll == capi.OK and gat[name] == 0, (rank, name, call, poll, gat[name])
            assert np.all(ids == -5) and np.all(dst == f32(-7.25)) and np.all(cnt == -1), (rank, name)
        for name in ("r_wrong_rank", "r_no_comm", "r_nprobe0", "r_x_walk"):
            status, total, gl, gi, gd = rg[name]
            assert status == capi.ERR_INVALID and gat[name] == 0 and np.all(gl == -3) and np.all(gi == -5) and np.all(gd == f32(-7.25)), (rank, name, status, gat[name])
        # top-k, one rank fails locally: every gather completes, the failing rank returns its own error, everyone latches VERS_ERR_COMM
        failing = rank == world - 1
        for name, n_gathers in (("fail_plain", 1), ("fail_adaptive", 2)):
            call, poll = tk[name][:2]
            assert call == (capi.ERR_HIP if failing else capi.OK) and poll == capi.ERR_COMM and gat[name] == n_gathers, (rank, name, call, poll, gat[name])
        # range: every rank returns the failing rank's status after ONE gather, outputs untouched
        status, total, gl, gi, gd = rg["fail_range"]
        assert status == capi.ERR_HIP and gat["fail_range"] == 1 and np.all(gl == -3) and np.all(gi == -5) and np.all(gd == f32(-7.25)), (rank, status, gat["fail_range"])
        # still in step
        call, poll, ids, dst, cnt, npr = tk["again"]
        assert call == capi.OK and poll == capi.OK and gat["again"] == 2 and np.array_equal(npr.view(np.uint32), want["f3_adaptive"][3]), (rank, call, poll)
        assert np.array_equal(cnt.view(np.uint32), want["f3_adaptive"][2])
