"""Range search on handles sharded by cluster, emulated on ONE GPU the way tests/test_shard_gpu.py emulates the sharded top-k search: `world`
handles each keep only their lists; every shard's vers_ivf_range_search_partial_dev result is laid out the way the all-gather would lay it
out ([world][2][T_max], keys | ids, padded with 0xFF) and merged with vers_range_merge_dev.  The result must equal the UNSHARDED index's
range search in limits, ids and distance bits, in default and walk order -- and the oracle's nprobe search cut at dist <= r.  The same for
the exhaustive partial against range_search_exhaustive.  Every comparison is np.array_equal."""
import ctypes as C

import numpy as np
import pytest

from oracle import c_oracle as co
from tests import datagen as dg
from tests.golden import make_golden as mg
from vers_amd import capi
from vers_amd.index import IVFFlatIndex

pytestmark = pytest.mark.gpu

B = 37
INF = np.float32(np.inf)
WALK = capi.RANGE_WALK_ORDER
NPROBES = (1, 5, 24)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def dev_i64(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def reshard(whole, world):
    """`world` handles over the fields of `whole` as they are on the host (vers_ivf_upload_dev + set_shard)"""
    import torch
    n, d = whole.values.shape
    Xd = torch.from_numpy(np.ascontiguousarray(whole.values)).cuda()
    Cd = torch.from_numpy(np.ascontiguousarray(whole.centroids)).cuda()
    Ad = dev_i64(whole.assignments)
    shards = []
    for r in range(world):
        ix = IVFFlatIndex(d)
        if world > 1:
            ix.set_shard(r, world)
        ix.upload_dev(Xd.data_ptr(), n, d, Cd.data_ptr(), whole.centroids.shape[0], d, Ad.data_ptr())
        shards.append(ix)
    torch.cuda.synchronize()
    return shards


class Case:
    """An unsharded index + its shards + the queries on the device."""

    def __init__(self, n, d, k, world, seed, built_per_rank):
        import torch
        X = dg.dist_c(seed, n, d, 30, dg.default_sigma(d))
        init = mg.init_draws(9, 1, k, n)
        self.whole = IVFFlatIndex.build_index(k, 1, 4, X, init_indices=init)
        self.world, self.d, self.k = world, d, k
        extra = dg.dist_u(77, 2, d)
        if built_per_rank:   # tests/test_shard_gpu.py: the same deterministic build on every rank, each keeps its own lists; then the same adds
            self.shards = []
            for r in range(world):
                ix = IVFFlatIndex(d)
                ix.set_shard(r, world)
                cent = np.zeros((k, d), np.float32); asg = np.zeros(n, np.uint64)
                cost = C.c_float(0); kept = C.c_int32(0)
                capi.check(capi.lib().vers_ivf_build(ix._h, capi._ptr(X), n, 4 * d, k, 1, 4, capi._ptr(init), capi._ptr(cent), 4 * d,
                                                     capi._ptr(asg), C.byref(cost), C.byref(kept), None))
                assert np.array_equal(asg, self.whole.assignments)
                assert np.array_equal(ix.owners(), capi.shard_plan(self.whole.list_lengths(), world))   # dealt over the build's lengths
                self.shards.append(ix)
            for x in extra:   # every rank adds the same two vectors: only the owner stores them, everyone counts them
                c0, v0 = self.whole.add(x)
                for ix in self.shards:
                    c = C.c_uint64(0); v = C.c_uint64(0)
                    capi.check(capi.lib().vers_ivf_add(ix._h, capi._ptr(np.ascontiguousarray(x)), C.byref(c), C.byref(v)))
                    assert (c.value, v.value) == (c0, v0)
        else:
            for x in extra:
                self.whole.add(x)
            self.shards = reshard(self.whole, world)
        self.owners = self.shards[0].owners()
        self.Q = dg.dist_c(seed + 1, B, d, 30, dg.default_sigma(d)); self.Q[3] = extra[1]
        self.Qd = torch.from_numpy(self.Q).cuda()

    def close(self):
        for ix in self.shards:
            ix.close()
        self.whole.close()

    def radii(self, full, m):
        """per query the distance of its m-th result in `full` = (lims, ids, dist) of the unsharded index at radius +inf -- a radius EXACTLY
        equal to a stored distance, the <= boundary -- with one negative radius and one +inf among them"""
        lims, _, dist = full
        r = np.zeros(B, dtype=np.float32)
        for q in range(B):
            run = dist[int(lims[q]):int(lims[q + 1])]
            r[q] = run[min(m, run.size) - 1] if run.size else np.float32(1.0)
        r[5] = np.float32(-1.0); r[7] = INF
        return r

    def partials(self, rd, nprobe, flags, metric=None):
        """every shard's partial, laid out as the all-gather would: -> (buffer [world][2][t_max] on the device, rank limits [world][B + 1])"""
        import torch
        world = self.world
        lims = torch.zeros(world, B + 1, dtype=torch.int64, device="cuda")
        totals = [ix.range_search_partial_dev(self.Qd.data_ptr(), self.d, B, rd.data_ptr(), nprobe, flags, lims[r].data_ptr(), 0, 0, 0,
                                              exhaustive_metric=metric) for r, ix in enumerate(self.shards)]   # the size query
        t_max = max(totals)
        buf = torch.full((world, 2, max(t_max, 1)), -1, dtype=torch.int64, device="cuda")
        for r, ix in enumerate(self.shards):
            l2 = torch.zeros(B + 1, dtype=torch.int64, device="cuda")
            got = ix.range_search_partial_dev(self.Qd.data_ptr(), self.d, B, rd.data_ptr(), nprobe, flags, l2.data_ptr(), buf[r, 0].data_ptr(),
                                              buf[r, 1].data_ptr(), totals[r], exhaustive_metric=metric)
            assert got == totals[r] and torch.equal(l2, lims[r]) and int(l2[B]) == got
        return buf, lims, t_max

    def sharded(self, radii, nprobe, flags, metric=None):
        import torch
        rd = torch.from_numpy(np.ascontiguousarray(radii, dtype=np.float32)).cuda()
        buf, lims, t_max = self.partials(rd, nprobe, flags, metric)
        total = int(lims[:, B].sum())
        o_lims = torch.full((B + 1,), -3, dtype=torch.int64, device="cuda")
        o_ids = torch.full((total + 8,), -5, dtype=torch.int64, device="cuda")
        o_dist = torch.full((total + 8,), -7.25, dtype=torch.float32, device="cuda")
        stride = 2 * max(t_max, 1)
        IVFFlatIndex.merge_range_partials_dev(buf.data_ptr(), buf[0, 1].data_ptr(), stride, lims.data_ptr(), self.world, B, flags, o_lims.data_ptr(),
                                              o_ids.data_ptr(), o_dist.data_ptr())
        torch.cuda.synchronize()
        assert bool((o_ids[total:] == -5).all()) and bool((o_dist[total:] == -7.25).all())
        return o_lims.cpu().numpy().view(np.uint64), o_ids.cpu().numpy().view(np.uint64)[:total], o_dist.cpu().numpy()[:total]


def same(got, want, what):
    assert np.array_equal(got[0], want[0]), (what, "lims")
    assert np.array_equal(got[1], want[1]), (what, "ids")
    assert np.array_equal(bits(got[2]), bits(want[2])), (what, "distance bits")


def check_probed(case, nprobes=NPROBES, ms=(1, 10, 200), oracle=True):
    whole = case.whole
    live = whole.live_count()
    for nprobe in nprobes:
        full = whole.range_search(case.Q, INF, nprobe)
        for m in ms:
            radii = case.radii(full, m)
            for walk in (False, True):
                want = whole.range_search(case.Q, radii, nprobe, walk_order=walk)
                got = case.sharded(radii, nprobe, WALK if walk else 0)
                same(got, want, (case.world, nprobe, m, walk))
                assert want[0][6] == want[0][5] and want[0][8] - want[0][7] == full[0][8] - full[0][7]   # the negative and the infinite radius
            if oracle and m == 10:
                got = case.sharded(radii, nprobe, 0)
                for q in (0, 3, 36):
                    oi, od = co.search_nprobe(whole.values, whole.centroids, whole.ids, case.Q[q], live, nprobe)
                    keep = int(np.count_nonzero(od <= radii[q]))
                    lo, hi = int(got[0][q]), int(got[0][q + 1])
                    assert hi - lo == keep and np.array_equal(got[1][lo:hi], oi[:keep]) and np.array_equal(bits(got[2][lo:hi]), bits(od[:keep])), (nprobe, q)


def check_exhaustive(case, ms=(10, 200)):
    whole = case.whole
    for metric in (capi.METRIC_L2SQ, capi.METRIC_COSDIST):
        full = whole.range_search_exhaustive(case.Q, INF, metric)
        for m in ms:
            radii = case.radii(full, m)
            if metric == capi.METRIC_COSDIST:
                radii[5] = np.float32(-5.0)
            want = whole.range_search_exhaustive(case.Q, radii, metric)
            same(case.sharded(radii, 0, 0, metric), want, (case.world, "exhaustive", metric, m))
            assert want[0][6] == want[0][5] and want[0][8] - want[0][7] == whole.live_count()


@pytest.fixture(scope="module", params=[2, 3])
def main_case(request):
    c = Case(3000, 40, 24, request.param, 0x51, built_per_rank=True)
    yield c
    c.close()


def test_probed_partials_merge_to_the_unsharded_result(main_case):
    assert len({int(o) for o in main_case.owners}) == main_case.world   # every rank stores some list
    check_probed(main_case)


def test_exhaustive_partials_merge_to_the_unsharded_result(main_case):
    check_exhaustive(main_case)
    # storage order across ranks has no key: the exhaustive partial refuses the walk order, before it touches anything
    import torch
    rd = torch.zeros(B, device="cuda")
    lims = torch.full((B + 1,), -3, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(capi.VersError) as e:
        main_case.shards[0].range_search_partial_dev(main_case.Qd.data_ptr(), main_case.d, B, rd.data_ptr(), 0, WALK, lims.data_ptr(), 0, 0, 0,
                                                     exhaustive_metric=capi.METRIC_L2SQ)
    assert e.value.status == capi.ERR_INVALID and bool((lims == -3).all())


def test_cap_protocol_of_the_partial_call(main_case):
    """the local total exceeds cap: VERS_OK, the limits complete, keys and ids untouched"""
    import torch
    case = main_case
    rd = torch.full((B,), float("inf"), device="cuda")
    for metric in (None, capi.METRIC_L2SQ):
        ix = case.shards[0]
        lims0 = torch.zeros(B + 1, dtype=torch.int64, device="cuda")
        total = ix.range_search_partial_dev(case.Qd.data_ptr(), case.d, B, rd.data_ptr(), 5, 0, lims0.data_ptr(), 0, 0, 0, exhaustive_metric=metric)
        assert total > 1
        keys = torch.full((total,), -11, dtype=torch.int64, device="cuda"); ids = torch.full((total,), -13, dtype=torch.int64, device="cuda")
        lims = torch.full((B + 1,), -3, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        got = ix.range_search_partial_dev(case.Qd.data_ptr(), case.d, B, rd.data_ptr(), 5, 0, lims.data_ptr(), keys.data_ptr(), ids.data_ptr(), total - 1,
                                          exhaustive_metric=metric)
        assert got == total and torch.equal(lims, lims0) and int(lims[B]) == total and int(lims[0]) == 0
        assert bool((keys == -11).all()) and bool((ids == -13).all())


def test_unsharded_handle_gives_the_whole_result_as_keys(main_case):
    """world == 1: the partial of an unsharded handle, merged with itself alone, is its own range search"""
    one = Case.__new__(Case)
    one.whole, one.shards, one.world, one.d, one.k, one.Q, one.Qd = main_case.whole, [main_case.whole], 1, main_case.d, main_case.k, main_case.Q, main_case.Qd
    check_probed(one, nprobes=(5,), ms=(10,), oracle=False)
    check_exhaustive(one, ms=(10,))


def test_a_rank_that_owns_no_list():
    case = Case(600, 40, 3, 4, 0x53, built_per_rank=False)
    try:
        owned = {int(o) for o in case.owners}
        assert len(owned) < 4   # three lists, four ranks: some rank stores nothing
        check_probed(case, ms=(1, 10, 200))
        check_exhaustive(case, ms=(10,))
    finally:
        case.close()


def test_after_remove_and_compact(main_case):
    """remove_batch + compact on the unsharded index, the same removals replayed on every shard: the sharded removal's one exchange (the
    per-list removed counts, [k] u32 per rank) is answered from the unsharded index's own lengths -- every rank's part is the removed count
    of the lists it owns."""
    import torch
    from vers_amd.dist import _AG, VersComm, _Mem
    case = main_case
    whole, world, k = case.whole, case.world, case.k
    rng = np.random.default_rng(0x77)
    gone = np.unique(rng.integers(0, whole.values.shape[0], 700)).astype(np.uint64)
    before = whole.list_lengths().astype(np.int64)
    removed = whole.remove_batch(gone)
    per_list = before - whole.list_lengths().astype(np.int64)
    assert removed == gone.size == int(per_list.sum())
    table = np.zeros((world, k), dtype=np.uint32)
    for c in range(k):
        table[int(case.owners[c]), c] = per_list[c]
    seen = []

    def all_gather(_ctx, send_ptr, recv_ptr, nbytes):
        try:
            if nbytes != 4 * k:
                return 1
            seen.append(torch.as_tensor(_Mem(send_ptr, nbytes), device="cuda").cpu().numpy().view(np.uint32).copy())
            torch.as_tensor(_Mem(recv_ptr, nbytes * world), device="cuda").copy_(torch.from_numpy(table.reshape(-1).view(np.uint8)))
            torch.cuda.synchronize()
            return 0
        except Exception:   # never unwind through the C frame
            return 1

    cb = _AG(all_gather)
    gd = dev_i64(gone)
    for r, ix in enumerate(case.shards):
        comm = VersComm(None, r, world, cb)
        n_removed = C.c_uint64(0)
        capi.check(capi.lib().vers_ivf_remove_batch_dev(ix._h, capi._vp(gd.data_ptr()), gone.size, C.byref(comm), C.byref(n_removed)))
        assert n_removed.value == removed and np.array_equal(seen[-1], table[r])   # what the rank sent IS its row of the table
        assert np.array_equal(ix.list_lengths(), whole.list_lengths())
    whole.compact()
    for ix in case.shards[::2]:   # compaction is local: some ranks do, some do not
        ix.compact()
    check_probed(case, nprobes=(5,), ms=(10, 200))
    check_exhaustive(case, ms=(200,))
