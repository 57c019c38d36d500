"""vers_ivf_fetch_sharded_dev, emulated on ONE GPU: `world` handles each keep only their lists (tests/test_range_shard_gpu.py's Case /
reshard), and every rank's all_gather is ANSWERED from tables computed on the host from the unsharded index and owners() -- the where
table ([world][n + 1] u32: the cluster on the owner, 0xFFFFFFFF elsewhere, the status word) and every row chunk ([world][pad][d] f32, the
found rows packed in request order, zeros behind a shorter rank).  What the rank SENT must be its own row of each table, the number of
callbacks 1 + (non-empty chunks), and what it returns must be what fetch_dev returns on the unsharded index: rows (bits), clusters, status,
counts, with the padding of a wider output pitch untouched.  N = 3000, d = 40 (ld is padded), k = 24; worlds 2 and 3 built per rank, 1, 5
and 30 (ranks that own no list) resharded; after a removal of ~700 ids, two adds and an update."""
import ctypes as C

import numpy as np
import pytest

from tests import datagen as dg
from tests.test_fetch_gpu import GUARD, fetch_dev, round_up
from tests.test_range_shard_gpu import Case, dev_i64, reshard
from vers_amd import capi
from vers_amd.dist import _AG, VersComm, _Mem

pytestmark = pytest.mark.gpu

N, D, K = 3000, 40, 24
NONE = 0xFFFFFFFF


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


class Answered:
    """a vers_comm_t whose all_gather is answered from a list of prepared tables ([world, bytes] u8 each); returns 1 on any surprise"""

    def __init__(self, rank, world):
        self.rank, self.world = rank, world
        self.answers, self.sent, self.calls = [], [], 0
        self._cb = _AG(self._all_gather)
        self.struct = VersComm(None, rank, world, self._cb)

    def ptr(self):
        return C.byref(self.struct)

    def expect(self, answers):
        self.answers, self.sent, self.calls = list(answers), [], 0

    def _all_gather(self, _ctx, send_ptr, recv_ptr, nbytes):
        import torch
        try:
            i = self.calls
            self.calls += 1
            if i >= len(self.answers) or self.answers[i].shape != (self.world, nbytes):
                return 1
            self.sent.append(torch.as_tensor(_Mem(send_ptr, nbytes), device="cuda").cpu().numpy().copy())
            torch.as_tensor(_Mem(recv_ptr, nbytes * self.world), device="cuda").copy_(torch.from_numpy(self.answers[i].reshape(-1).copy()))
            torch.cuda.synchronize()
            return 0
        except Exception:   # never unwind through the C frame
            return 1


def in_list(whole):
    m = np.zeros(len(whole.assignments), dtype=bool)
    for lst in whole.ids:
        m[np.asarray(lst, dtype=np.int64)] = True
    return m


def tables(whole, owners, world, ids, R, want_rows):
    """the answers of one call, from the host fields of the unsharded index: [where table] + [a table per non-empty chunk]"""
    ids = np.asarray(ids, dtype=np.int64)
    n = ids.size
    ok = in_list(whole)[ids] if n else np.zeros(0, dtype=bool)
    cl = whole.assignments[ids].astype(np.int64) if n else np.zeros(0, dtype=np.int64)
    who = np.where(ok, owners[cl].astype(np.int64), -1) if n else np.zeros(0, dtype=np.int64)
    where = np.full((world, n + 1), NONE, dtype=np.uint32)
    where[:, n] = 0
    where[who[ok], np.nonzero(ok)[0]] = cl[ok]
    out = [where.view(np.uint8).reshape(world, -1)]
    if want_rows:
        for i0 in range(0, n, R):
            sl = np.arange(i0, min(n, i0 + R))
            per = [sl[who[sl] == r] for r in range(world)]
            pad = max(p.size for p in per)
            if pad == 0:
                continue
            buf = np.zeros((world, pad, whole.d), dtype=np.float32)
            for r in range(world):
                buf[r, :per[r].size] = whole.values[ids[per[r]]]
            out.append(buf.view(np.uint8).reshape(world, -1))
    return out


def fetch_sharded(ix, comm, ids, pad=3, rows=True, clusters=True, status=True):
    """the sharded call on sentinel-filled outputs -> (rows [n, ld], clusters, status, counts)"""
    import torch
    n, ld = len(ids), round_up(ix.d + pad, 4)
    idd = torch.from_numpy(np.asarray(ids, dtype=np.uint64).view(np.int64).copy()).cuda()
    R = torch.full((max(n, 1), ld), float(GUARD), dtype=torch.float32, device="cuda")
    Cl = torch.full((max(n, 1),), 9, dtype=torch.int64, device="cuda")
    St = torch.full((max(n, 1),), 5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    try:
        counts = ix.fetch_sharded_dev(comm, idd.data_ptr(), n, R.data_ptr() if rows else 0, ld, Cl.data_ptr() if clusters else 0, St.data_ptr() if status else 0)
    finally:
        torch.cuda.synchronize()
        fetch_sharded.last = (R.cpu().numpy()[:n], Cl.cpu().numpy().view(np.uint64)[:n], St.cpu().numpy()[:n])
    return fetch_sharded.last + (counts,)


def untouched(n):
    rows, cl, st = fetch_sharded.last
    return bool((rows == GUARD).all()) and bool((cl == 9).all()) and bool((st == 5).all())


def check_request(whole, shards, owners, ids, what, R=131072, rows=True, clusters=True, status=True):
    world = len(shards)
    want = fetch_dev(whole, ids, rows=rows, clusters=clusters, status=status)
    answers = tables(whole, owners, world, ids, R, rows)
    assert rows or len(answers) == 1   # membership only: the where round alone
    for r, ix in enumerate(shards):
        comm = Answered(r, world)
        comm.expect(answers)
        got = fetch_sharded(ix, comm, ids, rows=rows, clusters=clusters, status=status)
        assert comm.calls == len(answers) == len(comm.sent), (what, r, "callbacks", comm.calls, len(answers))
        for t, a in enumerate(answers):
            assert np.array_equal(comm.sent[t], a[r]), (what, r, "the rank did not send its own row of table", t)
        assert np.array_equal(bits(got[0]), bits(want[0])), (what, r, "rows and their padding")
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]) and got[3] == want[3], (what, r, "clusters / status / counts")
    return len(answers)


def requests(whole, gone, seed):
    n = len(whole.assignments)
    rng = np.random.default_rng(seed)
    live = np.nonzero(in_list(whole))[0]
    yield "every id", np.arange(n, dtype=np.uint64)
    yield "shuffled with repeats", rng.integers(0, n, size=n // 3 + 37).astype(np.uint64)
    yield "only removed ids", rng.permutation(gone)[:150].astype(np.uint64)
    # chunks of 64: two of live ids, one of removed ids alone (skipped), a ragged last one
    yield "a chunk of removed ids alone", np.concatenate([rng.permutation(live)[:128], gone[:64], rng.permutation(live)[:41], gone[64:70]]).astype(np.uint64)


def all_checks(whole, shards, owners, gone, what):
    for name, ids in requests(whole, gone, 0xF37C):
        n_default = check_request(whole, shards, owners, ids, (what, name))
        assert n_default == (2 if in_list(whole)[ids.astype(np.int64)].any() else 1)
        capi.set_option("add_batch_rows", 64)
        try:
            n_small = check_request(whole, shards, owners, ids, (what, name, "chunks of 64"), R=64)
        finally:
            capi.set_option("add_batch_rows", 131072)
        if name == "a chunk of removed ids alone":
            assert n_small == 1 + 3   # chunks 0, 1 and 3; chunk 2 holds removed ids only
        if name == "every id":
            assert n_small > 40
    ids = np.arange(0, len(whole.assignments), 7, dtype=np.uint64)
    check_request(whole, shards, owners, ids, (what, "rows only"), clusters=False, status=False)
    assert check_request(whole, shards, owners, ids, (what, "membership only"), rows=False) == 1
    for r, ix in enumerate(shards):   # n = 0: no callback at all
        comm = Answered(r, len(shards))
        assert fetch_sharded(ix, comm, np.zeros(0, dtype=np.uint64))[3] == (0, 0) and comm.calls == 0


def replay_removal(case, gone):
    """test_range_shard_gpu.py::test_after_remove_and_compact: the sharded removal's one exchange answered from the unsharded index"""
    import torch
    whole, world, k = case.whole, case.world, case.k
    before = whole.list_lengths().astype(np.int64)
    removed = whole.remove_batch(gone)
    per_list = before - whole.list_lengths().astype(np.int64)
    table = np.zeros((world, k), dtype=np.uint32)
    for c in range(k):
        table[int(case.owners[c]), c] = per_list[c]
    gd = dev_i64(gone)
    for r, ix in enumerate(case.shards):
        comm = Answered(r, world)
        comm.expect([table.view(np.uint8).reshape(world, -1)])
        assert ix.remove_batch_dev(gd.data_ptr(), gone.size, comm) == removed and comm.calls == 1
        assert np.array_equal(ix.list_lengths(), whole.list_lengths())
    torch.cuda.synchronize()


def reshard_live(whole, world):
    """reshard() uploads EVERY row with its assignment, removed ones too: the ids in no list of `whole` are removed from every shard again"""
    shards = reshard(whole, world)
    dead = np.nonzero(~in_list(whole))[0].astype(np.int64)
    owners = shards[0].owners() if world > 1 else np.zeros(K, dtype=np.uint8)
    per_list = np.bincount(whole.assignments[dead].astype(np.int64), minlength=K)
    table = np.zeros((world, K), dtype=np.uint32)
    for c in range(K):
        table[int(owners[c]), c] = per_list[c]
    gd = dev_i64(dead)
    for r, ix in enumerate(shards):
        comm = Answered(r, world) if world > 1 else None
        if comm is not None:
            comm.expect([table.view(np.uint8).reshape(world, -1)])
        assert ix.remove_batch_dev(gd.data_ptr(), dead.size, comm) == dead.size
        assert np.array_equal(ix.list_lengths(), whole.list_lengths())
    return shards, owners


@pytest.fixture(scope="module")
def state():
    """world -> (whole, shards, owners, gone): 2 and 3 built per rank, with the removal replayed through the sharded call"""
    rng = np.random.default_rng(0x77)
    gone = np.unique(rng.integers(0, N, 700)).astype(np.uint64)
    cases = {w: Case(N, D, K, w, 0x51, built_per_rank=True) for w in (2, 3)}
    for c in cases.values():
        replay_removal(c, gone)
    yield cases, gone
    for c in cases.values():
        c.close()


@pytest.mark.parametrize("world", [2, 3])
def test_shards_built_per_rank_after_a_removal_and_two_adds(state, world):
    cases, gone = state
    c = cases[world]
    assert len({int(o) for o in c.owners}) == world
    all_checks(c.whole, c.shards, c.owners, gone, ("built per rank", world))


@pytest.fixture(scope="module")
def updated(state):
    """the unsharded index of the cases above after an update with movers (replayed on shards by re-sharding)"""
    cases, gone = state
    whole = cases[3].whole
    rng = np.random.default_rng(0x99)
    v = rng.permutation(len(whole.assignments))[:400].astype(np.uint64)   # live and removed ids
    _, st = whole.update_batch(v, dg.dist_u(0xABC, v.size, D))
    assert (st == 1).any() and (st == 2).any()
    return whole, gone


@pytest.mark.parametrize("world", [1, 2, 3, 5, 30])
def test_resharded_after_an_update(updated, world):
    whole, gone = updated
    shards, owners = reshard_live(whole, world)
    try:
        if world == 30:
            assert len({int(o) for o in owners}) < world   # ranks that own no list
        all_checks(whole, shards, owners, gone, ("resharded", world))
    finally:
        for ix in shards:
            ix.close()


@pytest.mark.parametrize("source", ["rowmajor0", "fetch_map0"])
def test_both_local_sources_and_the_per_call_table(updated, source):
    whole, gone = updated
    opt, off, on = ("rowmajor", 0, -1) if source == "rowmajor0" else ("fetch_map", 0, 1)
    capi.set_option(opt, off)
    try:
        shards, owners = reshard_live(whole, 3)
        try:
            assert source != "rowmajor0" or all(ix.layout_bytes()["rowmajor"] == 0 for ix in shards)   # the tiles serve the packing
            all_checks(whole, shards, owners, gone, (source,))
        finally:
            for ix in shards:
                ix.close()
    finally:
        capi.set_option(opt, on)


def test_refusals_leave_the_outputs_untouched(state):
    cases, gone = state
    c = cases[2]   # (its unsharded index is not the one the update above went to)
    whole, owners, world = c.whole, c.owners, 2
    n = len(whole.assignments)
    ids = np.arange(0, 300, dtype=np.uint64)
    good = tables(whole, owners, world, ids, 131072, True)
    ix = c.shards[1]

    def refused(comm, req, status, calls):
        with pytest.raises(capi.VersError) as e:
            fetch_sharded(ix, comm, req)
        assert e.value.status == status and untouched(len(req))
        assert comm is None or comm.calls == calls

    comm = Answered(1, world); comm.expect(good)
    bad = ids.copy(); bad[17] = n
    refused(comm, bad, capi.ERR_INVALID, 0)             # an id >= n: decided before any exchange
    refused(None, ids, capi.ERR_INVALID, 0)             # NULL comm on a shard
    comm = Answered(0, world); comm.expect(good)
    refused(comm, ids, capi.ERR_INVALID, 0)             # a comm of the wrong rank
    comm = Answered(1, 4); comm.expect(good)
    refused(comm, ids, capi.ERR_INVALID, 0)             # ... of the wrong world
    poisoned = [good[0].copy()] + good[1:]
    poisoned[0].view(np.uint32).reshape(world, -1)[0, ids.size] = capi.ERR_HIP
    comm = Answered(1, world); comm.expect(poisoned)
    refused(comm, ids, capi.ERR_HIP, 1)                 # another rank's status word: that status, no second callback
    double = [good[0].copy()] + good[1:]
    w = double[0].view(np.uint32).reshape(world, -1)
    i = int(np.nonzero(w[0, :ids.size] != NONE)[0][0])
    w[1, i] = w[0, i]
    comm = Answered(1, world); comm.expect(double)
    refused(comm, ids, capi.ERR_HIP, 1)                 # an id claimed by two ranks
    capi.set_option("test_fail_sharded", 1)             # a local failure: this rank's status word says so, and it is the verdict
    comm = Answered(1, world)
    mine_failed = good[0].copy()
    mw = mine_failed.view(np.uint32).reshape(world, -1)
    mw[1, :ids.size] = NONE; mw[1, ids.size] = capi.ERR_HIP
    comm.expect([mine_failed])
    refused(comm, ids, capi.ERR_HIP, 1)
    assert np.array_equal(comm.sent[0], mine_failed[1])
    comm = Answered(1, world); comm.expect(good)        # and the handle serves the next call
    got = fetch_sharded(ix, comm, ids)
    want = fetch_dev(whole, ids)
    assert np.array_equal(bits(got[0]), bits(want[0])) and got[3] == want[3]
