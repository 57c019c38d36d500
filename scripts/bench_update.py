"""Update (vers_ivf_update_batch_dev): milliseconds per call and microseconds per updated vector at m = 1 / 4,096 / 65,536 / 1 % of N
distinct random ids, each three ways -- every row stays in its list, every row moves to another list, 10 % move -- split by phase
(vers_update_phases), next to two yardsticks taken IN THE SAME RUN on the same index: vers_ivf_remove_batch_dev of the same ids (the first
half of what a caller had to do before, and the part DESIGN.md section 6 measures) and a full vers_ivf_upload_dev.

Default index: N = 1M, d = 128, nlist = 1024; `--rows 10000000 --d 768 --nlist 4096` is cfg3.  The rows of an update are values the
corpus already holds: the first-minimum centroid of X[u] is known once every row has been updated with its own value (the un-timed
"settle" call: after it every row lies in the list of its own first-minimum centroid, out_clusters says which), so X[u] of a list-mate
stays and X[u] of another list's row moves, with no tuning.  A sample of lists is checked bit for bit (ids ascending, rows) after every
call.  Prints the takes to stderr and ONE JSON line to stdout; exit status 1 when a check fails.

    python scripts/bench_update.py
    python scripts/bench_update.py --sizes 65536 --ways stay      # one call (e.g. under rocprofv3 --kernel-trace --stats)
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--kmeans-iters", type=int, default=4)
    ap.add_argument("--modes-per-list", type=int, default=16)
    ap.add_argument("--sizes", default="1,4096,65536,1%")
    ap.add_argument("--ways", default="stay,move,mix")
    ap.add_argument("--takes", type=int, default=2)
    ap.add_argument("--check-lists", type=int, default=12)
    ap.add_argument("--no-reupload", action="store_true")
    ap.add_argument("--shards", type=int, default=0, help="W ranks emulated on this GPU: vers_ivf_update_batch_sharded_dev, time outside the (answered) callback")
    args = ap.parse_args()

    import torch
    from tests import datagen as dg
    from vers_amd import capi
    from vers_amd.index import IVFFlatIndex

    torch.cuda.set_device(0)
    n, d, nlist = args.rows, args.d, args.nlist
    ld = (d + 3) // 4 * 4
    n_modes = max(1, args.modes_per_list * nlist)
    X = torch.empty(n, ld, dtype=torch.float32, device="cuda")
    capi.gen_rows_dev(X.data_ptr(), n, d, ld, 1, 0x5EED0001, 0x5EEDC0DE, n_modes, float(dg.default_sigma(d)))   # bench.py's corpus
    init = (dg.mix64(np.uint64(0xB01D) + np.arange(nlist, dtype=np.uint64)) % np.uint64(n)).astype(np.uint64)
    index = IVFFlatIndex(d)
    t0 = time.perf_counter()
    assert index.build_dev(X.data_ptr(), n, nlist, 1, args.kmeans_iters, init, want_fields=True)
    t_build = time.perf_counter() - t0
    log(f"[bench_update] index N={n} d={d} nlist={nlist} built in {t_build:.2f} s")

    def call(ids, src):
        """values[ids[i]] = X[src[i]] -> (wall ms, clusters, status, counts)"""
        m = ids.size
        ids_d = torch.from_numpy(ids.astype(np.int64)).cuda()
        rows_d = X[torch.from_numpy(src.astype(np.int64)).cuda()].contiguous()
        cl_d = torch.zeros(m, dtype=torch.int64, device="cuda")
        st_d = torch.zeros(m, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        counts = index.update_batch_dev(ids_d.data_ptr(), rows_d.data_ptr(), m, ld, cl_d.data_ptr(), st_d.data_ptr())
        wall = (time.perf_counter() - t0) * 1e3
        return wall, cl_d.cpu().numpy(), st_d.cpu().numpy(), counts

    # settle: every row to the list of its own first-minimum centroid; own[u] = that list, a function of the value X[u] alone
    every = np.arange(n, dtype=np.int64)
    capi.update_phases(reset=True)
    ms, own, st, counts = call(every, every)
    log(f"[bench_update] settle: all {n} rows with their own values in {ms:.1f} ms: {counts} {capi.update_phases()}")
    assert counts[2] == 0 and counts[0] + counts[1] == n
    src = every.copy()                     # values[v] = X[src[v]]
    members = np.argsort(own, kind="stable")
    starts = np.concatenate([[0], np.cumsum(np.bincount(own, minlength=nlist))])
    full = np.flatnonzero(np.diff(starts) > 0)   # lists that have a donor
    alive = np.ones(n, dtype=bool)
    rng = np.random.default_rng(0x19D)

    def donor_in(lists_):
        """per entry: a random u with own[u] == that list"""
        lo, ln = starts[lists_], (starts[lists_ + 1] - starts[lists_])
        return members[lo + rng.integers(0, 1 << 62, lists_.size) % ln]

    def check_lists():
        cl = own[src]
        ok = True
        for c in np.linspace(0, nlist - 1, args.check_lists).astype(int):
            want_ids = np.flatnonzero((cl == c) & alive)
            rows, ids = index.get_list(int(c))
            ok &= np.array_equal(ids, want_ids.astype(np.uint64))
            want = X[torch.from_numpy(src[want_ids]).cuda(), :d].cpu().numpy()
            ok &= np.array_equal(rows.view(np.uint32), want.view(np.uint32))
        return bool(ok)

    sizes = [max(1, n // 100) if s.strip() == "1%" else int(s) for s in args.sizes.split(",")]
    ways = args.ways.split(",")
    perm = rng.permutation(n)
    taken = 0
    all_ok = check_lists()
    res, stay_ids = {}, {}
    keys = ("stage_ms", "assign_ms", "locate_ms", "overwrite_ms", "merge_ms", "derive_ms")
    call(perm[-64:], src[perm[-64:]])   # warm-up: first launches and the scratch
    if args.shards:
        # W ranks EMULATED on this one GPU: W handles over the settled index (vers_ivf_set_shard + vers_ivf_upload_dev), the one all_gather of a
        # call answered from the where table the unsharded index implies.  Reported per size (10 % movers): the slowest rank's time OUTSIDE
        # the callback, the bytes the exchange would carry, and the unsharded call on the same index in the same run.  The exchange itself,
        # and any run on more than one physical GPU, is NOT measured.
        from vers_amd.dist import _AG, VersComm, _Mem
        W_ = args.shards
        cent = torch.zeros(nlist, ld, dtype=torch.float32, device="cuda")
        cent[:, :d] = torch.from_numpy(np.ascontiguousarray(index.get_centroids())).cuda()
        own_d = torch.from_numpy(own.astype(np.int64)).cuda()
        shards = []
        for r in range(W_):
            sx = IVFFlatIndex(d)
            sx.set_shard(r, W_)
            sx.upload_dev(X.data_ptr(), n, ld, cent.data_ptr(), nlist, ld, own_d.data_ptr())
            shards.append(sx)
        owners = shards[0].owners().astype(np.int64)
        sharded = {}
        for m in sizes:
            ids = perm[taken:taken + m].copy()
            taken += m
            now = own[src[ids]]
            move = rng.random(m) < 0.10
            shift = 1 + rng.integers(0, max(1, full.size - 1), m)
            target = np.where(move, full[(np.searchsorted(full, now) + shift) % full.size], now)
            move &= target != now
            new_src = donor_in(target)
            table = np.full((W_, m + 1), 0xFFFFFFFF, dtype=np.uint32)
            table[:, m] = 0
            table[owners[now], np.arange(m)] = now
            ans = torch.from_numpy(table.reshape(-1).view(np.uint8).copy()).cuda()
            spent = [0.0]

            def all_gather(_ctx, send_ptr, recv_ptr, nbytes):
                try:
                    t0 = time.perf_counter()
                    if ans.numel() != nbytes * W_:
                        return 1
                    torch.as_tensor(_Mem(recv_ptr, nbytes * W_), device="cuda").copy_(ans)
                    torch.cuda.synchronize()
                    spent[0] += time.perf_counter() - t0
                    return 0
                except Exception:   # never unwind through the C frame
                    return 1

            cb = _AG(all_gather)
            ids_d = torch.from_numpy(ids.astype(np.int64)).cuda()
            rows_d = X[torch.from_numpy(new_src.astype(np.int64)).cuda()].contiguous()
            worst, ok = 0.0, True
            for r, sx in enumerate(shards):
                comm = VersComm(None, r, W_, cb)
                cl_d = torch.zeros(m, dtype=torch.int64, device="cuda"); st_d = torch.zeros(m, dtype=torch.uint8, device="cuda")
                counts4 = np.zeros(4, dtype=np.uint64)
                spent[0] = 0.0
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                capi.check(capi.lib().vers_ivf_update_batch_sharded_dev(sx._h, C.byref(comm), capi._vp(ids_d.data_ptr()), capi._vp(rows_d.data_ptr()), m, ld,
                                                                        capi._vp(cl_d.data_ptr()), capi._vp(st_d.data_ptr()), counts4.ctypes.data_as(C.POINTER(C.c_uint64))))
                worst = max(worst, (time.perf_counter() - t0 - spent[0]) * 1e3)
                ok &= np.array_equal(cl_d.cpu().numpy(), target) and np.array_equal(st_d.cpu().numpy(), move.astype(np.uint8))
            ms, cl, st, counts = call(ids, new_src)   # the unsharded call on the same index, the same rows
            ok &= np.array_equal(cl, target) and np.array_equal(st, move.astype(np.uint8))
            src[ids] = new_src
            for sx in shards:
                ok &= np.array_equal(sx.list_lengths(), index.list_lengths())
            all_ok &= bool(ok)
            sharded[str(m)] = {"slowest_rank_ms_outside_callback": round(worst, 3), "unsharded_ms": round(ms, 3), "moved": int(move.sum()),
                               "where_bytes_per_rank": 4 * (m + 1), "same_as_unsharded": bool(ok)}
            log(f"[bench_update] shards={W_} mix_{m}: {sharded[str(m)]}")
        for sx in shards:
            sx.close()
        index.close()
        print(json.dumps({"metric": f"update_batch_sharded_dev, {W_} ranks emulated on one GPU, IVFFlat N={n} d={d} nlist={nlist}", "sizes": sharded,
                          "note": "callbacks answered from the unsharded index; the exchange itself is not measured", "same_as_unsharded": bool(all_ok)}), flush=True)
        return 0 if all_ok else 1
    for m in sizes:
        for way in ways:
            for take in range(args.takes):
                assert taken + m <= n - 64
                ids = perm[taken:taken + m].copy()
                taken += m
                now = own[src[ids]]
                move = np.ones(m, bool) if way == "move" else np.zeros(m, bool) if way == "stay" else (rng.random(m) < 0.10)
                shift = 1 + rng.integers(0, max(1, full.size - 1), m)
                target = np.where(move, full[(np.searchsorted(full, now) + shift) % full.size], now)
                move &= target != now   # (a single list with donors: nothing can move)
                new_src = donor_in(target)
                capi.update_phases(reset=True)
                ms, cl, st, counts = call(ids, new_src)
                ph = capi.update_phases()
                ok = np.array_equal(cl, target) and np.array_equal(st, move.astype(np.uint8)) and counts[:3] == (int((~move).sum()), int(move.sum()), 0)
                src[ids] = new_src
                ok = bool(ok) and check_lists() and index.live_count() == int(alive.sum())
                all_ok &= ok
                key = f"{way}_{m}_take{take}"
                res[key] = {"ms": round(ms, 3), "us_per_vector": round(ms * 1e3 / m, 3), "stayed": counts[0], "moved": counts[1], "relayouts": counts[3],
                            "split_ms": {k[:-3]: round(ph[k], 3) for k in keys}, "lists_bitwise_equal": ok}
                log(f"[bench_update] {key}: {res[key]}")
                if way == ways[0] and take == 0:
                    stay_ids[m] = ids
    # yardstick 1: remove_batch_dev of the same ids as the first update call of each size
    removal = {}
    for m, ids in stay_ids.items():
        dev = torch.from_numpy(ids.astype(np.int64)).cuda()
        removed = C.c_uint64(0)
        torch.cuda.synchronize()
        capi.remove_phases(reset=True)
        t0 = time.perf_counter()
        capi.check(capi.lib().vers_ivf_remove_batch_dev(index._h, capi._vp(dev.data_ptr()), m, None, C.byref(removed)))
        ms = (time.perf_counter() - t0) * 1e3
        ph = capi.remove_phases()
        alive[ids] = False
        ok = removed.value == m and check_lists()
        all_ok &= bool(ok)
        removal[str(m)] = {"ms": round(ms, 3), "split_ms": {k[:-3]: round(ph[k], 3) for k in ("stage_ms", "mark_ms", "compact_ms", "tables_ms", "derive_ms")},
                           "lists_bitwise_equal": bool(ok)}
        log(f"[bench_update] remove_batch_dev of the same {m} ids: {removal[str(m)]}")
    # yardstick 2: the full re-upload of the index
    reupload = None
    if not args.no_reupload:
        cent = torch.from_numpy(np.ascontiguousarray(index.centroids)).cuda()
        asg_d = torch.from_numpy(index.assignments.astype(np.int64)).cuda()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        index.upload_dev(X.data_ptr(), n, ld, cent.data_ptr(), nlist, d, asg_d.data_ptr())
        torch.cuda.synchronize()
        reupload = round((time.perf_counter() - t0) * 1e3, 1)
        log(f"[bench_update] full vers_ivf_upload_dev: {reupload} ms")
    line = {"metric": f"update_batch_dev ms per call, IVFFlat N={n} d={d} nlist={nlist}", "build_s": round(t_build, 2), "calls": res,
            "remove_batch_dev_same_ids": removal, "reupload_dev_ms": reupload, "lists_bitwise_equal": bool(all_ok)}
    index.close()
    print(json.dumps(line), flush=True)
    return 0 if all_ok else 1


if __name__ == "__main__":
    sys.exit(main())
