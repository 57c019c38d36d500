"""Fetch (vers_ivf_fetch_dev) and search by stored id (vers_ivf_search_by_id_dev): milliseconds per call and USEFUL bytes per second (found
rows x d x 4), for both sources of the rows -- the row-major copy (default options) and the f32 tiles alone (option "rowmajor" = 0):
    all_ids_first        every id, ascending: the first call, which builds the vec id -> storage row map (map_ms is its share)
    all_ids              ... later calls
    random_1pct / random_001pct / one_id
    after_add_first      the first call after an add_batch into slack (the map takes the appended id range alone)
    after_remove_first   the first call after a remove_batch (a full rebuild of the map)
    host_all_ids         the host-pointer vers_ivf_fetch of every id: rows, clusters and status into host arrays, staged in chunks
and the crossover of the tile gather's two forms (--sweep): 1, 2, 4, 8, 16, 32 and 64 wanted rows per touched tile, timed with option
"fetch_lds_min" = 1 (every tile turned through LDS) and = 1000 (every wanted row's 16-byte pieces read directly).  T = the smallest count at
which the LDS form wins.
    by_id                vers_ivf_search_by_id_dev at b = 1 / 64 / 1024 against vers_ivf_search_dev on the same vectors already resident as
                         queries: the difference is the feature's cost

--yardsticks measures what there was BEFORE this call, with calls that exist without it: vers_ivf_recluster's gather phase (the same bytes,
tiles to row-major), k calls of vers_ivf_get_list for the whole index, and vers_ivf_search_dev at b = 1 / 64 / 1024.  --root PATH imports the
package from another checkout (the parent commit), so the yardsticks never run on the code under test.

Default index: N = 1M, d = 128, nlist = 1024; `--rows 10000000 --d 768 --nlist 4096` is cfg3.  Takes to stderr, ONE JSON line to stdout.

    python scripts/bench_fetch.py
    python scripts/bench_fetch.py --sweep --rows 200000 --d 768 --nlist 256
    python scripts/bench_fetch.py --yardsticks --root /path/to/parent/checkout
    python scripts/bench_fetch.py --shards 4      (vers_ivf_fetch_sharded_dev, the ranks emulated on this GPU; the exchange is not measured)
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--kmeans-iters", type=int, default=2)
    ap.add_argument("--takes", type=int, default=3)
    ap.add_argument("--sweep", action="store_true", help="the crossover of the tile gather's two forms only")
    ap.add_argument("--shards", type=int, default=0, help="W ranks emulated on this GPU: vers_ivf_fetch_sharded_dev, time outside the (answered) callbacks")
    ap.add_argument("--yardsticks", action="store_true", help="the calls that existed before fetch, only")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="the checkout to import vers_amd and tests from")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))

    import torch
    from tests import datagen as dg
    from vers_amd import capi
    from vers_amd.index import IVFFlatIndex

    torch.cuda.set_device(0)
    n, d, nlist = args.rows, args.d, args.nlist
    ld = (d + 3) // 4 * 4
    extra = 1000
    X = torch.empty(n + extra, ld, dtype=torch.float32, device="cuda")
    capi.gen_rows_dev(X.data_ptr(), n + extra, d, ld, 1, 0x5EED0001, 0x5EEDC0DE, max(1, 16 * nlist), float(dg.default_sigma(d)))   # bench.py's corpus
    init = (dg.mix64(np.uint64(0xB01D) + np.arange(nlist, dtype=np.uint64)) % np.uint64(n)).astype(np.uint64)
    rng = np.random.default_rng(0xFE7C)

    def build():
        ix = IVFFlatIndex(d)
        assert ix.build_dev(X.data_ptr(), n, nlist, 1, args.kmeans_iters, init)
        return ix

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def search_dev_ms(ix, Q, b):
        oi = torch.zeros((b, 10), dtype=torch.int64, device="cuda"); od = torch.zeros((b, 10), device="cuda"); oc = torch.zeros(b, dtype=torch.int32, device="cuda")
        best = None
        for _ in range(args.takes + 2):
            ms, _ = timed(lambda: ix.search_dev(Q.data_ptr(), ld, b, 10, 8, oi.data_ptr(), od.data_ptr(), oc.data_ptr()))
            best = ms if best is None else min(best, ms)
        ix.poll(0)
        return best, oi.clone()

    line = {"metric": f"IVFFlat N={n} d={d} nlist={nlist}"}
    if args.yardsticks:
        ix = build()
        # k calls of get_list: the whole index to the host, the only export there was
        t0 = time.perf_counter()
        rows = 0
        for c in range(nlist):
            r, _ = ix.get_list(c)
            rows += r.shape[0]
        ms = (time.perf_counter() - t0) * 1e3
        line["get_list_all"] = {"ms": round(ms, 2), "rows": rows, "useful_GBps": round(rows * d * 4 / ms / 1e6, 2)}
        log(f"[bench_fetch] get_list x {nlist}: {line['get_list_all']}")
        line["search_dev"] = {}
        for b in (1, 64, 1024):
            Q = X[torch.from_numpy(rng.integers(0, n, b)).cuda()].contiguous()
            line["search_dev"][b] = round(search_dev_ms(ix, Q, b)[0], 4)
        log(f"[bench_fetch] search_dev ms: {line['search_dev']}")
        capi.recluster_phases(reset=True)
        draws = (dg.mix64(np.uint64(0xD2A5) + np.arange(nlist, dtype=np.uint64)) % np.uint64(n)).astype(np.uint64)
        cost, kept = C.c_float(0), C.c_int32(0)
        capi.check(capi.lib().vers_ivf_recluster(ix._h, nlist, 1, 1, capi._ptr(draws), None, 0, None, C.byref(cost), C.byref(kept), None))
        g = capi.recluster_phases()["gather_ms"]
        line["recluster_gather"] = {"ms": round(g, 2), "rows": n, "useful_GBps": round(n * d * 4 / g / 1e6, 2)}
        log(f"[bench_fetch] recluster gather phase: {line['recluster_gather']}")
        ix.close()
        print(json.dumps(line), flush=True)
        return 0

    def fetch_ms(ix, ids_dev, m, out):
        capi.fetch_phases(reset=True)
        ms, counts = timed(lambda: ix.fetch_dev(ids_dev.data_ptr(), m, out.data_ptr(), ld))
        ph = capi.fetch_phases()
        return ms, ph, counts

    def report(name, ix, ids, out, takes):
        ids_dev = torch.from_numpy(np.asarray(ids, dtype=np.int64)).cuda()
        best = None
        for _ in range(takes):
            ms, ph, counts = fetch_ms(ix, ids_dev, len(ids), out)
            if best is None or ms < best[0]:
                best = (ms, ph, counts)
        ms, ph, counts = best
        r = {"ids": len(ids), "found": counts[0], "ms": round(ms, 4), "map_ms": round(ph["map_ms"], 4), "gather_ms": round(ph["gather_ms"], 4),
             "useful_GBps": round(counts[0] * d * 4 / ms / 1e6, 3)}
        log(f"[bench_fetch] {name}: {r}")
        return r

    if args.sweep:
        capi.set_option("rowmajor", 0)
        ix = build()
        assert ix.layout_bytes()["rowmajor"] == 0
        out = torch.empty(n, ld, dtype=torch.float32, device="cuda")
        table = {}
        lens = ix.list_lengths().astype(np.int64)
        # the ids of every list in storage order: rows below the list's length, tile by tile
        all_ids = torch.arange(n, dtype=torch.int64, device="cuda")
        cl = torch.zeros(n, dtype=torch.int64, device="cuda")
        ix.fetch_dev(all_ids.data_ptr(), n, 0, 0, cl.data_ptr(), 0)
        order = np.argsort(cl.cpu().numpy(), kind="stable")          # list by list, ascending vec id inside a list = storage order after a build
        starts = np.concatenate([[0], np.cumsum(lens)])
        for w in (1, 2, 4, 8, 16, 32, 64):
            pick = []
            for c in range(nlist):
                L = order[starts[c]:starts[c + 1]]
                full = (L.size // 64) * 64
                if full:
                    pick.append(L[:full].reshape(-1, 64)[:, :w].reshape(-1))     # w rows of every whole tile of the list
            ids = np.concatenate(pick)
            row = {"tiles": int(ids.size // w)}
            for name, v in (("lds_ms", 1), ("direct_ms", 1000)):
                capi.set_option("fetch_lds_min", v)
                row[name] = report(f"sweep w={w} {name}", ix, ids, out, args.takes + 1)["gather_ms"]
            table[w] = row
        capi.set_option("fetch_lds_min", 64)
        wins = [w for w, r in table.items() if r["lds_ms"] < r["direct_ms"]]
        line["sweep"] = table
        line["T_smallest_count_where_lds_wins"] = min(wins) if wins else None
        ix.close()
        print(json.dumps(line), flush=True)
        return 0

    if args.shards:
        # W ranks EMULATED on this one GPU: W handles, each keeping its own lists of the same index; every rank's all_gather is answered from
        # tables made on the device from the unsharded index (where words from its clusters / status and owners(), row chunks from its rows).
        # Reported: the slowest rank's time OUTSIDE callbacks, the bytes each exchange would carry, the unsharded call in the same run.  The
        # exchange itself, and any run on more than one physical GPU, is NOT measured.
        from vers_amd.dist import _AG, VersComm, _Mem

        class _Ptr:   # what IVFFlatIndex.fetch_sharded_dev takes: something with ptr()
            def __init__(self, p):
                self.p = p

            def ptr(self):
                return self.p
        W_ = args.shards
        ix = build()
        every = torch.arange(n, dtype=torch.int64, device="cuda")
        cl = torch.zeros(n, dtype=torch.int64, device="cuda"); st = torch.zeros(n, dtype=torch.uint8, device="cuda")
        rows = torch.empty(n, ld, dtype=torch.float32, device="cuda")
        ix.fetch_dev(every.data_ptr(), n, rows.data_ptr(), ld, cl.data_ptr(), st.data_ptr())
        assert bool((st == 0).all())   # (a fresh build: every id is in a list)
        cent = torch.zeros(nlist, ld, dtype=torch.float32, device="cuda")
        cent[:, :d] = torch.from_numpy(np.ascontiguousarray(ix.get_centroids())).cuda()
        shards = []
        for r in range(W_):
            sx = IVFFlatIndex(d)
            sx.set_shard(r, W_)
            sx.upload_dev(rows.data_ptr(), n, ld, cent.data_ptr(), nlist, ld, cl.data_ptr())
            shards.append(sx)
        owners = torch.from_numpy(shards[0].owners().astype(np.int64)).cuda()
        R = 131072

        def answers(ids_dev):
            m = ids_dev.numel()
            c, who = cl[ids_dev], owners[cl[ids_dev]]
            where = torch.full((W_, m + 1), -1, dtype=torch.int32, device="cuda")
            where[:, m] = 0
            where[who, torch.arange(m, device="cuda")] = c.to(torch.int32)
            out_t = [where.view(torch.uint8).reshape(-1)]
            for i0 in range(0, m, R):
                sl = slice(i0, min(m, i0 + R))
                per = [ids_dev[sl][who[sl] == r] for r in range(W_)]
                pad = max(int(p.numel()) for p in per)
                buf = torch.zeros((W_, pad, d), dtype=torch.float32, device="cuda")
                for r in range(W_):
                    buf[r, :per[r].numel()] = rows[per[r], :d]
                out_t.append(buf.view(torch.uint8).reshape(-1))
            return out_t

        res = {"shards": W_, "note": "ranks emulated on one GPU, callbacks answered from the unsharded index; the exchange itself is not measured"}
        out = torch.empty(n, ld, dtype=torch.float32, device="cuda")
        for name, ids in (("all_ids", np.arange(n, dtype=np.int64)), ("random_1pct", rng.choice(n, n // 100, replace=False).astype(np.int64))):
            ids_dev = torch.from_numpy(ids).cuda()
            ans = answers(ids_dev)
            state = {"i": 0, "s": 0.0}

            def all_gather(_ctx, send_ptr, recv_ptr, nbytes):
                try:
                    t0 = time.perf_counter()
                    a = ans[state["i"]]
                    state["i"] += 1
                    if a.numel() != nbytes * W_:
                        return 1
                    torch.as_tensor(_Mem(recv_ptr, nbytes * W_), device="cuda").copy_(a)
                    torch.cuda.synchronize()
                    state["s"] += time.perf_counter() - t0
                    return 0
                except Exception:   # never unwind through the C frame
                    return 1

            cb = _AG(all_gather)
            worst = None
            for r, sx in enumerate(shards):
                comm = VersComm(None, r, W_, cb)
                best = None
                for _ in range(args.takes + 1):   # (the first take builds the rank's map)
                    state["i"], state["s"] = 0, 0.0
                    ms, counts = timed(lambda: sx.fetch_sharded_dev(_Ptr(C.byref(comm)), ids_dev.data_ptr(), len(ids), out.data_ptr(), ld))
                    outside = ms - state["s"] * 1e3
                    best = outside if best is None else min(best, outside)
                worst = best if worst is None else max(worst, best)
            un = report(f"unsharded {name}", ix, ids, out, args.takes)
            res[name] = {"ids": len(ids), "slowest_rank_ms_outside_callbacks": round(worst, 4), "unsharded_ms": un["ms"],
                         "where_bytes_per_rank": 4 * (len(ids) + 1), "row_chunk_bytes_per_rank": [int(a.numel() // W_) for a in ans[1:]]}
            log(f"[bench_fetch] shards={W_} {name}: {res[name]}")
        line["sharded"] = res
        for sx in shards:
            sx.close()
        ix.close()
        print(json.dumps(line), flush=True)
        return 0

    for source, opt in (("row_major_copy", -1), ("tiles_only", 0)):
        capi.set_option("rowmajor", opt)
        ix = build()
        assert (ix.layout_bytes()["rowmajor"] == 0) == (opt == 0)
        out = torch.empty(n + extra, ld, dtype=torch.float32, device="cuda")
        res = {}
        every = np.arange(n, dtype=np.int64)
        res["all_ids_first"] = report(f"{source} all ids, first call", ix, every, out, 1)
        res["all_ids"] = report(f"{source} all ids", ix, every, out, args.takes)
        res["random_1pct"] = report(f"{source} random 1 %", ix, rng.choice(n, n // 100, replace=False), out, args.takes)
        res["random_001pct"] = report(f"{source} random 0.01 %", ix, rng.choice(n, max(1, n // 10000), replace=False), out, args.takes)
        res["one_id"] = report(f"{source} one id", ix, np.asarray([n // 2]), out, args.takes + 2)
        # the host-pointer call: rows, clusters and status of every id into host arrays (what k calls of vers_ivf_get_list did before)
        h_ids = every.astype(np.uint64)
        h_rows = np.empty((n, d), dtype=np.float32); h_cl = np.empty(n, dtype=np.uint64); h_st = np.empty(n, dtype=np.uint8)
        h_rows.fill(0)                                  # (first touch outside the timed call)
        best = None
        for _ in range(args.takes):
            t0 = time.perf_counter()
            capi.check(capi.lib().vers_ivf_fetch(ix._h, capi._ptr(h_ids), n, capi._ptr(h_rows), 4 * d, capi._ptr(h_cl), capi._ptr(h_st), None))
            ms = (time.perf_counter() - t0) * 1e3
            best = ms if best is None else min(best, ms)
        res["host_all_ids"] = {"ms": round(best, 2), "useful_GBps": round(n * d * 4 / best / 1e6, 2)}
        log(f"[bench_fetch] {source} host-pointer call, all ids: {res['host_all_ids']}")
        # search by id against the search on resident queries
        by = {}
        for b in (1, 64, 1024):
            ids = rng.integers(0, n, b)
            ids_dev = torch.from_numpy(ids).cuda()
            Q = X[ids_dev].contiguous()
            base_ms, want = search_dev_ms(ix, Q, b)
            oi = torch.zeros((b, 10), dtype=torch.int64, device="cuda"); od = torch.zeros((b, 10), device="cuda"); oc = torch.zeros(b, dtype=torch.int32, device="cuda")
            best = None
            for _ in range(args.takes + 2):
                ms, _ = timed(lambda: ix.search_by_id_dev(ids_dev.data_ptr(), b, 10, 8, oi.data_ptr(), od.data_ptr(), oc.data_ptr()))
                best = ms if best is None else min(best, ms)
            ix.poll(0)
            by[b] = {"search_dev_ms": round(base_ms, 4), "by_id_ms": round(best, 4), "cost_ms": round(best - base_ms, 4), "same_ids": bool(torch.equal(oi, want))}
        log(f"[bench_fetch] {source} by id: {by}")
        res["by_id"] = by
        first, added = ix.add_batch_dev(X[n:].data_ptr(), extra, ld)
        res["after_add_first"] = report(f"{source} first call after add_batch of {extra}", ix, np.arange(n + added, dtype=np.int64), out, 1)
        gone = torch.from_numpy(rng.choice(n, 1000, replace=False).astype(np.int64)).cuda()
        ix.remove_batch_dev(gone.data_ptr(), 1000)
        res["after_remove_first"] = report(f"{source} first call after remove_batch of 1000", ix, np.arange(n + added, dtype=np.int64), out, 1)
        line[source] = res
        ix.close()
        del out
    capi.set_option("rowmajor", -1)
    print(json.dumps(line), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
