"""Compaction (vers_ivf_compact) on the cfg3 index (N = 10M, d = 768, nlist = 4096): after removing 1,048,576 uniformly random ids and
after removing half the index, the time of one compact call with the fused kernel (option "compact_fused" = 1) and with the unfused
sequence (0), split by phase (vers_compact_phases), storage rows and vers_mem_stats before / after and the call's peak -- next to the
only way to the same storage that existed before: a full vers_ivf_upload_dev of the index, timed in the same process (it also starts
every scenario from the same state).  After every compaction a sample of lists is checked against the expected survivors bit for bit
and a batch of queries must return what it returned just before the call.  Prints ONE JSON line; exit status 1 when a check fails.

    python scripts/bench_compact.py
    python scripts/bench_compact.py --removals 1048576 --modes 1     # one call (e.g. under rocprofv3 --kernel-trace --stats)
"""
from __future__ import annotations

import argparse
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
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--nlist", type=int, default=4096)
    ap.add_argument("--kmeans-iters", type=int, default=4)
    ap.add_argument("--modes-per-list", type=int, default=16)
    ap.add_argument("--removals", default="1048576,half")
    ap.add_argument("--modes", default="1,0", help="values of option compact_fused to time")
    ap.add_argument("--check-lists", type=int, default=16)
    ap.add_argument("--batch", type=int, default=256)
    args = ap.parse_args()

    import torch
    from tests import datagen as dg
    from vers_amd import capi
    from vers_amd.index import IVFFlatIndex

    torch.cuda.set_device(0)
    n, d, nlist = args.rows, args.d, args.nlist
    ld = (d + 3) // 4 * 4
    ld_tile = (d + 63) // 64 * 64   # columns of a stored row (csrc: kColAlign)
    n_modes = max(1, args.modes_per_list * nlist)
    sigma = float(dg.default_sigma(d))
    SEED_X, SEED_C = 0x5EED0001, 0x5EEDC0DE   # bench.py's corpus
    X = torch.empty(n, ld, dtype=torch.float32, device="cuda")
    capi.gen_rows_dev(X.data_ptr(), n, d, ld, 1, SEED_X, SEED_C, n_modes, sigma)
    Q = torch.empty(args.batch, ld, dtype=torch.float32, device="cuda")
    capi.gen_rows_dev(Q.data_ptr(), args.batch, d, ld, 1, SEED_X + 1, SEED_C, n_modes, sigma)
    init = (dg.mix64(np.uint64(0xB01D) + np.arange(nlist, dtype=np.uint64)) % np.uint64(n)).astype(np.uint64)
    index = IVFFlatIndex(d)
    t0 = time.perf_counter()
    assert index.build_dev(X.data_ptr(), n, nlist, 1, args.kmeans_iters, init, want_fields=True)
    t_build = time.perf_counter() - t0
    log(f"[bench_compact] cfg3 index built in {t_build:.2f} s")
    asg = index.assignments.astype(np.int64)
    order = np.argsort(asg, kind="stable")
    starts = np.concatenate([[0], np.cumsum(np.bincount(asg, minlength=nlist))])
    cent = torch.from_numpy(np.ascontiguousarray(index.centroids)).cuda()
    asg_d = torch.from_numpy(asg).cuda()
    perm = np.random.default_rng(0xC0A0).permutation(n)

    def upload():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        index.upload_dev(X.data_ptr(), n, ld, cent.data_ptr(), nlist, d, asg_d.data_ptr())
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def search():
        top_k, nprobe, b = 10, 32, args.batch
        oi = torch.zeros(b, top_k, dtype=torch.int64, device="cuda"); od = torch.zeros(b, top_k, device="cuda")
        oc = torch.zeros(b, dtype=torch.int32, device="cuda")
        index.search_dev(Q.data_ptr(), ld, b, top_k, nprobe, oi.data_ptr(), od.data_ptr(), oc.data_ptr())
        index.poll(); torch.cuda.synchronize()
        return oi.cpu().numpy(), od.cpu().numpy().view(np.uint32), oc.cpu().numpy()

    def check_lists(alive):
        ok = True
        for c in np.linspace(0, nlist - 1, args.check_lists).astype(int):
            want_ids = order[starts[c]:starts[c + 1]]
            want_ids = want_ids[alive[want_ids]]
            rows, ids = index.get_list(int(c))
            ok &= np.array_equal(ids, want_ids.astype(np.uint64))
            want = X[torch.from_numpy(want_ids).cuda(), :d].cpu().numpy()
            ok &= np.array_equal(rows.view(np.uint32), want.view(np.uint32))
        return bool(ok)

    def plan_rows(alive):
        lens = np.bincount(asg[alive], minlength=nlist)
        return int(((lens + np.maximum(8, lens // 16) + 63) // 64 * 64).sum())

    res, uploads, all_ok = {}, [], True
    try:
        for what in args.removals.split(","):
            m = n // 2 if what == "half" else int(what)
            ids = np.ascontiguousarray(perm[:m], dtype=np.uint64)
            alive = np.ones(n, dtype=bool); alive[perm[:m]] = False
            for mode in (int(x) for x in args.modes.split(",")):
                uploads.append(upload())     # the same start for every scenario -- and the parent commit's only way to tight storage
                dev = torch.from_numpy(ids.astype(np.int64)).cuda()
                assert index.remove_batch_dev(dev.data_ptr(), m) == m
                before_res = search()
                lb0 = index.layout_bytes()
                capi.set_option("compact_fused", mode)
                capi.compact_phases(reset=True)
                now0, _ = capi.mem_stats(reset_peak=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                rows_before, rows_after = index.compact()
                ms = (time.perf_counter() - t0) * 1e3
                now1, peak = capi.mem_stats()
                ph = capi.compact_phases()
                after_res = search()
                ok = (check_lists(alive) and index.live_count() == int(alive.sum()) and rows_after == plan_rows(alive)
                      and all(np.array_equal(a, b) for a, b in zip(before_res, after_res)))
                all_ok &= ok
                tiles = int(((np.bincount(asg[alive], minlength=nlist) + 63) // 64).sum())
                moved = tiles * 64 * ld_tile * 4
                lb1 = index.layout_bytes()
                key = f"removed_{what}_{'fused' if mode else 'unfused'}"
                res[key] = {"ms": round(ms, 2), "rows_before": rows_before, "rows_after": rows_after,
                            "split_ms": {k[:-3]: round(ph[k], 2) for k in ("plan_ms", "move_ms", "derive_ms", "tables_ms")},
                            "tile_bytes_moved": moved,
                            "move_TBps_read_plus_written": round(moved * (1 + 1 + (0.5 if lb1["shadow"] else 0) + (1 if lb1["rowmajor"] else 0)) / (ph["move_ms"] * 1e-3) / 1e12, 3) if mode and ph["move_ms"] > 0 else None,
                            "layout_bytes_before": lb0, "layout_bytes_after": lb1,
                            "mem_now_before": now0, "mem_now_after": now1, "mem_peak_during": peak, "same_lists_and_results": ok}
                log(f"[bench_compact] {key}: {res[key]}")
    finally:
        capi.set_option("compact_fused", 1)
    line = {"metric": "vers_ivf_compact ms, IVFFlat cfg3 (N=10M d=768 nlist=4096)", "build_s": round(t_build, 2), "calls": res,
            "reupload_dev_ms": [round(u, 1) for u in uploads], "same_lists_and_results": bool(all_ok)}
    index.close()
    print(json.dumps(line), flush=True)
    return 0 if all_ok else 1


if __name__ == "__main__":
    sys.exit(main())
