"""Range search (vers_ivf_range_search_dev) on the cfg3 index (N = 10M, d = 768, nlist = 4096), nprobe = 32, a batch of 1024 queries and a
single query.  The radius of every query is the distance of its 10th, 100th and 1000th nearest probed row, taken from a top-k search, so a
call returns about 10 / 100 / 1000 results per query.  Per (batch, radius) the call's phases (vers_range_phases: plan, count pass, prefix +
read-back, fill pass, sort + decode) over --reps calls, in sorted order and in walk order.

The yardstick of the count pass is the ordered-chain list scan of the SAME shape: vers_ivf_last_scan under option "prescan" = 0, top_k = 10,
measured in the same process and ALTERNATING with the range calls (the count pass does the same loads and the same chains without the
top-k folds).  Both are reported as median [min, max] over the repetitions: the spread is what a difference has to exceed.
Prints ONE JSON line.

--recall: the ground truth instead.  On the same index, for a sample of queries (--recall-queries, default 64) and every --ranks radius:
range recall = |approximate ∩ exhaustive| / |exhaustive| of vers_ivf_range_search_dev at --nprobe against vers_ivf_range_search_exhaustive_dev,
and the exhaustive call's phases.  The yardstick of the exhaustive count pass is the brute-force top-k scan of the same shape -- the same
loads and chains plus the top-k folds: vers_flat_last_scan_ms of vers_flat_search_dev at top_k = 10 under option "single_shadow" = 0 on a
flat handle holding the same rows, in the same process and ALTERNATING with vers_flat_range_search_dev calls, for b = 1 and b = 64; both
as median [min, max].

    python scripts/bench_range.py
    python scripts/bench_range.py --rows 2000000 --nlist 2048 --reps 5
    python scripts/bench_range.py --recall --rows 1000000 --d 128 --nlist 1024
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


def mms(v):
    v = np.asarray(v, dtype=np.float64)
    return {"median": round(float(np.median(v)), 4), "min": round(float(v.min()), 4), "max": round(float(v.max()), 4)}


def recall_mode(args, index, X, ld, n_modes, sigma, ranks, seed_x, seed_c):
    import torch
    from vers_amd import capi

    n, d, nprobe, nq, top = args.rows, args.d, args.nprobe, args.recall_queries, max(ranks)
    Q = torch.empty(nq, ld, dtype=torch.float32, device="cuda")
    capi.gen_rows_dev(Q.data_ptr(), nq, d, ld, 1, seed_x + 1, seed_c, n_modes, sigma)
    oi = torch.zeros(nq, top, dtype=torch.int64, device="cuda"); od = torch.zeros(nq, top, device="cuda")
    oc = torch.zeros(nq, dtype=torch.int32, device="cuda")
    index.search_dev(Q.data_ptr(), ld, nq, top, nprobe, oi.data_ptr(), od.data_ptr(), oc.data_ptr())
    index.poll(); torch.cuda.synchronize()
    assert int(oc.min()) == top, "fewer probed rows than the largest rank"
    radii = {m: od[:, m - 1].contiguous() for m in ranks}

    def csr(call, b, *a):   # the two-call protocol on device pointers -> (lims, ids) on the host, and the buffers for timed repeats
        lims = torch.zeros(b + 1, dtype=torch.int64, device="cuda")
        total = call(*a, lims.data_ptr(), 0, 0, 0)
        ids = torch.zeros(max(total, 1), dtype=torch.int64, device="cuda"); dist = torch.zeros(max(total, 1), device="cuda")
        assert call(*a, lims.data_ptr(), ids.data_ptr(), dist.data_ptr(), total) == total
        return lims, ids, dist, total

    out = {}
    for m in ranks:
        r = radii[m]
        al, ai, _, _ = csr(index.range_search_dev, nq, Q.data_ptr(), ld, nq, r.data_ptr(), nprobe, capi.RANGE_WALK_ORDER)
        el, ei, ed, et = csr(index.range_search_exhaustive_dev, nq, Q.data_ptr(), ld, nq, r.data_ptr(), capi.METRIC_L2SQ, 0)
        al, ai, el_h, ei_h = al.cpu().numpy(), ai.cpu().numpy(), el.cpu().numpy(), ei.cpu().numpy()
        hit = [np.intersect1d(ai[al[q]:al[q + 1]], ei_h[el_h[q]:el_h[q + 1]]).size for q in range(nq)]
        true = np.diff(el_h)
        phases = []
        for _ in range(args.reps):
            capi.range_phases(reset=True)
            assert index.range_search_exhaustive_dev(Q.data_ptr(), ld, nq, r.data_ptr(), capi.METRIC_L2SQ, 0, el.data_ptr(), ei.data_ptr(), ed.data_ptr(), et) == et
            phases.append(capi.range_phases())
        out[f"rank{m}"] = {"recall": round(float(np.sum(hit)) / max(1, int(true.sum())), 4),
                           "recall_mean_per_query": round(float(np.mean([h / t for h, t in zip(hit, true) if t])), 4),
                           "exhaustive_results_per_query": round(float(true.mean()), 1), "approximate_results_per_query": round(float(np.diff(al).mean()), 1),
                           "exhaustive_phases_ms": {k: mms([p[k] for p in phases]) for k in ("plan_ms", "count_ms", "scan_ms", "fill_ms", "sort_ms")}}
        log(f"[bench_range] recall at rank {m}: {out[f'rank{m}']}")

    # the yardstick: the brute-force top-k scan of the same shape, alternating with the flat range call
    fc = capi.FlatCorpus(d)
    fc.upload_dev(X.data_ptr(), n, ld)
    found = capi.env_option("single_shadow", 1)
    yard = {}
    try:
        capi.set_option("single_shadow", 0)
        s_i = torch.zeros(64, 10, dtype=torch.int64, device="cuda"); s_d = torch.zeros(64, 10, device="cuda")
        s_c = torch.zeros(64, dtype=torch.int32, device="cuda")
        r = radii[ranks[0]]
        for b in (1, min(64, nq)):
            lims, ids, dist, total = csr(fc.range_search_dev, b, Q.data_ptr(), ld, b, r.data_ptr(), capi.METRIC_L2SQ, 0)

            def scan():
                fc.search_dev(Q.data_ptr(), ld, b, 10, capi.METRIC_L2SQ, s_i.data_ptr(), s_d.data_ptr(), s_c.data_ptr())
                fc.poll()
                return fc.last_scan_ms()

            def count():
                capi.range_phases(reset=True)
                assert fc.range_search_dev(Q.data_ptr(), ld, b, r.data_ptr(), capi.METRIC_L2SQ, 0, lims.data_ptr(), ids.data_ptr(), dist.data_ptr(), total) == total
                return capi.range_phases()

            scan(); count()
            scans, counts = [], []
            for _ in range(args.reps):
                scans.append(scan()); counts.append(count())
            yard[f"batch{b}"] = {"flat_topk10_scan_ms": mms(scans), "results_per_query": round(total / b, 1),
                                 **{"range_" + k: mms([p[k] for p in counts]) for k in ("plan_ms", "count_ms", "scan_ms", "fill_ms", "sort_ms")}}
            log(f"[bench_range] yardstick batch {b}: {yard[f'batch{b}']}")
    finally:
        capi.set_option("single_shadow", found)
        fc.close()
    return {"metric": f"range recall of vers_ivf_range_search_dev at nprobe={nprobe} against vers_ivf_range_search_exhaustive_dev, IVFFlat (N={n} d={d} "
                      f"nlist={args.nlist}), {nq} queries; phases in ms", "reps": args.reps, **out, "flat_yardstick": yard}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--nlist", type=int, default=4096)
    ap.add_argument("--kmeans-iters", type=int, default=4)
    ap.add_argument("--modes-per-list", type=int, default=16)
    ap.add_argument("--nprobe", type=int, default=32)
    ap.add_argument("--batches", default="1024,1")
    ap.add_argument("--ranks", default="10,100,1000", help="radius = distance of the m-th nearest probed row")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--recall", action="store_true", help="range recall against the exhaustive range search + its phases and yardstick")
    ap.add_argument("--recall-queries", type=int, default=64)
    args = ap.parse_args()

    import torch
    from tests import datagen as dg
    from vers_amd import capi
    from vers_amd.index import IVFFlatIndex

    torch.cuda.set_device(0)
    n, d, nlist, nprobe = args.rows, args.d, args.nlist, args.nprobe
    ld = (d + 3) // 4 * 4
    n_modes = max(1, args.modes_per_list * nlist)
    sigma = float(dg.default_sigma(d))
    SEED_X, SEED_C = 0x5EED0001, 0x5EEDC0DE   # bench.py's corpus
    X = torch.empty(n, ld, dtype=torch.float32, device="cuda")
    capi.gen_rows_dev(X.data_ptr(), n, d, ld, 1, SEED_X, SEED_C, n_modes, sigma)
    init = (dg.mix64(np.uint64(0xB01D) + np.arange(nlist, dtype=np.uint64)) % np.uint64(n)).astype(np.uint64)
    index = IVFFlatIndex(d)
    t0 = time.perf_counter()
    assert index.build_dev(X.data_ptr(), n, nlist, 1, args.kmeans_iters, init)
    t_build = time.perf_counter() - t0
    log(f"[bench_range] index built in {t_build:.2f} s")
    ranks = [int(x) for x in args.ranks.split(",")]
    top = max(ranks)
    if args.recall:
        line = recall_mode(args, index, X, ld, n_modes, sigma, ranks, SEED_X, SEED_C)
        line["build_s"] = round(t_build, 2)
        index.close()
        print(json.dumps(line), flush=True)
        return 0
    out = {}
    # the two options the yardstick switches go back to what this process started with (VERS_OPTIONS included)
    found = {"prescan": capi.env_option("prescan", 1), "scan_events": capi.env_option("scan_events", 2)}
    try:
        for b in (int(x) for x in args.batches.split(",")):
            Q = torch.empty(b, ld, dtype=torch.float32, device="cuda")
            capi.gen_rows_dev(Q.data_ptr(), b, d, ld, 1, SEED_X + 1, SEED_C, n_modes, sigma)
            oi = torch.zeros(b, top, dtype=torch.int64, device="cuda"); od = torch.zeros(b, top, device="cuda")
            oc = torch.zeros(b, dtype=torch.int32, device="cuda")
            index.search_dev(Q.data_ptr(), ld, b, top, nprobe, oi.data_ptr(), od.data_ptr(), oc.data_ptr())
            index.poll(); torch.cuda.synchronize()
            assert int(oc.min()) == top, "fewer probed rows than the largest rank"
            radii = {m: od[:, m - 1].contiguous() for m in ranks}
            lims = torch.zeros(b + 1, dtype=torch.int64, device="cuda")
            totals = {m: index.range_search_dev(Q.data_ptr(), ld, b, radii[m].data_ptr(), nprobe, 0, lims.data_ptr(), 0, 0, 0) for m in ranks}
            cap = max(totals.values())
            ids = torch.zeros(cap, dtype=torch.int64, device="cuda"); dist = torch.zeros(cap, device="cuda")
            s_i = torch.zeros(b, 10, dtype=torch.int64, device="cuda"); s_d = torch.zeros(b, 10, device="cuda")

            def yardstick():
                capi.set_option("prescan", 0)
                capi.set_option("scan_events", 1)
                try:
                    index.search_dev(Q.data_ptr(), ld, b, 10, nprobe, s_i.data_ptr(), s_d.data_ptr(), oc.data_ptr())
                    index.poll(); torch.cuda.synchronize()
                    return index.last_scan()["ms"]
                finally:
                    capi.set_option("prescan", found["prescan"])
                    capi.set_option("scan_events", found["scan_events"])

            def one(m, flags):
                capi.range_phases(reset=True)
                t0 = time.perf_counter()
                got = index.range_search_dev(Q.data_ptr(), ld, b, radii[m].data_ptr(), nprobe, flags, lims.data_ptr(), ids.data_ptr(), dist.data_ptr(), cap)
                ms = (time.perf_counter() - t0) * 1e3
                assert got == totals[m]
                ph = capi.range_phases()
                ph["call_ms"] = ms
                return ph

            yardstick()
            for m in ranks:   # warm-up of every shape the timed window uses
                one(m, 0); one(m, capi.RANGE_WALK_ORDER)
            scan_ms, runs = [], {(m, f): [] for m in ranks for f in (0, capi.RANGE_WALK_ORDER)}
            for _ in range(args.reps):   # alternating: the yardstick and every range shape share whatever else the machine is doing
                scan_ms.append(yardstick())
                for key in runs:
                    runs[key].append(one(*key))
            res = {"ordered_chain_scan_ms_top10": mms(scan_ms)}
            for (m, f), v in runs.items():
                res[f"rank{m}_{'walk' if f else 'sorted'}"] = {
                    "results_per_query": round(totals[m] / b, 1),
                    **{k: mms([p[k] for p in v]) for k in ("call_ms", "plan_ms", "count_ms", "scan_ms", "fill_ms", "sort_ms")}}
            out[f"batch{b}"] = res
            log(f"[bench_range] batch {b}: {res}")
    finally:
        capi.set_option("prescan", found["prescan"])
        capi.set_option("scan_events", found["scan_events"])
    line = {"metric": f"vers_ivf_range_search_dev phases in ms, IVFFlat (N={n} d={d} nlist={nlist}) nprobe={nprobe}", "build_s": round(t_build, 2),
            "reps": args.reps, **out}
    index.close()
    print(json.dumps(line), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
