"""Filtered top-k search (vers_ivf_search_filtered_dev): what a filter costs and what it saves.  Default shape: N = 1M, d = 128,
nlist = 1024, nprobe = 8, top_k = 10, batches of 1, 64 and 1024 queries (scripts/bench_range.py's --recall shape); --rows / --d / --nlist /
--nprobe take it to cfg3 where memory allows.

Filters: random at selectivity 1, 0.5, 0.1, 0.01, 0.001, and a contiguous vec-id range of 1 %.  Per (batch, filter), over --reps repeats
ALTERNATING with the yardsticks (they share whatever else the machine is doing), as median [min, max]:
  call_ms   the whole filtered call, device events around it on the stream
  mask_ms   the tile-mask kernel    } the two records a filtered call leaves in the scan-timing ring (vers_ivf_scan_times)
  scan_ms   the filtered list scan  }
  tiles_planned / tiles_loaded / items_skipped / rows_allowed (vers_ivf_filter_stats) and bytes_not_read = (planned - loaded) * 64 * ld * 4
Yardsticks, same process, same shape:
  chain     the unfiltered ordered-chain search (option "prescan" = 0 for batches, "single_shadow" = 0 for b = 1; its code does not change
            with this feature): call_ms and its list scan (vers_ivf_last_scan)
  default   the unfiltered search as shipped (matrix cores + exact finish): call_ms
What to read off: at selectivity 1 the filtered scan should cost the chain scan (+ the mask kernel per call) within the yardstick's spread;
scan_ms should fall with tiles_loaded / tiles_planned; a RANDOM 1 % filter still loads about half the tiles -- a 64-row tile holds no
allowed row with probability 0.99^64 = 0.526, so ~47 % of the tiles stay live -- while a contiguous 1 % range empties almost all of them.
Prints ONE JSON line.

    python scripts/bench_filtered.py
    python scripts/bench_filtered.py --rows 10000000 --d 768 --nlist 4096 --nprobe 32
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--kmeans-iters", type=int, default=4)
    ap.add_argument("--modes-per-list", type=int, default=16)
    ap.add_argument("--nprobe", type=int, default=8)
    ap.add_argument("--top-k", type=int, default=10)
    ap.add_argument("--batches", default="1,64,1024")
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    assert args.reps >= 5, "at least 5 alternating repeats per point"

    import torch
    from tests import datagen as dg
    from vers_amd import capi
    from vers_amd.index import IVFFlatIndex

    torch.cuda.set_device(0)
    n, d, nlist, nprobe, top_k = args.rows, args.d, args.nlist, args.nprobe, args.top_k
    ld = (d + 3) // 4 * 4
    ld_rows = (d + 63) // 64 * 64   # columns of a stored row (padded to the scan's step)
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
    log(f"[bench_filtered] index built in {t_build:.2f} s")

    rng = np.random.default_rng(0xF117E2)
    filters = {f"random_{s:g}": (rng.random(n) < s) if s < 1 else np.ones(n, dtype=bool) for s in (1, 0.5, 0.1, 0.01, 0.001)}
    lo = n // 3
    contiguous = np.zeros(n, dtype=bool); contiguous[lo:lo + n // 100] = True
    filters["contiguous_0.01"] = contiguous
    words = {k: torch.from_numpy(capi.allowed_bitmap(v, n).view(np.int64)).cuda() for k, v in filters.items()}

    found = {k: capi.env_option(k, v) for k, v in (("prescan", 1), ("single_shadow", 1), ("scan_events", 2))}
    out = {}
    try:
        capi.set_option("scan_events", 1)
        for b in (int(x) for x in args.batches.split(",")):
            Q = torch.empty(b, ld, dtype=torch.float32, device="cuda")
            capi.gen_rows_dev(Q.data_ptr(), b, d, ld, 1, SEED_X + 1, SEED_C, n_modes, sigma)
            oi = torch.zeros(b, top_k, dtype=torch.int64, device="cuda"); od = torch.zeros(b, top_k, device="cuda")
            oc = torch.zeros(b, dtype=torch.int32, device="cuda")
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

            def timed(fn):
                torch.cuda.synchronize()
                e0.record(); fn(); e1.record()
                index.poll(); torch.cuda.synchronize()
                return e0.elapsed_time(e1)

            def unfiltered():
                index.search_dev(Q.data_ptr(), ld, b, top_k, nprobe, oi.data_ptr(), od.data_ptr(), oc.data_ptr())

            def chain():
                capi.set_option("prescan", 0); capi.set_option("single_shadow", 0)
                try:
                    ms = timed(unfiltered)
                    return {"call_ms": ms, "scan_ms": index.last_scan()["ms"]}
                finally:
                    capi.set_option("prescan", found["prescan"]); capi.set_option("single_shadow", found["single_shadow"])

            def default():
                return {"call_ms": timed(unfiltered)}

            def filtered(name):
                index.scan_times(reset=True)
                ms = timed(lambda: index.search_filtered_dev(Q.data_ptr(), ld, b, top_k, nprobe, words[name].data_ptr(), n, oi.data_ptr(), od.data_ptr(), oc.data_ptr()))
                ring = index.scan_times(reset=True)
                st = index.filter_stats()["last"]
                return {"call_ms": ms, "mask_ms": float(ring[-2]), "scan_ms": float(ring[-1]), **st}

            chain(); default()
            for name in filters:   # warm-up of every shape the timed window uses
                filtered(name)
            runs = {"chain": [], "default": [], **{name: [] for name in filters}}
            for _ in range(args.reps):
                runs["chain"].append(chain()); runs["default"].append(default())
                for name in filters:
                    runs[name].append(filtered(name))
            res = {"chain": {k: mms([r[k] for r in runs["chain"]]) for k in ("call_ms", "scan_ms")}, "default": {"call_ms": mms([r["call_ms"] for r in runs["default"]])}}
            for name in filters:
                v = runs[name]
                st = {k: v[0][k] for k in ("tiles_planned", "tiles_loaded", "items_skipped", "rows_allowed")}
                assert all(all(r[k] == st[k] for k in st) for r in v), "the counters are functions of the data and the plan"
                res[name] = {**{k: mms([r[k] for r in v]) for k in ("call_ms", "mask_ms", "scan_ms")}, **st,
                             "tiles_loaded_fraction": round(st["tiles_loaded"] / max(1, st["tiles_planned"]), 4),
                             "bytes_not_read": (st["tiles_planned"] - st["tiles_loaded"]) * 64 * ld_rows * 4}
            out[f"batch{b}"] = res
            log(f"[bench_filtered] batch {b}: {json.dumps(res)}")
    finally:
        for k, v in found.items():
            capi.set_option(k, v)
    line = {"metric": f"vers_ivf_search_filtered_dev in ms, IVFFlat (N={n} d={d} nlist={nlist}) nprobe={nprobe} top_k={top_k}", "build_s": round(t_build, 2),
            "reps": args.reps, **out}
    index.close()
    print(json.dumps(line), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
