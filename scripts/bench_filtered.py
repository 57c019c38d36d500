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
    python scripts/bench_filtered.py --range        # the filtered RANGE search: range_main below
    python scripts/bench_filtered.py --multi        # a filter per query against one per-call search per tenant: multi_main below
    python scripts/bench_filtered.py --range --multi   # the same for the RANGE search: range_multi_main below
    python scripts/bench_filtered.py --adaptive     # a depth per query against one nprobe for the batch: adaptive_main below
    python scripts/bench_filtered.py --shards 8     # the index sharded over 8 ranks, emulated on one GPU: shards_main below
    python scripts/bench_filtered.py --prepared     # masks kept across calls against the per-call entry points: prepared_main below
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


def range_main(args):
    """--range: the filtered RANGE search (vers_ivf_range_search_filtered_dev), same corpus and index.  Filters: selectivity 1, random 1 %,
    random 0.1 %, a contiguous 1 % id range.  Radii: each query's 10th / 100th-nearest ALLOWED probed distance (from a filtered top-k search
    with top_k = 100; the last allowed one where fewer are allowed).  Per (batch, filter, radius), over --reps repeats alternating with the
    yardstick, as median [min, max]:
      wall_ms    host clock around the synchronous call + the device-to-host copy of limits, ids and distances
      plan_ms / count_ms / prefix_ms / fill_ms / sort_ms   vers_range_phases (plan_ms includes the tile-mask kernel)
      total, tiles_planned / tiles_loaded / items_skipped / rows_allowed (vers_ivf_filter_stats: the count pass)
    Yardstick, same process, same radii: vers_ivf_range_search_dev (unchanged code = the parent commit's kernels) -- at selectivity 1 the
    same result; for the selective filters followed by the HOST-SIDE DISCARD a caller without this feature runs: copy the whole result
    out, keep the entries whose id is allowed, rebuild the limits.  The kept count must equal the filtered call's total.  Prints ONE JSON line."""
    import torch
    from tests import datagen as dg
    from vers_amd import capi
    from vers_amd.index import IVFFlatIndex

    torch.cuda.set_device(0)
    n, d, nlist, nprobe = args.rows, args.d, args.nlist, args.nprobe
    ld = (d + 3) // 4 * 4
    ld_rows = (d + 63) // 64 * 64
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
    log(f"[bench_filtered --range] index built in {t_build:.2f} s")

    rng = np.random.default_rng(0xF117E2)
    filters = {"random_1": np.ones(n, dtype=bool), "random_0.01": rng.random(n) < 0.01, "random_0.001": rng.random(n) < 0.001}
    lo = n // 3
    contiguous = np.zeros(n, dtype=bool); contiguous[lo:lo + n // 100] = True
    filters["contiguous_0.01"] = contiguous
    words = {k: torch.from_numpy(capi.allowed_bitmap(v, n).view(np.int64)).cuda() for k, v in filters.items()}
    PH = (("plan_ms", "plan_ms"), ("count_ms", "count_ms"), ("prefix_ms", "scan_ms"), ("fill_ms", "fill_ms"), ("sort_ms", "sort_ms"))
    out = {}
    for b in (int(x) for x in args.batches.split(",")):
        Q = torch.empty(b, ld, dtype=torch.float32, device="cuda")
        capi.gen_rows_dev(Q.data_ptr(), b, d, ld, 1, SEED_X + 1, SEED_C, n_modes, sigma)
        lims = torch.zeros(b + 1, dtype=torch.int64, device="cuda")
        res = {}
        for name, allowed in filters.items():
            # radii: the 10th / 100th-nearest allowed probed distance of each query
            oi = torch.zeros(b, 100, dtype=torch.int64, device="cuda"); od = torch.zeros(b, 100, device="cuda"); oc = torch.zeros(b, dtype=torch.int32, device="cuda")
            index.search_filtered_dev(Q.data_ptr(), ld, b, 100, nprobe, words[name].data_ptr(), n, oi.data_ptr(), od.data_ptr(), oc.data_ptr())
            index.poll(); torch.cuda.synchronize()
            odh, och = od.cpu().numpy(), oc.cpu().numpy().astype(np.int64)
            for m in (10, 100):
                col = np.clip(np.minimum(m, och) - 1, 0, 99)
                rad_h = np.where(och > 0, odh[np.arange(b), col], np.float32(0)).astype(np.float32)
                rad = torch.from_numpy(rad_h).cuda()
                # capacities: one size query each
                tot_f = index.range_search_filtered_dev(Q.data_ptr(), ld, b, rad.data_ptr(), nprobe, 0, words[name].data_ptr(), n, lims.data_ptr(), 0, 0, 0)
                tot_u = index.range_search_dev(Q.data_ptr(), ld, b, rad.data_ptr(), nprobe, 0, lims.data_ptr(), 0, 0, 0)
                cap = max(tot_f, tot_u, 1)
                ids = torch.zeros(cap, dtype=torch.int64, device="cuda"); dist = torch.zeros(cap, dtype=torch.float32, device="cuda")

                def filtered():
                    capi.range_phases(reset=True)
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    total = index.range_search_filtered_dev(Q.data_ptr(), ld, b, rad.data_ptr(), nprobe, 0, words[name].data_ptr(), n, lims.data_ptr(), ids.data_ptr(),
                                                            dist.data_ptr(), cap)
                    lh, ih, dh = lims.cpu().numpy(), ids[:total].cpu().numpy(), dist[:total].cpu().numpy()
                    wall = (time.perf_counter() - t) * 1e3
                    ph = capi.range_phases(reset=True)
                    st = index.filter_stats()["last"]
                    return {"wall_ms": wall, **{k: ph[src] for k, src in PH}, "total": total, **st}

                def yardstick():
                    capi.range_phases(reset=True)
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    total = index.range_search_dev(Q.data_ptr(), ld, b, rad.data_ptr(), nprobe, 0, lims.data_ptr(), ids.data_ptr(), dist.data_ptr(), cap)
                    lh, ih, dh = lims.cpu().numpy(), ids[:total].cpu().numpy(), dist[:total].cpu().numpy()
                    kept = total
                    if name != "random_1":   # the host-side discard
                        keep = allowed[ih]
                        ih, dh = ih[keep], dh[keep]
                        lh = np.concatenate([[0], np.cumsum(keep)])[lh]
                        kept = int(lh[-1])
                    wall = (time.perf_counter() - t) * 1e3
                    ph = capi.range_phases(reset=True)
                    return {"wall_ms": wall, **{k: ph[src] for k, src in PH}, "total": total, "kept": kept}

                filtered(); yardstick()   # warm-up of both shapes
                runs_f, runs_y = [], []
                for _ in range(args.reps):
                    runs_f.append(filtered()); runs_y.append(yardstick())
                keys = ("wall_ms",) + tuple(k for k, _ in PH)
                st = {k: runs_f[0][k] for k in ("total", "tiles_planned", "tiles_loaded", "items_skipped", "rows_allowed")}
                assert all(all(r[k] == st[k] for k in st) for r in runs_f), "totals and counters are functions of the data and the plan"
                assert all(r["kept"] == st["total"] for r in runs_y), "the discard keeps what the filtered call returns"
                res[f"{name}/r{m}"] = {"filtered": {**{k: mms([r[k] for r in runs_f]) for k in keys}, **st,
                                                    "tiles_loaded_fraction": round(st["tiles_loaded"] / max(1, st["tiles_planned"]), 4),
                                                    "bytes_not_read_per_pass": (st["tiles_planned"] - st["tiles_loaded"]) * 64 * ld_rows * 4},
                                       "unfiltered" + ("" if name == "random_1" else "+host_discard"): {**{k: mms([r[k] for r in runs_y]) for k in keys},
                                                                                                       "total": runs_y[0]["total"]}}
                del ids, dist
        out[f"batch{b}"] = res
        log(f"[bench_filtered --range] batch {b}: {json.dumps(res)}")
    line = {"metric": f"vers_ivf_range_search_filtered_dev in ms, IVFFlat (N={n} d={d} nlist={nlist}) nprobe={nprobe}", "build_s": round(t_build, 2), "reps": args.reps, **out}
    index.close()
    print(json.dumps(line), flush=True)
    return 0


def multi_main(args):
    """--multi: a batch whose queries belong to different tenants (vers_ivf_search_filtered_multi_dev), same corpus and index.  Batches of 64
    and 1024, the queries assigned round-robin to F = 1, 8, 64 tenants (query q: tenant q % F); two tenant layouts: `contiguous` (tenant f
    owns the vec ids [f n / F, (f + 1) n / F)) and `random` (every id drawn a tenant).  Per combination, over --reps repeats ALTERNATING between
    the three, each a window of --inner back-to-back calls between two device events, ms PER CALL as median [min, max]:
      multi      (a) the one multi call
      per_call   (b) what a caller does today: F vers_ivf_search_filtered_dev calls, call f over tenant f's queries (rows f, f + F, ... of the
                 batch, addressed through the query stride: no gather) into a tenant-major block, then the result rows put back in batch order
                 (one index_select per output array)
      whole      (c) F = 1 only: the per-call search of the whole batch -- the price of the new kernel at no benefit
    + vers_ivf_filter_stats of (a) and summed over (b)'s calls, as tile fractions.  (a)'s rows are checked equal to (b)'s before timing.
    Prints ONE JSON line."""
    import torch
    from tests import datagen as dg
    from vers_amd import capi
    from vers_amd.index import IVFFlatIndex

    torch.cuda.set_device(0)
    n, d, nlist, nprobe, top_k = args.rows, args.d, args.nlist, args.nprobe, args.top_k
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
    log(f"[bench_filtered --multi] index built in {t_build:.2f} s")

    rng = np.random.default_rng(0xF117E3)
    draw = rng.integers(0, 64, n)
    KEYS = ("tiles_planned", "tiles_loaded", "items_skipped", "rows_allowed")
    out = {}
    for b in (int(x) for x in args.multi_batches.split(",")):
        Q = torch.empty(b, ld, dtype=torch.float32, device="cuda")
        capi.gen_rows_dev(Q.data_ptr(), b, d, ld, 1, SEED_X + 1, SEED_C, n_modes, sigma)
        res = {}
        for F in (1, 8, 64):
            assert b % F == 0
            bf = b // F
            for layout in (("contiguous", "random") if F > 1 else ("all",)):
                tenant = (np.arange(n, dtype=np.int64) * F) // n if layout != "random" else draw % F
                words_h = capi.allowed_bitmaps([tenant == f for f in range(F)], n)
                stride = words_h.shape[1]
                words = torch.from_numpy(words_h.view(np.int64)).cuda()
                fo = torch.from_numpy((np.arange(b) % F).astype(np.int32)).cuda()
                # batch row of tenant-major row f * bf + i is i * F + f; back[q] = the tenant-major row of batch row q
                back = torch.from_numpy(((np.arange(b) % F) * bf + np.arange(b) // F).astype(np.int64)).cuda()
                oi = torch.zeros(b, top_k, dtype=torch.int64, device="cuda"); od = torch.zeros(b, top_k, device="cuda"); oc = torch.zeros(b, dtype=torch.int32, device="cuda")
                ti = torch.zeros(b, top_k, dtype=torch.int64, device="cuda"); td = torch.zeros(b, top_k, device="cuda"); tc = torch.zeros(b, dtype=torch.int32, device="cuda")
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                got = {}

                def multi():
                    index.search_filtered_multi_dev(Q.data_ptr(), ld, b, top_k, nprobe, words.data_ptr(), stride, F, n, fo.data_ptr(), oi.data_ptr(), od.data_ptr(),
                                                    oc.data_ptr())

                def per_call(stats=None):
                    for f in range(F):
                        index.search_filtered_dev(Q.data_ptr() + 4 * ld * f, ld * F, bf, top_k, nprobe, words.data_ptr() + 8 * stride * f, n,
                                                  ti.data_ptr() + 8 * top_k * bf * f, td.data_ptr() + 4 * top_k * bf * f, tc.data_ptr() + 4 * bf * f)
                        if stats is not None:
                            st = index.filter_stats()["last"]
                            for k in KEYS:
                                stats[k] = stats.get(k, 0) + st[k]
                    got["ids"], got["dist"], got["cnt"] = ti.index_select(0, back), td.index_select(0, back), tc.index_select(0, back)

                def whole():
                    index.search_filtered_dev(Q.data_ptr(), ld, b, top_k, nprobe, words.data_ptr(), n, ti.data_ptr(), td.data_ptr(), tc.data_ptr())

                def timed(fn):
                    torch.cuda.synchronize()
                    e0.record()
                    for _ in range(args.inner):
                        fn()
                    e1.record()
                    index.poll(); torch.cuda.synchronize()
                    return e0.elapsed_time(e1) / args.inner

                # warm-up of every shape the timed window uses; (a)'s rows are (b)'s; the counters
                multi(); index.poll(); torch.cuda.synchronize()
                st_a = index.filter_stats()["last"]
                st_b = {}
                per_call(st_b); index.poll(); torch.cuda.synchronize()
                cnt = oc.cpu().numpy()
                assert np.array_equal(cnt, got["cnt"].cpu().numpy()), "counts of the multi call and of the per-call calls differ"
                live = torch.arange(top_k, device="cuda")[None, :] < oc[:, None]
                assert bool(((oi == got["ids"]) | ~live).all()) and bool(((od.view(torch.int32) == got["dist"].view(torch.int32)) | ~live).all()), "rows differ"
                whole(); index.poll(); torch.cuda.synchronize()
                kinds = {"multi": multi, "per_call": per_call, **({"whole": whole} if F == 1 else {})}
                runs = {k: [] for k in kinds}
                for _ in range(args.reps):
                    for k, fn in kinds.items():
                        runs[k].append(timed(fn))
                frac = lambda st: round(st["tiles_loaded"] / max(1, st["tiles_planned"]), 4)
                res[f"F{F}/{layout}"] = {**{k: mms(v) for k, v in runs.items()},
                                         "multi_over_per_call": round(float(np.median(runs["multi"]) / np.median(runs["per_call"])), 3),
                                         "multi_stats": {**st_a, "tiles_loaded_fraction": frac(st_a)},
                                         "per_call_stats": {**st_b, "tiles_loaded_fraction": frac(st_b)},
                                         "mean_count": round(float(cnt.mean()), 2)}
                log(f"[bench_filtered --multi] batch {b} F{F}/{layout}: {json.dumps(res[f'F{F}/{layout}'])}")
        out[f"batch{b}"] = res
    line = {"metric": f"vers_ivf_search_filtered_multi_dev in ms per call, IVFFlat (N={n} d={d} nlist={nlist}) nprobe={nprobe} top_k={top_k}",
            "build_s": round(t_build, 2), "reps": args.reps, "inner": args.inner, **out}
    index.close()
    print(json.dumps(line), flush=True)
    return 0


def range_multi_main(args):
    """--range --multi: a RANGE batch whose queries belong to different tenants (vers_ivf_range_search_filtered_multi_dev), same corpus and
    index.  Batches of 64 and 1024 over F = 1, 8, 64 tenants.  Tenants round-robin and contiguous, on both sides: the vec ids (`round_robin`:
    id v belongs to tenant v % F, every tile holds rows of every tenant; `contiguous`: tenant f owns the ids [f n / F, (f + 1) n / F)) and
    the queries (`rr`: query q on tenant q % F; `blocks`: q // (b / F), so that a group of queries shares few bitmaps).  Radii: each query's
    10th / 100th-nearest probed distance among the rows its OWN bitmap allows (a filtered-multi top-k search with top_k = 100; the last
    allowed one where fewer are allowed).  Range calls are synchronous, so the clock is the host's around each variant, the device
    synchronised before and after; ms as median [min, max] over --reps repeats ALTERNATING between the variants:
      multi      (a) the one multi call, result in query order
      per_call   (b) what a caller does without it: F vers_ivf_range_search_filtered_dev calls, call f over tenant f's queries (rr: rows f,
                 f + F, ... of the batch, addressed through the query stride; the radii gathered per tenant beforehand) into a tenant-major CSR
                 block, then the segments put back in query order on the device (limits by a prefix sum, ids / distances by one gather each)
      whole      (c) F = 1 only: the per-call filtered range call of the whole batch -- the price of the new kernel at no benefit
    + vers_ivf_filter_stats of (a) and summed over (b)'s calls, as tile fractions.  Before timing, (a)'s limits, ids and distance bits are
    asserted equal to (b)'s.  Prints ONE JSON line."""
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
    log(f"[bench_filtered --range --multi] index built in {t_build:.2f} s")

    KEYS = ("tiles_planned", "tiles_loaded", "items_skipped", "rows_allowed")
    out = {}
    for b in (int(x) for x in args.multi_batches.split(",")):
        Q = torch.empty(b, ld, dtype=torch.float32, device="cuda")
        capi.gen_rows_dev(Q.data_ptr(), b, d, ld, 1, SEED_X + 1, SEED_C, n_modes, sigma)
        res = {}
        for F in (1, 8, 64):
            assert b % F == 0
            bf = b // F
            for layout in (("round_robin", "contiguous") if F > 1 else ("all",)):
                tenant = (np.arange(n, dtype=np.int64) * F) // n if layout != "round_robin" else np.arange(n, dtype=np.int64) % F
                words_h = capi.allowed_bitmaps([tenant == f for f in range(F)], n)
                stride = words_h.shape[1]
                words = torch.from_numpy(words_h.view(np.int64)).cuda()
                for assign in (("rr", "blocks") if F > 1 else ("rr",)):
                    # query q on tenant q % F (rr) or q // (b / F) (blocks); tenant-major row f * bf + i is batch row i * F + f (rr) or itself
                    # (blocks); back[q] = the tenant-major row of batch row q
                    ar = np.arange(b)
                    fo_h = ar % F if assign == "rr" else ar // bf
                    tm_rows = torch.from_numpy(((ar % bf) * F + ar // bf if assign == "rr" else ar).astype(np.int64)).cuda()
                    back = torch.from_numpy(((ar % F) * bf + ar // F if assign == "rr" else ar).astype(np.int64)).cuda()
                    q_off, q_ld = (4 * ld, ld * F) if assign == "rr" else (4 * ld * bf, ld)   # tenant f's queries: Q + f q_off, q_ld floats apart
                    fo = torch.from_numpy(fo_h.astype(np.int32)).cuda()
                    oi = torch.zeros(b, 100, dtype=torch.int64, device="cuda"); od = torch.zeros(b, 100, device="cuda"); oc = torch.zeros(b, dtype=torch.int32, device="cuda")
                    index.search_filtered_multi_dev(Q.data_ptr(), ld, b, 100, nprobe, words.data_ptr(), stride, F, n, fo.data_ptr(), oi.data_ptr(), od.data_ptr(), oc.data_ptr())
                    index.poll(); torch.cuda.synchronize()
                    odh, och = od.cpu().numpy(), oc.cpu().numpy().astype(np.int64)
                    for m in (10, 100):
                        col = np.clip(np.minimum(m, och) - 1, 0, 99)
                        rad_h = np.where(och > 0, odh[np.arange(b), col], np.float32(0)).astype(np.float32)
                        rad = torch.from_numpy(rad_h).cuda()
                        rad_tm = rad.index_select(0, tm_rows).contiguous()   # the radii per tenant, as the caller of (b) holds them
                        lims = torch.zeros(b + 1, dtype=torch.int64, device="cuda")
                        total = index.range_search_filtered_multi_dev(Q.data_ptr(), ld, b, rad.data_ptr(), nprobe, 0, words.data_ptr(), stride, F, n, fo.data_ptr(),
                                                                      lims.data_ptr(), 0, 0, 0)   # the size query
                        cap = max(total, 1)
                        ids = torch.zeros(cap, dtype=torch.int64, device="cuda"); dist = torch.zeros(cap, dtype=torch.float32, device="cuda")
                        t_lims = torch.zeros(F * (bf + 1), dtype=torch.int64, device="cuda")   # call f's limits: [f (bf + 1), (f + 1)(bf + 1))
                        t_ids = torch.zeros(cap, dtype=torch.int64, device="cuda"); t_dist = torch.zeros(cap, dtype=torch.float32, device="cuda")
                        w_lims = torch.zeros(b + 1, dtype=torch.int64, device="cuda")
                        w_ids = torch.zeros(cap, dtype=torch.int64, device="cuda"); w_dist = torch.zeros(cap, dtype=torch.float32, device="cuda")
                        got = {}
                        ar_b = torch.arange(b, device="cuda")

                        def multi():
                            t = index.range_search_filtered_multi_dev(Q.data_ptr(), ld, b, rad.data_ptr(), nprobe, 0, words.data_ptr(), stride, F, n, fo.data_ptr(),
                                                                      lims.data_ptr(), ids.data_ptr(), dist.data_ptr(), cap)
                            assert t == total

                        def per_call(stats=None):
                            off = 0
                            for f in range(F):
                                t = index.range_search_filtered_dev(Q.data_ptr() + q_off * f, q_ld, bf, rad_tm.data_ptr() + 4 * bf * f, nprobe, 0,
                                                                    words.data_ptr() + 8 * stride * f, n, t_lims.data_ptr() + 8 * (bf + 1) * f,
                                                                    t_ids.data_ptr() + 8 * off, t_dist.data_ptr() + 4 * off, cap - off)
                                assert off + t <= cap
                                if stats is not None:
                                    st = index.filter_stats()["last"]
                                    for k in KEYS:
                                        stats[k] = stats.get(k, 0) + st[k]
                                off += t
                            # the segments back in query order: counts and block starts per tenant-major row, limits by a prefix sum, one gather each
                            tl = t_lims.view(F, bf + 1)
                            cnt_tm = (tl[:, 1:] - tl[:, :-1]).reshape(-1)
                            base = torch.cumsum(tl[:, -1], 0) - tl[:, -1]                    # where call f's block starts
                            start_tm = (tl[:, :-1] + base[:, None]).reshape(-1)
                            cnt_q = cnt_tm.index_select(0, back)
                            q_lims = torch.zeros(b + 1, dtype=torch.int64, device="cuda")
                            q_lims[1:] = torch.cumsum(cnt_q, 0)
                            owner = torch.repeat_interleave(ar_b, cnt_q, output_size=off)
                            src = start_tm.index_select(0, back).index_select(0, owner) + (torch.arange(off, device="cuda") - q_lims.index_select(0, owner))
                            got["lims"], got["ids"], got["dist"] = q_lims, t_ids.index_select(0, src), t_dist.index_select(0, src)

                        def whole():
                            t = index.range_search_filtered_dev(Q.data_ptr(), ld, b, rad.data_ptr(), nprobe, 0, words.data_ptr(), n, w_lims.data_ptr(), w_ids.data_ptr(),
                                                                w_dist.data_ptr(), cap)
                            assert t == total

                        def timed(fn):
                            torch.cuda.synchronize()
                            t = time.perf_counter()
                            fn()
                            torch.cuda.synchronize()
                            return (time.perf_counter() - t) * 1e3

                        # warm-up of every shape the timed window uses; (a)'s result is (b)'s; the counters
                        multi(); torch.cuda.synchronize()
                        st_a = index.filter_stats()["last"]
                        st_b = {}
                        per_call(st_b); torch.cuda.synchronize()
                        assert torch.equal(lims, got["lims"]), "limits of the multi call and of the per-call calls differ"
                        assert torch.equal(ids[:total], got["ids"]), "ids differ"
                        assert torch.equal(dist[:total].view(torch.int32), got["dist"].view(torch.int32)), "distance bits differ"
                        kinds = {"multi": multi, "per_call": per_call}
                        if F == 1:
                            whole(); torch.cuda.synchronize()
                            assert torch.equal(lims, w_lims) and torch.equal(ids[:total], w_ids[:total]) and torch.equal(dist[:total].view(torch.int32), w_dist[:total].view(torch.int32))
                            kinds["whole"] = whole
                        runs = {k: [] for k in kinds}
                        for _ in range(args.reps):
                            for k, fn in kinds.items():
                                runs[k].append(timed(fn))
                        frac = lambda st: round(st["tiles_loaded"] / max(1, st["tiles_planned"]), 4)
                        key = f"F{F}/{layout}/{assign}/r{m}"
                        res[key] = {**{k: mms(v) for k, v in runs.items()},
                                    "multi_over_per_call": round(float(np.median(runs["multi"]) / np.median(runs["per_call"])), 3),
                                    "total": total,
                                    "multi_stats": {**st_a, "tiles_loaded_fraction": frac(st_a)},
                                    "per_call_stats": {**st_b, "tiles_loaded_fraction": frac(st_b)}}
                        log(f"[bench_filtered --range --multi] batch {b} {key}: {json.dumps(res[key])}")
                        del ids, dist, t_ids, t_dist, w_ids, w_dist
        out[f"batch{b}"] = res
    line = {"metric": f"vers_ivf_range_search_filtered_multi_dev in ms per call (host clock), IVFFlat (N={n} d={d} nlist={nlist}) nprobe={nprobe}",
            "build_s": round(t_build, 2), "reps": args.reps, **out}
    index.close()
    print(json.dumps(line), flush=True)
    return 0


def adaptive_main(args):
    """--adaptive: the filtered search to a depth per query (vers_ivf_search_filtered_adaptive_dev), same corpus and index.  Filters: random 1 %,
    random 0.1 %, a contiguous 1 % id range.  min_allowed = top_k, nprobe_min = --nprobe, nprobe_max = --nprobe-max (default: nlist).  Per (batch, filter):
      depth            the distribution of P_q = out_nprobe (mean, median, max)
      short            the share of queries with out_count < top_k, under the adaptive call and under the plain call at nprobe_min
      recall           recall@top_k against vers_ivf_search_exhaustive_filtered_dev, for both
    and, over --reps repeats ALTERNATING between the variants, whole-call ms (device events around the call) and the records the call leaves
    in the scan-timing ring (mask_ms, count_ms of the adaptive calls, scan_ms), as median [min, max]:
      adaptive         the call as described
      adaptive_m0      min_allowed = 0: every depth is nprobe_min, the scan is the plain call's; what differs is the count kernel, the plan not
                       fused into the selection, and the ranking of nprobe_max lists
      adaptive_m0_p    ... with nprobe_max = nprobe_min as well: the count kernel and the unfused plan alone
      plain_min        (a) vers_ivf_search_filtered_dev at nprobe_min (unchanged code = the parent commit's kernels)
      plain_max        (b) the same at nprobe = max_q P_q, the one setting that serves every query without this feature
      exhaustive       (c) vers_ivf_search_exhaustive_filtered_dev
    (The rows themselves are held to the oracle by tests/test_filtered_adaptive_gpu.py, not here.)  Prints ONE JSON line."""
    import torch
    from tests import datagen as dg
    from vers_amd import capi
    from vers_amd.index import IVFFlatIndex

    torch.cuda.set_device(0)
    n, d, nlist, p_min, top_k = args.rows, args.d, args.nlist, args.nprobe, args.top_k
    p_max, m = (args.nprobe_max or nlist), top_k
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
    log(f"[bench_filtered --adaptive] index built in {t_build:.2f} s")

    rng = np.random.default_rng(0xF117E2)
    filters = {"random_0.01": rng.random(n) < 0.01, "random_0.001": rng.random(n) < 0.001}
    lo = n // 3
    contiguous = np.zeros(n, dtype=bool); contiguous[lo:lo + n // 100] = True
    filters["contiguous_0.01"] = contiguous
    words = {k: torch.from_numpy(capi.allowed_bitmap(v, n).view(np.int64)).cuda() for k, v in filters.items()}
    found = capi.env_option("scan_events", 2)
    out = {}
    try:
        capi.set_option("scan_events", 1)
        for b in (int(x) for x in args.batches.split(",")):
            Q = torch.empty(b, ld, dtype=torch.float32, device="cuda")
            capi.gen_rows_dev(Q.data_ptr(), b, d, ld, 1, SEED_X + 1, SEED_C, n_modes, sigma)
            oi = torch.zeros(b, top_k, dtype=torch.int64, device="cuda"); od = torch.zeros(b, top_k, device="cuda")
            oc = torch.zeros(b, dtype=torch.int32, device="cuda"); on = torch.zeros(b, dtype=torch.int32, device="cuda")
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            res = {}
            for name in filters:
                w = words[name].data_ptr()

                def adaptive(lo_=p_min, hi_=p_max, m_=m):
                    index.search_filtered_adaptive_dev(Q.data_ptr(), ld, b, top_k, lo_, hi_, m_, w, n, oi.data_ptr(), od.data_ptr(), oc.data_ptr(), on.data_ptr())

                def plain(nprobe):
                    index.search_filtered_dev(Q.data_ptr(), ld, b, top_k, nprobe, w, n, oi.data_ptr(), od.data_ptr(), oc.data_ptr())

                def exhaustive():
                    index.search_exhaustive_filtered_dev(Q.data_ptr(), ld, b, top_k, capi.METRIC_L2SQ, w, n, oi.data_ptr(), od.data_ptr(), oc.data_ptr())

                def result(fn):
                    fn(); index.poll(); torch.cuda.synchronize()
                    return oi.cpu().numpy().copy(), oc.cpu().numpy().astype(np.int64).copy()

                def recall(ids, cnt, ex_ids, ex_cnt):
                    hit = sum(len(np.intersect1d(ids[q, :cnt[q]], ex_ids[q, :ex_cnt[q]])) for q in range(b))
                    return round(hit / max(1, int(ex_cnt.sum())), 4)

                # results first (also the warm-up of the shapes): depths, short counts, recall
                ex_ids, ex_cnt = result(exhaustive)
                a_ids, a_cnt = result(adaptive)
                depth = on.cpu().numpy().astype(np.int64)
                p_ids, p_cnt = result(lambda: plain(p_min))
                deep = int(depth.max())
                variants = {"adaptive": (adaptive, 3), "adaptive_m0": (lambda: adaptive(p_min, p_max, 0), 3), "adaptive_m0_p": (lambda: adaptive(p_min, p_min, 0), 3),
                            "plain_min": (lambda: plain(p_min), 2), "plain_max": (lambda: plain(deep), 2), "exhaustive": (exhaustive, 2)}

                def timed(fn, n_rec):
                    index.scan_times(reset=True)
                    torch.cuda.synchronize()
                    e0.record(); fn(); e1.record()
                    index.poll(); torch.cuda.synchronize()
                    ring = index.scan_times(reset=True)
                    assert len(ring) == n_rec, (len(ring), n_rec)
                    r = {"call_ms": e0.elapsed_time(e1), "mask_ms": float(ring[0]), "scan_ms": float(ring[-1])}
                    if n_rec == 3:
                        r["count_ms"] = float(ring[1])
                    return r

                for fn, n_rec in variants.values():
                    timed(fn, n_rec)
                runs = {k: [] for k in variants}
                for _ in range(args.reps):
                    for k, (fn, n_rec) in variants.items():
                        runs[k].append(timed(fn, n_rec))
                med = lambda k, f: float(np.median([r[f] for r in runs[k]]))
                res[name] = {"depth": {"mean": round(float(depth.mean()), 2), "median": float(np.median(depth)), "max": deep},
                             "short": {"adaptive": round(float((a_cnt < top_k).mean()), 4), "plain_min": round(float((p_cnt < top_k).mean()), 4)},
                             "recall": {"adaptive": recall(a_ids, a_cnt, ex_ids, ex_cnt), "plain_min": recall(p_ids, p_cnt, ex_ids, ex_cnt)},
                             **{k: {f: mms([r[f] for r in v]) for f in v[0]} for k, v in runs.items()},
                             "m0_minus_plain_min_call_ms": round(med("adaptive_m0", "call_ms") - med("plain_min", "call_ms"), 4),
                             "m0_p_minus_plain_min_call_ms": round(med("adaptive_m0_p", "call_ms") - med("plain_min", "call_ms"), 4),
                             "adaptive_over_plain_max_call": round(med("adaptive", "call_ms") / med("plain_max", "call_ms"), 3),
                             "adaptive_over_exhaustive_call": round(med("adaptive", "call_ms") / med("exhaustive", "call_ms"), 3)}
                log(f"[bench_filtered --adaptive] batch {b} {name}: {json.dumps(res[name])}")
            out[f"batch{b}"] = res
    finally:
        capi.set_option("scan_events", found)
    line = {"metric": f"vers_ivf_search_filtered_adaptive_dev in ms, IVFFlat (N={n} d={d} nlist={nlist}) nprobe_min={p_min} nprobe_max={p_max} min_allowed={m} top_k={top_k}",
            "build_s": round(t_build, 2), "reps": args.reps, **out}
    index.close()
    print(json.dumps(line), flush=True)
    return 0


def shards_main(args):
    """--shards W: filtered search on an index sharded by cluster over W ranks, EMULATED on one GPU the way scripts/emulate_shard.py does it: W
    handles, each keeping the lists LPT deals to its rank (vers_ivf_set_shard + vers_ivf_upload_dev from the device-resident fields of one
    build), their partials timed one rank at a time.  No exchange is timed: the all-gather's bytes are 16 * b * top_k per rank.
    Batches of 64 and 1024; filters: `all` (one bitmap of ones), `random_0.01` (one random 1 % bitmap), `tenants8` (F = 8 contiguous id
    ranges, query q in tenant q % 8, the per-query kernels).  Per combination, over --reps repeats ALTERNATING between the kinds, ms as median
    [min, max] over the repeats (each repeat: device events around one call):
      partial    the SLOWEST rank's vers_ivf_search_filtered_partial_dev
      merge      vers_topk_merge_dev over the W partials laid out as the all-gather lays them out
      sharded    partial + merge: what a rank waits for, less the exchange
      unsharded  the existing filtered call of the same batch on the unsharded handle (vers_ivf_search_filtered_dev / _multi_dev)
      discard    what a sharded deployment has without these calls: the slowest rank's UNFILTERED vers_ivf_search_partial_dev + merge at
                 top_k' = min(1024, ceil(top_k / selectivity)) -- enough results that about top_k survive --, the result copied to the host and
                 the rows outside the query's bitmap dropped there (numpy), wall clock around all of it
    Before timing the merged partials are checked equal to the unsharded call's rows.  Prints ONE JSON line."""
    import torch
    from tests import datagen as dg
    from vers_amd import capi
    from vers_amd.index import IVFFlatIndex

    torch.cuda.set_device(0)
    W = args.shards
    n, d, nlist, nprobe, top_k = args.rows, args.d, args.nlist, args.nprobe, args.top_k
    ld = (d + 3) // 4 * 4
    n_modes = max(1, args.modes_per_list * nlist)
    sigma = float(dg.default_sigma(d))
    SEED_X, SEED_C = 0x5EED0001, 0x5EEDC0DE   # bench.py's corpus
    X = torch.empty(n, ld, dtype=torch.float32, device="cuda")
    capi.gen_rows_dev(X.data_ptr(), n, d, ld, 1, SEED_X, SEED_C, n_modes, sigma)
    init = (dg.mix64(np.uint64(0xB01D) + np.arange(nlist, dtype=np.uint64)) % np.uint64(n)).astype(np.uint64)
    whole = IVFFlatIndex(d)
    t0 = time.perf_counter()
    assert whole.build_dev(X.data_ptr(), n, nlist, 1, args.kmeans_iters, init, want_fields=True)
    t_build = time.perf_counter() - t0
    Cd = torch.from_numpy(np.ascontiguousarray(whole.centroids)).cuda()
    Ad = torch.from_numpy(whole.assignments.astype(np.int64)).cuda()
    shards = []
    for r in range(W):
        ix = IVFFlatIndex(d)
        if W > 1:
            ix.set_shard(r, W)
        ix.upload_dev(X.data_ptr(), n, ld, Cd.data_ptr(), nlist, d, Ad.data_ptr())
        shards.append(ix)
    torch.cuda.synchronize()
    log(f"[bench_filtered --shards {W}] index built in {t_build:.2f} s, {W} shards uploaded")

    rng = np.random.default_rng(0xF117E5)
    tenant = (np.arange(n, dtype=np.int64) * 8) // n
    sets = {"all": ([np.ones(n, dtype=bool)], None, 1.0), "random_0.01": ([rng.random(n) < 0.01], None, 0.01),
            "tenants8": ([tenant == f for f in range(8)], 8, 0.125)}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn, polls):
        torch.cuda.synchronize()
        e0.record(); fn(); e1.record()
        for ix in polls:
            ix.poll()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    out = {}
    for b in (int(x) for x in args.multi_batches.split(",")):
        Q = torch.empty(b, ld, dtype=torch.float32, device="cuda")
        capi.gen_rows_dev(Q.data_ptr(), b, d, ld, 1, SEED_X + 1, SEED_C, n_modes, sigma)
        res = {}
        for name, (masks, F, sel) in sets.items():
            words_h = capi.allowed_bitmaps(masks, n)
            words = torch.from_numpy(words_h.view(np.int64)).cuda()
            fo_h = (np.arange(b) % F).astype(np.int32) if F else None
            fo = torch.from_numpy(fo_h).cuda() if F else None
            filt = (words.data_ptr(), words_h.shape[1], len(masks), n, fo.data_ptr() if F else 0)
            k_unf = min(1024, int(np.ceil(top_k / sel)))
            buf = torch.zeros(W, 2, b, top_k, dtype=torch.int64, device="cuda")
            ubuf = torch.zeros(W, 2, b, k_unf, dtype=torch.int64, device="cuda")
            oi = torch.zeros(b, top_k, dtype=torch.int64, device="cuda"); od = torch.zeros(b, top_k, device="cuda"); oc = torch.zeros(b, dtype=torch.int32, device="cuda")
            wi = torch.zeros(b, top_k, dtype=torch.int64, device="cuda"); wd = torch.zeros(b, top_k, device="cuda"); wc = torch.zeros(b, dtype=torch.int32, device="cuda")
            ui = torch.zeros(b, k_unf, dtype=torch.int64, device="cuda"); ud = torch.zeros(b, k_unf, device="cuda"); uc = torch.zeros(b, dtype=torch.int32, device="cuda")

            def partial(r):
                shards[r].search_filtered_partial_dev(Q.data_ptr(), ld, b, top_k, nprobe, filt, buf[r, 0].data_ptr(), buf[r, 1].data_ptr())

            def merge():
                IVFFlatIndex.merge_partials_dev(buf.data_ptr(), buf[0, 1].data_ptr(), 2 * b * top_k, W, b, top_k, nprobe, oi.data_ptr(), od.data_ptr(), oc.data_ptr())

            def unsharded():
                if F:
                    whole.search_filtered_multi_dev(Q.data_ptr(), ld, b, top_k, nprobe, words.data_ptr(), words_h.shape[1], F, n, fo.data_ptr(), wi.data_ptr(), wd.data_ptr(),
                                                    wc.data_ptr())
                else:
                    whole.search_filtered_dev(Q.data_ptr(), ld, b, top_k, nprobe, words.data_ptr(), n, wi.data_ptr(), wd.data_ptr(), wc.data_ptr())

            def upartial(r):
                shards[r].search_partial_dev(Q.data_ptr(), ld, b, k_unf, nprobe, ubuf[r, 0].data_ptr(), ubuf[r, 1].data_ptr())

            def discard_tail():
                """merge at top_k', the result to the host, the rows outside each query's bitmap dropped there -> wall ms"""
                torch.cuda.synchronize()
                t = time.perf_counter()
                IVFFlatIndex.merge_partials_dev(ubuf.data_ptr(), ubuf[0, 1].data_ptr(), 2 * b * k_unf, W, b, k_unf, nprobe, ui.data_ptr(), ud.data_ptr(), uc.data_ptr())
                ids = ui.cpu().numpy(); cnt = uc.cpu().numpy()
                live = np.arange(k_unf)[None, :] < cnt[:, None]
                m = np.stack(masks)[(fo_h if F else np.zeros(b, dtype=np.int32))[:, None], np.where(live, ids, 0)] & live
                kept = [ids[q][m[q]][:top_k] for q in range(b)]
                return (time.perf_counter() - t) * 1e3, float(np.mean([len(x) for x in kept]))

            # warm-up of every shape; the merged partials are the unsharded call's rows
            for r in range(W):
                partial(r); upartial(r)
            merge(); unsharded(); discard_tail()
            for ix in shards + [whole]:
                ix.poll()
            torch.cuda.synchronize()
            assert torch.equal(oc, wc), "counts of the merged partials and of the unsharded call differ"
            live = torch.arange(top_k, device="cuda")[None, :] < oc[:, None]
            assert bool(((oi == wi) | ~live).all()) and bool(((od.view(torch.int32) == wd.view(torch.int32)) | ~live).all()), "rows differ"
            runs = {k: [] for k in ("partial", "merge", "sharded", "unsharded", "discard")}
            kept_mean = 0.0
            for _ in range(args.reps):
                p = max(timed(lambda r=r: partial(r), [shards[r]]) for r in range(W))
                mg = timed(merge, [])
                runs["partial"].append(p); runs["merge"].append(mg); runs["sharded"].append(p + mg)
                runs["unsharded"].append(timed(unsharded, [whole]))
                up = max(timed(lambda r=r: upartial(r), [shards[r]]) for r in range(W))
                tail, kept_mean = discard_tail()
                runs["discard"].append(up + tail)
            res[name] = {**{k: mms(v) for k, v in runs.items()}, "discard_top_k": k_unf, "discard_mean_kept": round(kept_mean, 2),
                         "mean_count": round(float(oc.float().mean()), 2),
                         "sharded_over_unsharded": round(float(np.median(runs["sharded"]) / np.median(runs["unsharded"])), 3),
                         "discard_over_sharded": round(float(np.median(runs["discard"]) / np.median(runs["sharded"])), 2)}
            log(f"[bench_filtered --shards {W}] batch {b} {name}: {json.dumps(res[name])}")
        out[f"batch{b}"] = res
    line = {"metric": f"vers_ivf_search_filtered_partial_dev + vers_topk_merge_dev in ms, {W} ranks emulated on one GPU, IVFFlat (N={n} d={d} nlist={nlist}) "
                      f"nprobe={nprobe} top_k={top_k}", "build_s": round(t_build, 2), "reps": args.reps, **out}
    for ix in shards + [whole]:
        ix.close()
    print(json.dumps(line), flush=True)
    return 0


def prepared_main(args):
    """--prepared: a prepared filter (vers_ivf_filter_prepare + vers_ivf_search_prepared_dev) against the per-call entry point it replaces, on the
    same handle in the same run.  Batches of --batches queries; F = 1, 8, 64 bitmaps (F = 1: one bitmap for the batch, the per-call kernels and
    vers_ivf_search_filtered_dev as yardstick; else query q uses bitmap q % F and the yardstick is vers_ivf_search_filtered_multi_dev); the
    script's selectivities, drawn per bitmap.  Per point, over --reps repeats ALTERNATING between the variants, whole-call ms (device events
    around the call) as median [min, max]:
      per_call   the existing entry point (unchanged code = the parent commit's), with the mask record it leaves in the scan-timing ring
      fresh      (a) the prepared call on a fresh object
      tail       (b) the first prepared call after an in-place add_batch of 64 rows whose ids the bitmaps cover (a take whose add re-laid-out
                 storage is a rebuild, not a tail refresh: it is dropped and counted in `tail_dropped`)
      rebuild    (c) the first prepared call after a remove_batch of one row
    and, at b = 64, selectivity 0.01, F = 1 and 8: the adaptive call (nprobe_min = --nprobe, nprobe_max = nlist, min_allowed = top_k) and one
    range shape (radius: each query's 10th allowed probed distance; wall clock around the synchronous call).  Every take goes to --out.
    Prints ONE JSON line."""
    import torch
    from tests import datagen as dg
    from vers_amd import capi
    from vers_amd.index import IVFFlatIndex

    torch.cuda.set_device(0)
    n, d, nlist, nprobe, top_k = args.rows, args.d, args.nlist, args.nprobe, args.top_k
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
    log(f"[bench_filtered --prepared] index built in {t_build:.2f} s")
    del X

    room = 1 << 18                      # vec ids beyond n the bitmaps cover: the rows the tail takes add
    n_bits = n + room
    stride = (n_bits + 63) // 64
    fresh_rows = torch.empty(64, ld, dtype=torch.float32, device="cuda")
    state = {"added": 0, "removed": 0}
    takes = open(args.out, "w")
    takes.write(f"# scripts/bench_filtered.py --prepared: N={n} d={d} nlist={nlist} nprobe={nprobe} top_k={top_k} reps={args.reps}; every take, ms\n")

    made = {}

    def bitmaps(sel, F, seed):
        if (sel, F) not in made:
            made[(sel, F)] = make_bitmaps(sel, F, seed)
        return made[(sel, F)]

    def make_bitmaps(sel, F, seed):
        rng = np.random.default_rng(seed)
        out = np.zeros((F, stride), dtype=np.uint64)
        for f in range(F):
            if sel == "contiguous_0.01":
                a = np.zeros(stride * 64, dtype=bool)
                lo = (n // 3 + f * (n // max(F, 1))) % n
                a[lo:lo + n // 100] = True
                a[n:n_bits] = True      # (the rows added later are allowed: the tail refresh has bits to set)
            else:
                a = np.ones(stride * 64, dtype=bool) if sel >= 1 else rng.random(stride * 64) < sel
                a[n_bits:] = False
            out[f] = np.packbits(a, bitorder="little").view(np.uint64)
        return out

    def append_in_place():
        capi.gen_rows_dev(fresh_rows.data_ptr(), 64, d, ld, 1, SEED_X + 7 + state["added"], SEED_C, n_modes, sigma)
        first, added = index.add_batch_dev(fresh_rows.data_ptr(), 64, ld)
        assert added == 64 and first + 64 <= n_bits
        state["added"] += 1

    one_id = torch.zeros(1, dtype=torch.int64, device="cuda")

    def remove_one():
        one_id[0] = 17 + 31 * state["removed"]      # a row of the build, still there
        assert index.remove_batch_dev(one_id.data_ptr(), 1) == 1
        state["removed"] += 1

    found = capi.env_option("scan_events", 2)
    sels = (1, 0.5, 0.1, 0.01, 0.001, "contiguous_0.01")
    out = {}
    try:
        capi.set_option("scan_events", 1)
        for b in (int(x) for x in args.batches.split(",")):
            Q = torch.empty(b, ld, dtype=torch.float32, device="cuda")
            capi.gen_rows_dev(Q.data_ptr(), b, d, ld, 1, SEED_X + 1, SEED_C, n_modes, sigma)
            oi = torch.zeros(b, top_k, dtype=torch.int64, device="cuda"); od = torch.zeros(b, top_k, device="cuda")
            oc = torch.zeros(b, dtype=torch.int32, device="cuda"); on = torch.zeros(b, dtype=torch.int32, device="cuda")
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            res = {}

            def timed(fn):
                index.scan_times(reset=True)
                torch.cuda.synchronize()
                e0.record(); fn(); e1.record()
                index.poll(); torch.cuda.synchronize()
                return e0.elapsed_time(e1), index.scan_times(reset=True)

            for F in (1, 8, 64):
                fo = torch.from_numpy((np.arange(b) % F).astype(np.int32)).cuda()
                for sel in sels:
                    name = f"F{F}/" + (sel if isinstance(sel, str) else f"random_{sel:g}")
                    w = torch.from_numpy(bitmaps(sel, F, 0xF117E2 + F).view(np.int64)).cuda()
                    pf = index.prepare_filter_dev(w.data_ptr(), stride, F, n_bits)
                    fop = fo.data_ptr() if F > 1 else 0
                    out_p = (oi.data_ptr(), od.data_ptr(), oc.data_ptr())

                    def per_call(adaptive=False):
                        if F == 1 and adaptive:
                            index.search_filtered_adaptive_dev(Q.data_ptr(), ld, b, top_k, nprobe, nlist, top_k, w.data_ptr(), n_bits, *out_p, on.data_ptr())
                        elif F == 1:
                            index.search_filtered_dev(Q.data_ptr(), ld, b, top_k, nprobe, w.data_ptr(), n_bits, *out_p)
                        elif adaptive:
                            index.search_filtered_multi_adaptive_dev(Q.data_ptr(), ld, b, top_k, nprobe, nlist, top_k, w.data_ptr(), stride, F, n_bits, fop, *out_p, on.data_ptr())
                        else:
                            index.search_filtered_multi_dev(Q.data_ptr(), ld, b, top_k, nprobe, w.data_ptr(), stride, F, n_bits, fop, *out_p)

                    def prepared(adaptive=False):
                        index.search_prepared_dev(Q.data_ptr(), ld, b, top_k, nlist if adaptive else nprobe, pf, fop, *out_p,
                                                  adaptive=(nprobe, top_k, 0, on.data_ptr()) if adaptive else None)

                    def take(kind, adaptive=False):
                        i0 = pf.info()
                        if kind == "tail":
                            append_in_place()
                        elif kind == "rebuild":
                            remove_one()
                        ms, ring = timed((lambda: per_call(adaptive)) if kind == "per_call" else (lambda: prepared(adaptive)))
                        i1 = pf.info()
                        r = {"call_ms": ms}
                        if kind == "per_call":
                            r["mask_ms"] = float(ring[0])
                            if adaptive:
                                r["count_ms"] = float(ring[1])
                        else:   # what the object did is part of the take
                            did = (i1["builds"] - i0["builds"], i1["tail_refreshes"] - i0["tail_refreshes"], i1["hits"] - i0["hits"])
                            want = {"fresh": (0, 0, 1), "tail": (0, 1, 0), "rebuild": (1, 0, 0)}[kind]
                            if kind == "tail" and did == (1, 0, 0):
                                return None   # the add re-laid-out storage
                            assert did == want, (name, kind, did)
                            if kind != "fresh":
                                r["refresh_ms"] = float(ring[0])
                        takes.write(f"b={b} {name} {'adaptive ' if adaptive else ''}{kind} " + " ".join(f"{k}={v:.4f}" for k, v in r.items()) + "\n")
                        return r

                    def point(adaptive=False):
                        kinds = ("per_call", "fresh", "tail", "rebuild")
                        for k in ("per_call", "fresh"):
                            take(k, adaptive)   # warm-up of both shapes
                        runs = {k: [] for k in kinds}
                        for _ in range(args.reps):
                            for k in kinds:
                                r = take(k, adaptive)
                                if r is not None:
                                    runs[k].append(r)
                        p = {k: {f: mms([r[f] for r in v]) for f in v[0]} for k, v in runs.items() if v}
                        p["tail_dropped"] = args.reps - len(runs["tail"])
                        med = lambda k: p[k]["call_ms"]["median"]
                        p["per_call_minus_fresh_ms"] = round(med("per_call") - med("fresh"), 4)
                        p["rebuild_minus_per_call_ms"] = round(med("rebuild") - med("per_call"), 4)
                        return p

                    res[name] = point()
                    if b == 64 and sel == 0.01 and F in (1, 8):
                        res[name + "/adaptive"] = point(adaptive=True)
                        # one range shape: each query's 10th allowed probed distance
                        per_call(); index.poll(); torch.cuda.synchronize()
                        odh, och = od.cpu().numpy(), oc.cpu().numpy().astype(np.int64)
                        rad = torch.from_numpy(np.where(och > 0, odh[np.arange(b), np.clip(och - 1, 0, top_k - 1)], np.float32(0)).astype(np.float32)).cuda()
                        lims = torch.zeros(b + 1, dtype=torch.int64, device="cuda")
                        filt = (w.data_ptr(), stride, F, n_bits, fop)
                        cap = max(1, index.range_search_filtered_sharded_dev(None, Q.data_ptr(), ld, b, rad.data_ptr(), nprobe, 0, filt, lims.data_ptr(), 0, 0, 0))
                        ids = torch.zeros(cap, dtype=torch.int64, device="cuda"); dist = torch.zeros(cap, device="cuda")

                        def wall(fn):
                            torch.cuda.synchronize()
                            t = time.perf_counter(); fn()
                            return (time.perf_counter() - t) * 1e3

                        rng_calls = {"per_call": lambda: index.range_search_filtered_sharded_dev(None, Q.data_ptr(), ld, b, rad.data_ptr(), nprobe, 0, filt, lims.data_ptr(),
                                                                                                 ids.data_ptr(), dist.data_ptr(), cap),
                                     "fresh": lambda: index.range_search_prepared_dev(Q.data_ptr(), ld, b, rad.data_ptr(), nprobe, 0, pf, fop, lims.data_ptr(), ids.data_ptr(),
                                                                                      dist.data_ptr(), cap)}
                        for fn in rng_calls.values():
                            fn()
                        rr = {k: [] for k in rng_calls}
                        for _ in range(args.reps):
                            for k, fn in rng_calls.items():
                                rr[k].append(wall(fn))
                                takes.write(f"b={b} {name} range {k} wall_ms={rr[k][-1]:.4f}\n")
                        res[name + "/range"] = {**{k: {"wall_ms": mms(v)} for k, v in rr.items()}, "total": cap,
                                                "per_call_minus_fresh_ms": round(float(np.median(rr["per_call"]) - np.median(rr["fresh"])), 4)}
                    log(f"[bench_filtered --prepared] batch {b} {name}: {json.dumps({k: v for k, v in res.items() if k.startswith(name)})}")
                    pf.close()
                    del w
            out[f"batch{b}"] = res
    finally:
        capi.set_option("scan_events", found)
        takes.close()
    line = {"metric": f"vers_ivf_search_prepared_dev against the per-call filtered entry points in ms, IVFFlat (N={n} d={d} nlist={nlist}) nprobe={nprobe} top_k={top_k}",
            "build_s": round(t_build, 2), "reps": args.reps, "rows_added": 64 * state["added"], "rows_removed": state["removed"], **out}
    index.close()
    print(json.dumps(line), flush=True)
    return 0


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
    ap.add_argument("--range", action="store_true", help="the filtered RANGE search instead (vers_ivf_range_search_filtered_dev): see range_main")
    ap.add_argument("--multi", action="store_true", help="a filter per query instead (vers_ivf_search_filtered_multi_dev) against one per-call search per tenant: see multi_main")
    ap.add_argument("--adaptive", action="store_true", help="the adaptive depth (vers_ivf_search_filtered_adaptive_dev) against the plain and exhaustive filtered calls: see adaptive_main")
    ap.add_argument("--nprobe-max", type=int, default=0, help="--adaptive: nprobe_max (0: nlist)")
    ap.add_argument("--multi-batches", default="64,1024", help="--multi: the batch sizes (multiples of 64); with --range too")
    ap.add_argument("--inner", type=int, default=8, help="--multi: back-to-back calls per timed window")
    ap.add_argument("--prepared", action="store_true", help="a prepared filter (vers_ivf_filter_prepare + the _prepared_dev calls) against the per-call entry points: see prepared_main")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_filtered_prepared.txt"), help="--prepared: the file every take is written to")
    ap.add_argument("--shards", type=int, default=0, help="filtered search on an index sharded over this many ranks, emulated on one GPU (partials + merge): see shards_main")
    args = ap.parse_args()
    assert args.reps >= 5, "at least 5 alternating repeats per point"
    if args.shards:
        return shards_main(args)
    if args.prepared:
        return prepared_main(args)
    if args.adaptive:
        return adaptive_main(args)
    if args.range and args.multi:
        return range_multi_main(args)
    if args.range:
        return range_main(args)
    if args.multi:
        return multi_main(args)

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
