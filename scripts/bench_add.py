"""Batched add (vers_ivf_add_batch / _dev) on the cfg3 index (N = 10M, d = 768, nlist = 4096): microseconds per vector at
1,024 / 65,536 / 1,048,576 rows for both entry points, split by phase (vers_add_batch_phases: staging, assign, grouping,
re-layout, placement, derived arrays), against single vers_ivf_add calls in the same process.  The last batch is checked
against what single adds would have left: on a sample of lists, the old rows then the batch's rows of that list in ascending
vec id, bit for bit, and its clusters against the oracle on a sample of rows.  Prints ONE JSON line.

    python scripts/bench_add.py                          # everything
    python scripts/bench_add.py --sizes 1048576 --paths host --no-single   # one batch (e.g. under rocprofv3 --kernel-trace --stats)
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
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--nlist", type=int, default=4096)
    ap.add_argument("--kmeans-iters", type=int, default=4)
    ap.add_argument("--modes-per-list", type=int, default=16)
    ap.add_argument("--sizes", default="1024,65536,1048576")
    ap.add_argument("--paths", default="dev,host")
    ap.add_argument("--singles", type=int, default=256)
    ap.add_argument("--no-single", action="store_true")
    ap.add_argument("--check-lists", type=int, default=16)
    ap.add_argument("--warmup-rows", type=int, default=131072)
    args = ap.parse_args()

    import torch
    from oracle import c_oracle as co
    from tests import datagen as dg
    from vers_amd import capi
    from vers_amd.index import IVFFlatIndex

    torch.cuda.set_device(0)
    n, d, nlist = args.rows, args.d, args.nlist
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
    del X
    torch.cuda.empty_cache()
    cent = index.get_centroids()
    log(f"[bench_add] cfg3 index built in {t_build:.2f} s")

    seed = [0xADD00]

    def new_rows(m):
        seed[0] += 1
        R = torch.empty(m, d, dtype=torch.float32, device="cuda")
        capi.gen_rows_dev(R.data_ptr(), m, d, d, 1, seed[0], SEED_C, n_modes, sigma)
        torch.cuda.synchronize()
        return R

    def run(path, R, want_host=False):
        m = R.shape[0]
        first = C.c_uint64(0); added = C.c_uint64(0)
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if path == "host":
            Xh = np.ascontiguousarray(R.cpu().numpy())
            cl = np.zeros(m, np.uint64)
            torch.cuda.synchronize()
            ev0.record(); t0 = time.perf_counter()
            capi.check(capi.lib().vers_ivf_add_batch(index._h, capi._ptr(Xh), m, 4 * d, capi._ptr(cl), C.byref(first), C.byref(added)))
            ev1.record(); wall = time.perf_counter() - t0
        else:
            Xh = None
            out = torch.empty(m, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            ev0.record(); t0 = time.perf_counter()
            capi.check(capi.lib().vers_ivf_add_batch_dev(index._h, capi._vp(R.data_ptr()), m, d, capi._vp(out.data_ptr()), C.byref(first),
                                                         C.byref(added)))
            ev1.record(); wall = time.perf_counter() - t0
            cl = out.cpu().numpy().astype(np.uint64) if want_host else None
        torch.cuda.synchronize()
        assert added.value == m
        return ev0.elapsed_time(ev1), wall * 1e3, cl, Xh, int(first.value)

    # warm-up: first launches, the assign pass's scratch and the staging buffers at their full size (one chunk: 131072 rows)
    for p in args.paths.split(","):
        run(p, new_rows(args.warmup_rows))
    res = {}
    sizes = [int(s) for s in args.sizes.split(",")]
    paths = args.paths.split(",")
    check = None
    for m in sizes:
        for p in paths:
            R = new_rows(m)
            last = (m == sizes[-1] and p == paths[-1])
            before = None
            if last:
                lens = index.list_lengths()
                sample = [int(c) for c in np.linspace(0, nlist - 1, args.check_lists).astype(int)]
                before = {c: index.get_list(c) for c in sample}
            capi.add_batch_phases(reset=True)
            n0 = index.info()[0]
            ms_ev, ms_wall, cl, Xh, first = run(p, R, want_host=last)
            ph = capi.add_batch_phases()
            assert first == n0
            key = f"{p}_{m}"
            res[key] = {"us_per_vector": round(ms_ev * 1e3 / m, 4), "ms": round(ms_ev, 3), "wall_ms": round(ms_wall, 3),
                        "relayouts": int(ph["relayouts"]),
                        "split_us_per_vector": {k[:-3]: round(ph[k] * 1e3 / m, 4) for k in
                                                ("stage_ms", "assign_ms", "group_ms", "relayout_ms", "place_ms", "derive_ms")}}
            log(f"[bench_add] {key}: {res[key]}")
            if last:
                Xl = Xh if Xh is not None else R.cpu().numpy()
                ok = True
                for c, (r0, i0) in before.items():
                    r1, i1 = index.get_list(c)
                    mine = np.nonzero(cl == c)[0]
                    ok &= np.array_equal(i1, np.concatenate([i0, (first + mine).astype(np.uint64)]))
                    ok &= np.array_equal(r1.view(np.uint32), np.concatenate([r0, Xl[mine]]).view(np.uint32))
                rows_checked = list(range(0, m, max(1, m // 16)))
                ok_cl = all(int(cl[i]) == co.add_cluster(cent, Xl[i]) for i in rows_checked)
                ok &= ok_cl and np.array_equal(index.list_lengths(), lens + np.bincount(cl.astype(np.int64), minlength=nlist).astype(np.uint64))
                check = {"batch": key, "lists": len(before), "oracle_rows": len(rows_checked), "bitwise_equal": bool(ok)}
            del R
            torch.cuda.empty_cache()
    single = None
    if not args.no_single:
        Xs = np.ascontiguousarray(new_rows(args.singles).cpu().numpy())
        c_, v_ = C.c_uint64(0), C.c_uint64(0)
        ta = []
        for i in range(args.singles):
            t0 = time.perf_counter()
            capi.check(capi.lib().vers_ivf_add(index._h, C.c_void_p(Xs[i].ctypes.data), C.byref(c_), C.byref(v_)))
            ta.append(time.perf_counter() - t0)
        single = {"us_per_vector": round(float(np.median(ta)) * 1e6, 1), "calls": args.singles}
    big = f"host_{sizes[-1]}"
    line = {"metric": "add_batch us per vector, IVFFlat cfg3 (N=10M d=768 nlist=4096)", "build_s": round(t_build, 2),
            "batches": res, "single_add": single, "check": check, "n_total": index.info()[0],
            "target_us_per_vector_1M_host": 1.3,
            "speedup_vs_single": (round(single["us_per_vector"] / res[big]["us_per_vector"], 1) if single and big in res else None)}
    index.close()
    print(json.dumps(line), flush=True)
    return 0 if (check is None or check["bitwise_equal"]) else 1


if __name__ == "__main__":
    sys.exit(main())
