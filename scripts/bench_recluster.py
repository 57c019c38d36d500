"""Recluster (vers_ivf_recluster): milliseconds per call split by phase (vers_recluster_phases), after 10 % random removals and again after
10 % removals plus 10 % add_batch, next to the only route there was before, taken IN THE SAME RUN on the same rows with the same draws:
vers_ivf_build_dev on a second handle over the live rows X' already row-major in HBM (vers_build_phases) -- the identical k-means, so the
difference is what keeping the ids costs -- and that route with the host -> device copy of X' in front of it.  Two ratios per scenario:
    gather_over_build_install   the gather (rank table + rows) / build_dev's install phase
    call_over_build_dev         the whole call / the whole build_dev
(the id relabel is one pass inside the call's install phase: install_over_build_install shows it together with the placement).  The two
handles must agree bit for bit on the centroids and on every list length, and a sample of lists on ids (mapped through L) and rows.

Default index: N = 1M, d = 128, nlist = 1024; `--rows 10000000 --d 768 --nlist 4096` is cfg3 (the call holds X' and the new tiles beside
the index; the yardstick handle is closed before the call is timed).  Prints the takes to stderr and ONE JSON line to stdout; exit status 1
when a check fails.

    python scripts/bench_recluster.py
    python scripts/bench_recluster.py --new-nlist 2048          # change k on the way
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
    ap.add_argument("--new-nlist", type=int, default=0, help="k' of the recluster (default: nlist)")
    ap.add_argument("--kmeans-iters", type=int, default=4)
    ap.add_argument("--modes-per-list", type=int, default=16)
    ap.add_argument("--takes", type=int, default=2)
    ap.add_argument("--check-lists", type=int, default=12)
    ap.add_argument("--no-host-upload", action="store_true", help="do not time the host -> device copy of X' (it needs X' in pinned host memory)")
    args = ap.parse_args()

    import torch
    from tests import datagen as dg
    from vers_amd import capi
    from vers_amd.index import IVFFlatIndex

    torch.cuda.set_device(0)
    n, d, nlist = args.rows, args.d, args.nlist
    kp = args.new_nlist or nlist
    ld = (d + 3) // 4 * 4
    extra = n // 10
    n_modes = max(1, args.modes_per_list * nlist)
    X = torch.empty(n + extra, ld, dtype=torch.float32, device="cuda")     # the corpus, and behind it the rows the second scenario adds
    capi.gen_rows_dev(X.data_ptr(), n + extra, d, ld, 1, 0x5EED0001, 0x5EEDC0DE, n_modes, float(dg.default_sigma(d)))   # bench.py's corpus
    init = (dg.mix64(np.uint64(0xB01D) + np.arange(nlist, dtype=np.uint64)) % np.uint64(n)).astype(np.uint64)
    index = IVFFlatIndex(d)
    t0 = time.perf_counter()
    assert index.build_dev(X.data_ptr(), n, nlist, 1, args.kmeans_iters, init)
    log(f"[bench_recluster] index N={n} d={d} nlist={nlist} built in {time.perf_counter() - t0:.2f} s")
    rng = np.random.default_rng(0x2EC1)
    alive = np.zeros(n + extra, dtype=bool)
    alive[:n] = True
    all_ok = True
    scenarios = {}

    def remove(ids):
        dev = torch.from_numpy(ids.astype(np.int64)).cuda()
        removed = C.c_uint64(0)
        capi.check(capi.lib().vers_ivf_remove_batch_dev(index._h, capi._vp(dev.data_ptr()), ids.size, None, C.byref(removed)))
        assert removed.value == ids.size
        alive[ids] = False

    def measure(name):
        nonlocal all_ok
        n_now = index.info()[0]
        L = np.flatnonzero(alive[:n_now])
        m = L.size
        draws = (dg.mix64(np.uint64(0xD2A5) + np.arange(kp, dtype=np.uint64)) % np.uint64(m)).astype(np.uint64)
        Xl = X[torch.from_numpy(L).cuda()].contiguous()        # X' row-major in HBM: what the old route starts from
        Xl_host = None if args.no_host_upload else Xl.cpu().pin_memory()
        torch.cuda.synchronize()
        takes = []
        for take in range(args.takes):
            # the old route: host -> device copy of X', then build_dev on a second handle (ids 0 .. m-1: every vec id is lost)
            upload_ms = None
            if Xl_host is not None:
                t0 = time.perf_counter()
                Xup = Xl_host.cuda(non_blocking=False)
                torch.cuda.synchronize()
                upload_ms = (time.perf_counter() - t0) * 1e3
                del Xup
            other = IVFFlatIndex(d)
            capi.build_phases(reset=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            assert other.build_dev(Xl.data_ptr(), m, kp, 1, args.kmeans_iters, draws)
            build_ms = (time.perf_counter() - t0) * 1e3
            bp = capi.build_phases()
            cent_b, lens_b = other.get_centroids(), other.list_lengths()
            sample = {int(c): other.get_list(int(c)) for c in np.linspace(0, kp - 1, args.check_lists).astype(int)}
            other.close()
            # the call
            capi.recluster_phases(reset=True)
            cost, kept = C.c_float(0), C.c_int32(0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            capi.check(capi.lib().vers_ivf_recluster(index._h, kp, 1, args.kmeans_iters, capi._ptr(draws), None, 0, None, C.byref(cost), C.byref(kept), None))
            call_ms = (time.perf_counter() - t0) * 1e3
            ph = capi.recluster_phases()
            ok = kept.value == 1 and index.info()[0] == n_now and index.live_count() == m
            ok = ok and np.array_equal(index.get_centroids().view(np.uint32), cent_b.view(np.uint32)) and np.array_equal(index.list_lengths(), lens_b)
            for c, (rows_b, ids_b) in sample.items():
                rows_a, ids_a = index.get_list(c)
                ok = ok and np.array_equal(ids_a, L[ids_b.astype(np.int64)].astype(np.uint64)) and np.array_equal(rows_a.view(np.uint32), rows_b.view(np.uint32))
            all_ok &= bool(ok)
            install_b = bp["install_lists_ms"]
            r = {"live_rows": int(m), "k": int(kp), "call_ms": round(call_ms, 2),
                 "split_ms": {key[:-3]: round(ph[key], 2) for key in ("gather_ms", "kmeans_ms", "install_ms", "derive_ms", "tables_ms")},
                 "build_dev_ms": round(build_ms, 2), "build_dev_split_ms": {key[:-3]: bp[key] for key in ("alloc_ms", "assign_ms", "update_ms", "cost_ms", "install_lists_ms", "derive_ms")},
                 "host_upload_ms": None if upload_ms is None else round(upload_ms, 2),
                 "upload_plus_build_dev_ms": None if upload_ms is None else round(upload_ms + build_ms, 2),
                 "gather_over_build_install": round(ph["gather_ms"] / install_b, 3) if install_b else None,
                 "install_over_build_install": round((ph["install_ms"] + ph["tables_ms"]) / install_b, 3) if install_b else None,
                 "call_over_build_dev": round(call_ms / build_ms, 4), "call_over_upload_plus_build_dev": None if upload_ms is None else round(call_ms / (upload_ms + build_ms), 4),
                 "gather_bytes": int(2 * m * index_ld * 4), "same_bits_as_build_dev": bool(ok)}
            log(f"[bench_recluster] {name} take {take}: {r}")
            takes.append(r)
        scenarios[name] = takes
        del Xl, Xl_host

    index_ld = (d + 63) // 64 * 64
    remove(rng.choice(n, n // 10, replace=False))
    measure("after_10pct_removed")
    first, added = index.add_batch_dev(X[n:].data_ptr(), extra, ld)
    assert (first, added) == (n, extra)
    alive[n:] = True
    measure("after_10pct_removed_10pct_added")
    line = {"metric": f"vers_ivf_recluster ms per call against vers_ivf_build_dev over the live rows, IVFFlat N={n} d={d} nlist={nlist} -> {kp}, "
                      f"{args.kmeans_iters} k-means iterations, 1 attempt", "scenarios": scenarios, "same_bits_as_build_dev": bool(all_ok)}
    index.close()
    print(json.dumps(line), flush=True)
    return 0 if all_ok else 1


if __name__ == "__main__":
    sys.exit(main())
