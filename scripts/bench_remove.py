"""Removal (vers_ivf_remove_batch / _dev) on the cfg3 index (N = 10M, d = 768, nlist = 4096): microseconds per removed vector at
1,024 / 65,536 / 1,048,576 uniformly random distinct ids for both entry points, split by phase (vers_remove_phases: staging of the ids,
marking, compaction, tables, derived arrays), the bytes of the touched tiles (read + written) and the fraction of 8 TB/s the compaction
phase reaches on them -- next to the only alternative that existed before: a full vers_ivf_upload_dev of the index, timed in the same
process on the same index.  A sample of lists is checked against the expected survivors bit for bit after every call.  Prints ONE JSON
line; exit status 1 when a check fails or removing 65,536 ids is not faster than the re-upload.

    python scripts/bench_remove.py
    python scripts/bench_remove.py --sizes 65536 --paths dev     # one call (e.g. under rocprofv3 --kernel-trace --stats)
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

HBM_BYTES_PER_S = 8e12


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
    ap.add_argument("--check-lists", type=int, default=16)
    ap.add_argument("--no-reupload", action="store_true")
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
    init = (dg.mix64(np.uint64(0xB01D) + np.arange(nlist, dtype=np.uint64)) % np.uint64(n)).astype(np.uint64)
    index = IVFFlatIndex(d)
    t0 = time.perf_counter()
    assert index.build_dev(X.data_ptr(), n, nlist, 1, args.kmeans_iters, init, want_fields=True)
    t_build = time.perf_counter() - t0
    log(f"[bench_remove] cfg3 index built in {t_build:.2f} s")
    asg = index.assignments.astype(np.int64)
    order = np.argsort(asg, kind="stable")
    starts = np.concatenate([[0], np.cumsum(np.bincount(asg, minlength=nlist))])
    lists = [order[starts[c]:starts[c + 1]] for c in range(nlist)]   # ids[c]: ascending vec id
    alive = np.ones(n, dtype=bool)
    assert np.array_equal(index.list_lengths(), np.diff(starts).astype(np.uint64))

    sizes = [int(s) for s in args.sizes.split(",")]
    paths = args.paths.split(",")
    perm = np.random.default_rng(0x4E30).permutation(n)
    assert sum(sizes) * len(paths) + 4096 <= n
    taken = [0]

    def fresh(m):
        ids = perm[taken[0]:taken[0] + m]
        taken[0] += m
        return np.ascontiguousarray(ids, dtype=np.uint64)

    def run(path, ids):
        removed = C.c_uint64(0)
        m = ids.size
        if path == "host":
            t0 = time.perf_counter()
            capi.check(capi.lib().vers_ivf_remove_batch(index._h, capi._ptr(ids), m, C.byref(removed)))
        else:
            dev = torch.from_numpy(ids.astype(np.int64)).cuda()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            capi.check(capi.lib().vers_ivf_remove_batch_dev(index._h, capi._vp(dev.data_ptr()), m, None, C.byref(removed)))
        wall = time.perf_counter() - t0
        assert removed.value == m, (removed.value, m)
        return wall * 1e3

    def mirror(ids):
        """Shortens the host lists; returns (bytes of the touched tiles: read + written, lists touched)."""
        ii = ids.astype(np.int64)
        alive[ii] = False
        cl = asg[ii]
        o = np.lexsort((ii, cl))
        cl, ii = cl[o], ii[o]
        firsts = np.nonzero(np.concatenate([[True], cl[1:] != cl[:-1]]))[0]
        tiles = 0
        for f in firsts:
            c = int(cl[f])
            pos = int(np.searchsorted(lists[c], ii[f]))   # first row of the list that leaves
            tiles += (len(lists[c]) + 63) // 64 - pos // 64
            lists[c] = lists[c][alive[lists[c]]]
        return tiles * 64 * ld_tile * 4 * 2, len(firsts)

    def check_lists():
        ok = True
        for c in np.linspace(0, nlist - 1, args.check_lists).astype(int):
            rows, ids = index.get_list(int(c))
            ok &= np.array_equal(ids, lists[c].astype(np.uint64))
            want = X[torch.from_numpy(lists[c]).cuda(), :d].cpu().numpy()
            ok &= np.array_equal(rows.view(np.uint32), want.view(np.uint32))
        return bool(ok)

    for p in paths:   # warm-up: first launches, the bitmap and the staging buffers
        ids = fresh(2048)
        run(p, ids)
        mirror(ids)
    res, all_ok = {}, check_lists()
    for m in sizes:
        for p in paths:
            ids = fresh(m)
            capi.remove_phases(reset=True)
            ms = run(p, ids)
            ph = capi.remove_phases()
            nbytes, touched = mirror(ids)
            ok = check_lists() and index.live_count() == int(alive.sum())
            all_ok &= ok
            key = f"{p}_{m}"
            res[key] = {"us_per_vector": round(ms * 1e3 / m, 4), "ms": round(ms, 3), "lists_touched": touched,
                        "split_ms": {k[:-3]: round(ph[k], 3) for k in ("stage_ms", "mark_ms", "compact_ms", "tables_ms", "derive_ms")},
                        "touched_tile_bytes_rw": int(nbytes),
                        "compact_fraction_of_8TBps": round(nbytes / (ph["compact_ms"] * 1e-3) / HBM_BYTES_PER_S, 4) if ph["compact_ms"] > 0 else None,
                        "lists_bitwise_equal": ok}
            log(f"[bench_remove] {key}: {res[key]}")
    reupload = None
    if not args.no_reupload:
        # the alternative at the parent commit: rebuild the whole device cache (which also brings every removed vector back)
        cent = torch.from_numpy(np.ascontiguousarray(index.centroids)).cuda()
        asg_d = torch.from_numpy(asg).cuda()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        index.upload_dev(X.data_ptr(), n, ld, cent.data_ptr(), nlist, d, asg_d.data_ptr())
        torch.cuda.synchronize()
        reupload = (time.perf_counter() - t0) * 1e3
        assert index.live_count() == n
        log(f"[bench_remove] full vers_ivf_upload_dev: {reupload:.1f} ms")
    gate = None
    if reupload is not None:
        ms_64k = [v["ms"] for k_, v in res.items() if k_.endswith("_65536")]
        gate = bool(ms_64k and max(ms_64k) < reupload)
    line = {"metric": "remove_batch us per removed vector, IVFFlat cfg3 (N=10M d=768 nlist=4096)", "build_s": round(t_build, 2),
            "calls": res, "reupload_dev_ms": None if reupload is None else round(reupload, 1),
            "remove_65536_faster_than_reupload": gate, "lists_bitwise_equal": bool(all_ok)}
    index.close()
    print(json.dumps(line), flush=True)
    return 0 if all_ok and gate is not False else 1


if __name__ == "__main__":
    sys.exit(main())
