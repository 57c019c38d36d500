"""cfg2 micro-benchmark: brute-force scan N=1M d=128 f32, batch=1 (HBM-bound kernel).
Rotates several corpora so the 256 MiB Infinity Cache cannot serve the re-reads."""
import argparse
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from vers_amd import capi

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1_000_000)
ap.add_argument("--d", type=int, default=128)
ap.add_argument("--b", type=int, default=1)
ap.add_argument("--k", type=int, default=10)
ap.add_argument("--corpora", type=int, default=4)
ap.add_argument("--iters", type=int, default=40)
ap.add_argument("--prescan-leg", action="store_true",
                help="time option flat_prescan 0 against 1 on the same handles: b in {8, 64, 1024}, both metrics, at --n / --d / --k")
args = ap.parse_args()


def prescan_leg():
    """Batches through the ordered chains (flat_prescan = 0) and through the matrix-core scan of the fp16 shadow with its exact finish
    (= 1), same handles, corpora in rotation.  Per shape: the median HIP-event time of a whole call (staging + scan + finish) and of the
    handle's own scan events (= 0: the chain scan without its merge; = 1: scan + finish), and what share of the queries took the exact
    re-scan.  One JSON line per shape."""
    import json
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    corp = []
    for i in range(args.corpora):
        x = torch.randn(args.n, args.d, device=dev)
        x = x / x.norm(dim=1, keepdim=True)
        fc = capi.FlatCorpus(args.d)
        fc.upload_dev(x.data_ptr(), args.n, args.d)
        del x
        corp.append(fc)
    st = torch.cuda.current_stream().cuda_stream
    iters = max(8, args.iters // 2)
    for b in (8, 64, 1024):
        q = torch.randn(b, args.d, device=dev); q = q / q.norm(dim=1, keepdim=True)
        for metric in (0, 1):
            res = {}
            for opt in (0, 1):
                capi.set_option("flat_prescan", opt)
                ids = torch.zeros(b, args.k, dtype=torch.int64, device=dev)
                dist = torch.zeros(b, args.k, dtype=torch.float32, device=dev)
                cnt = torch.zeros(b, dtype=torch.int32, device=dev)
                def run(fc):
                    fc.search_dev(q.data_ptr(), args.d, b, args.k, metric, ids.data_ptr(), dist.data_ptr(), cnt.data_ptr(), st)
                for fc in corp: run(fc)
                torch.cuda.synchronize()
                s0 = [fc.prescan_stats() for fc in corp]
                call_ms, scan_ms = [], []
                for it in range(iters):
                    fc = corp[it % len(corp)]
                    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
                    e0.record(); run(fc); e1.record(); torch.cuda.synchronize()
                    call_ms.append(e0.elapsed_time(e1)); scan_ms.append(fc.last_scan_ms())
                corp[0].poll(st)
                s1 = [fc.prescan_stats() for fc in corp]
                served = sum(a[1] - c[1] for a, c in zip(s1, s0)); redo = sum(a[2] - c[2] for a, c in zip(s1, s0))
                resc = sum(a[3] - c[3] for a, c in zip(s1, s0))
                res[opt] = dict(call_ms=float(np.median(call_ms)), call_min_ms=float(np.min(call_ms)), events_ms=float(np.median(scan_ms)),
                                queries=served, rescan=redo, rescored=resc, last=(ids.cpu().numpy(), dist.cpu().numpy()))
            capi.set_option("flat_prescan", 0)
            same = bool(np.array_equal(res[0]["last"][0], res[1]["last"][0]) and
                        np.array_equal(res[0]["last"][1].view(np.uint32), res[1]["last"][1].view(np.uint32)))
            for r in res.values(): del r["last"]
            print(json.dumps(dict(n=args.n, d=args.d, b=b, k=args.k, metric=metric, chains=res[0], prescan=res[1],
                                  ratio=res[1]["call_ms"] / res[0]["call_ms"], rescan_rate=res[1]["rescan"] / max(1, res[1]["queries"]),
                                  same_results=same)), flush=True)
    for fc in corp: fc.close()


if args.prescan_leg:
    prescan_leg()
    sys.exit(0)

dev = torch.device("cuda:0")
torch.manual_seed(0)
ld = (args.d + 3) // 4 * 4
corp = []
for i in range(args.corpora):
    x = torch.randn(args.n, ld, device=dev)
    x = x / x.norm(dim=1, keepdim=True)
    fc = capi.FlatCorpus(args.d)
    fc.upload_dev(x.data_ptr(), args.n, ld)
    fc._keep = x
    corp.append(fc)
q = torch.randn(args.b, args.d, device=dev); q = q / q.norm(dim=1, keepdim=True)
ids = torch.zeros(args.b, args.k, dtype=torch.int64, device=dev)
dist = torch.zeros(args.b, args.k, dtype=torch.float32, device=dev)
cnt = torch.zeros(args.b, dtype=torch.int32, device=dev)
st = torch.cuda.current_stream().cuda_stream
def run(fc):
    fc.search_dev(q.data_ptr(), args.d, args.b, args.k, 0, ids.data_ptr(), dist.data_ptr(), cnt.data_ptr(), st)
for fc in corp: run(fc)
torch.cuda.synchronize()
scan_ms = []
e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
e0.record()
for it in range(args.iters):
    run(corp[it % len(corp)])
e1.record(); torch.cuda.synchronize()
tot = e0.elapsed_time(e1) / args.iters
for it in range(8):
    fc = corp[it % len(corp)]; run(fc); scan_ms.append(fc.last_scan_ms())
corp[0].poll(st)
scan = float(np.median(scan_ms))
on_shadow = args.b == 1 and args.k + 6 <= 64 and capi.env_option("shadow", 1) != 0 and capi.env_option("single_shadow", 1) != 0
bytes_ = args.n * (args.d * 2 + 4) if on_shadow else args.n * args.d * 4   # (the fp16 shadow row + its |x|^2, or the f32 row)
print("list scan on", "the fp16 shadow (flat1h_kernel)" if on_shadow else "the f32 rows (ordered chains)")
print(f"n={args.n} d={args.d} b={args.b}: call {tot*1e3:.1f} us/batch  scan kernel {scan*1e3:.1f} us  "
      f"-> scan {bytes_/scan/1e6:.1f} GB/s ({bytes_/scan/1e6/8000*100:.1f}% of 8 TB/s), end-to-end {args.b/tot*1e3:.0f} q/s")
# sanity vs torch
ref = ((corp[(args.iters+7) % len(corp)]._keep[:, :args.d] - q[0:1]) ** 2).sum(1).topk(args.k, largest=False)
print("ids match torch topk:", bool((ref.indices.sort().values == ids[0].sort().values).all()))
