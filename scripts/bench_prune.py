"""A/B of the list scan's early abandon (option "pre_prune") on a corpus of one's choosing: batches of BATCH queries against an IVFFlat
index of ROWS x D rows in NLIST lists, NPROBE probes, one batch in flight.  DIST=c: the clustered generator of bench.py (16 modes per
list: cluster contrast, most tiles of the lists that are nobody's nearest are abandoned); DIST=u: uniform rows and queries (no
contrast: nothing is abandoned, the test must cost nothing).  Prints one JSON line: step and list-scan time, queries per second,
the step counters of the last launch (vers_ivf_prune_stats; absent on a build without them), the int8 head's state and filter
counters (vers_ivf_head_state; option "pre_head" through VERS_OPTIONS) and the re-scanned queries.
usage: [DIST=u] [ROWS=2000000] [D=768] [NLIST=1024] [BATCH=1024] [NPROBE=32] [STEPS=20] [PRUNE=0|1] python scripts/bench_prune.py"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from tests import datagen as dg
from vers_amd import capi
from vers_amd.index import IVFFlatIndex

E = lambda k, v: type(v)(os.environ.get(k, v))
dist, n, d, nlist, B, nprobe, steps, top_k = E("DIST", "u"), E("ROWS", 2_000_000), E("D", 768), E("NLIST", 1024), E("BATCH", 1024), E("NPROBE", 32), E("STEPS", 20), 10
kind, modes = (1, 16 * nlist) if dist == "c" else (0, 1)
if "PRUNE" in os.environ and hasattr(IVFFlatIndex, "prune_stats"):
    capi.set_option("pre_prune", int(os.environ["PRUNE"]))
dev = torch.device("cuda:0")
X = torch.empty(n, d, dtype=torch.float32, device=dev)
capi.gen_rows_dev(X.data_ptr(), n, d, d, kind, 0x5EED0001, 0x5EEDC0DE, modes, float(dg.default_sigma(d)))
ix = IVFFlatIndex(d, device=0)
ix.build_dev(X.data_ptr(), n, nlist, 1, 4, (np.arange(nlist, dtype=np.uint64) * np.uint64(n // nlist)).astype(np.uint64))
del X; torch.cuda.empty_cache()
Q = torch.empty(4 * B, d, dtype=torch.float32, device=dev)
capi.gen_rows_dev(Q.data_ptr(), 4 * B, d, d, kind, 0x5EED0002, 0x5EEDC0DE, modes, float(dg.default_sigma(d)))
oi = torch.zeros(B, top_k, dtype=torch.int64, device=dev); od = torch.zeros(B, top_k, device=dev); oc = torch.zeros(B, dtype=torch.int32, device=dev)
st = torch.cuda.current_stream().cuda_stream
warm = 5
for i in range(warm + steps):
    if i == warm:
        torch.cuda.synchronize(); ix.scan_times(reset=True); t0 = time.perf_counter()
    ix.search_dev(Q[(i % 4) * B:].data_ptr(), d, B, top_k, nprobe, oi.data_ptr(), od.data_ptr(), oc.data_ptr(), st)
torch.cuda.synchronize(); dt = (time.perf_counter() - t0) / steps
ix.poll(st)
ls = ix.last_scan()
out = {"dist": dist, "rows": n, "d": d, "nlist": nlist, "batch": B, "nprobe": nprobe, "step_ms": round(dt * 1e3, 4),
       "list_scan_ms": round(float(np.mean(ix.scan_times())), 4), "queries_per_sec": round(B / dt, 1),
       "planned_gb": round(ls["streamed_rows"] * (2 * d + 4) / 1e9, 3), "rescanned_queries": int(ix.prescan_stats()["fallback_queries"]),
       "prune_last": ix.prune_stats()["last"] if hasattr(ix, "prune_stats") else None,
       "head": ix.head_state() if hasattr(ix, "head_state") else None,
       "balls": ix.ball_state() if hasattr(ix, "ball_state") else None,
       "derive_ms": round(float(capi.build_phases()["derive_ms"]), 1) if hasattr(capi, "build_phases") else None}
print(json.dumps(out))
