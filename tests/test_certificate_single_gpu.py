"""The certificates of the ONE-QUERY scans on the fp16 shadow, audited value by value: the inverted lists' (scan1h_kernel, behind
Index::search_approximate's one query per call) and the flat corpus' (flat1h_kernel, behind utils::search_exhaustive).

tests/test_certificate_gpu.py and tests/test_certificate_mutation_gpu.py audit the batched matrix-core list scan (b >= 32).  A single
query runs other kernels: a per-lane chain of fused multiply-adds over the shadow rows instead of the matrix cores, charged
pre_bound(shadow = 1) all the same, and -- the flat corpus -- its own maxima (flat_shadow_derive) and a silent retreat to the f32 scan
when the shadow is missing.  tests/test_single_query_gpu.py and the flat shadow tests compare final results with the oracle, which a
bound that is too tight or a wrong derived value almost never moves.  Here, for every (row, val, bound) a scan left in its slots,

        | val + |q|^2 - D_ref | / bound <= 1        (cosine: | 1 + val - D_ref | / bound <= 1),

D_ref the oracle's ordered chain; the worst ratio per configuration is printed (DESIGN.md section 1 quotes them).  Then the two branches
of the lone finishing block (ivf_rescore_kernel<16>) that no other test shape reaches -- a slot area beyond 131072 keys, more than
1024 keys inside the counting cut -- whose preconditions are asserted from the arithmetic in that kernel's comments, single queries
after every kind of mutation, the flat shadow's presence after each upload, and device queries that are not 16-byte aligned."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import c_oracle as co
from tests import datagen as dg
from tests.golden import make_golden as mg
from tests.test_certificate_gpu import bits, corpus, d_ref
from tests.test_certificate_mutation_gpu import r2_ref, row_r2, row_x2, xmax2_ref
from vers_amd import capi, testhooks
from vers_amd.index import IVFFlatIndex

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def kp_of(top_k):
    """candidate keys per slot on the shadow (ivf_plan.hip, flat_shadow_search1)"""
    return min(64, top_k + max(24, top_k))


def ref_dists(rows, q, metric):
    """D_ref of every row: the oracle's own ordered chains, all rows in one call (utils::search_exhaustive keeps every distance when
    top_k = the number of rows); the first rows are held against d_ref bit for bit"""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    m = rows.shape[0]
    oi, od = co.search_exhaustive(rows, q, m, metric)
    D = np.empty(m, dtype=np.float32)
    D[oi.astype(np.int64)] = od
    for i in range(min(m, 2)):
        assert bits(D[i]) == bits(np.float32(d_ref(rows[i], q, metric))), (i, D[i])
    return D


def worst_of(X_all, q, metric, vids, vals, bnd, info, label):
    """the per-value criterion; -> the worst ratio"""
    v = vids.astype(np.int64)
    D = ref_dists(X_all[v], q, metric).astype(np.float64)
    val = vals.astype(np.float64)
    err = np.abs(1.0 + val - D) if metric else np.abs(val + info["qn"] - D)
    assert np.all(np.isfinite(bnd)) and np.all(bnd > 0), label
    ratio = err / bnd
    i = int(np.argmax(ratio))
    assert ratio[i] <= 1.0, (label, "a val outside its bound", int(v[i]), float(vals[i]), float(D[i]), float(err[i]), float(bnd[i]))
    return float(ratio[i])


class DevIO:
    """one query and its result block in device memory, for the _dev entry points"""

    def __init__(self, top_k):
        import torch
        self.torch = torch
        self.dev = torch.device("cuda:0")
        self.top_k = top_k
        self.ids = torch.zeros(max(top_k, 1), dtype=torch.int64, device=self.dev)
        self.dist = torch.zeros(max(top_k, 1), dtype=torch.float32, device=self.dev)
        self.cnt = torch.zeros(1, dtype=torch.int32, device=self.dev)
        self.q = None   # (kept alive: the inverted lists' hook reads the query where the search left it -- the caller's block when it was used in place)

    def put(self, q, offset_floats=0):
        """the query in a fresh tensor, `offset_floats` floats behind its (256-byte aligned) start -> the pointer"""
        buf = self.torch.zeros(q.shape[0] + 64, dtype=self.torch.float32, device=self.dev)
        buf[offset_floats:offset_floats + q.shape[0]] = self.torch.from_numpy(np.array(q, dtype=np.float32)).to(self.dev)
        self.q = buf
        assert buf.data_ptr() % 16 == 0
        return buf.data_ptr() + 4 * offset_floats

    def result(self):
        self.torch.cuda.synchronize()
        c = int(self.cnt.item())
        return self.ids.cpu().numpy()[:c].astype(np.uint64), self.dist.cpu().numpy()[:c].copy()


def ivf_search1(ix, q, top_k, nprobe, how, io, offset_floats=0):
    if how == "host":
        ids, dist, cnt = ix.search_batch(q, top_k, nprobe)
        return ids[0, :cnt[0]].copy(), dist[0, :cnt[0]].copy()
    ptr = io.put(q, offset_floats)
    ix.search_dev(ptr, ix.d, 1, top_k, nprobe, io.ids.data_ptr(), io.dist.data_ptr(), io.cnt.data_ptr(), 0)
    r = io.result()
    ix.poll(0)
    return r


def live_ids(ix):
    return np.sort(np.concatenate([np.asarray(l, dtype=np.int64) for l in ix.ids] + [np.zeros(0, np.int64)]))


def audit_single(ix, Q, queries, top_k, nprobe, label, *, hows=("host", "dev"), maxima="pristine", cap=32768, expect_shadow=1):
    """Every query of `queries` on its own, as a host-pointer call and as a _dev call.  After each: the shadow path ran (one more
    pre-filter batch), every dumped val inside its bound, the dumped ids live rows of exactly the probed lists, the maxima the bound
    charges against the host restatements (`maxima`: "pristine" = equal to those over every row ever stored, "tight" = equal to those
    over the live rows, "upper" = between the two), the result the oracle's bit for bit.  -> worst ratio, vals, queries re-scanned."""
    metric = ix.metric
    n_ever = ix.values.shape[0]
    live = live_ids(ix)
    is_live = np.zeros(n_ever, dtype=bool); is_live[live] = True
    x2, r2 = row_x2(ix.values), row_r2(ix.values)
    x_lo, x_hi, r_lo, r_hi = float(x2[live].max()), float(x2.max()), float(r2[live].max()), float(r2.max())
    asg = ix.assignments.astype(np.int64)
    lens = np.array([len(l) for l in ix.ids])
    io = DevIO(top_k)
    out = dict(worst=0.0, n_vals=0, fallback=0, info=None)
    for qi in queries:
        q = Q[qi]
        cd = np.array([d_ref(c, q, metric) for c in ix.centroids], dtype=np.float32)
        probed = np.argsort(cd, kind="stable")[:nprobe]
        oi, od = co.search_nprobe(ix.values, ix.centroids, ix.ids, q, top_k, nprobe, metric)
        for how in hows:
            st0 = ix.prescan_stats()
            ids, dist = ivf_search1(ix, q, top_k, nprobe, how, io)
            st1 = ix.prescan_stats()
            assert st1["batches"] == st0["batches"] + 1, (label, qi, how, "the single query did not run the shadow scan")
            out["fallback"] += st1["fallback_queries"] - st0["fallback_queries"]
            vids, vals, bnd, info = testhooks.last_vals(ix, 0, cap=cap)
            assert 0 < len(vids) < cap, (label, qi, how, len(vids))
            assert info["metric"] == metric and info["shadow"] == expect_shadow and info["kp"] == kp_of(top_k), (label, qi, how, info)
            v = vids.astype(np.int64)
            assert np.all(v < n_ever) and np.all(is_live[np.minimum(v, n_ever - 1)]), (label, qi, how, "a removed or unknown vec id was dumped")
            assert np.unique(v).size == v.size, (label, qi, how, "a row was dumped twice")
            assert set(asg[v].tolist()) == set(int(c) for c in probed if lens[c] > 0), (label, qi, how, "the dumped rows are not of exactly the probed lists")
            out["worst"] = max(out["worst"], worst_of(ix.values, q, metric, vids, vals, bnd, info, (label, qi, how)))
            out["n_vals"] += v.size
            assert x_lo <= info["xmax2"] <= x_hi and r_lo <= info["r2"] <= r_hi, (label, qi, how, info, x_lo, x_hi, r_lo, r_hi)
            if maxima == "pristine":
                assert info["xmax2"] == x_hi and info["r2"] == r_hi, (label, qi, how, info, x_hi, r_hi)
            if maxima == "tight":
                assert info["xmax2"] == x_lo and info["r2"] == r_lo, (label, qi, how, info, x_lo, r_lo)
            assert len(ids) == len(oi) and np.array_equal(ids, oi) and np.array_equal(bits(dist), bits(od)), (label, qi, how, "result differs from the oracle")
            out["info"] = info
    print(f"one query, metric {metric} {label:52s}: worst |val - exact| / bound = {out['worst']:.4f} over {out['n_vals']} dumped vals ({out['fallback']} searches re-scanned)")
    assert out["n_vals"] > 0 and out["worst"] <= 1.0
    return out


SIX = range(0, 12, 2)


# ---- (a) inverted lists, ordinary corpora ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["dist_c", "dist_u", "norm_300", "mixed_subnormal"])
@pytest.mark.parametrize("metric", [0, 1])
def test_one_query_every_dumped_val_is_inside_its_bound(metric, kind):
    n, d, k, nprobe = 6000, 96, 12, 6
    X = corpus(kind, n, d, 0xA10 + metric)
    Q = corpus(kind, 12, d, 0xA20 + metric)
    ix = IVFFlatIndex.build_index(k, 1, 3, X, init_indices=mg.init_draws(0xA10, 1, k, n), metric=metric)
    assert ix.shadow_state()["active"]
    for top_k in (10, 40):
        assert kp_of(top_k) == (34 if top_k == 10 else 64)
        audit_single(ix, Q, SIX, top_k, nprobe, f"{kind}, top_k {top_k}")
    ix.close()


@pytest.mark.parametrize("metric", [0, 1])
def test_one_query_padded_rows(metric):
    """d = 300: ld pads to 320, the padding columns ride through the chain as zeros"""
    n, d, k, nprobe = 6000, 300, 12, 6
    X = corpus("dist_c", n, d, 0xA30 + metric)
    Q = corpus("dist_c", 12, d, 0xA31 + metric)
    ix = IVFFlatIndex.build_index(k, 1, 3, X, init_indices=mg.init_draws(0xA30, 1, k, n), metric=metric)
    for top_k in (10, 40):
        audit_single(ix, Q, SIX, top_k, nprobe, f"d 300, top_k {top_k}")
    ix.close()


def test_one_query_long_rows_keep_the_full_query():
    """d = 1536: a batch's query block is fp16 hi ONLY there (shadow code 2, the query's residual is charged); the single query
    multiplies by the f32 query itself and is charged shadow code 1"""
    n, d, k, nprobe = 2500, 1536, 8, 4
    X = corpus("dist_c", n, d, 0xA40)
    Q = corpus("dist_c", 32, d, 0xA41)
    ix = IVFFlatIndex.build_index(k, 1, 2, X, init_indices=mg.init_draws(0xA40, 1, k, n))
    ix.search_batch(Q, 10, nprobe)
    assert testhooks.last_vals(ix, 0)[3]["shadow"] == 2, "a batch at d = 1536 should run hi-only query blocks"
    for top_k in (10, 40):
        r = audit_single(ix, Q, SIX, top_k, nprobe, f"d 1536, top_k {top_k}")
        assert r["info"]["shadow"] == 1
    ix.close()


def test_one_query_record_lengths():
    """option "seg_rows": records of one tile (64 rows), of four (256, the most a block of scan1h_kernel takes), and the default"""
    n, d, k, nprobe, top_k = 6000, 96, 12, 6, 10
    X = corpus("dist_c", n, d, 0xA50)
    Q = corpus("dist_c", 12, d, 0xA51)
    ix = IVFFlatIndex.build_index(k, 1, 3, X, init_indices=mg.init_draws(0xA50, 1, k, n))
    n_vals = {}
    try:
        for seg in (64, 256, 0):
            capi.set_option("seg_rows", seg)
            n_vals[seg] = audit_single(ix, Q, SIX, top_k, nprobe, f"seg_rows {seg if seg else 'default'}")["n_vals"]
    finally:
        capi.set_option("seg_rows", 0)
    assert n_vals[64] > n_vals[256], n_vals   # (a slot per record: shorter records leave more keys behind)
    ix.close()


# ---- (b) the shadow term attained -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def aligned_corpus():
    """the corpus of test_shadow_rounding_errors_aligned_with_the_query (tests/test_certificate_gpu.py): every element of x sits 0.49
    ulp(fp16) off its fp16 value on the side of the query's sign, all in one binade -- x - fp16(x) is parallel to q"""
    n, d, b = 4096, 128, 32
    rng = np.random.default_rng(0x5AD)
    h = (0.03125 + rng.integers(0, 1024, (n, d)) * 2.0 ** -15).astype(np.float32)
    sgn = rng.choice([-1.0, 1.0], d).astype(np.float32)
    X = (h * rng.choice([-1.0, 1.0], (n, d))).astype(np.float32)
    X = (X + np.sign(X) * 0 + (sgn[None, :] * np.float32(0.49 * 2.0 ** -15))).astype(np.float32)
    assert np.array_equal(X.astype(np.float16).astype(np.float32) != X, np.ones_like(X, dtype=bool))
    Q = np.tile((sgn / np.sqrt(np.float32(d)))[None, :], (b, 1)).astype(np.float32)
    Q += (1e-3 * rng.standard_normal((b, d))).astype(np.float32)
    X.setflags(write=False); Q.setflags(write=False)
    return X, Q


def test_one_query_shadow_rounding_errors_aligned_with_the_query():
    """The Cauchy-Schwarz step of the shadow term 2 R |q| attained, one query at a time.  The lower limit is the batched test's own; a
    CPU emulation of scan1h_kernel's arithmetic (fp16 rows times the f32 -2q, one rounding per fused step, then xn + dot) against
    pre_bound(shadow = 1) gives 0.89 on this corpus over the 34 smallest vals -- independent of the kernel under test."""
    X, Q = aligned_corpus()
    n, k, top_k = X.shape[0], 8, 10
    ix = IVFFlatIndex.build_index(k, 1, 2, X, init_indices=mg.init_draws(0x5AD, 1, k, n))
    assert ix.shadow_state()["active"]
    r = audit_single(ix, Q, range(0, 32, 5), top_k, k, "aligned shadow residuals")
    assert 0.3 < r["worst"] <= 1.0, r["worst"]
    ix.close()


# ---- (c) the accumulation terms alone ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [768, 1536])
def test_one_query_accumulation_terms_alone(d):
    """Rows that ARE fp16 numbers (R = 0: the shadow term leaves the bound) and products x~_j q'_j of ONE sign, so that the roundings of
    the d / 2 fused steps of a lane's chain, of the two halves' sum and of xn + dot cannot cancel: what is left of the bound is (1) - (4).
    Term (3) was measured for the matrix cores' accumulation (tests/test_mfma_model_gpu.py); a sequential f32 chain of m = d / 2 + 1
    steps is within m u of sum |x_j q'_j| <= |x| |q'|, under the (3) charged with shadow = 1 (4 d u |x||q|).  No lower limit: the
    printed ratio is the measurement (0.0074 at either d).  At d = 1536 these near-identical rows lie denser around
    the 10th neighbour than the 24 keys of slack (about 29 rows inside a window of 1e-3): every search there is re-scanned exactly; the
    dumped vals are audited all the same."""
    n, k, nprobe, top_k = 2500, 8, 4, 10
    rng = np.random.default_rng(0x5B0 + d)
    sgn = rng.choice([-1.0, 1.0], d).astype(np.float32)
    X = (sgn[None, :] * (0.015625 + rng.integers(0, 1024, (n, d)) * 2.0 ** -16)).astype(np.float32)      # fp16 values in [2^-6, 2^-5), along sgn
    assert np.array_equal(X.astype(np.float16).astype(np.float32), X)
    Q = np.tile((sgn / np.sqrt(np.float32(d)))[None, :], (12, 1)).astype(np.float32)
    Q += (1e-3 * rng.standard_normal((12, d))).astype(np.float32)
    assert np.all(np.sign(Q) == sgn[None, :])                                                          # every product x_j * (-2 q_j) is negative
    ix = IVFFlatIndex.build_index(k, 1, 2, X, init_indices=mg.init_draws(0x5B0, 1, k, n))
    r = audit_single(ix, Q, SIX, top_k, nprobe, f"fp16-exact rows, one-signed products, d {d}")
    assert r["info"]["r2"] == 0.0 and r["info"]["shadow"] == 1
    print(f"one query, accumulation terms alone, d {d}: worst |val - exact| / bound = {r['worst']:.4f}")
    assert r["worst"] <= 1.0
    ix.close()


# ---- (d) the flat corpus ------------------------------------------------------------------------------------------------------------
def flat_upload_checked(fc, X, present=True):
    fc.upload(X)
    st = testhooks.flat_shadow_state(fc)
    assert st["present"] == present and st["n"] == X.shape[0], st
    if present:
        assert st["rows_built"] == X.shape[0] and st["failed"] == 0 and st["n_slots"] > 0 and st["ld"] == (X.shape[1] + 63) // 64 * 64, st
        assert st["xmax2"] == xmax2_ref(X) and st["r2"] == r2_ref(X), (st, xmax2_ref(X), r2_ref(X))
    return st


def audit_flat(fc, X, Q, queries, top_k, metric, label):
    """every query on its own: the dumped rows exist, every val inside its bound, the result utils::search_exhaustive's.  -> worst
    ratio, vals, and the queries whose certificate failed"""
    n = X.shape[0]
    worst, n_vals, failed = 0.0, 0, []
    for qi in queries:
        f0 = testhooks.flat_shadow_state(fc)["failed"]
        ids, dist, cnt = fc.search(Q[qi], top_k, metric)
        st = testhooks.flat_shadow_state(fc)
        assert st["present"]
        vids, vals, bnd, info = testhooks.flat_last_vals(fc, Q[qi], top_k, metric)
        assert info["kp"] == kp_of(top_k) and info["metric"] == metric and info["xmax2"] == st["xmax2"] and info["r2"] == st["r2"], (label, info, st)
        v = vids.astype(np.int64)
        assert v.size >= min(n, kp_of(top_k)) and np.all(v < n), (label, qi, "a padding row was dumped", v[v >= n])
        assert np.unique(v).size == v.size, (label, qi, "a row was dumped twice")
        worst = max(worst, worst_of(X, Q[qi], metric, vids, vals, bnd, info, (label, qi)))
        n_vals += v.size
        oi, od = co.search_exhaustive(X, Q[qi], top_k, metric)
        assert cnt[0] == len(oi) and np.array_equal(ids[0, :len(oi)], oi) and np.array_equal(bits(dist[0, :len(oi)]), bits(od)), (label, qi)
        if st["failed"] != f0:
            assert st["failed"] == f0 + 1
            failed.append(qi)
    print(f"flat, one query, metric {metric} {label:40s}: worst |val - exact| / bound = {worst:.4f} over {n_vals} dumped vals (certificates failed: {failed})")
    assert worst <= 1.0
    return worst, n_vals, failed


@pytest.mark.parametrize("n,d,kind", [(40000, 128, "dist_u"), (9000, 300, "dist_c"), (130, 64, "dist_u")])
def test_flat_one_query_every_dumped_val_is_inside_its_bound(n, d, kind):
    """(130, 64): three tiles, the last one holds two rows and 62 padding rows"""
    X = corpus(kind, n, d, 0xF10 + n)
    Q = corpus(kind, 6, d, 0xF20 + n).copy()
    Q[2] = X[n // 3]
    fc = capi.FlatCorpus(d)
    flat_upload_checked(fc, X)
    for metric in (0, 1):
        for top_k in (1, 10, 48):
            w, nv, failed = audit_flat(fc, X, Q, range(6), top_k, metric, f"({n}, {d}, {kind}) top_k {top_k}")
            if not (n == 130 and top_k == 48):   # (top_k = 48 of 130 rows: the 64 keys of a slot are half the corpus -- nothing says such a list certifies)
                assert not failed, (metric, top_k, "certificates failed on an ordinary corpus, queries", failed)
    fc.close()


def test_flat_one_query_shadow_rounding_errors_aligned_with_the_query():
    """the aligned corpus of the inverted lists' test, as a flat corpus: the same limits, for both metrics.  The cosine certificate
    charges the same 2 R |q| (the shadow term is written for q' = -2 q) where -<x - x~, q> can reach R |q|: at most about half the
    bound, 0.39 here -- still above the lower limit, which a cosine bound another factor of two looser would miss."""
    X, Q = aligned_corpus()
    fc = capi.FlatCorpus(X.shape[1])
    flat_upload_checked(fc, X)
    for top_k in (1, 10, 48):
        w, nv, failed = audit_flat(fc, X, Q, range(0, 32, 6), top_k, 0, f"aligned shadow residuals, top_k {top_k}")
        assert 0.3 < w <= 1.0, (top_k, w)
        w, nv, failed = audit_flat(fc, X, Q, range(0, 32, 6), top_k, 1, f"aligned shadow residuals, top_k {top_k}")
        assert 0.3 < w <= 1.0, (top_k, w)
    fc.close()


def test_flat_shadow_presence_follows_the_uploads():
    """flat_shadow_derive leaves the f32 scan in charge without a word when the shadow is unusable: an element beyond fp16's range makes
    the measured residual infinite.  Results are exact either way; only the state hook tells the two paths apart."""
    n, d, top_k = 3000, 64, 10
    X = corpus("dist_u", n, d, 0xF30)
    Q = corpus("dist_u", 4, d, 0xF31)
    fc = capi.FlatCorpus(d)
    flat_upload_checked(fc, X)
    audit_flat(fc, X, Q, range(4), top_k, 0, "before the overflow")
    Xo = X.copy(); Xo[1234, 17] = np.float32(7e4)
    st = flat_upload_checked(fc, Xo, present=False)
    assert st["n_slots"] == 0 and st["failed"] == 0
    for metric in (0, 1):
        for qi in range(4):
            ids, dist, cnt = fc.search(Q[qi], top_k, metric)
            oi, od = co.search_exhaustive(Xo, Q[qi], top_k, metric)
            assert cnt[0] == len(oi) and np.array_equal(ids[0, :len(oi)], oi) and np.array_equal(bits(dist[0, :len(oi)]), bits(od)), (metric, qi)
    with pytest.raises(capi.VersError):
        testhooks.flat_last_vals(fc, Q[0], top_k, 0)
    assert not testhooks.flat_shadow_state(fc)["present"]
    flat_upload_checked(fc, X)
    audit_flat(fc, X, Q, range(4), top_k, 0, "an ordinary corpus again")
    flat_upload_checked(fc, X[:0], present=False)
    ids, dist, cnt = fc.search(Q[0], top_k)
    assert cnt[0] == 0
    fc.close()


FORCED_BODY = r'''
import numpy as np
from oracle import c_oracle as co
from tests import datagen as dg
from vers_amd import capi, testhooks
def bits(a): return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
n, d = 5000, 128
X = dg.dist_u(0xF40, n, d); Q = dg.dist_u(0xF41, 6, d)
fc = capi.FlatCorpus(d); fc.upload(X)
st = testhooks.flat_shadow_state(fc)
assert st["present"] and st["failed"] == 0, st
done = 0
for metric in (0, 1):
    for top_k in (1, 10, 48):
        for qi in range(6):
            ids, dist, cnt = fc.search(Q[qi], top_k, metric)
            oi, od = co.search_exhaustive(X, Q[qi], top_k, metric)
            assert cnt[0] == len(oi) and np.array_equal(ids[0, :len(oi)], oi) and np.array_equal(bits(dist[0, :len(oi)]), bits(od)), (metric, top_k, qi)
            done += 1
            assert testhooks.flat_shadow_state(fc)["failed"] == done, (metric, top_k, qi, testhooks.flat_shadow_state(fc), done)
ids, dist, cnt = fc.search(Q[:3], 10)                     # a batch does not take the shadow: the count stays
assert testhooks.flat_shadow_state(fc)["failed"] == done
fc.close()
print("forced", done)
'''


def test_flat_every_forced_failure_is_counted_once():
    """VERS_OPTIONS=prescan=2 (every certificate fails, the exact re-scan decides): the failed count rises by exactly one per single query"""
    env = dict(os.environ); env["VERS_OPTIONS"] = "prescan=2"
    r = subprocess.run([sys.executable, "-c", FORCED_BODY], capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "forced 36" in r.stdout


# ---- (e) a slot area beyond 131072 keys ---------------------------------------------------------------------------------------------
def test_one_query_slot_area_beyond_the_counting_merge():
    """ivf_rescore_kernel<16> merges a single query's slots by counting while the slot area P * S_max * kp is at most 8 * 16 * 64 * 16 =
    131072 keys, slot by slot beyond.  One list of ~4400 rows (a cluster that k-means keeps whole: one initial centroid inside it, 31
    among the other rows), records of 64 rows, all 32 lists probed, 64 keys per slot: 32 * 69 * 64 keys.  The same queries at top_k = 10
    (34 keys per slot: ~75 k keys) take the counting merge on the same index.  (Checked once with a library whose slot-by-slot merge
    yields nothing: this test fails -- DESIGN.md section 8.)"""
    d, k, nprobe, n_cl, n_bg = 64, 32, 32, 4400, 3600
    Xc = dg.dist_c(0xE10, n_cl, d, 1, 0.5 * dg.default_sigma(d))
    Xb = dg.dist_u(0xE11, n_bg, d)
    perm = np.random.default_rng(0xE12).permutation(n_cl + n_bg)
    X = np.concatenate([Xc, Xb])[perm]
    pos = np.empty_like(perm); pos[perm] = np.arange(perm.size)           # row i of [Xc, Xb] is X[pos[i]]
    init = np.concatenate([pos[:1], pos[n_cl:n_cl + k - 1]])              # one initial centroid in the cluster, 31 outside
    Q = np.concatenate([dg.dist_c(0xE13, 3, d, 1, 0.5 * dg.default_sigma(d), seed_c=0xE10 ^ 0xC0FFEE), dg.dist_u(0xE14, 3, d)])
    ix = IVFFlatIndex.build_index(k, 1, 3, X, init_indices=init)
    max_len = int(ix.list_lengths().max())
    s_max = (max_len + 63) // 64
    try:
        capi.set_option("seg_rows", 64)
        assert kp_of(40) == 64 and 32 * s_max * 64 > 131072, (max_len, "the slot area would still fit the counting merge")
        big = audit_single(ix, Q, range(6), 40, nprobe, f"slot area {32 * s_max * 64} keys", cap=200000)
        assert kp_of(10) == 34 and 32 * s_max * 34 <= 131072
        small = audit_single(ix, Q, range(6), 10, nprobe, f"slot area {32 * s_max * 34} keys", cap=200000)
    finally:
        capi.set_option("seg_rows", 0)
    # (a certificate that fails sends the query to the exact re-scan, which does not read the merged list: some must hold)
    assert big["fallback"] < 12 and small["fallback"] < 12, (big["fallback"], small["fallback"])
    ix.close()


# ---- (f) more than 1024 keys inside the counting cut --------------------------------------------------------------------------------
def test_one_query_more_ties_inside_the_cut_than_the_counting_merge_holds():
    """The counting merge keeps every key with val <= T, T the kp-th smallest slot minimum, in a buffer of 1024 keys, and gives up
    (slot by slot instead) when more survive.  3000 exact copies of one row in one list: every 64-row record that holds copies leaves up
    to 34 keys of the SAME val behind.  The list is then full of ties and cannot certify: the exact re-scan decides, ties by list
    position."""
    n0, d, k, top_k, nprobe, copies = 5000, 64, 10, 10, 4, 3000
    X0 = dg.dist_c(0x71E, n0, d, 40, dg.default_sigma(d))
    base = X0[17].copy()
    near = np.tile(base[None, :], (70, 1))
    for t in range(70):
        near[t, t % d] = np.nextafter(near[t, t % d], np.float32(2.0) if t % 2 else np.float32(-2.0))   # one element, one ulp
    X = np.concatenate([X0, np.tile(base[None, :], (copies, 1)), near]).astype(np.float32)
    Q = np.stack([base, base * np.float32(1.0001)])
    ix = IVFFlatIndex.build_index(k, 1, 3, X, init_indices=np.arange(k) * 499 + 3)      # (distinct initial centroids, none of them a copy)
    c = int(ix.assignments[17])
    lst = np.asarray(ix.ids[c], dtype=np.int64)
    is_copy = (lst == 17) | ((lst >= n0) & (lst < n0 + copies))
    assert is_copy.sum() == copies + 1 and np.all(ix.assignments[n0:] == c), "the copies and their neighbours must share a list"
    seg = 64
    kept = sum(min(kp_of(top_k), int(is_copy[s:s + seg].sum())) for s in range(0, lst.size, seg))
    s_max = (int(ix.list_lengths().max()) + seg - 1) // seg
    try:
        capi.set_option("seg_rows", seg)
        assert kp_of(top_k) == 34 and kept > 1024, kept
        assert nprobe * s_max * 34 <= 131072            # (so the counting merge IS tried)
        r = audit_single(ix, Q, range(2), top_k, nprobe, f"{kept} tied keys inside the cut", maxima="pristine")
    finally:
        capi.set_option("seg_rows", 0)
    assert r["fallback"] == 4, r["fallback"]            # one per search: two queries, host and device call
    ix.close()


@pytest.mark.parametrize("metric", [0, 1])
def test_flat_more_ties_inside_the_cut_than_the_counting_merge_holds(metric):
    """every even row a copy of row 0, the query row 0: each of the scan's blocks leaves 34 keys of one val in its slot"""
    n, d, top_k = 16384, 64, 10
    X = dg.dist_u(0xF50, n, d)
    X[::2] = X[0]
    fc = capi.FlatCorpus(d)
    st = flat_upload_checked(fc, X)
    blocks = min(st["n_slots"], (n // 64 + 3) // 4)     # (flat_shadow_search1: a block of four waves per four tiles, at most n_slots)
    assert blocks == min(st["n_slots"], 64) and blocks >= 31 and kp_of(top_k) * blocks > 1024, (st, blocks)
    w, nv, failed = audit_flat(fc, X, X, [0], top_k, metric, "8192 tied rows")
    assert failed == [0] and testhooks.flat_shadow_state(fc)["failed"] == 1
    assert nv == kp_of(top_k) * blocks
    fc.close()


# ---- (g) one query after mutations ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("way", ["add_batch", "single adds", "add_batch into freed slack"])
def test_one_query_after_mutations(way):
    """the three ways of test_aligned_shadow_residuals_arrive_after_the_build (tests/test_certificate_mutation_gpu.py), then a
    remove_batch of every third id and a compact: single queries audited at every step.  The maxima the bound charges: those of every row
    ever stored until the first removal, at least the live rows' afterwards, exactly the live rows' after compact."""
    n, d, k, top_k, m = 4096, 128, 8, 10, 512
    rng = np.random.default_rng(0x5AF)
    sgn = rng.choice([-1.0, 1.0], d).astype(np.float32)
    X = ((0.03125 + rng.integers(0, 1024, (n, d)) * 2.0 ** -15) * rng.choice([-1.0, 1.0], (n, d))).astype(np.float32)
    assert np.array_equal(X.astype(np.float16).astype(np.float32), X)
    A = ((0.03125 + rng.integers(0, 1024, (m, d)) * 2.0 ** -15) * rng.choice([-1.0, 1.0], (m, d))).astype(np.float32)
    A = (A + sgn[None, :] * np.float32(0.49 * 2.0 ** -15)).astype(np.float32)
    assert not np.any(A.astype(np.float16).astype(np.float32) == A)
    Q = np.tile((sgn / np.sqrt(np.float32(d)))[None, :], (12, 1)).astype(np.float32)
    Q += (1e-3 * rng.standard_normal((12, d))).astype(np.float32)
    ix = IVFFlatIndex.build_index(k, 1, 2, X, init_indices=mg.init_draws(0x5AF, 1, k, n))
    assert ix.shadow_state()["active"]
    r = audit_single(ix, Q, SIX, top_k, k, f"fp16-exact rows ({way})")
    assert r["info"]["r2"] == 0.0
    removed = False
    if way == "add_batch":
        ix.add_batch(A)
    elif way == "single adds":
        for x in A:
            ix.add(x)
    else:
        cl = np.array([co.add_cluster(ix.centroids, x) for x in A])
        gone = np.concatenate([np.asarray(l[::3], dtype=np.int64) for l in ix.ids])
        assert np.all(np.bincount(cl, minlength=k) <= np.array([len(l[::3]) for l in ix.ids])), "the added rows would not fit the freed slack"
        assert ix.remove_batch(gone) == gone.size
        removed = True
        ix.add_batch(A)
    r = audit_single(ix, Q, SIX, top_k, k, f"aligned residuals by {way}", maxima="upper" if removed else "pristine")
    assert r["info"]["r2"] == r2_ref(ix.values) > 0.0
    live = live_ids(ix)
    assert ix.remove_batch(live[::3]) == live[::3].size
    audit_single(ix, Q, SIX, top_k, k, "... remove_batch of every third id", maxima="upper")
    ix.compact()
    live = live_ids(ix)
    r = audit_single(ix, Q, SIX, top_k, k, "... compact", maxima="tight")
    assert r["info"]["xmax2"] == xmax2_ref(ix.values[live]) and r["info"]["r2"] == r2_ref(ix.values[live])
    ix.close()


# ---- (h) device queries that are not 16-byte aligned --------------------------------------------------------------------------------
def test_unaligned_device_queries():
    """d == ld == 128: a single _dev query is read where the caller left it when it is 16-byte aligned and re-staged otherwise
    (flat_search_dev_locked, plan_search).  A pointer one float into a larger tensor: the aligned call's bits."""
    n, d, k, top_k, nprobe = 6000, 128, 12, 10, 6
    X = corpus("dist_c", n, d, 0xA60)
    Q = corpus("dist_c", 4, d, 0xA61)
    io = DevIO(top_k)
    fc = capi.FlatCorpus(d)
    flat_upload_checked(fc, X)
    ix = IVFFlatIndex.build_index(k, 1, 3, X, init_indices=mg.init_draws(0xA60, 1, k, n))
    for qi in range(4):
        for metric in (0, 1):
            got = []
            for off in (0, 1):
                ptr = io.put(Q[qi], off)
                assert ptr % 16 == 4 * off
                fc.search_dev(ptr, d, 1, top_k, metric, io.ids.data_ptr(), io.dist.data_ptr(), io.cnt.data_ptr(), 0)
                got.append(io.result())
                fc.poll(0)
                vids, vals, bnd, info = testhooks.flat_last_vals(fc, Q[qi], top_k, metric)
                assert worst_of(X, Q[qi], metric, vids, vals, bnd, info, ("flat", qi, metric, off)) <= 1.0
            oi, od = co.search_exhaustive(X, Q[qi], top_k, metric)
            for ids, dist in got:
                assert np.array_equal(ids, oi) and np.array_equal(bits(dist), bits(od)), ("flat", qi, metric)
        oi, od = co.search_nprobe(ix.values, ix.centroids, ix.ids, Q[qi], top_k, nprobe)
        for off in (0, 1):
            b0 = ix.prescan_stats()["batches"]
            ids, dist = ivf_search1(ix, Q[qi], top_k, nprobe, "dev", io, offset_floats=off)
            assert ix.prescan_stats()["batches"] == b0 + 1
            vids, vals, bnd, info = testhooks.last_vals(ix, 0, cap=32768)
            assert worst_of(X, Q[qi], 0, vids, vals, bnd, info, ("ivf", qi, off)) <= 1.0
            assert np.array_equal(ids, oi) and np.array_equal(bits(dist), bits(od)), ("ivf", qi, off)
    fc.close()
    ix.close()
