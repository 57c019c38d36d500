"""The coarse quantiser's and the k-means assign pass's certificates, audited with measurements.

Both pre-filters charge E, a bound on |approximate value - reference distance| (gemm.hip.h), and certify a result only if no
centroid outside the candidates can win within E.  On corpora whose nearest centroid wins by far more than E a bound that is too
small never changes a result, so bit-exact end-to-end tests cannot see it.  Here every approximate value the kernels produced is
held against the reference's ordered chain:
  coarse   (vers_ivf_test_last_coarse): | G + |q|^2 - D_ref | <= E for every centroid of the dumped queries (cosine: | 1 + G - D_ref |),
           G, |q|^2 and E as the selection kernel saw them;
  assign   (vers_test_assign_filter, every filter forced in turn): the candidate's value, the second-smallest value g2 and, per tile of
           128 centroids, the smallest and second-smallest value (what assign_tile_rescan_kernel picks its tiles and halves by) -- each
           within E of the matching order statistic of the reference's distances (order statistics are 1-Lipschitz);
  bf16x3   on its own (vers_test_mfma kind 4, host-split operands): the split's share of G against kX3Slack (|a|^2 + |b|^2).
The worst ratio of each certificate, filter, metric and corpus is printed (DESIGN.md sections 1 and 8 quote them)."""
import numpy as np
import pytest

from oracle import c_oracle as co
from oracle import np_oracle as npo
from tests import datagen as dg
from tests.golden import make_golden as mg
from vers_amd import capi, testhooks
from vers_amd.index import IVFFlatIndex

pytestmark = pytest.mark.gpu
F32 = np.float32
X0 = F32(1.0 + 2.0 ** -8 - 2.0 ** -17 - 2.0 ** -23)   # bf16 split: hi = 1, lo = 2^-8 - 2^-16, residual 2^-17 - 2^-23 (aligned with x)
PARENT_SLACK = 1.6e-5                                   # what the bf16x3 share was charged before (printed for the record)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def bf16_bits(x):
    """round-to-nearest-even f32 -> bf16 bit patterns (the split kernels' conversion)"""
    b = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_f32(b):
    return (b.astype(np.uint32) << 16).view(np.float32)


def split(x):
    hi = bf16_bits(x)
    lo = bf16_bits((np.asarray(x, dtype=np.float32) - bf16_f32(hi)).astype(np.float32))
    return hi, lo


def ref_matrix(X, Cn, metric):
    """the reference's distances of every (point, centroid) pair, n x k, in its own arithmetic: a strictly ordered f32 chain over the
    columns, product and sum rounded separately (base.rs:119-126; cosine 1 - dot, base.rs:91-93,153-155).  One elementwise op per
    rounding on the GPU (no fusion in eager mode); a sample is checked bit for bit against the C oracle."""
    import torch
    dev = torch.device("cuda:0")
    x = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)).to(dev)
    c = torch.from_numpy(np.ascontiguousarray(Cn, dtype=np.float32)).to(dev)
    acc = torch.zeros((x.shape[0], c.shape[0]), dtype=torch.float32, device=dev)
    for j in range(x.shape[1]):
        if metric == 0:
            t = torch.sub(x[:, j, None], c[None, :, j])
            acc = torch.add(acc, torch.mul(t, t))
        else:
            acc = torch.add(acc, torch.mul(x[:, j, None], c[None, :, j]))
    if metric:
        acc = torch.sub(torch.ones_like(acc), acc)
    D = acc.cpu().numpy()
    rng = np.random.default_rng(X.shape[0] * 31 + Cn.shape[0])
    for _ in range(16):
        i, j = int(rng.integers(X.shape[0])), int(rng.integers(Cn.shape[0]))
        want = F32(1.0) - co.dot(X[i], Cn[j]) if metric else co.squared_euclidean(X[i], Cn[j])
        assert bits(D[i, j]) == bits(np.float32(want)), (i, j, D[i, j], want)
    return D


# ---- the bf16x3 product on its own ---------------------------------------------------------------------------------------------------
def coarse_slack():
    """the slack constant the coarse selection charges for the bf16x3 share, as the coarse hook reports it"""
    n, d, k = 2000, 64, 16
    X = dg.dist_c(0xB16, n, d, 32, dg.default_sigma(d))
    ix = IVFFlatIndex.build_index(k, 1, 2, X, init_indices=mg.init_draws(0xB16, 1, k, n))
    try:
        ix.search_batch(X[:32], 5, 4)
        _, info = testhooks.last_coarse(ix, 0)
    finally:
        ix.close()
    return info["slack"]


def aligned_operands(K, rng, scale_rows=False):
    """32 rows / 32 columns of +-X0 with sign patterns: columns 0-7 parallel to rows 0-7, 8-15 antiparallel to rows 8-15, the rest random
    (optionally rows scaled by powers of two: the split is scale-free)"""
    s = rng.choice([-1.0, 1.0], (32, K)).astype(np.float32)
    t = rng.choice([-1.0, 1.0], (K, 32)).astype(np.float32)
    t[:, 0:8] = s[0:8].T
    t[:, 8:16] = -s[8:16].T
    A = (s * X0).astype(np.float32)
    if scale_rows:
        A = (A * (2.0 ** rng.integers(-3, 4, (32, 1)))).astype(np.float32)
    B = (t * X0).astype(np.float32)
    return A, B


def test_bf16x3_split_share_stays_inside_its_slack():
    """Host-split operands (hi = RNE bf16(x), lo = RNE bf16(x - hi)) through the three bf16 products of dist_gemm_x3_kernel, in its order,
    into one accumulator.  On +-X0 every product and partial sum is a multiple of 2^-16 below 2^8: the accumulation is exact, the measured
    error is the split's alone.  2 |mfma - <a, b>| (G = norm - 2 dot) must stay within slack (|a|^2 + |b|^2) -- the share the coarse and
    assign certificates charge.  (At the old 1.6e-5 this is 1.87: the test that found the bound derived for the wrong precision.)"""
    slack = coarse_slack()
    rng = np.random.default_rng(0xB163)
    worst = worst_parent = 0.0
    for K, scaled in ((64, False), (128, False), (128, True)):
        A, B = aligned_operands(K, rng, scaled)
        ah, al = split(A)
        bh, bl = split(B)
        assert np.all(np.abs(bf16_f32(ah)) * F32(2.0 ** -8 - 2.0 ** -16) == np.abs(bf16_f32(al)))   # hi = +-2^e, lo = +-2^e (2^-8 - 2^-16)
        got = testhooks.mfma(4, np.stack([ah, al]), np.stack([bh, bl])).astype(np.float64)
        exact = A.astype(np.float64) @ B.astype(np.float64)
        share = (np.sum(A.astype(np.float64) ** 2, axis=1)[:, None] + np.sum(B.astype(np.float64) ** 2, axis=0)[None, :])
        gerr = 2.0 * np.abs(got - exact)
        r, rp = float((gerr / (slack * share)).max()), float((gerr / (PARENT_SLACK * share)).max())
        print(f"bf16x3 split share, aligned +-X0, K = {K:4d}{' rows scaled 2^-3..2^3' if scaled else ''}: worst G error / (slack (|a|^2 + |b|^2)) "
              f"= {r:.4f} at slack {slack:.4g}  ({rp:.3f} at the former {PARENT_SLACK})")
        worst, worst_parent = max(worst, r), max(worst_parent, rp)
        assert r <= 1.0, (K, scaled, r)
    assert worst > 0.9, worst                    # the corpus does attain the bound: the test has teeth
    assert worst_parent > 1.0                    # ... and would have caught the former constant
    # random operands through the same path: the split's error is far below the share (sanity of the hook itself)
    A = rng.standard_normal((32, 256)).astype(np.float32); B = rng.standard_normal((256, 32)).astype(np.float32)
    ah, al = split(A); bh, bl = split(B)
    got = testhooks.mfma(4, np.stack([ah, al]), np.stack([bh, bl])).astype(np.float64)
    exact = A.astype(np.float64) @ B.astype(np.float64)
    s1 = np.abs(A.astype(np.float64)) @ np.abs(B.astype(np.float64))
    assert (np.abs(got - exact) <= (2.0 ** -15 + 256 * 2.0 ** -24) * s1).all()


# ---- the coarse quantiser ------------------------------------------------------------------------------------------------------------
def corpus(kind, n, d, seed):
    if kind == "dist_c":
        return dg.dist_c(seed, n, d, 48, dg.default_sigma(d))
    if kind == "dist_u":
        return dg.dist_u(seed, n, d)
    if kind == "norm_300":
        return (dg.dist_c(seed, n, d, 48, dg.default_sigma(d)) * np.float32(300.0)).astype(np.float32)
    if kind == "mixed_subnormal":
        X = dg.dist_c(seed, n, d, 48, dg.default_sigma(d))
        X[:, ::3] *= np.float32(2.0 ** -13)
        return X
    raise ValueError(kind)


def coarse_worst(ix, Q, metric, queries):
    Cn = ix.centroids
    worst = 0.0
    for qi in queries:
        g, info = testhooks.last_coarse(ix, qi)
        assert len(g) == Cn.shape[0] and info["metric"] == metric and np.isfinite(info["E"]) and info["E"] > 0
        D = npo._dist(Cn, Q[qi][None, :], metric).astype(np.float64)
        off = 1.0 if metric else info["qn"]
        worst = max(worst, float((np.abs(g.astype(np.float64) + off - D) / info["E"]).max()))
    return worst, info


@pytest.mark.parametrize("x3", [1, 0])
@pytest.mark.parametrize("metric", [0, 1])
def test_coarse_certificate_holds_for_every_centroid(metric, x3):
    n, b = 6000, 64
    capi.set_option("gemm_x3", 3 if x3 else 1)
    try:
        for d in (16, 64, 96, 768):
            for kind in ("dist_c", "dist_u", "norm_300", "mixed_subnormal"):
                X = corpus(kind, n, d, 0xC0A + d + metric)
                Q = corpus(kind, b, d, 0xC1A + d + metric)
                k = 160
                ix = IVFFlatIndex.build_index(k, 1, 2, X, init_indices=mg.init_draws(0xC0A + d, 1, k, n), metric=metric)
                try:
                    for nprobe in (8, 60):   # the narrow selection (a key per lane) and the wide one (P + 16 > 64)
                        b0 = ix.coarse_stats()["mfma_batches"]
                        ix.search_batch(Q, 10, nprobe)
                        assert ix.coarse_stats()["mfma_batches"] == b0 + 1
                        w, info = coarse_worst(ix, Q, metric, range(0, b, 3))
                        assert info["x3"] == x3 and info["d_pad"] >= d and info["P"] == nprobe
                        print(f"coarse {'bf16x3' if x3 else 'f32   '} metric {metric} d {d:4d} {kind:16s} nprobe {nprobe:2d}: "
                              f"worst |G + |q|^2 - D_ref| / E = {w:.4f}")
                        assert w <= 1.0, (d, kind, nprobe, w)
                finally:
                    ix.close()
    finally:
        capi.set_option("gemm_x3", 3)


# ---- the k-means assign pass ---------------------------------------------------------------------------------------------------------
def order2(D):
    """smallest and second-smallest value of every row"""
    p = np.partition(D, 1, axis=-1)
    return p[..., 0], p[..., 1]


def assign_audit(X, Cn, metric, mode, D=None):
    """runs the forced filter, checks every audited value against D_ref and the final result against the reference; returns (worst ratio, r)"""
    n, k = X.shape[0], Cn.shape[0]
    r = testhooks.assign_filter(X, Cn, metric, mode)
    assert r["batches"] == 1 and r["status"] == 0
    assert r["wide"] == (mode >= 2 or (mode == 1 and k % 256 == 0)) and r["hi_only"] == (mode >= 2) and r["used_h"] == (mode == 3)
    if D is None:
        D = ref_matrix(X, Cn, metric)
    D64 = D.astype(np.float64)
    want = np.argmin(D, axis=1)                             # first minimum: the reference's min_by
    assert np.array_equal(r["assign"], want), int(np.sum(r["assign"] != want))
    assert np.array_equal(bits(r["mind"]), bits(D[np.arange(n), want]))
    off = np.ones(n) if metric else npo.dot(X, X).astype(np.float64)   # |x|^2 exactly as assign_rescore_kernel sums it
    E = r["E"].astype(np.float64)
    fin = np.isfinite(E)
    assert not np.isnan(E).any() and (E[fin] > 0).all()
    nt = r["n_tiles"]
    pv1, pv2, pc1 = r["part_v1"].astype(np.float64), r["part_v2"].astype(np.float64), r["part_c1"].astype(np.int64)
    # the candidate and g2
    cand = r["cand"].astype(np.int64)
    assert np.all(pc1[cand // 128, np.arange(n)] == cand)
    v_cand = pv1[cand // 128, np.arange(n)]
    assert np.all(v_cand == pv1.min(axis=0))
    d1, d2 = order2(D64)
    pad = nt * 128 - k
    Dt = np.concatenate([D64, np.full((n, pad), np.inf)], axis=1).reshape(n, nt, 128) if pad else D64.reshape(n, nt, 128)
    t1, t2 = order2(Dt)                                     # per tile: smallest, second smallest [n, nt]
    with np.errstate(invalid="ignore"):   # (an infinite E -- elements beyond fp16's range -- certifies nothing: such ratios are dropped)
        ratios = [np.abs(v_cand + off - D64[np.arange(n), cand]) / E, np.abs(r["g2"].astype(np.float64) + off - d2) / E,
                  (np.abs(pv1.T + off[:, None] - t1) / E[:, None]).ravel(), (np.abs(pv2.T + off[:, None] - t2) / E[:, None])[np.isfinite(t2)]]
    tiles = np.arange(nt)[:, None]
    assert np.all((pc1 >= tiles * 128) & (pc1 < np.minimum(k, tiles * 128 + 128))), "part_c1 outside its tile"
    worst = max(float(np.nanmax(x[np.isfinite(x)])) if np.isfinite(x).any() else 0.0 for x in ratios)
    # fb_thr: queued points of the tile re-scan carry a threshold, no tile that holds the reference's first minimum lies above it
    q = r["queued"]
    if r["tile_rescan"]:
        qf = q & fin
        thr = r["thr"].astype(np.float64)
        assert np.isfinite(thr[qf]).all()
        tw = want // 128
        assert np.all(~(pv1[tw, np.arange(n)][qf] > thr[qf]))   # the tile that holds the reference's first minimum is a candidate ...
        same_half = ((want % 128) >= 64) == ((pc1[tw, np.arange(n)] % 128) >= 64)
        assert np.all((same_half | ~(pv2[tw, np.arange(n)] > thr))[qf])   # ... and so is its half (the re-scan's half selection)
    assert int(q.sum()) == r["n_queued"]
    return worst, r


ASSIGN_SHAPES = [(4096, 768, 4096), (1024, 64, 4096), (512, 16, 4096)]


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("k,d,n", ASSIGN_SHAPES)
def test_assign_certificate_every_filter(k, d, n, metric):
    X = dg.dist_c(0xA55 + d, n, d, k // 2, dg.default_sigma(d))
    Cn = X[(np.arange(k) * 7919) % n].copy()
    Cn = (Cn + np.float32(0.05 / np.sqrt(d)) * dg.dist_u(0xA56 + d, k, d)).astype(np.float32)   # (no centroid equals a point)
    D = ref_matrix(X, Cn, metric)
    for mode in (0, 1, 2, 3):
        if mode == 3 and d % 128:
            continue   # (dist_gemm_h_kernel reads whole 128-column groups: the assign pass never picks it at this d)
        w, r = assign_audit(X, Cn, metric, mode, D)
        print(f"assign {testhooks.ASSIGN_MODES[mode]:36s} metric {metric} k {k:4d} d {d:3d}: worst |value - D_ref| / E = {w:.4f} "
              f"(candidate, g2, tile minima and seconds; {r['n_queued']} of {n} open, {r['n_full']} to the full scan)")
        assert w <= 1.0, (mode, w)


def aligned_split_corpus(n, k, d, seed):
    """(i) +-X0 elements: every row's bf16 residual is aligned with the row; points parallel to centroids (scaled by 1 or 1/2)"""
    rng = np.random.default_rng(seed)
    Cn = (rng.choice([-1.0, 1.0], (k, d)) * X0 * (2.0 ** rng.integers(-1, 1, (k, 1)))).astype(np.float32)
    src = rng.integers(0, k, n)
    X = (Cn[src] * (2.0 ** rng.integers(-1, 1, (n, 1)))).astype(np.float32)
    return X, Cn


def aligned_f16_corpus(n, k, d, seed):
    """(ii) elements 0.49 ulp(fp16) off their fp16 value along one sign pattern: the residuals x - fp16(x) of points and centroids are
    parallel to each other and to the rows (the Cauchy-Schwarz steps of the single product's bound are attained)"""
    rng = np.random.default_rng(seed)
    sgn = rng.choice([-1.0, 1.0], d).astype(np.float32)
    def rows(m):
        h = (0.03125 + rng.integers(0, 1024, (m, d)) * 2.0 ** -15).astype(np.float32)   # fp16 values in [2^-5, 2^-4): ulp 2^-15
        return (h * sgn + sgn * np.float32(0.49 * 2.0 ** -15)).astype(np.float32)
    X, Cn = rows(n), rows(k)
    assert np.all(X.astype(np.float16).astype(np.float32) != X)
    return X, Cn


@pytest.mark.parametrize("metric", [0, 1])
def test_assign_certificate_adversarial_corpora(metric):
    for d in (64, 128):
        X, Cn = aligned_split_corpus(2048, 256, d, 0xAD1 + d)
        D = ref_matrix(X, Cn, metric)
        for mode in (0, 1, 2, 3):
            if mode == 3 and d % 128:
                continue
            w, r = assign_audit(X, Cn, metric, mode, D)
            print(f"assign (i) bf16-split aligned  {testhooks.ASSIGN_MODES[mode]:36s} metric {metric} d {d:3d}: worst ratio {w:.4f} ({r['n_queued']} open)")
            assert w <= 1.0, (d, mode, w)
    X, Cn = aligned_f16_corpus(2048, 256, 128, 0xAD2)
    D = ref_matrix(X, Cn, metric)
    for mode in (2, 3, 1):
        w, r = assign_audit(X, Cn, metric, mode, D)
        print(f"assign (ii) fp16-residual aligned {testhooks.ASSIGN_MODES[mode]:36s} metric {metric} d 128: worst ratio {w:.4f} ({r['n_queued']} open)")
        assert w <= 1.0, (mode, w)
    # (iii) elements beyond fp16's range: the single product's residual is infinite -- such a point must never certify
    X, Cn = aligned_f16_corpus(1024, 256, 128, 0xAD3)
    big = np.arange(0, 1024, 7)
    X[big, 5] = np.float32(70000.0)
    X[big[::2], 77] = np.float32(-1.0e5)
    D = ref_matrix(X, Cn, metric)
    for mode in (2, 3):
        w, r = assign_audit(X, Cn, metric, mode, D)
        assert not np.isfinite(r["E"][big]).any() and r["queued"][big].all()
        print(f"assign (iii) elements beyond +-65504 {testhooks.ASSIGN_MODES[mode]:36s} metric {metric}: worst ratio {w:.4f} over the finite E; "
              f"all {len(big)} such points open")
        assert w <= 1.0, (mode, w)
    Cn2 = Cn.copy(); Cn2[100, 3] = np.float32(66000.0)   # a centroid beyond the range: R_c infinite, nothing certifies
    r = testhooks.assign_filter(X, Cn2, metric, 3)
    assert r["queued"].all() and np.array_equal(r["assign"], np.argmin(ref_matrix(X, Cn2, metric), axis=1))


# ---- the tile re-scan, end to end ----------------------------------------------------------------------------------------------------
CASCADE_OPTS = {"assign": 2, "assign_terms": 1, "assign_glds": 1}
DEFAULT_OPTS = {"assign": 0, "assign_terms": 0, "assign_glds": -1}   # (the values the library reads when an option was never set)


def assign_through_the_abi(X, Cn):
    """vers_kmeans_assign (the reference's metric) with the cascade forced: (assignments, minimum distances, assign_stats of the call)"""
    capi.assign_stats(reset=True)
    try:
        for name, v in CASCADE_OPTS.items():
            capi.set_option(name, v)
        a, md = capi.kmeans_assign(X, Cn, want_min_dist=True)
    finally:
        for name, v in DEFAULT_OPTS.items():
            capi.set_option(name, v)
    return a.astype(np.int64), md, capi.assign_stats(reset=True)


@pytest.mark.parametrize("metric", [0, 1])
def test_tile_rescan_half_selection_and_deferral(metric):
    d, k = 128, 256
    # pairs of centroids in one 128-centroid tile, one in each 64-row half (j and j + 64), within the fp16 window of their points
    base = dg.dist_u(0x7E6, 128, d)
    Cn = np.zeros((k, d), dtype=np.float32)
    eps = np.float32(0.004)
    X = []
    for p in range(128):
        t, j = divmod(p, 64)
        a, b = t * 128 + j, t * 128 + 64 + j
        Cn[a] = base[p] + eps * dg.dist_u(0x7E7 + p, 1, d)[0]
        Cn[b] = base[p] + eps * dg.dist_u(0x9E7 + p, 1, d)[0]
        for s in range(16):
            X.append(base[p] + eps * dg.dist_u(0xBE7 + 16 * p + s, 1, d)[0])
    X = np.asarray(X, dtype=np.float32)
    if metric:
        X = npo.normalize(X); Cn = npo.normalize(Cn)
    D = ref_matrix(X, Cn, metric)
    want = np.argmin(D, axis=1)
    r = testhooks.assign_filter(X, Cn, metric, 3)
    assert r["tile_rescan"] and r["n_queued"] > 0
    other_half = r["queued"] & ((want // 128) == (r["cand"] // 128)) & (((want % 128) >= 64) != ((r["cand"] % 128) >= 64))
    print(f"tile re-scan metric {metric}: {r['n_queued']} of {len(X)} open, {int(other_half.sum())} whose reference minimum sits in the other "
          f"half of the candidate's tile, {r['n_full']} to the full scan")
    assert other_half.sum() > 0
    assert np.array_equal(r["assign"], want) and np.array_equal(bits(r["mind"]), bits(D[np.arange(len(X)), want]))
    if metric == 0:
        a, md, (pts, fb) = assign_through_the_abi(X, Cn)
        assert pts == len(X) and np.array_equal(a, want) and np.array_equal(bits(md), bits(D[np.arange(len(X)), want]))
    # more than kRescanTiles = 8 candidate tiles: twelve copies of one centroid in twelve tiles -- the full exact scan decides
    k = 2048
    Cn = dg.dist_u(0x7E8, k, d)
    dup = np.arange(12) * 128 + 5
    Cn[dup] = Cn[dup[0]]
    X = (Cn[dup[0]][None, :] + np.float32(1e-3) * dg.dist_u(0x7E9, 64, d)).astype(np.float32)
    X = np.concatenate([X, dg.dist_u(0x7EA, 448, d)]).astype(np.float32)
    r = testhooks.assign_filter(X, Cn, metric, 3)
    D = ref_matrix(X, Cn, metric)
    want = np.argmin(D, axis=1)
    assert np.all(want[:64] == dup[0])
    assert r["n_full"] >= 64
    assert np.array_equal(r["assign"], want) and np.array_equal(bits(r["mind"]), bits(D[np.arange(len(X)), want]))
    msg = ""
    if metric == 0:
        a, md, (pts, fb) = assign_through_the_abi(X, Cn)
        assert pts == len(X) and fb >= 64, (pts, fb)
        assert np.array_equal(a, want) and np.array_equal(bits(md), bits(D[np.arange(len(X)), want]))
        msg = f"; through vers_kmeans_assign: assign_stats {fb} of {pts} re-done by the full scan"
    print(f"tile re-scan metric {metric}: 12 tied tiles -> {r['n_full']} points to the full exact scan{msg}")


# ---- production shapes against a full reference ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("k,d", [(4096, 768), (8192, 768), (4096, 1536), (8192, 1536)])
def test_production_shapes_default_rules(k, d, metric):
    """No forcing: the filter the options pick at this size (the probed cascade, the LDS-DMA contraction).  Every point against the
    ordered-chain GPU scan (option assign = 1, itself tested against the oracle), and against the C oracle every point the filter left
    open plus a seeded sample of 256 others."""
    n = 32768
    X = dg.dist_c(0x9D0 + d + k, n, d, k, dg.default_sigma(d))
    Cn = X[np.random.default_rng(k + d).choice(n, k, replace=False)].copy()
    Cn = (Cn + np.float32(0.1 / np.sqrt(d)) * dg.dist_u(0x9D1 + d, k, d)).astype(np.float32)
    if metric:
        Cn = npo.normalize(Cn)
    r = testhooks.assign_filter(X, Cn, metric, 4)
    assert r["status"] == 0 and r["batches"] >= 1
    D = ref_matrix(X, Cn, metric)
    full = np.argmin(D, axis=1).astype(np.uint32)
    del D
    assert np.array_equal(r["assign"], full), int(np.sum(r["assign"] != full))
    exact = None
    if metric == 0:   # (the C ABI's assign takes the reference's metric only)
        try:
            capi.set_option("assign", 1)
            exact = capi.kmeans_assign(X, Cn).astype(np.uint32)
        finally:
            capi.set_option("assign", 0)
    open_pts = np.flatnonzero(r["queued"])
    rng = np.random.default_rng(0x9D2 + k + d + metric)
    sample = np.union1d(open_pts, rng.choice(n, 256, replace=False))
    want = co.assign_to_clusters(X[sample], Cn, metric).astype(np.uint32)
    assert np.array_equal(r["assign"][sample], want), int(np.sum(r["assign"][sample] != want))
    ref_m = np.array([(F32(1.0) - co.dot(X[i], Cn[int(a)])) if metric else co.squared_euclidean(X[i], Cn[int(a)]) for i, a in zip(sample, want)],
                     dtype=np.float32)
    assert np.array_equal(bits(r["mind"][sample]), bits(ref_m))
    if exact is not None:
        assert np.array_equal(r["assign"], exact), int(np.sum(r["assign"] != exact))
    print(f"production k {k} d {d} metric {metric}: filter {'fp16 x1' if r['hi_only'] else 'bf16x3/f32'}{' (LDS-DMA)' if r['used_h'] else ''}, "
          f"{len(open_pts)} of {n} open, {r['n_full']} to the full scan; {len(sample)} points == the oracle"
          f", all == the ordered chains{' and the exact GPU scan' if exact is not None else ''}")
