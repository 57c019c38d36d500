"""The probed range search behind the matrix-core pre-filter on the fp16 shadow (csrc/range_prescan.hip.h; option "range_prescan",
vers_ivf_range_stats).  The filter only rules out rows that are provably beyond the radius and the finish is the reference's ordered chain,
so limits, ids and distance BITS must equal the oracle's -- co.search_nprobe with top_k = every live row, cut at dist <= r, exactly as
tests/test_range_gpu.py builds it -- with np.array_equal, in both orders."""
import numpy as np
import pytest

from tests import datagen as dg
from tests.test_certificate_gpu import corpus
from tests.test_range_gpu import INF, Ref, check_range, make, queries, radii_mth, raw_call
from vers_amd import capi
from vers_amd.index import IVFFlatIndex

pytestmark = pytest.mark.gpu

@pytest.fixture(autouse=True)
def prescan_on():
    capi.set_option("range_prescan", 1)   # (the library's default is 0: DESIGN.md section 6)
    yield
    capi.set_option("range_prescan", 0)


B = 40   # two full groups of 16 and one of 8 on the most probed list
SHAPES = {"d96": (6000, 96, 12, 6), "d300": (6000, 300, 2, 2),   # n, d, k, nprobe; d = 300: ld 320 (padded columns), lists of ~47 tiles
          "d40": (600, 40, 12, 6)}   # ld 64: a tile is two steps, fewer than the load ring primes; lists of ~50 rows: most items are one tile


def rows_and_queries(kind, n, d, seed):
    if kind != "aligned":
        return corpus(kind, n, d, seed), corpus(kind, B, d, seed + 0x10)
    # every element 0.49 ulp(fp16) off its fp16 value on the side of the query's sign: the residual x - fp16(x) is parallel to q
    rng = np.random.default_rng(seed)
    h = (0.03125 + rng.integers(0, 1024, (n, d)) * 2.0 ** -15).astype(np.float32)
    sgn = rng.choice([-1.0, 1.0], d).astype(np.float32)
    X = ((h * rng.choice([-1.0, 1.0], (n, d))).astype(np.float32) + sgn[None, :] * np.float32(0.49 * 2.0 ** -15)).astype(np.float32)
    Q = np.tile((sgn / np.sqrt(np.float32(d)))[None, :], (B, 1)).astype(np.float32) + (1e-3 * rng.standard_normal((B, d))).astype(np.float32)
    return X, Q


def all_radii(ref):
    """per query EXACTLY the 1st / 10th / 100th nearest probed distance (the boundary row must survive the filter), the f32 just below the
    nearest (an empty result), +inf and -1"""
    below = np.nextafter(radii_mth(ref, 1), np.float32(-np.inf))
    return [radii_mth(ref, 1), radii_mth(ref, 10), radii_mth(ref, 100), below, INF, np.float32(-1.0)]


@pytest.mark.parametrize("kind", ["dist_c", "norm_300", "mixed_subnormal", "aligned"])
@pytest.mark.parametrize("metric", [capi.METRIC_L2SQ, capi.METRIC_COSDIST])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_prefiltered_range_search_equals_the_oracle(shape, metric, kind):
    n, d, k, nprobe = SHAPES[shape]
    X, Q = rows_and_queries(kind, n, d, 0xA500 + metric)
    ix = make(n, d, k, metric=metric, seed=0xA510, iters=3, X=X)
    try:
        assert ix.shadow_state()["active"]
        ref = Ref(ix, Q, nprobe)
        before = ix.range_stats()
        for i, r in enumerate(all_radii(ref)):
            lims, _, _ = check_range(ref, r, singles=False)
            assert i != 3 or int(lims[-1]) == 0   # just below the nearest: empty
        assert ix.range_stats()["calls"] > before["calls"]   # the new path served them
        if kind == "dist_c" and shape == "d96" and metric == capi.METRIC_L2SQ:
            counters_and_mutations(ix, ref)
    finally:
        ix.close()


def counters_and_mutations(ix, ref):
    """on the Dist-C case at the 10th-nearest radius: the counters; then the same index after add_batch + remove_batch, not compacted"""
    radii, Q, nprobe = radii_mth(ref, 10), ref.Q, ref.nprobe
    lims, _, _ = ix.range_search(Q, radii, nprobe)   # (sizes the binding's capacity: the next call is ONE call of the C ABI)
    s0 = ix.range_stats()
    lims, _, _ = ix.range_search(Q, radii, nprobe)
    s1 = ix.range_stats()
    pairs = sum(len(ix.ids[c]) for p in ref.probes for c in p)
    assert s1["calls"] - s0["calls"] == 1 and s1["pairs"] - s0["pairs"] == pairs and s1["hits"] - s0["hits"] == int(lims[-1])
    assert s1["hits"] - s0["hits"] <= s1["candidates"] - s0["candidates"] < pairs   # the filter ran and ruled something out
    try:
        capi.set_option("range_prescan", 0)
        check_range(ref, radii, singles=False)
        assert ix.range_stats() == s1   # the chains: the counters do not move
    finally:
        capi.set_option("range_prescan", 1)
    ix.add_batch(dg.dist_c(0xA520, 500, ix.d, 2 * ix.num_centroids, dg.default_sigma(ix.d)))
    ix.remove_batch(list(range(0, 6000, 3)))
    ref2 = Ref(ix, Q, nprobe)   # the shadow, |x|^2 and the maxima must still carry the cut
    for r in (radii_mth(ref2, 1), radii_mth(ref2, 10), radii_mth(ref2, 100)):
        check_range(ref2, r, singles=False)
    assert ix.range_stats()["calls"] > s1["calls"]


@pytest.mark.parametrize("poison", [1e5, np.nan])
def test_non_finite_rows(poison):
    """1e5 is fp16 inf: the measured residual is infinite, every row stays a candidate and the result is the oracle's.  A NaN in a probed
    row: the status of the chain path (option 0)."""
    src = make(3000, 96, 8, seed=0xA530)
    ix = IVFFlatIndex(96)
    try:
        ix.num_centroids, ix.centroids, ix.assignments, ix.ids = src.num_centroids, src.centroids, src.assignments, [list(l) for l in src.ids]
        ix.values = src.values.copy()
        ix.values[int(src.ids[2][70]), 7] = poison
        ix._upload()
        Q = queries(src, 0xA531, B)
        if poison == poison:
            ref = Ref(ix, Q, 8)   # every list probed
            for r in (radii_mth(ref, 10), INF):
                check_range(ref, r, singles=False)
        else:
            rcs = []
            for opt in (1, 0):
                capi.set_option("range_prescan", opt)
                rcs.append(raw_call(ix, Q, INF, 8, 0, 0)[0])
                rcs.append(raw_call(ix, Q, 0.5, 8, 0, 0)[0])
            assert rcs == [capi.ERR_NAN] * 4
    finally:
        ix.close()
        src.close()
