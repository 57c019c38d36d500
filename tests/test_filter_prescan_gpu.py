"""vers_ivf_search_filtered behind the matrix-core scan of the allowed rows on the fp16 shadow (csrc/filter_prescan.hip.h; option
"filter_prescan", vers_ivf_filter_prescan_stats).  The scan only pre-selects and the finish is the unfiltered search's exact one, so ids,
order, counts and distance BITS must equal the oracle's -- the unfiltered search on an index with the other ids removed, exactly as
tests/test_filtered_gpu.py builds it -- with np.array_equal."""
import numpy as np
import pytest

from tests import datagen as dg
from tests.golden import make_golden as mg
from tests.test_certificate_gpu import corpus
from tests.test_filtered_gpu import Ref, allowed_set, check_probed, make, queries, random_filter
from vers_amd import capi
from vers_amd.index import IVFFlatIndex

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def prescan_on():
    capi.set_option("filter_prescan", 1)   # (the library's default is 0: DESIGN.md section 6)
    yield
    capi.set_option("filter_prescan", 0)


B = 40   # two full groups of 16 and one of 8 on the most probed list
SHAPES = {"d96": (6000, 96, 12, 6), "d300": (6000, 300, 2, 2),   # n, d, k, nprobe; d = 300: ld 320 (padded columns), lists of ~47 tiles
          "d40": (600, 40, 12, 6)}   # ld 64: a tile is two steps, fewer than the load ring primes; lists of ~50 rows: most items are one tile
TOP_KS = (1, 10, 48)


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


def filters(ix, n, nprobe, Q):
    """everything | random 50 % | random 2 % | a contiguous id range that ends inside a tile | empty | five ids of the first query's nearest
    list: fewer than top_k allowed rows in reach"""
    near = int(np.argmin(((ix.centroids - Q[0]) ** 2).sum(1)))
    few = np.asarray(ix.ids[near][3:8], dtype=np.uint64)
    return [np.ones(n, dtype=bool), random_filter(n, 0.5, 0xB501), random_filter(n, 0.02, 0xB502), np.arange(700, 2737, dtype=np.uint64),
            np.zeros(n, dtype=bool), few]


def check_all(ix, Q, nprobe, n):
    before = ix.filter_prescan_stats()
    calls = 0
    for allowed in filters(ix, n, nprobe, Q):
        ref = Ref(ix, Q, allowed_set(n, allowed, n))
        for top_k in TOP_KS:
            _, _, cnt = check_probed(ref, top_k, nprobe, allowed, n)
            calls += 1
        if allowed.dtype != np.bool_ and allowed.size == 5:
            assert cnt.max() <= 5 < top_k   # counts below top_k: padded as the chain path pads
    after = ix.filter_prescan_stats()
    assert after["calls"] - before["calls"] == calls   # the new path served every one of them


@pytest.mark.parametrize("kind", ["dist_c", "norm_300", "mixed_subnormal", "aligned"])
@pytest.mark.parametrize("metric", [capi.METRIC_L2SQ, capi.METRIC_COSDIST])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_filtered_prescan_equals_the_oracle(shape, metric, kind):
    n, d, k, nprobe = SHAPES[shape]
    X, Q = rows_and_queries(kind, n, d, 0xB500 + metric)
    ix = IVFFlatIndex.build_index(k, 1, 3, X, init_indices=mg.init_draws(0xB511, 1, k, n), metric=metric)
    try:
        assert ix.shadow_state()["active"]
        check_all(ix, Q, nprobe, n)
    finally:
        ix.close()


def test_items_of_more_than_64_tiles():
    ix = make(12000, 32, 2, seed=0xF180)   # (tests/test_filtered_gpu.py's construction: the longer list reaches into a second window)
    try:
        assert max(len(l) for l in ix.ids) > 4096 + 64
        capi.set_option("seg_rows", 8192)
        check_all(ix, queries(ix, 0xB520, B), 2, 12000)
    finally:
        capi.set_option("seg_rows", 0)
        ix.close()


@pytest.fixture(scope="module")
def main_case():
    ix = make(6000, 96, 12)
    Q = queries(ix, 0xB530, B)
    allowed = random_filter(6000, 0.5, 0xB531)
    yield ix, Q, allowed, Ref(ix, Q, allowed)
    ix.close()


def test_the_counter_tells_the_paths_apart(main_case):
    ix, Q, allowed, ref = main_case
    s0 = ix.filter_prescan_stats()
    check_probed(ref, 10, 6, allowed)
    s1 = ix.filter_prescan_stats()
    assert s1["calls"] - s0["calls"] == 1 and s1["fallback_queries"] == s0["fallback_queries"]
    f = ix.filter_stats()["last"]
    assert 0 < f["tiles_loaded"] <= f["tiles_planned"]   # vers_ivf_filter_stats keeps counting on the new path
    capi.set_option("filter_prescan", 0)
    check_probed(ref, 10, 6, allowed)
    assert ix.filter_prescan_stats() == s1   # the chains: the counters do not move
    capi.set_option("filter_prescan", 1)
    check_probed(ref, 10, 6, allowed, qs=[0, 1])   # a batch below the matrix-core scan's smallest keeps the chains
    check_probed(ref, 49, 6, allowed)              # ... and so does a result wider than the candidate lists allow
    assert ix.filter_prescan_stats() == s1


def test_every_certificate_fails_and_the_fallback_serves(main_case):
    ix, Q, allowed, ref = main_case
    found = capi.env_option("prescan", 1)
    s0 = ix.filter_prescan_stats()
    try:
        capi.set_option("prescan", 2)
        for top_k in TOP_KS:
            check_probed(ref, top_k, 6, allowed)
    finally:
        capi.set_option("prescan", found)
    s1 = ix.filter_prescan_stats()
    assert s1["calls"] - s0["calls"] == len(TOP_KS) and s1["fallback_queries"] - s0["fallback_queries"] == len(TOP_KS) * B


def test_mutated_index_not_compacted():
    ix = make(6000, 96, 12, seed=0xB540)
    try:
        ix.add_batch(dg.dist_c(0xB541, 500, ix.d, 2 * ix.num_centroids, dg.default_sigma(ix.d)))
        ix.remove_batch(list(range(0, 6000, 3)))
        n = 6500
        Q = queries(ix, 0xB542, B)
        s0 = ix.filter_prescan_stats()
        for allowed in (np.ones(n, dtype=bool), random_filter(n, 0.5, 0xB543)):
            ref = Ref(ix, Q, allowed)
            for top_k in (10, 48):
                check_probed(ref, top_k, 6, allowed)
        assert ix.filter_prescan_stats()["calls"] - s0["calls"] == 4
    finally:
        ix.close()


@pytest.mark.parametrize("bad_allowed", [True, False])
def test_nan_row(bad_allowed):
    """an ALLOWED NaN row: the chain path's status; a NaN row outside the filter: never looked at, the result is clean"""
    src = make(1500, 48, 6, seed=0xF1E0)
    ix = IVFFlatIndex(48)
    try:
        bad = int(src.ids[2][70])   # a row in the second tile of list 2
        ix.num_centroids, ix.centroids, ix.assignments, ix.ids = src.num_centroids, src.centroids, src.assignments, [list(l) for l in src.ids]
        ix.values = src.values.copy()
        ix.values[bad, 7] = np.nan
        ix._upload()
        Q = queries(src, 0xB550, B)
        allowed = random_filter(1500, 0.5, 0xB551)
        allowed[[int(v) for v in src.ids[2][64:128]]] = True   # the rest of its tile is allowed: the tile IS loaded
        allowed[bad] = bad_allowed
        s0 = ix.filter_prescan_stats()
        if bad_allowed:
            with pytest.raises(capi.VersError) as e:
                ix.search_filtered(Q, 10, 6, allowed)
            assert e.value.status == capi.ERR_NAN
        else:
            check_probed(Ref(ix, Q, allowed), 10, 6, allowed)
            assert ix.filter_prescan_stats()["fallback_queries"] == s0["fallback_queries"]   # no allowed row was poisoned
        assert ix.filter_prescan_stats()["calls"] - s0["calls"] == 1
    finally:
        ix.close()
        src.close()
