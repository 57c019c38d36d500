"""Batches of the brute-force scan on the matrix cores (option "flat_prescan"; csrc/flat_prescan.hip.h) against the oracle's
search_exhaustive per query: ids and order identical, distances BIT-identical, counts equal -- and the path really taken
(vers_flat_prescan_stats), so that no case passes by falling back to the ordered chains."""
import numpy as np
import pytest

from oracle import c_oracle as co
from tests import datagen as dg
from vers_amd import capi

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check(fc, X, Q, k, metric=0):
    ids, dist, cnt = fc.search(Q, k, metric)
    for qi in range(len(Q)):
        oi, od = co.search_exhaustive(X, Q[qi], k, metric)
        assert cnt[qi] == len(oi)
        assert np.array_equal(ids[qi, :len(oi)], oi) and np.array_equal(bits(dist[qi, :len(oi)]), bits(od))


def corpus(n, d, b):
    X = dg.dist_u(0xF1A0 + n, n, d); Q = dg.dist_u(0xF2B0 + n, b, d)
    fc = capi.FlatCorpus(d); fc.upload(X)
    return X, Q, fc


# one tile, ld padding | padding rows in the last tile, widest kp | hi-only query block, several column blocks | d not a multiple of 16 |
# two query blocks, the second with one query | cosine on a partial block | many segments per query, threshold sharing | n < top_k |
# more than 32 queries at d = 768: the 64-query block is hi ONLY there (98 KB), on three waves
CASES = [(64, 4, 2, 5, 0), (65, 5, 3, 48, 1), (257, 768, 8, 10, 0), (3001, 300, 9, 7, 0), (5000, 128, 65, 10, 0), (5000, 128, 19, 10, 1),
         (20000, 32, 2, 10, 0), (30, 16, 4, 48, 0), (257, 768, 33, 10, 0)]


@pytest.mark.parametrize("n,d,b,k,metric", CASES)
def test_parity(n, d, b, k, metric):
    X, Q, fc = corpus(n, d, b)
    try:
        capi.set_option("flat_prescan", 1)
        before = fc.prescan_stats()
        check(fc, X, Q, k, metric)
        after = fc.prescan_stats()
        assert after[0] == before[0] + 1 and after[1] == before[1] + b
    finally:
        capi.set_option("flat_prescan", 0)
        fc.close()


@pytest.mark.parametrize("n,d,b,k,metric", [CASES[3], CASES[5]])
def test_every_certificate_fails(n, d, b, k, metric):
    X, Q, fc = corpus(n, d, b)
    try:
        capi.set_option("flat_prescan", 2)
        before = fc.prescan_stats()
        check(fc, X, Q, k, metric)
        after = fc.prescan_stats()
        assert after[0] == before[0] + 1 and after[2] == before[2] + b
    finally:
        capi.set_option("flat_prescan", 0)
        fc.close()


def test_ties():
    """100 bit-identical copies among 200 rows: the certificate fails or resolves; the copies come out in ascending id order."""
    X = dg.dist_u(0x71E5, 200, 16)
    copies = np.arange(0, 200, 2)
    X[copies] = X[0]
    fc = capi.FlatCorpus(16); fc.upload(X)
    try:
        capi.set_option("flat_prescan", 1)
        Q = np.stack([X[0], X[0]])
        ids, dist, cnt = fc.search(Q, 10)
        assert fc.prescan_stats()[0] == 1
        for qi in range(2):
            assert list(ids[qi]) == list(copies[:10]) and cnt[qi] == 10
        check(fc, X, Q, 10)
    finally:
        capi.set_option("flat_prescan", 0)
        fc.close()


def test_dispatch():
    X, Q, fc = corpus(3001, 40, 3)
    try:
        capi.set_option("flat_prescan", 1)
        check(fc, X, Q, 49)      # wider than 48 results: the ordered chains
        check(fc, X, Q[:1], 10)  # a single query: its own path
        assert fc.prescan_stats()[0] == 0
        Qn = Q.copy(); Qn[1, 3] = np.nan
        with pytest.raises(capi.VersError) as e:
            fc.search(Qn, 5)
        assert e.value.status == capi.ERR_NAN
        check(fc, X, Q, 5)       # the latch is cleared, the handle still works
        assert fc.prescan_stats()[0] == 2
    finally:
        capi.set_option("flat_prescan", 0)
        fc.close()
