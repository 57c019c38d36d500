"""vers_range_merge_dev alone: `world` variable-length sorted runs of (key, id) pairs per query -> one CSR result.  The inputs are made by
hand in numpy; the expected output is np.sort of each query's concatenated keys (a sort by the low word under VERS_RANGE_WALK_ORDER), the ids
permuted alike, the distances decoded from the keys' high words.  Everything is compared bitwise, out_lims included."""
import numpy as np
import pytest

from vers_amd import capi
from vers_amd.index import IVFFlatIndex

pytestmark = pytest.mark.gpu

B = 7


def order_bits(x):
    """f32 -> the order-preserving u32 of the keys' high word (scan.hip.h: f32_to_order_bits)"""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def decode_bits(keys):
    k = (keys >> np.uint64(32)).astype(np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32)


def run_lengths(world):
    """[world][B]: q0 nothing anywhere | q1 held by one rank | q2 5000 / 3 / 0: one run longer than a block's share | q3 the equal-distance
    query | q4 .. q6 odd sizes; the LAST rank's runs are all empty (world > 1)."""
    n = np.zeros((world, B), dtype=np.int64)
    n[min(1, world - 1), 1] = 40
    n[0, 2] = 5000
    if world > 1:
        n[1, 2] = 3
    rng = np.random.default_rng(world)
    live = max(1, world - 1)
    n[:live, 3] = 9
    n[:live, 4] = rng.integers(0, 300, live)
    n[:live, 5] = rng.integers(0, 70, live)
    n[:live, 6] = rng.integers(1, 130, live)
    if world > 1:
        assert not n[world - 1].any()
    return n


def make_case(world):
    rng = np.random.default_rng(0xA11 + world)
    n = run_lengths(world)
    keys = [[None] * B for _ in range(world)]
    for q in range(B):
        tot = int(n[:, q].sum())
        # few distinct distances (negative ones, zero and ties among them), unique low words: unique keys
        if q == 3:   # ONE distance everywhere: the keys differ in the low word only, and the ranks' low words interleave
            k = (order_bits(np.full(tot, 2.5, np.float32)).astype(np.uint64) << np.uint64(32)) | np.arange(tot, dtype=np.uint64)
            live = max(1, world - 1)
            for r in range(world):
                keys[r][q] = k[r::live][:int(n[r, q])]
            continue
        dist = rng.choice(np.array([-0.5, 0.0, 0.25, 1.0, 3.5, 1e-30, 7.0e8], dtype=np.float32), tot)
        low = rng.permutation(max(tot * 3, 1))[:tot].astype(np.uint64)
        k = (order_bits(dist).astype(np.uint64) << np.uint64(32)) | low
        assert np.unique(k).size == tot
        at = 0
        for r in rng.permutation(world):
            m = int(n[r, q])
            keys[r][q] = k[at:at + m]
            at += m
    return n, keys


def id_of(keys):
    """an id per key that is no function the merge could guess: the key scrambled"""
    return (keys * np.uint64(0x9E3779B97F4A7C15)) ^ (keys >> np.uint64(7))


@pytest.mark.parametrize("walk", [False, True])
@pytest.mark.parametrize("world", [1, 3, 5])
def test_merge_equals_numpy_sort(world, walk):
    import torch
    n, keys = make_case(world)
    low = np.uint64(0xFFFFFFFF)
    runs = [[np.asarray(sorted(keys[r][q].tolist(), key=(lambda v: v & 0xFFFFFFFF) if walk else None), dtype=np.uint64) for q in range(B)]
            for r in range(world)]
    totals = n.sum(axis=1)
    t_max = int(totals.max())
    stride = 2 * t_max + 5   # larger than the longest total: the padding is 0xFF and must never surface
    buf = np.full((world, stride), 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    rank_lims = np.zeros((world, B + 1), dtype=np.uint64)
    for r in range(world):
        cat = np.concatenate(runs[r]) if totals[r] else np.zeros(0, np.uint64)
        buf[r, :cat.size] = cat
        buf[r, t_max:t_max + cat.size] = id_of(cat)
        rank_lims[r, 1:] = np.cumsum(n[r])
    # expected
    e_lims = np.zeros(B + 1, dtype=np.uint64); e_keys = []
    for q in range(B):
        cat = np.concatenate([runs[r][q] for r in range(world)])
        cat = cat[np.argsort(cat & low, kind="stable")] if walk else np.sort(cat)
        e_keys.append(cat)
        e_lims[q + 1] = e_lims[q] + np.uint64(cat.size)
    e_keys = np.concatenate(e_keys)
    total = int(e_lims[B])
    assert total == int(totals.sum()) and e_lims[1] == 0 and (world == 1 or n[0, 2] == 5000)
    dev = torch.device("cuda", 0)
    bd = torch.from_numpy(buf.view(np.int64)).to(dev)
    ld = torch.from_numpy(rank_lims.view(np.int64)).to(dev)
    pad = 16
    o_lims = torch.full((B + 1,), -3, dtype=torch.int64, device=dev)
    o_ids = torch.full((total + pad,), -5, dtype=torch.int64, device=dev)
    o_dist = torch.full((total + pad,), -7.25, dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)
    IVFFlatIndex.merge_range_partials_dev(bd.data_ptr(), bd.data_ptr() + 8 * t_max, stride, ld.data_ptr(), world, B,
                                          capi.RANGE_WALK_ORDER if walk else 0, o_lims.data_ptr(), o_ids.data_ptr(), o_dist.data_ptr())
    torch.cuda.synchronize(dev)
    g_lims = o_lims.cpu().numpy().view(np.uint64)
    g_ids = o_ids.cpu().numpy().view(np.uint64)
    g_dist = o_dist.cpu().numpy().view(np.uint32)
    assert np.array_equal(g_lims, e_lims)
    assert np.array_equal(g_ids[:total], id_of(e_keys))
    assert np.array_equal(g_dist[:total], decode_bits(e_keys))
    assert np.all(o_ids.cpu().numpy()[total:] == -5) and np.all(o_dist.cpu().numpy()[total:] == np.float32(-7.25))   # nothing past the total
    assert not np.any(g_ids[:total] == np.uint64(0xFFFFFFFFFFFFFFFF))


def test_merge_of_nothing_writes_the_limits_alone():
    """every run empty: rank_stride 0, NULL arrays -- the limits are all zero and nothing else is touched"""
    import torch
    dev = torch.device("cuda", 0)
    ld = torch.zeros((3, B + 1), dtype=torch.int64, device=dev)
    o_lims = torch.full((B + 1,), -3, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    IVFFlatIndex.merge_range_partials_dev(0, 0, 0, ld.data_ptr(), 3, B, 0, o_lims.data_ptr(), 0, 0)
    torch.cuda.synchronize(dev)
    assert np.all(o_lims.cpu().numpy() == 0)
