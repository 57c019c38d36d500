"""The filtered top-k search at the drop-in boundary, without a GPU: the four search calls and the stats hook are declared in
include/vers_hip.h, bound in capi.SIGNATURES with the argument counts of their prototypes, exported by the built library and reachable from
the Python mirrors; capi.allowed_bitmap packs a filter into the u64 words the C ABI takes, checked against a plain loop."""
import ctypes
import os
import re

import numpy as np
import pytest

from vers_amd import build as vbuild
from vers_amd import capi
from vers_amd.index import IVFFlatIndex

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"vers_ivf_search_filtered": 11, "vers_ivf_search_filtered_dev": 12, "vers_ivf_search_exhaustive_filtered": 11,
         "vers_ivf_search_exhaustive_filtered_dev": 12, "vers_ivf_filter_stats": 3}


def test_declared_bound_and_exported():
    txt = open(os.path.join(ROOT, "include", "vers_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    lib = ctypes.CDLL(vbuild.build())
    for name, n_args in NAMES.items():
        m = re.search(r"int32_t\s+" + name + r"\s*\(([^)]*)\)\s*;", txt)
        assert m, f"{name} is not declared in include/vers_hip.h"
        assert len(m.group(1).split(",")) == n_args, name
        res, args = capi.SIGNATURES[name]
        assert res is ctypes.c_int32 and len(args) == n_args, name
        assert hasattr(lib, name), f"{name} is not exported"


def test_python_mirrors_have_the_calls():
    for name in ("search_filtered", "search_filtered_dev", "search_exhaustive_filtered", "search_exhaustive_filtered_dev", "filter_stats"):
        assert callable(getattr(IVFFlatIndex, name)), name
    assert callable(capi.allowed_bitmap)


def loop_bitmap(allowed_ids, n_bits):
    """bit (v & 63) of word (v >> 6), one id at a time, in Python integers"""
    words = [0] * max(1, (n_bits + 63) // 64)
    for v in allowed_ids:
        if v < n_bits:
            words[v >> 6] |= 1 << (v & 63)
    return np.asarray(words, dtype=np.uint64)


@pytest.mark.parametrize("n_bits", [0, 1, 63, 64, 65, 130])
def test_allowed_bitmap_against_a_plain_loop(n_bits):
    rng = np.random.default_rng(0xF117 + n_bits)
    # a bool array, of the filter's length, shorter and longer (positions at or beyond n_bits are not allowed)
    for length in sorted({n_bits, max(0, n_bits - 3), n_bits + 70}):
        mask = rng.random(length) < 0.4
        want = loop_bitmap(np.flatnonzero(mask).tolist(), n_bits)
        got = capi.allowed_bitmap(mask, n_bits)
        assert got.dtype == np.uint64 and got.shape == want.shape and np.array_equal(got, want), (n_bits, length)
    # an id array with repeats, unsorted, some ids at or beyond n_bits
    ids = rng.integers(0, n_bits + 9, size=3 * n_bits + 5).astype(np.uint64)
    ids = np.concatenate([ids, ids[:7]])
    want = loop_bitmap(ids.tolist(), n_bits)
    for arr in (ids, ids.astype(np.int64), ids.tolist()):
        got = capi.allowed_bitmap(arr, n_bits)
        assert got.dtype == np.uint64 and np.array_equal(got, want), n_bits
    # the edges by hand: the last valid bit, the first invalid one, nothing, everything
    if n_bits:
        assert np.array_equal(capi.allowed_bitmap([n_bits - 1, n_bits], n_bits), loop_bitmap([n_bits - 1], n_bits))
        full = capi.allowed_bitmap(np.ones(n_bits, dtype=bool), n_bits)
        assert sum(bin(int(w)).count("1") for w in full) == n_bits
    assert not capi.allowed_bitmap(np.zeros(0, dtype=np.uint64), n_bits).any()
