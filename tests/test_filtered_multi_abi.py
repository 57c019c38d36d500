"""The filtered top-k search with a filter per query at the drop-in boundary, without a GPU: the four _multi calls are declared in
include/vers_hip.h, bound in capi.SIGNATURES with the argument counts of their prototypes, exported by the built library and reachable from
the Python mirrors; capi.allowed_bitmaps stacks the filters at a common stride, checked against a plain loop."""
import ctypes
import os
import re

import numpy as np
import pytest

from vers_amd import build as vbuild
from vers_amd import capi
from vers_amd.index import IVFFlatIndex

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"vers_ivf_search_filtered_multi": 14, "vers_ivf_search_filtered_multi_dev": 15, "vers_ivf_search_exhaustive_filtered_multi": 14,
         "vers_ivf_search_exhaustive_filtered_multi_dev": 15}


def test_declared_bound_and_exported():
    txt = open(os.path.join(ROOT, "include", "vers_hip.h")).read()
    assert re.search(r"#define\s+VERS_FILTER_MAX\s+64\b", txt) and capi.FILTER_MAX == 64
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    lib = ctypes.CDLL(vbuild.build())
    for name, n_args in NAMES.items():
        m = re.search(r"int32_t\s+" + name + r"\s*\(([^)]*)\)\s*;", txt)
        assert m, f"{name} is not declared in include/vers_hip.h"
        assert len(m.group(1).split(",")) == n_args, name
        res, args = capi.SIGNATURES[name]
        assert res is ctypes.c_int32 and len(args) == n_args, name
        assert hasattr(lib, name), f"{name} is not exported"
    assert lib.vers_abi_version() == 2   # additions only


def test_python_mirrors_have_the_calls():
    for name in ("search_filtered_multi", "search_filtered_multi_dev", "search_exhaustive_filtered_multi", "search_exhaustive_filtered_multi_dev"):
        assert callable(getattr(IVFFlatIndex, name)), name
    assert callable(capi.allowed_bitmaps)


def loop_bitmaps(id_lists, n_bits, stride):
    """bit (v & 63) of word f * stride + (v >> 6), one id at a time, in Python integers"""
    words = [[0] * stride for _ in id_lists]
    for f, ids in enumerate(id_lists):
        for v in ids:
            if v < n_bits:
                words[f][v >> 6] |= 1 << (v & 63)
    return np.asarray(words, dtype=np.uint64).reshape(len(id_lists), stride)


@pytest.mark.parametrize("n_bits", [0, 1, 63, 64, 65, 130])
def test_allowed_bitmaps_against_a_plain_loop(n_bits):
    rng = np.random.default_rng(0xF300 + n_bits)
    need = max(1, (n_bits + 63) // 64)
    masks = [rng.random(length) < 0.4 for length in (n_bits, max(0, n_bits - 3), n_bits + 70)]
    ids = rng.integers(0, n_bits + 9, size=3 * n_bits + 5).astype(np.uint64)
    filters = masks + [ids, np.zeros(0, dtype=np.uint64), np.ones(n_bits, dtype=bool)]
    id_lists = [np.flatnonzero(m).tolist() for m in masks] + [ids.tolist(), [], list(range(n_bits))]
    for stride in (None, need, need + 1, need + 5):
        got = capi.allowed_bitmaps(filters, n_bits) if stride is None else capi.allowed_bitmaps(filters, n_bits, stride)
        s = need if stride is None else stride
        want = loop_bitmaps(id_lists, n_bits, s)
        assert got.dtype == np.uint64 and got.shape == (len(filters), s) and got.flags["C_CONTIGUOUS"], (n_bits, stride)
        assert np.array_equal(got, want), (n_bits, stride)
        assert not got[:, need:].any()                                   # the padding of a larger stride is zero
        for f, x in enumerate(filters):                                  # row f is the single-filter packing
            assert np.array_equal(got[f, :need], capi.allowed_bitmap(x, n_bits)), (n_bits, stride, f)
    assert sum(bin(int(w)).count("1") for w in capi.allowed_bitmaps(filters, n_bits)[-1]) == n_bits
    assert capi.allowed_bitmaps([], n_bits).shape == (0, need)
    if need > 1:
        with pytest.raises(ValueError):
            capi.allowed_bitmaps(filters, n_bits, need - 1)
