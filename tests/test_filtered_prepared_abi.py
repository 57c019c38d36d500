"""Prepared filters at the drop-in boundary, without a GPU: the nine calls and vers_filter_t are declared in include/vers_hip.h, bound in
capi.SIGNATURES with the argument counts of their prototypes, exported by the built library and reachable from the Python mirrors; the ABI
version stays 2 (additions only); what a call can refuse without a device -- a NULL handle, before any argument is looked at -- is
VERS_ERR_INVALID."""
import ctypes
import os
import re

from vers_amd import build as vbuild
from vers_amd import capi
from vers_amd.index import IVFFlatIndex, PreparedFilter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"vers_ivf_filter_prepare": 6, "vers_ivf_filter_prepare_dev": 6, "vers_ivf_filter_refresh": 3, "vers_ivf_filter_info": 3,
         "vers_ivf_filter_destroy": 2,
         "vers_ivf_search_prepared_dev": 13, "vers_ivf_search_exhaustive_prepared_dev": 12,
         "vers_ivf_range_search_prepared_dev": 15, "vers_ivf_range_search_exhaustive_prepared_dev": 15}


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vers_hip.h")).read(), flags=re.S)


def test_declared_bound_and_exported():
    txt = header()
    lib = ctypes.CDLL(vbuild.build())
    assert len(NAMES) == 9
    assert re.search(r"typedef\s+struct\s+vers_filter\s+vers_filter_t\s*;", txt), "vers_filter_t is not declared in include/vers_hip.h"
    for name, n_args in NAMES.items():
        m = re.search(r"int32_t\s+" + name + r"\s*\(([^)]*)\)\s*;", txt)
        assert m, f"{name} is not declared in include/vers_hip.h"
        assert len(m.group(1).split(",")) == n_args, name
        res, args = capi.SIGNATURES[name]
        assert res is ctypes.c_int32 and len(args) == n_args, name
        assert hasattr(lib, name), f"{name} is not exported"
    assert lib.vers_abi_version() == 2   # additions only


def test_prepared_searches_are_the_sharded_calls_less_the_exchange_and_the_bitmaps():
    """g / comm dropped, `f` in the place of filters_dev, filter_stride_words, n_filters, n_bits: four arguments fewer"""
    for name in ("vers_ivf_search", "vers_ivf_search_exhaustive", "vers_ivf_range_search", "vers_ivf_range_search_exhaustive"):
        assert len(capi.SIGNATURES[name + "_prepared_dev"][1]) == len(capi.SIGNATURES[name + "_filtered_sharded_dev"][1]) - 4, name


def test_a_null_handle_is_refused_without_a_device():
    lib = capi.lib()
    total = ctypes.c_uint64(7)
    out = ctypes.c_void_p(5)
    for name in NAMES:
        _, args = capi.SIGNATURES[name]
        call = [ctypes.byref(total) if a is ctypes.POINTER(ctypes.c_uint64) else ctypes.byref(out) if a is ctypes.POINTER(ctypes.c_void_p)
                else (None if a is ctypes.c_void_p else 1) for a in args]
        assert getattr(lib, name)(*call) == capi.ERR_INVALID, name
    assert total.value == 7 and out.value == 5   # nothing was written


def test_python_mirrors_have_the_calls():
    for name in ("prepare_filter", "prepare_filter_dev", "search_prepared_dev", "search_exhaustive_prepared_dev", "range_search_prepared_dev",
                 "range_search_exhaustive_prepared_dev"):
        assert callable(getattr(IVFFlatIndex, name)), name
    for name in ("refresh", "info", "close"):
        assert callable(getattr(PreparedFilter, name)), name
    assert len(PreparedFilter.INFO) == 8
