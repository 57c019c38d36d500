"""Filtered search on sharded handles at the drop-in boundary, without a GPU: the nine calls and vers_adaptive_t are declared in
include/vers_hip.h, bound in capi.SIGNATURES with the argument counts of their prototypes, exported by the built library and reachable from
the Python mirrors; the ABI version stays 2 (additions only); what a call can refuse without a device -- a NULL handle, before any argument
is looked at -- is VERS_ERR_INVALID."""
import ctypes
import os
import re

from vers_amd import build as vbuild
from vers_amd import capi
from vers_amd.index import IVFFlatIndex

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"vers_ivf_filter_allowed_len_dev": 7,
         "vers_ivf_search_filtered_partial_dev": 15, "vers_ivf_search_exhaustive_filtered_partial_dev": 14,
         "vers_ivf_search_filtered_sharded_dev": 17, "vers_ivf_search_exhaustive_filtered_sharded_dev": 16,
         "vers_ivf_range_search_filtered_partial_dev": 18, "vers_ivf_range_search_exhaustive_filtered_partial_dev": 18,
         "vers_ivf_range_search_filtered_sharded_dev": 19, "vers_ivf_range_search_exhaustive_filtered_sharded_dev": 19}


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vers_hip.h")).read(), flags=re.S)


def test_declared_bound_and_exported():
    txt = header()
    lib = ctypes.CDLL(vbuild.build())
    assert len(NAMES) == 9
    for name, n_args in NAMES.items():
        m = re.search(r"int32_t\s+" + name + r"\s*\(([^)]*)\)\s*;", txt)
        assert m, f"{name} is not declared in include/vers_hip.h"
        assert len(m.group(1).split(",")) == n_args, name
        res, args = capi.SIGNATURES[name]
        assert res is ctypes.c_int32 and len(args) == n_args, name
        assert hasattr(lib, name), f"{name} is not exported"
    assert lib.vers_abi_version() == 2   # additions only


def test_adaptive_struct_matches_the_header():
    m = re.search(r"typedef\s+struct\s+vers_adaptive\s*\{([^}]*)\}\s*vers_adaptive_t\s*;", header())
    assert m, "vers_adaptive_t is not declared in include/vers_hip.h"
    fields = [f.strip() for f in m.group(1).split(";") if f.strip()]
    assert fields == ["uint32_t nprobe_min, min_allowed", "const uint32_t* allowed_len_dev", "uint32_t* out_nprobe_dev"]
    assert [n for n, _ in capi.Adaptive._fields_] == ["nprobe_min", "min_allowed", "allowed_len_dev", "out_nprobe_dev"]
    assert ctypes.sizeof(capi.Adaptive) == 8 + 2 * ctypes.sizeof(ctypes.c_void_p)
    assert capi.Adaptive.allowed_len_dev.offset == 8


def test_a_null_handle_is_refused_without_a_device():
    lib = capi.lib()
    total = ctypes.c_uint64(7)
    for name in NAMES:
        _, args = capi.SIGNATURES[name]
        call = [ctypes.byref(total) if a is ctypes.POINTER(ctypes.c_uint64) else (None if a is ctypes.c_void_p else 1) for a in args]
        assert getattr(lib, name)(*call) == capi.ERR_INVALID, name


def test_python_mirrors_have_the_calls():
    for name in ("filter_allowed_len_dev", "search_filtered_partial_dev", "search_exhaustive_filtered_partial_dev", "search_filtered_sharded_dev",
                 "search_exhaustive_filtered_sharded_dev", "range_search_filtered_partial_dev", "range_search_exhaustive_filtered_partial_dev",
                 "range_search_filtered_sharded_dev", "range_search_exhaustive_filtered_sharded_dev"):
        assert callable(getattr(IVFFlatIndex, name)), name
