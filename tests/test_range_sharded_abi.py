"""The sharded range search at the drop-in boundary, without a GPU: the five calls are declared in include/vers_hip.h, bound in
capi.SIGNATURES with the argument counts of their prototypes, exported by the built library and reachable from the Python mirror; and
vers_range_merge_dev refuses a world of 0 and NULL arrays with b > 0 before it touches a device."""
import ctypes
import os
import re

from vers_amd import build as vbuild
from vers_amd import capi
from vers_amd.index import IVFFlatIndex

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"vers_ivf_range_search_partial_dev": 13, "vers_ivf_range_search_exhaustive_partial_dev": 13, "vers_range_merge_dev": 11,
         "vers_ivf_range_search_sharded_dev": 14, "vers_ivf_range_search_exhaustive_sharded_dev": 14}


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


def test_python_mirror_has_the_calls():
    for name in ("range_search_partial_dev", "merge_range_partials_dev", "range_search_sharded_dev", "range_search_exhaustive_sharded_dev"):
        assert callable(getattr(IVFFlatIndex, name)), name
    assert isinstance(IVFFlatIndex.__dict__["merge_range_partials_dev"], staticmethod)   # beside merge_partials_dev: no handle


def test_merge_refuses_bad_arguments_without_a_device():
    """Nothing here is a device pointer: every call must be answered from its arguments alone."""
    L = capi.lib()
    one = ctypes.c_uint64(0)   # a non-NULL stand-in; never dereferenced
    p = ctypes.cast(ctypes.byref(one), ctypes.c_void_p)
    assert L.vers_range_merge_dev(p, p, 4, p, 0, 7, 0, p, p, p, None) == capi.ERR_INVALID          # world == 0
    assert b"world" in L.vers_last_error()
    assert L.vers_range_merge_dev(None, None, 4, None, 3, 7, 0, None, None, None, None) == capi.ERR_INVALID   # NULL arrays, b > 0
    assert L.vers_range_merge_dev(p, p, 4, None, 3, 7, 0, p, p, p, None) == capi.ERR_INVALID      # no limits
    assert L.vers_range_merge_dev(None, p, 4, p, 3, 7, 0, p, p, p, None) == capi.ERR_INVALID      # entries without keys
    assert L.vers_range_merge_dev(p, p, 4, p, 3, 7, 2, p, p, p, None) == capi.ERR_INVALID         # an unknown flag bit
    assert L.vers_range_merge_dev(None, None, 0, None, 3, 0, 0, None, None, None, None) == capi.OK  # b == 0: a no-op
