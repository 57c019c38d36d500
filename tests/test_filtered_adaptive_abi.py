"""The adaptive filtered search at the drop-in boundary, without a GPU: the four calls are declared in include/vers_hip.h, bound in
capi.SIGNATURES with the argument counts of their prototypes, exported by the built library and reachable from the Python mirrors; the ABI
version stays 2 (additions only)."""
import ctypes
import os
import re

from vers_amd import build as vbuild
from vers_amd import capi
from vers_amd.index import IVFFlatIndex

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"vers_ivf_search_filtered_adaptive": 14, "vers_ivf_search_filtered_adaptive_dev": 15,
         "vers_ivf_search_filtered_multi_adaptive": 17, "vers_ivf_search_filtered_multi_adaptive_dev": 18}


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
    assert lib.vers_abi_version() == 2   # additions only


def test_python_mirrors_have_the_calls():
    for name in ("search_filtered_adaptive", "search_filtered_adaptive_dev", "search_filtered_multi_adaptive", "search_filtered_multi_adaptive_dev"):
        assert callable(getattr(IVFFlatIndex, name)), name
