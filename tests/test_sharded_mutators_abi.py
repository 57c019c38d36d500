"""The update, the fetch and the search by id on handles sharded by cluster at the drop-in boundary, without a GPU: the calls are declared in
include/vers_hip.h, bound in capi.SIGNATURES with the argument counts of their prototypes, exported by the built library and reachable from
the Python mirror; the ABI version stays 2 (additions only); a NULL handle is VERS_ERR_INVALID before anything else is looked at, with
nothing written and nothing counted."""
import ctypes
import os
import re

import numpy as np

from vers_amd import build as vbuild
from vers_amd import capi
from vers_amd.index import IVFFlatIndex

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"vers_ivf_fetch_sharded_dev": 10, "vers_ivf_update_batch_sharded_dev": 9, "vers_ivf_search_by_id_sharded_dev": 12}


def test_declared_bound_and_exported():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vers_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(vbuild.build())
    for name, n_args in NAMES.items():
        m = re.search(r"int32_t\s+" + name + r"\s*\(([^)]*)\)\s*;", txt)
        assert m, f"{name} is not declared in include/vers_hip.h"
        assert len(m.group(1).split(",")) == n_args, name
        res, args = capi.SIGNATURES[name]
        assert res is ctypes.c_int32 and len(args) == n_args, name
        assert hasattr(lib, name), f"{name} is not exported"
    args = re.search(r"int32_t\s+vers_ivf_fetch_sharded_dev\s*\(([^)]*)\)", txt).group(1)
    assert "const vers_comm_t* comm" in args and args.strip().endswith("void* stream")
    args = re.search(r"int32_t\s+vers_ivf_update_batch_sharded_dev\s*\(([^)]*)\)", txt).group(1)
    assert "const vers_comm_t* comm" in args and "const float* rows_dev" in args and args.strip().endswith("uint64_t* out_counts")
    args = re.search(r"int32_t\s+vers_ivf_search_by_id_sharded_dev\s*\(([^)]*)\)", txt).group(1)
    assert "const vers_comm_t* comm" in args and "const vers_gather_t* g" in args
    assert lib.vers_abi_version() == 2   # additions only


def test_a_null_handle_is_refused_without_a_device():
    lib = capi.lib()
    capi.fetch_phases(reset=True)
    ids = np.arange(3, dtype=np.uint64)
    rows = np.full((3, 4), 7.0, dtype=np.float32)
    cl = np.full(3, 9, dtype=np.uint64)
    st = np.full(3, 5, dtype=np.uint8)
    counts = np.full(2, 11, dtype=np.uint64)
    cp = counts.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    assert lib.vers_ivf_fetch_sharded_dev(None, None, capi._ptr(ids), 3, capi._ptr(rows), 4, capi._ptr(cl), capi._ptr(st), cp, None) == capi.ERR_INVALID
    assert lib.vers_ivf_fetch_sharded_dev(None, None, None, 0, None, 0, None, None, None, None) == capi.ERR_INVALID
    c4 = np.full(4, 11, dtype=np.uint64)
    c4p = c4.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    assert lib.vers_ivf_update_batch_sharded_dev(None, None, capi._ptr(ids), capi._ptr(rows), 3, 4, capi._ptr(cl), capi._ptr(st), c4p) == capi.ERR_INVALID
    assert lib.vers_ivf_update_batch_sharded_dev(None, None, None, None, 0, 0, None, None, None) == capi.ERR_INVALID
    assert (c4 == 11).all()
    oi = np.full((3, 2), 13, dtype=np.uint64)
    od = np.full((3, 2), -2.0, dtype=np.float32)
    oc = np.full(3, 17, dtype=np.uint32)
    for flags in (0, capi.BYID_EXCLUDE_SELF, 0x80):
        assert lib.vers_ivf_search_by_id_sharded_dev(None, None, None, capi._ptr(ids), 3, 2, 1, flags, capi._ptr(oi), capi._ptr(od), capi._ptr(oc),
                                                     None) == capi.ERR_INVALID
    assert (rows == 7.0).all() and (cl == 9).all() and (st == 5).all() and (counts == 11).all()   # nothing was written
    assert (oi == 13).all() and (od == -2.0).all() and (oc == 17).all()
    ph = capi.fetch_phases()
    assert len(ph) == 8 and "callback_ms" in ph and all(v == 0.0 for v in ph.values())   # (the refused calls counted nowhere)


def test_python_mirror_has_the_calls():
    for name in ("fetch_sharded_dev", "update_batch_sharded_dev", "search_by_id_sharded_dev"):
        assert callable(getattr(IVFFlatIndex, name)), name
