"""vers_ivf_fetch and vers_ivf_search_by_id at the drop-in boundary, without a GPU: the five calls are declared in include/vers_hip.h, bound
in capi.SIGNATURES with the argument counts of their prototypes, exported by the built library and reachable from the Python mirror; the ABI
version stays 2 (additions only); the header states the status codes, the all-or-nothing rule and the identity behind
VERS_BYID_EXCLUDE_SELF; what a call can refuse without a device -- a NULL handle, before any argument is looked at -- is VERS_ERR_INVALID
with nothing written and nothing counted."""
import ctypes
import os
import re

import numpy as np

from vers_amd import build as vbuild
from vers_amd import capi
from vers_amd.index import IVFFlatIndex

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"vers_ivf_fetch": 8, "vers_ivf_fetch_dev": 9, "vers_fetch_phases": 2, "vers_ivf_search_by_id": 9, "vers_ivf_search_by_id_dev": 10}


def header(strip=True):
    txt = open(os.path.join(ROOT, "include", "vers_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S) if strip else txt


def test_declared_bound_and_exported():
    txt = header()
    lib = ctypes.CDLL(vbuild.build())
    for name, n_args in NAMES.items():
        m = re.search(r"int32_t\s+" + name + r"\s*\(([^)]*)\)\s*;", txt)
        assert m, f"{name} is not declared in include/vers_hip.h"
        assert len(m.group(1).split(",")) == n_args, name
        res, args = capi.SIGNATURES[name]
        assert res is ctypes.c_int32 and len(args) == n_args, name
        assert hasattr(lib, name), f"{name} is not exported"
    assert re.search(r"#define\s+VERS_BYID_EXCLUDE_SELF\s+1u", txt) and capi.BYID_EXCLUDE_SELF == 1
    assert lib.vers_abi_version() == 2   # additions only


def test_the_header_states_the_status_codes_the_all_or_nothing_rule_and_the_identity():
    txt = " ".join(re.sub(r"\n \*", "\n", header(strip=False)).split())   # (a sentence may run over the comment's lines: their " *" goes)
    at, end = txt.index("Fetch (extension"), txt.index("int32_t vers_ivf_fetch(")
    spec = txt[at:end]
    assert "out_status[i] = 0" in spec and "out_clusters[i] = UINT64_MAX; out_status[i] = 2" in spec
    assert "ALL OR NOTHING" in spec and "no output byte is written" in spec
    assert "Columns d .. pitch - 1 of an output row are NEVER written" in spec
    assert ("SEARCH top_k + 1, DROP THE ENTRY WHOSE ID IS vec_ids[q] IF IT IS THERE AND THE LAST ENTRY OTHERWISE, out_count[q] = min(count, top_k)") in txt
    assert "With nprobe == 0 the flag is refused" in txt


def test_a_null_handle_is_refused_without_a_device():
    lib = capi.lib()
    capi.fetch_phases(reset=True)
    ids = np.arange(3, dtype=np.uint64)
    rows = np.full((3, 4), 7.0, dtype=np.float32)
    cl = np.full(3, 9, dtype=np.uint64)
    st = np.full(3, 5, dtype=np.uint8)
    counts = np.full(2, 11, dtype=np.uint64)
    cp = counts.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    assert lib.vers_ivf_fetch(None, capi._ptr(ids), 3, capi._ptr(rows), 16, capi._ptr(cl), capi._ptr(st), cp) == capi.ERR_INVALID
    assert lib.vers_ivf_fetch_dev(None, capi._ptr(ids), 3, capi._ptr(rows), 4, capi._ptr(cl), capi._ptr(st), cp, None) == capi.ERR_INVALID
    assert lib.vers_ivf_fetch(None, None, 0, None, 0, None, None, None) == capi.ERR_INVALID   # before anything else is looked at
    oi = np.full((3, 2), 13, dtype=np.uint64)
    od = np.full((3, 2), -2.0, dtype=np.float32)
    oc = np.full(3, 17, dtype=np.uint32)
    for flags in (0, capi.BYID_EXCLUDE_SELF, 0x80):
        assert lib.vers_ivf_search_by_id(None, capi._ptr(ids), 3, 2, 1, flags, capi._ptr(oi), capi._ptr(od), capi._ptr(oc)) == capi.ERR_INVALID
        assert lib.vers_ivf_search_by_id_dev(None, capi._ptr(ids), 3, 2, 1, flags, capi._ptr(oi), capi._ptr(od), capi._ptr(oc), None) == capi.ERR_INVALID
    assert (rows == 7.0).all() and (cl == 9).all() and (st == 5).all() and (counts == 11).all()   # nothing was written
    assert (oi == 13).all() and (od == -2.0).all() and (oc == 17).all()
    ph = capi.fetch_phases()
    assert len(ph) == 8 and all(v == 0.0 for v in ph.values())   # (the refused calls above counted nowhere)


def test_python_mirror_has_the_calls():
    for name in ("fetch", "fetch_dev", "search_by_id", "search_by_id_dev", "sync_from_device"):
        assert callable(getattr(IVFFlatIndex, name)), name
    assert callable(capi.fetch_phases)
