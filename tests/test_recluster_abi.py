"""vers_ivf_recluster at the drop-in boundary, without a GPU: the two calls are declared in include/vers_hip.h, bound in capi.SIGNATURES
with the argument counts of their prototypes, exported by the built library and reachable from the Python mirror; the ABI version stays 2
(additions only); the header states the specification in its one sentence and the all-or-nothing rule; what a call can refuse without a
device -- a NULL handle, before any argument is looked at -- is VERS_ERR_INVALID with nothing written."""
import ctypes
import os
import re

import numpy as np

from vers_amd import build as vbuild
from vers_amd import capi
from vers_amd.index import IVFFlatIndex

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"vers_ivf_recluster": 11, "vers_recluster_phases": 2}


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
    assert lib.vers_abi_version() == 2   # additions only


def test_the_header_states_the_specification_and_the_all_or_nothing_rule():
    txt = " ".join(re.sub(r"\n \*", "\n", header(strip=False)).split())   # (a sentence may run over the comment's lines: their " *" goes)
    assert ("AFTER A RECLUSTER THE HANDLE IS, BIT FOR BIT IN EVERYTHING OBSERVABLE, A HANDLE THAT RECEIVED vers_ivf_upload(values, centroids', "
            "assignments') FOLLOWED BY vers_ivf_remove_batch OF THE IDS THAT ARE IN NO LIST") in txt
    at = txt.index("AFTER A RECLUSTER THE HANDLE IS")
    assert "ALL OR NOTHING" in txt[at:txt.index("int32_t vers_ivf_recluster(")]
    assert "DIFFERS FROM vers_ivf_build ON PURPOSE" in txt


def test_a_null_handle_is_refused_without_a_device():
    lib = capi.lib()
    capi.recluster_phases(reset=True)
    init = np.zeros(4, dtype=np.uint64)
    cent = np.full((2, 4), 7.0, dtype=np.float32)
    asg = np.full(5, 9, dtype=np.uint64)
    iters = np.full(2, 3, dtype=np.uint64)
    cost, kept = ctypes.c_float(-1.0), ctypes.c_int32(-5)
    rc = lib.vers_ivf_recluster(None, 2, 2, 3, capi._ptr(init), capi._ptr(cent), 16, capi._ptr(asg), ctypes.byref(cost), ctypes.byref(kept), capi._ptr(iters))
    assert rc == capi.ERR_INVALID
    assert lib.vers_ivf_recluster(None, 0, 0, 0, None, None, 0, None, None, None, None) == capi.ERR_INVALID   # before anything else is looked at
    assert (cent == 7.0).all() and (asg == 9).all() and (iters == 3).all() and cost.value == -1.0 and kept.value == -5   # nothing was written
    ph = capi.recluster_phases()
    assert len(ph) == 8 and all(v == 0.0 for v in ph.values())   # (the refused calls above counted nowhere)


def test_python_mirror_has_the_call():
    assert callable(getattr(IVFFlatIndex, "recluster"))
    assert callable(capi.recluster_phases)
