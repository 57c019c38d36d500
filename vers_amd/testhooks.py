"""ctypes binding of libvers_hip_test.so (include/vers_hip_test.h, include/vers_hip_audit.h): the TEST and one-GPU-emulation hooks.  They are NOT in the
product library (libvers_hip.so exports nothing named *test*): this second library links against it and takes its handles.
Used by tests/ and by the emulation / nominal-rank scripts only."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import capi
from .capi import _ptr, _vp, check

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libvers_hip_test.so")

# name -> (restype, argtypes); one entry per declaration in include/vers_hip_test.h
SIGNATURES = {
    "vers_ivf_test_poison_slack": (C.c_int32, [_vp, C.c_float]),
    "vers_ivf_test_last_vals": (C.c_int32, [_vp, C.c_uint32, _vp, _vp, _vp, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_double)]),
    "vers_test_mfma": (C.c_int32, [C.c_int32, C.c_uint32, _vp, _vp, C.c_uint32, _vp]),
    "vers_test_standin_gather": (C.c_int32, [_vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]),
    "vers_test_wave_net": (C.c_int32, [C.c_int32, _vp, _vp]),
    "vers_test_wide_net": (C.c_int32, [C.c_int32, _vp, _vp]),
}
# the certificate audit hooks (include/vers_hip_audit.h), in the same library
AUDIT_SIGNATURES = {
    "vers_ivf_test_last_coarse": (C.c_int32, [_vp, C.c_uint32, _vp, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_double)]),
    "vers_test_assign_filter": (C.c_int32, [C.c_int32, _vp, C.c_uint32, C.c_uint32, _vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int32, C.c_uint32,
                                            _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "vers_flat_test_shadow_state": (C.c_int32, [_vp, C.POINTER(C.c_double)]),
    "vers_flat_test_last_vals": (C.c_int32, [_vp, _vp, C.c_uint32, C.c_uint32, _vp, _vp, _vp, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_double)]),
}
_lib = None


def lib():
    global _lib
    if _lib is None:
        capi.lib()  # the product library first: the hooks library resolves its internals against the copy already mapped
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: build it with `python -m vers_amd.build`")
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in list(SIGNATURES.items()) + list(AUDIT_SIGNATURES.items()):
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
        _lib = L
    return _lib


def poison_slack(index, value: float):
    """fill the storage rows of `index` (vers_amd.index.IVFFlatIndex) that hold no vector with `value` (what uninitialised memory may look like)"""
    check(lib().vers_ivf_test_poison_slack(index._h, C.c_float(value)))


def last_vals(index, q: int, cap: int = 8192):
    """(vec_ids, vals, per-candidate bounds, info dict) of query q of the last nprobe search on `index` that ran a pre-filter list scan: a
    batch on the matrix cores, or a single query on the fp16 shadow (scan1h_kernel; q = 0)"""
    ids = np.zeros(cap, dtype=np.uint64); vals = np.zeros(cap, dtype=np.float32); bnd = np.zeros(cap, dtype=np.float64)
    n = C.c_uint32(0); info = (C.c_double * 8)()
    check(lib().vers_ivf_test_last_vals(index._h, q, _ptr(ids), _ptr(vals), _ptr(bnd), cap, C.byref(n), info))
    m = min(n.value, cap)
    keys = ("qn", "xmax2", "r2", "bound_outside", "bound_common", "kp", "shadow", "metric")
    return ids[:m].copy(), vals[:m].copy(), bnd[:m].copy(), dict(zip(keys, (float(x) for x in info)))


def flat_shadow_state(fc) -> dict:
    """the fp16 shadow of `fc` (vers_amd.capi.FlatCorpus) as the device holds it: present, n_slots, xmax2, r2, failed, ld, n, rows_built"""
    st = (C.c_double * 8)()
    check(lib().vers_flat_test_shadow_state(fc._h, st))
    keys = ("present", "n_slots", "xmax2", "r2", "failed", "ld", "n", "rows_built")
    r = dict(zip(keys, (float(x) for x in st)))
    for k in ("n_slots", "failed", "ld", "n", "rows_built"):
        r[k] = int(r[k])
    r["present"] = bool(r["present"])
    return r


def flat_last_vals(fc, query, top_k: int, metric: int = 0, cap: int = 65536):
    """(vec_ids, vals, per-candidate bounds, info dict) of the last single-query search on `fc`, which ran on the shadow with this query,
    top_k and metric: every non-empty key of the scan's slots (last_vals' conventions)"""
    q = np.ascontiguousarray(query, dtype=np.float32).reshape(fc.d)
    ids = np.zeros(cap, dtype=np.uint64); vals = np.zeros(cap, dtype=np.float32); bnd = np.zeros(cap, dtype=np.float64)
    n = C.c_uint32(0); info = (C.c_double * 8)()
    check(lib().vers_flat_test_last_vals(fc._h, _ptr(q), top_k, metric, _ptr(ids), _ptr(vals), _ptr(bnd), cap, C.byref(n), info))
    assert n.value <= cap, (n.value, cap)
    m = n.value
    keys = ("qn", "xmax2", "r2", "bound_outside", "bound_common", "kp", "shadow", "metric")
    return ids[:m].copy(), vals[:m].copy(), bnd[:m].copy(), dict(zip(keys, (float(x) for x in info)))


def mfma(kind: int, A: np.ndarray, B: np.ndarray, device: int = 0) -> np.ndarray:
    """A [rows, K] x B [K, cols] on one wave of the matrix-core instruction `kind`, f32 result.
    kind 4 (bf16x3): A [2, 32, K], B [2, K, 32] bf16 bit patterns, hi plane then lo plane"""
    A = np.ascontiguousarray(A); B = np.ascontiguousarray(B)
    rows, cols = (64, 16) if kind == 3 else (32, 32)
    if kind == 4:
        assert A.shape[0] == 2 and B.shape[0] == 2
        a2, b2 = A[0], B[0]
    else:
        a2, b2 = A, B
    assert a2.shape[0] == rows and b2.shape[1] == cols and a2.shape[1] == b2.shape[0] and A.dtype == B.dtype
    assert A.dtype == (np.uint16 if kind in (0, 1, 4) else np.float32)
    out = np.zeros((rows, cols), dtype=np.float32)
    check(lib().vers_test_mfma(device, kind, _ptr(A), _ptr(B), a2.shape[1], _ptr(out)))
    return out


def last_coarse(index, q: int):
    """(G row [k], info dict) of query q of the last batched search on `index` whose coarse quantiser ran on the matrix cores"""
    k = int(index.centroids.shape[0])
    g = np.zeros(k, dtype=np.float32)
    n = C.c_uint32(0); info = (C.c_double * 8)()
    check(lib().vers_ivf_test_last_coarse(index._h, q, _ptr(g), k, C.byref(n), info))
    keys = ("qn", "cmax2", "d_pad", "metric", "x3", "slack", "E", "P")
    return g[:n.value].copy(), dict(zip(keys, (float(x) for x in info)))


ASSIGN_MODES = {0: "f32 MFMA", 1: "bf16x3", 2: "fp16 x1 (dist_gemm_x3w_kernel<2,1>)", 3: "fp16 x1 (dist_gemm_h_kernel)", 4: "as the options decide"}


def assign_filter(X: np.ndarray, Cn: np.ndarray, metric: int, mode: int, device: int = 0) -> dict:
    """one batch of the matrix-core assign pass with the filter forced to `mode` (ASSIGN_MODES): what its certificate and tile
    re-scan saw, per point and per (tile, point), and the final assignment (include/vers_hip_test.h)"""
    X = np.asarray(X, dtype=np.float32); Cn = np.asarray(Cn, dtype=np.float32)
    n, d = X.shape
    k = Cn.shape[0]
    ld = (d + 3) // 4 * 4
    Xp = np.zeros((n, ld), dtype=np.float32); Xp[:, :d] = X
    Cp = np.zeros((k, ld), dtype=np.float32); Cp[:, :d] = Cn
    n_tiles = (k + 127) // 128
    r = {"cand": np.zeros(n, np.uint32), "g2": np.zeros(n, np.float32), "E": np.zeros(n, np.float32), "queued": np.zeros(n, np.uint8),
         "thr": np.zeros(n, np.float32), "part_v1": np.zeros((n_tiles, n), np.float32), "part_c1": np.zeros((n_tiles, n), np.uint32),
         "part_v2": np.zeros((n_tiles, n), np.float32), "assign": np.zeros(n, np.uint32), "mind": np.zeros(n, np.float32)}
    info = np.zeros(10, dtype=np.uint32)
    check(lib().vers_test_assign_filter(device, _ptr(Xp), n, ld, _ptr(Cp), k, ld, d, metric, mode, _ptr(r["cand"]), _ptr(r["g2"]), _ptr(r["E"]),
                                        _ptr(r["queued"]), _ptr(r["thr"]), _ptr(r["part_v1"]), _ptr(r["part_c1"]), _ptr(r["part_v2"]),
                                        _ptr(r["assign"]), _ptr(r["mind"]), _ptr(info)))
    r["queued"] = r["queued"].astype(bool)
    r.update(zip(("n_tiles", "wide", "hi_only", "used_h", "tile_rescan", "n_queued", "n_full", "status", "batches", "mode"), (int(v) for v in info)))
    return r


def wave_net(keys: np.ndarray, device: int = 0) -> np.ndarray:
    """the kernels' lane networks on 128 keys in one wave -> 640 words (include/vers_hip_test.h)"""
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    assert keys.size == 128
    out = np.zeros(640, dtype=np.uint64)
    check(lib().vers_test_wave_net(device, _ptr(keys), _ptr(out)))
    return out


def wide_net(keys: np.ndarray, device: int = 0) -> np.ndarray:
    """the wide lists' networks (wide.hip.h) on 512 keys in one wave -> 771 words (include/vers_hip_test.h)"""
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    assert keys.size == 512
    out = np.zeros(771, dtype=np.uint64)
    check(lib().vers_test_wide_net(device, _ptr(keys), _ptr(out)))
    return out


def standin_gather(gather_struct, rank: int, world: int, workgroups: int, spin_us: int, threads: int, lds_bytes: int):
    """fills a vers_gather_t (ctypes structure) with the exchange stand-in that has RCCL's footprint"""
    check(lib().vers_test_standin_gather(C.cast(C.byref(gather_struct), _vp), rank, world, workgroups, spin_us, threads, lds_bytes))
