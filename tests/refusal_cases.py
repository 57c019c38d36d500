"""What the filtered search calls (and the unfiltered range calls that share their scaffold) refuse, as a list: every entry point of
include/vers_hip.h that takes a filter x every way of handing it arguments it must turn down before it touches the device.  The same list is
run by scripts/record_refusals.py (once, writes tests/golden/filter_refusals.json) and replayed by tests/test_filter_refusals_gpu.py, which holds
status and vers_last_error() text to the record byte for byte.

One tiny index: n = 256, d = 8, 4 lists, b = 2, bitmaps of 256 bits.  Every call starts from arguments that are valid for it; a case overrides
a few of them.  No case passes a bad device pointer that the device would read: a call that is not refused would be an ordinary small search.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from vers_amd import capi

N, D, K, B, TOP_K, N_BITS, WORDS, CAP = 256, 8, 4, 2, 3, 256, 4, 16
WALK = capi.RANGE_WALK_ORDER


class Entry:
    def __init__(self, name, params, host, probed, rng, form, kind="plain", adaptive=None):
        self.name, self.params, self.host, self.probed, self.range, self.form, self.kind, self.adaptive = name, params, host, probed, rng, form, kind, adaptive

    @property
    def filtered(self):
        return self.form is not None

    @property
    def multi_form(self):   # the bitmaps come as (filters, stride_words, n_filters, n_bits, filter_of)
        return self.form == "multi"


def entries():
    q = ["queries", "ldq", "b"]
    flt = {"one": ["bits", "n_bits"], "multi": ["filters", "stride_words", "n_filters", "n_bits", "filter_of"], "prep": ["f", "filter_of"]}
    topk_out, range_out = ["out_ids", "out_dist", "out_count"], ["out_lims", "out_ids", "out_dist", "cap", "out_total"]
    out = []
    for host in (True, False):
        sfx, tail = ("", []) if host else ("_dev", ["stream"])
        for probed in (True, False):
            ex, pm = ("", "nprobe") if probed else ("_exhaustive", "metric")
            for form in ("one", "multi"):
                m = "" if form == "one" else "_multi"
                out.append(Entry(f"vers_ivf_search{ex}_filtered{m}{sfx}", ["h"] + q + ["top_k", pm] + flt[form] + topk_out + tail, host, probed, False, form))
                out.append(Entry(f"vers_ivf_range_search{ex}_filtered{m}{sfx}", ["h"] + q + ["radius", pm, "flags"] + flt[form] + range_out + tail, host, probed, True, form))
                if probed:
                    out.append(Entry(f"vers_ivf_search_filtered{m}_adaptive{sfx}", ["h"] + q + ["top_k", "nprobe_min", "nprobe_max", "min_allowed"] + flt[form] + topk_out +
                                     ["out_nprobe"] + tail, host, True, False, form, adaptive="args"))
            out.append(Entry(f"vers_ivf_range_search{ex}{sfx}", ["h"] + q + ["radius", pm, "flags"] + range_out + tail, host, probed, True, None))
    for probed in (True, False):
        ex, pm = ("", "nprobe") if probed else ("_exhaustive", "metric")
        ad = ["adaptive"] if probed else []
        adk = "struct" if probed else None
        out.append(Entry(f"vers_ivf_search{ex}_filtered_partial_dev", ["h"] + q + ["top_k", pm] + flt["multi"] + ad + ["out_keys", "out_ids", "stream"], False, probed, False,
                         "multi", "partial", adk))
        out.append(Entry(f"vers_ivf_search{ex}_filtered_sharded_dev", ["h", "g"] + q + ["top_k", pm] + flt["multi"] + ad + topk_out + ["stream"], False, probed, False, "multi",
                         "sharded", adk))
        out.append(Entry(f"vers_ivf_search{ex}_prepared_dev", ["h"] + q + ["top_k", pm] + flt["prep"] + ad + topk_out + ["stream"], False, probed, False, "prep", "prepared", adk))
        out.append(Entry(f"vers_ivf_range_search{ex}_filtered_partial_dev", ["h"] + q + ["radius", pm, "flags"] + flt["multi"] +
                         ["out_lims", "out_keys", "out_ids", "cap", "out_total", "stream"], False, probed, True, "multi", "partial"))
        out.append(Entry(f"vers_ivf_range_search{ex}_filtered_sharded_dev", ["h", "g"] + q + ["radius", pm, "flags"] + flt["multi"] + range_out + ["stream"], False, probed, True,
                         "multi", "sharded"))
        out.append(Entry(f"vers_ivf_range_search{ex}_prepared_dev", ["h"] + q + ["radius", pm, "flags"] + flt["prep"] + range_out + ["stream"], False, probed, True, "prep",
                         "prepared"))
        out.append(Entry(f"vers_ivf_range_search{ex}_partial_dev", ["h"] + q + ["radius", pm, "flags", "out_lims", "out_keys", "out_ids", "cap", "out_total", "stream"], False,
                         probed, True, None, "partial"))
    for e in out:
        assert len(e.params) == len(capi.SIGNATURES[e.name][1]), e.name
    return out


def _either(e):   # the shard and prepared calls: a NULL filter_of means one bitmap for the batch
    return e.kind in ("partial", "sharded", "prepared") and e.filtered


# (label, handle, applies(e), overrides(e)).  handle: "whole", "shard" (rank 0 of 2 on the same device), "empty" (no centroids).
# An override value AD(...) is a vers_adaptive_t for the calls that take one.
class AD:
    def __init__(self, nprobe_min=1, min_allowed=1, allowed_len=False):
        self.nprobe_min, self.min_allowed, self.allowed_len = nprobe_min, min_allowed, allowed_len


def _adaptive(e, nprobe_min, nprobe_max):
    if e.adaptive == "args":
        return {"nprobe_min": nprobe_min, "nprobe_max": nprobe_max}
    return {"adaptive": AD(nprobe_min, allowed_len=e.kind == "partial"), "nprobe": nprobe_max}


CASES = [
    ("null_queries", "whole", lambda e: True, lambda e: {"queries": None}),
    ("unknown_metric", "whole", lambda e: not e.probed, lambda e: {"metric": 7}),
    ("unknown_flag", "whole", lambda e: e.range, lambda e: {"flags": 2}),
    ("nprobe_0", "whole", lambda e: e.probed, lambda e: {"nprobe_max" if e.adaptive == "args" else "nprobe": 0}),
    ("null_bitmap", "whole", lambda e: e.form in ("one", "multi"), lambda e: {"bits" if e.form == "one" else "filters": None}),
    ("n_filters_0", "whole", lambda e: e.multi_form, lambda e: {"n_filters": 0}),
    ("n_filters_over_max", "whole", lambda e: e.multi_form, lambda e: {"n_filters": capi.FILTER_MAX + 1}),
    ("stride_too_small", "whole", lambda e: e.multi_form, lambda e: {"stride_words": WORDS - 1}),
    ("null_filter_of", "whole", lambda e: e.multi_form or e.form == "prep", lambda e: {"filter_of": None}),   # (_multi: required; either-form: n_filters is 2)
    ("filter_of_out_of_range", "whole", lambda e: e.host and e.multi_form, lambda e: {"filter_of": np.array([0, 5], np.uint32)}),
    ("nan_radius", "whole", lambda e: e.host and e.range, lambda e: {"radius": np.array([np.nan, 1.0], np.float32)}),
    ("no_out_total", "whole", lambda e: e.range, lambda e: {"out_total": None}),
    ("nprobe_min_0", "whole", lambda e: e.adaptive is not None, lambda e: _adaptive(e, 0, 2)),
    ("nprobe_max_below_min", "whole", lambda e: e.adaptive is not None, lambda e: _adaptive(e, 3, 2)),
    ("adaptive_partial_without_counts", "whole", lambda e: e.adaptive == "struct" and e.kind == "partial", lambda e: {"adaptive": AD(1, allowed_len=False)}),
    ("adaptive_with_counts", "whole", lambda e: e.adaptive == "struct" and e.kind in ("sharded", "prepared"), lambda e: {"adaptive": AD(1, allowed_len=True)}),
    ("walk_order_on_stored_partial", "whole", lambda e: e.range and not e.probed and e.kind != "plain", lambda e: {"flags": WALK}),
    ("no_centroids", "empty", lambda e: e.probed, lambda e: {}),
    ("sharded_handle", "shard", lambda e: e.kind != "partial", lambda e: {}),   # (a partial on a shard is the call's purpose: not a refusal)
    ("flag_and_nprobe_0", "whole", lambda e: e.range and e.probed, lambda e: {"flags": 2, "nprobe": 0}),
    ("n_filters_0_and_null_bitmap", "whole", lambda e: e.multi_form, lambda e: {"n_filters": 0, "filters": None}),
    ("stride_too_small_and_nprobe_0", "whole", lambda e: e.multi_form and e.probed and e.adaptive != "args", lambda e: {"stride_words": WORDS - 1, "nprobe": 0}),
    ("unknown_flag_and_n_filters_0", "whole", lambda e: e.range and e.multi_form, lambda e: {"flags": 2, "n_filters": 0}),   # (the _multi calls report n_filters, the shard calls the flag)
    ("nan_radius_and_nprobe_0", "whole", lambda e: e.host and e.range and e.probed, lambda e: {"radius": np.array([1.0, np.nan], np.float32), "nprobe": 0}),
    ("b_0_and_nprobe_0","whole", lambda e: e.probed and e.adaptive != "args", lambda e: {"b": 0, "nprobe": 0}),   # top-k checks first, range returns VERS_OK
]


def case_ids():
    return [f"{e.name}:{label}" for e in entries() for label, _, applies, _ in CASES if applies(e)]


class Env:
    """The three handles, the prepared object and one valid value per parameter name, host and device."""

    def __init__(self):
        import torch
        from tests import datagen as dg
        from tests.golden import make_golden as mg
        from vers_amd.index import IVFFlatIndex
        X = dg.dist_c(0x2EF, N, D, 8, dg.default_sigma(D))
        init = mg.init_draws(5, 1, K, N)
        self.whole = IVFFlatIndex.build_index(K, 1, 3, X, init_indices=init)
        self.shard = IVFFlatIndex(D)
        self.shard.set_shard(0, 2)
        cent = np.zeros((K, D), np.float32); asg = np.zeros(N, np.uint64); cost = C.c_float(0); kept = C.c_int32(0)
        capi.check(capi.lib().vers_ivf_build(self.shard._h, capi._ptr(X), N, 4 * D, K, 1, 3, capi._ptr(init), capi._ptr(cent), 4 * D, capi._ptr(asg), C.byref(cost),
                                             C.byref(kept), None))
        self.empty = IVFFlatIndex(D)
        rng = np.random.default_rng(0x2EF)
        filters = capi.allowed_bitmaps([rng.random(N) < 0.5, rng.random(N) < 0.5], N_BITS)
        self.total = C.c_uint64(0)
        host = {
            "queries": dg.dist_u(0x2F0, B, D), "ldq": 4 * D, "radius": np.ones(B, np.float32), "bits": np.ascontiguousarray(filters[0]), "filters": filters,
            "filter_of": np.array([0, 1], np.uint32), "out_ids": np.zeros(CAP, np.uint64), "out_dist": np.zeros(CAP, np.float32), "out_count": np.zeros(B, np.uint32),
            "out_nprobe": np.zeros(B, np.uint32), "out_lims": np.zeros(B + 1, np.uint64),
        }
        self.host = host
        self.keep = {k: torch.from_numpy(v.view(np.int64) if v.dtype == np.uint64 else v.view(np.int32) if v.dtype == np.uint32 else v).cuda()
                     for k, v in host.items() if isinstance(v, np.ndarray)}
        self.keep["out_keys"] = torch.zeros(CAP, dtype=torch.int64, device="cuda")
        self.keep["allowed_len"] = torch.zeros(2 * K, dtype=torch.int32, device="cuda")
        self.common = {"g": None, "b": B, "top_k": TOP_K, "nprobe": 2, "metric": capi.METRIC_L2SQ, "flags": 0, "nprobe_min": 1, "nprobe_max": 2, "min_allowed": 1,
                       "n_bits": N_BITS, "stride_words": WORDS, "n_filters": 2, "adaptive": None, "cap": CAP, "stream": None}
        self.f = C.c_void_p()
        capi.check(capi.lib().vers_ivf_filter_prepare(self.whole._h, capi._ptr(filters), WORDS, 2, N_BITS, C.byref(self.f)))
        torch.cuda.synchronize()

    def close(self):
        capi.lib().vers_ivf_filter_destroy(self.whole._h, self.f)
        for ix in (self.whole, self.shard, self.empty):
            ix.close()

    def value(self, e, name, handle, over):
        v = over[name] if name in over else None
        if name == "h":
            return getattr(self, handle)._h
        if name == "f":
            return self.f
        if name == "out_total":
            return None if name in over else C.byref(self.total)
        if name == "adaptive" and isinstance(v, AD):
            self.ad = capi.Adaptive(v.nprobe_min, v.min_allowed, self.keep["allowed_len"].data_ptr() if v.allowed_len else None, None)
            return C.cast(C.pointer(self.ad), C.c_void_p)
        if name in over:
            if isinstance(v, np.ndarray):   # (only host calls are handed arrays of their own)
                self.arr = np.ascontiguousarray(v)
                return capi._ptr(self.arr)
            return v
        if name in self.common:
            return self.common[name]
        if name == "ldq":
            return 4 * D if e.host else D
        if e.host:
            return capi._ptr(self.host[name])
        return self.keep[name].data_ptr()

    def run(self):
        """-> {"entry:case": [status, vers_last_error() text or "", *out_total after the call (it held 77 before) or -1 for a call without one]}"""
        L = capi.lib()
        got = {}
        for e in entries():
            fn = getattr(L, e.name)
            for label, handle, applies, overrides in CASES:
                if not applies(e):
                    continue
                over = overrides(e)
                self.total.value = 77
                rc = fn(*[self.value(e, p, handle, over) for p in e.params])
                got[f"{e.name}:{label}"] = [int(rc), L.vers_last_error().decode("utf-8", "replace") if rc else "", int(self.total.value) if e.range else -1]
        return got
