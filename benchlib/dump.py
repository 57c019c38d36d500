"""bench.py --dump-outputs DIR: what the timed path returned to its caller in the last timed step, one .npy file per array, so that
two builds of the project can be compared output for output on the same seeded inputs."""
from __future__ import annotations

import os

import numpy as np

LIMIT_BYTES = 64 << 20   # all files together


def dump_outputs(dirpath: str, arrays: dict, limit: int = LIMIT_BYTES, seed: int = 0) -> list:
    """arrays: name -> array whose first axis is the query.  Integers are written as float64 (exact below 2**53), floats as float32
    (float64 stays float64).  Above `limit` bytes in all, the same fixed seeded sample of queries is taken from every array and the
    sampled query numbers are written beside them as `query_rows`.  Returns the names written."""
    conv = {}
    for name, a in arrays.items():
        a = np.asarray(a)
        conv[name] = a.astype(np.float64) if a.dtype.kind in "iub" or a.dtype == np.float64 else a.astype(np.float32)
    rows = {a.shape[0] for a in conv.values()}
    assert len(rows) == 1, f"arrays disagree on the number of queries: {rows}"
    rows = rows.pop()
    total = sum(a.nbytes for a in conv.values())
    if total > limit:
        per_row = total / max(1, rows) + 8    # (+ the query number)
        pick = np.sort(np.random.default_rng(seed).choice(rows, size=max(1, int(limit // per_row)), replace=False))
        conv = {name: a[pick] for name, a in conv.items()}
        conv["query_rows"] = pick.astype(np.float64)
    os.makedirs(dirpath, exist_ok=True)
    for name, a in conv.items():
        np.save(os.path.join(dirpath, name + ".npy"), np.ascontiguousarray(a))
    return sorted(conv)
