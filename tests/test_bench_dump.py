"""benchlib/dump.py, the writer behind bench.py --dump-outputs: every array as float32 / float64 with integers exact, and above the
size limit the same seeded sample of queries from every array.  No GPU."""
import numpy as np

from benchlib.dump import dump_outputs


def test_dump_writes_each_array_as_float(tmp_path):
    ids = np.array([[3, 2 ** 40 + 1], [-1, 7]], dtype=np.int64)
    dst = np.array([[0.5, 1.25], [2.0, np.inf]], dtype=np.float32)
    cnt = np.array([2, 1], dtype=np.int32)
    assert dump_outputs(str(tmp_path), {"ids": ids, "distances": dst, "counts": cnt}) == ["counts", "distances", "ids"]
    got = {n: np.load(tmp_path / f"{n}.npy") for n in ("ids", "distances", "counts")}
    assert got["ids"].dtype == np.float64 and np.array_equal(got["ids"].astype(np.int64), ids)
    assert got["distances"].dtype == np.float32 and np.array_equal(got["distances"].view(np.uint32), dst.view(np.uint32))
    assert got["counts"].dtype == np.float64 and np.array_equal(got["counts"], cnt)


def test_dump_above_the_limit_is_a_fixed_sample_of_queries(tmp_path):
    ids = np.arange(4000 * 10, dtype=np.int64).reshape(4000, 10)
    dst = ids.astype(np.float32) * np.float32(0.5)
    a, b = tmp_path / "a", tmp_path / "b"
    for p in (a, b):
        assert dump_outputs(str(p), {"ids": ids, "distances": dst}, limit=64 << 10) == ["distances", "ids", "query_rows"]
    assert sum(f.stat().st_size for f in a.iterdir()) <= (64 << 10) + 3 * 128        # (+ one .npy header per file)
    rows = np.load(a / "query_rows.npy").astype(np.int64)
    assert len(rows) > 256 and np.all(np.diff(rows) > 0)
    assert np.array_equal(np.load(a / "ids.npy"), ids[rows].astype(np.float64)) and np.array_equal(np.load(a / "distances.npy"), dst[rows])
    assert all(np.array_equal(np.load(a / f.name), np.load(b / f.name)) for f in a.iterdir())   # the same sample every run
