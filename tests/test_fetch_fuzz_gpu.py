"""Fetch against the Model through a mutation plan.  The plans, the Model and the Run of tests/test_mutation_fuzz_gpu.py, with every mutator
going through its device-pointer call (the host mirror is not kept by them).  Per case -- the eight shapes, one metric each:
  1. after every one of the 12 steps every vec id ever issued is fetched through vers_ivf_fetch_dev and compared with the Model: rows ==
     values[v] bit for bit, clusters == assignments[v], status from list membership; zeros, UINT64_MAX and 2 for an id in no list;
  2. after the last step the mirror is thrown away and rebuilt by sync_from_device(): lists, assignments and values of the live ids and the
     centroids against the Model;
  3. save_index -> load_index of that mirror: check_state / check_search of the reloaded index, its lists against the Model's.
No tolerance anywhere.  A failing assertion names the case, the seed and the step."""
import time

import numpy as np
import pytest

from tests import mutation_model as mm
from tests.test_fetch_gpu import fetch_dev
from tests.test_mutation_fuzz_gpu import Run, bits
from tests.test_remove_gpu import check_search, check_state
from vers_amd import capi
from vers_amd.index import IVFFlatIndex

pytestmark = pytest.mark.gpu

CASE_IDS = [f"n{n}_d{d}_k{k}_{'l2' if i % 2 == 0 else 'cos'}" for i, (n, d, k, *_) in enumerate(mm.SHAPES)]


class FetchRun(Run):
    def __init__(self, case, tmp_path):
        super().__init__(case, tmp_path, dev=True)

    def fetch_all(self):
        m = self.model
        n = len(m.assignments)
        live = np.zeros(n, dtype=bool)
        live[m.live()] = True
        rows, cl, st, counts = fetch_dev(self.ix, np.arange(n, dtype=np.uint64))
        d = self.case.d
        want = np.where(live[:, None], m.values, np.float32(0.0)).astype(np.float32)
        assert np.array_equal(bits(rows[:, :d]), bits(want)), "rows"
        assert (rows[:, d:] == np.float32(-7.0)).all(), "padding"
        assert np.array_equal(cl, np.where(live, np.asarray(m.assignments, dtype=np.uint64), np.uint64(capi.NO_CLUSTER))), "clusters"
        assert np.array_equal(st, np.where(live, 0, 2).astype(np.uint8)), "status"
        assert counts == (int(live.sum()), int(n - live.sum())), "counts"

    def sync_and_reload(self):
        ix, m, case = self.ix, self.model, self.case
        live = np.asarray(m.live(), dtype=np.int64)
        ix.values, ix.assignments, ix.ids = np.zeros((3, case.d), dtype=np.float32), np.zeros(3, dtype=np.uint64), []   # a mirror nobody kept
        ix.centroids = np.zeros((0, case.d), dtype=np.float32)
        found, gone = ix.sync_from_device(chunk=97)
        assert (found, gone) == (live.size, len(m.assignments) - live.size)
        assert ix.ids == m.ids, "lists"
        assert np.array_equal(ix.assignments[live], np.asarray(m.assignments, dtype=np.uint64)[live]), "assignments of the live ids"
        assert np.array_equal(bits(ix.values[live]), bits(m.values[live])), "values of the live ids"
        assert np.array_equal(bits(ix.centroids), bits(m.centroids)), "centroids"
        check_state(ix)
        path = str(self.tmp_path / f"{case.id}_synced.idx")
        ix.save_index(path)
        re = IVFFlatIndex.load_index(path, case.d, metric=case.metric)
        try:
            assert re.ids == m.ids and re.info()[0] == len(m.assignments) and re.live_count() == live.size
            check_state(re)
            top_ks = tuple(t for t in (1, 10) if t <= live.size)
            check_search(re, mm.fixed_queries(case), top_ks=top_ks)
            rows, cl, st = re.fetch(live.astype(np.uint64))
            assert (st == 0).all() and np.array_equal(bits(rows), bits(m.values[live]))
        finally:
            re.close()

    def run(self):
        try:
            for self.i, self.step in enumerate(self.steps):
                self.device_step(self.step)
                self.fetch_all()
            self.sync_and_reload()
        except AssertionError as e:
            raise AssertionError(f"{self.context()} :: {e}") from e
        finally:
            self.close()


@pytest.mark.parametrize("case_id", CASE_IDS)
def test_fetch_follows_a_mutation_plan(case_id, tmp_path):
    t0 = time.time()
    FetchRun(case_id, tmp_path).run()
    print(f"fetch fuzz {case_id}: {time.time() - t0:.1f} s")
