"""A recluster in the middle of a mutation plan.  The plans, the Model and the Run of tests/test_mutation_fuzz_gpu.py, with one more mutator:
ReclusterModel.recluster restates the call from the oracle alone -- oracle.build_index on values[live()], then centroids, assignments (0
for an id in no list) and ids rewritten.  Per case a step j drawn from the seed:
  1. the plan's steps 0 .. j run on the handle and on the Model (return values, mirror and check_state after each);
  2. recluster on both, k' drawn from {k, k + 1, max(1, k // 2)}: outputs against the Model's, mirror, check_state, n, live count, and the
     whole search battery (families A .. I);
  3. the plan's remaining steps on both.  Their rows were aimed at the OLD centroids, so what the device returns -- clusters, status, counts,
     removed -- is compared with the MODEL's answer, never with the kinds the plan intended (its predicted re-layouts and storage rows are
     taken out of the steps); mirror, check_state and the step's families after every one, all families after the last.
Every comparison is np.array_equal on ids, distance bits and counts.  A failing assertion prints (case, seed, j, k')."""
import time

import numpy as np
import pytest

from oracle import c_oracle as co
from tests import mutation_model as mm
from tests.golden import make_golden as mg
from tests.test_mutation_fuzz_gpu import Run, bits
from vers_amd.index import IVFFlatIndex

pytestmark = pytest.mark.gpu

ATTEMPTS, ITERS = 2, 3
# the four smallest shapes of the plan generator, both metrics
SMALLEST = sorted(mm.SHAPES, key=lambda s: s[0])[:4]
CASE_IDS = [f"n{n}_d{d}_k{k}_{m}" for n, d, k, *_ in SMALLEST for m in ("l2", "cos")]


class ReclusterModel(mm.Model):
    def recluster(self, kp, attempts, iters, init):
        """-> the oracle's build over the live rows in ascending vec id; the fields follow when an attempt was kept"""
        L = self.live()
        ob = co.build_index(self.values[L], kp, attempts, iters, init, metric=self.metric)
        if ob["kept"]:
            self.centroids = np.array(ob["centroids"], dtype=np.float32)
            self.assignments = [0] * len(self.assignments)
            self.ids = [[] for _ in range(kp)]
            for j, v in enumerate(L):
                c = int(ob["assignments"][j])
                self.assignments[v] = c
                self.ids[c].append(v)
        return ob


class ReclusterRun(Run):
    def __init__(self, case, tmp_path, seed=None):
        super().__init__(case, tmp_path, seed)
        X, _, ob, _ = mm.base(self.case)
        self.model = ReclusterModel(X, ob["centroids"], ob["assignments"], self.case.metric)
        rng = np.random.default_rng(self.seed ^ 0x2EC1)
        self.j = int(rng.integers(0, len(self.steps) - 1))
        k = self.case.k
        self.kp = int((k, k + 1, max(1, k // 2))[int(rng.integers(3))])

    def twin(self):
        """Run.twin with the lists of the CURRENT centroids (the plan's k no longer holds)"""
        m = self.model
        t = IVFFlatIndex(self.case.d, metric=self.case.metric)
        t.num_centroids, t.values, t.centroids, t.assignments = len(m.ids), m.values.copy(), m.centroids.copy(), np.asarray(m.assignments, dtype=np.uint64)
        t._upload()
        t.ids = [[v for v, c in enumerate(m.assignments) if c == j] for j in range(len(m.ids))]
        t.remove_batch([v for v in range(len(m.assignments)) if not m.in_list(v)])
        assert t.ids == m.ids
        nprobe, top_k = min(5, len(m.ids)), min(10, sum(m.lens()))
        a, b = self.ix.search_batch(self.Q, top_k, nprobe), t.search_batch(self.Q, top_k, nprobe)
        on = np.arange(top_k)[None, :] < a[2][:, None]
        assert np.array_equal(a[2], b[2]) and np.array_equal(a[0][on], b[0][on]) and np.array_equal(bits(a[1])[on], bits(b[1])[on]), "A on a second handle"
        t.close()

    def recluster(self):
        ix, model, kp = self.ix, self.model, self.kp
        n, live = len(model.assignments), model.live()
        init = mg.init_draws(self.seed + self.j, ATTEMPTS, kp, len(live))
        want = model.recluster(kp, ATTEMPTS, ITERS, init)
        cost, kept, _ = ix.recluster(kp, ATTEMPTS, ITERS, init_indices=init)
        assert kept == int(want["kept"]) == 1
        assert bits(cost) == bits(want["cost"]), "cost"
        assert np.array_equal(bits(ix.centroids), bits(model.centroids)), "centroids"
        assert ix.info()[0] == n and ix.live_count() == len(live) and model.live() == live
        self.mirror_and_state()

    def model_step(self, step):
        """the step without the plan's predictions: re-layouts are not asserted, compact's storage rows are the Model's"""
        op, a = step
        if op == "update":
            a = dict(a, calls=[dict(c, relayout=None) for c in a["calls"]])
        elif op == "compact":
            a = dict(a, rows_after=self.model.compact())
        live = set(self.model.live())
        return op, dict(a, aim=[v for v in a["aim"] if v in live], touched=[v for v in a["touched"] if v in live])

    def run(self):
        try:
            for self.i, self.step in enumerate(self.steps[:self.j + 1]):
                self.device_step(self.step)
                self.mirror_and_state()
            self.recluster()
            self.battery(mm.FAMILIES)
            self.twin()
            last = len(self.steps) - 1
            for self.i in range(self.j + 1, last + 1):
                self.step = self.model_step(self.steps[self.i])
                self.device_step(self.step)
                self.mirror_and_state()
                op = self.step[0]
                self.battery(mm.FAMILIES if self.i == last or op in ("compact", "reload") else self.step[1]["fams"])
        except AssertionError as e:
            raise AssertionError(f"(case, seed, j, k') = ({self.case.id!r}, {self.seed:#x}, {self.j}, {self.kp}) at step {self.i}: {e}") from e
        finally:
            self.close()


@pytest.mark.parametrize("case_id", CASE_IDS)
def test_recluster_inside_a_mutation_plan(case_id, tmp_path):
    t0 = time.time()
    r = ReclusterRun(case_id, tmp_path)
    r.run()
    print(f"recluster fuzz {case_id}: j {r.j}, k' {r.kp}, {time.time() - t0:.1f} s")
