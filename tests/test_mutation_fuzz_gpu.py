"""Mutation sequences against the oracle through every search call.  tests/mutation_model.py draws a plan of 12 steps per (case, seed) --
add, add_batch, remove_batch (scattered, structured), update_batch (mixed, stays only, a list drained and refilled, a list crowded exactly to
its capacity and one row past it), compact, save_index -> load_index -- and keeps the Model: the reference's five fields restated from the
oracle alone.  After EVERY step:
  1. the device's return values against the Model (clusters, vec ids, removed count, update clusters / status / counts, the predicted
     re-layouts, compact's storage rows);
  2. the IVFFlatIndex host mirror against the Model (ids, assignments, values bits);
  3. check_state of tests/test_remove_gpu.py (info, live count, lengths, every list's ids and row bits);
  4. the search battery: family A (top-k, batch and single) always, three of B .. I by the plan, all of them after the last step, after
     compact and after reload -- B exhaustive, C range probed, D range exhaustive, E filtered + exhaustive filtered (a random 30 % bitmap over
     the ids ever issued; a bitmap of exactly the ids the step touched), F a filter per query (the third bitmap empty), G filtered range
     (one bitmap, a bitmap per query), H adaptive depth (a 2 % bitmap), I one PreparedFilter that lives through the plan.
The first six queries of every batch are exact copies of rows the step touched: a stale |x|^2, shadow row or row-major row of such a row is
a wrong answer, not a near miss.  Expected values: one Ref (tests/test_filtered_range_gpu.py) per step and filter.  Every comparison is
np.array_equal on ids, distance BITS and counts / limits: no tolerance anywhere in this file.

A failing assertion names the case, the seed, the step and the op log; tests/mutation_model.replay(case, seed, step, log) rebuilds the Model
and the steps, run_plan(case, tmp_path, seed, upto=step) here runs them on the device again."""
import time

import numpy as np
import pytest

from oracle import c_oracle as co
from tests import mutation_model as mm
from tests import test_filtered_adaptive_gpu as faa
from tests import test_filtered_range_gpu as frg
from tests.test_filtered_range_gpu import Ref, bits
from tests.test_remove_gpu import check_state
from vers_amd import capi, testhooks
from vers_amd.index import IVFFlatIndex

pytestmark = pytest.mark.gpu

NONE = np.float32(-1e30)   # the radius of the queries of a batch that are not checked: no result
EMPTY = (np.zeros(0, np.uint64), np.zeros(0, np.float32))


def round_up(x, m):
    return (x + m - 1) // m * m


class Run:
    def __init__(self, case, tmp_path, seed=None, dev=False, poison=False, cert=False, head=False):
        self.case = mm.CASES[case] if isinstance(case, str) else case
        self.seed = self.case.seed if seed is None else seed
        self.tmp_path, self.dev, self.poison, self.cert, self.head = tmp_path, dev, poison, cert, head
        case = self.case
        X, init, ob, _ = mm.base(case)
        self.model = mm.fresh_model(case)
        self.steps = mm.plan(case, self.seed)
        self.ix = IVFFlatIndex.build_index(case.k, 1, case.iters, X, init_indices=init, metric=case.metric)
        assert np.array_equal(self.ix.assignments, ob["assignments"]) and np.array_equal(bits(self.ix.centroids), bits(ob["centroids"]))
        self.pf_bits = np.random.default_rng(self.seed ^ 0xF1).random(case.n + 2000) < 0.3   # bits set for ids not yet issued too
        self.pf = self.prepare()
        self.i = -1

    def prepare(self):
        n_bits = self.case.n + 2000
        return self.ix.prepare_filter(capi.allowed_bitmap(self.pf_bits, n_bits), n_bits)

    def close(self):
        self.pf.close()
        self.ix.close()

    # ---- one step on the device, its return values against the Model ------------------------------------------------------------------
    def nan_padded(self, rows):
        import torch
        ld = round_up(self.case.d + 3, 4)     # (the _dev calls take a pitch that is a multiple of 4 floats)
        p = np.full((len(rows), ld), np.nan, dtype=np.float32)
        p[:, :self.case.d] = rows
        return torch.from_numpy(p).cuda(), ld

    def follow(self):
        """the _dev mutators leave the mirror to the caller: assigned from the Model"""
        m = self.model
        self.ix.values, self.ix.assignments, self.ix.ids = m.values.copy(), np.asarray(m.assignments, dtype=np.uint64), [list(l) for l in m.ids]

    def add_rows(self, rows, single):
        import torch
        ix = self.ix
        if self.dev:
            rd, ld = self.nan_padded(rows)
            cd = torch.zeros(len(rows), dtype=torch.int64, device="cuda")
            first, added = ix.add_batch_dev(rd.data_ptr(), len(rows), ld, cd.data_ptr())
            return cd.cpu().numpy().tolist(), list(range(first, first + added))
        if single:
            got = [ix.add(x) for x in rows]
            return [c for c, _ in got], [v for _, v in got]
        cl, vids = ix.add_batch(rows)
        return cl.tolist(), vids.tolist()

    def update_call(self, ids, rows):
        import torch
        ix = self.ix
        if self.dev:
            rd, ld = self.nan_padded(rows)
            idd = torch.from_numpy(np.asarray(ids, dtype=np.int64)).cuda()
            cd = torch.zeros(len(ids), dtype=torch.int64, device="cuda")
            sd = torch.full((len(ids),), 9, dtype=torch.uint8, device="cuda")
            counts = ix.update_batch_dev(idd.data_ptr(), rd.data_ptr(), len(ids), ld, cd.data_ptr(), sd.data_ptr())
            return cd.cpu().numpy().tolist(), sd.cpu().numpy().tolist(), counts
        cl, st = ix.update_batch(ids, rows)
        return cl.tolist(), st.tolist(), ix.last_update_counts

    def device_step(self, step):
        import torch
        op, a = step
        ix, model = self.ix, self.model
        if op in ("add", "add_batch"):
            rows = np.asarray(a["rows"], dtype=np.float32)
            want = mm.apply(model, step)
            assert self.add_rows(rows, op == "add") == want, "clusters / vec ids of the added rows"
        elif op == "remove":
            want = mm.apply(model, step)
            if self.dev:
                idd = torch.from_numpy(np.asarray(a["ids"], dtype=np.int64)).cuda()
                got = ix.remove_batch_dev(idd.data_ptr(), len(a["ids"]))
            else:
                got = ix.remove_batch(a["ids"])
            assert got == want, ("removed count", got, want)
        elif op == "update":
            for c in a["calls"]:
                rows = np.asarray(c["rows"], dtype=np.float32)
                builds = self.prepared_builds()                      # (a prepared search first: the masks are fresh before the call)
                wcl, wst, wcounts = model.update(c["ids"], rows)
                cl, st, counts = self.update_call(c["ids"], rows)
                assert cl == wcl, "update clusters"
                assert st == wst, "update status"
                assert tuple(counts[:3]) == wcounts, ("stayed / moved / skipped", counts, wcounts)
                if c["relayout"] is not None:
                    assert counts[3] == c["relayout"], ("re-layouts", counts[3], c["relayout"])
                if self.dev:
                    self.follow()
                # the prepared filter's counters: no build after a stays-only call, one more after a call with movers
                assert self.prepared_builds() == builds + (1 if wcounts[1] else 0), ("prepared filter builds", wcounts)
        elif op == "compact":
            want = mm.apply(model, step)
            assert want == a["rows_after"]
            before, after = ix.compact()
            assert after == want, ("storage rows after compact", after, want)
        else:
            assert op == "reload"
            path = str(self.tmp_path / f"{self.case.id}_{self.i}.idx")
            ix.save_index(path)
            self.close()
            self.ix = IVFFlatIndex.load_index(path, self.case.d, metric=self.case.metric)
            self.pf = self.prepare()
        if self.dev:
            self.follow()

    def mirror_and_state(self):
        ix, model = self.ix, self.model
        assert ix.ids == model.ids, "the mirror's lists"
        assert np.array_equal(ix.assignments, np.asarray(model.assignments, dtype=np.uint64)), "the mirror's assignments"
        assert np.array_equal(bits(ix.values), bits(model.values)), "the mirror's values"
        check_state(ix)

    # ---- the search battery ----------------------------------------------------------------------------------------------------------
    def same_topk(self, got, rows, want, what):
        ids, dist, cnt = got
        for r, (ei, ed) in zip(rows, want):
            assert cnt[r] == len(ei), (what, r, int(cnt[r]), len(ei))
            assert np.array_equal(ids[r, :len(ei)], ei), (what, r, "ids")
            assert np.array_equal(bits(dist[r, :len(ei)]), bits(ed)), (what, r, "distance bits")

    def topk_family(self, call, want, what):
        """call(Q, sel) -> (ids, dist, cnt) of the queries sel of the batch; want(q) -> (ids, dist): the whole batch compared on the checked
        queries, the first and the last query alone"""
        self.same_topk(call(self.Q, np.arange(self.case.b)), self.qs, [want(q) for q in self.qs], what + ("batch",))
        for q in (0, self.case.b - 1):
            self.same_topk(call(self.Q[q:q + 1], np.asarray([q])), [0], [want(q)], what + ("single", q))

    def range_family(self, call, want, radii, what):
        """call(Q, r, walk) -> CSR; want(q, r, walk); radii: {q: r} of the checked queries -- the others ask for nothing"""
        b = self.case.b
        r = np.full(b, NONE, dtype=np.float32)
        for q in self.qs:
            r[q] = radii[q]
        for walk in (False, True):
            frg.same(call(self.Q, r, walk), [want(q, r[q], walk) if q in radii else EMPTY for q in range(b)], what + (walk, "batch"))
            for q in (0, b - 1):
                frg.same(call(self.Q[q:q + 1], r[q:q + 1], walk), [want(q, r[q], walk)], what + (walk, "single", q))

    def ref(self, name):
        if name not in self.refs:
            n_ever = len(self.model.assignments)
            rng = np.random.default_rng(self.seed + 31 * self.i)
            if name == "all":
                sem = np.ones(n_ever, dtype=bool)
            elif name == "r30":
                sem = rng.random(n_ever) < 0.30            # over the ids ever issued: removed ids stay set
            elif name == "touched":
                sem = np.zeros(n_ever, dtype=bool); sem[self.step[1]["touched"]] = True
            elif name == "empty":
                sem = np.zeros(n_ever, dtype=bool)
            elif name == "r02":
                sem = rng.random(n_ever) < 0.02
            else:
                sem = self.pf_bits[:n_ever]
            self.refs[name] = (faa.ARef if name == "r02" else Ref)(self.ix, self.Q, sem)
        return self.refs[name]

    def first(self, full, top_k):
        return full[0][:top_k], full[1][:top_k]

    def family_A(self):
        ix, k, metric = self.ix, self.case.k, self.case.metric
        live = sum(self.model.lens())
        ref = self.ref("all")
        for nprobe in sorted({0, 1, min(5, k), k}):
            for top_k in sorted({1, min(10, live), min(200, live)}):
                if nprobe == 0:
                    want = lambda q: co.search_approximate(ix.values, ix.centroids, ix.ids, self.Q[q], top_k, metric)
                else:
                    want = lambda q: self.first(ref.probed(q, nprobe), top_k)
                self.topk_family(lambda Q, sel: ix.search_batch(Q, top_k, nprobe), want, ("A", nprobe, top_k))

    def family_B(self):
        ref, top_k = self.ref("all"), min(10, sum(self.model.lens()))
        for m2 in (mm.L2, mm.COS):
            self.topk_family(lambda Q, sel: self.ix.search_exhaustive(Q, top_k, m2), lambda q: self.first(ref.exhaustive(q, m2), top_k), ("B", m2))

    def family_C(self):
        ref, k = self.ref("all"), self.case.k
        for nprobe in sorted({1, min(5, k), k}):
            radii = dict(zip(self.qs, frg.mixed_radii(ref, self.qs, nprobe)))
            self.range_family(lambda Q, r, w: self.ix.range_search(Q, r, nprobe, walk_order=w), lambda q, r, w: ref.want(q, r, nprobe, None, w), radii, ("C", nprobe))

    def family_D(self):
        ref, metric = self.ref("all"), self.case.metric
        radii = dict(zip(self.qs, frg.mixed_radii(ref, self.qs, self.case.k)))
        self.range_family(lambda Q, r, w: self.ix.range_search_exhaustive(Q, r, metric, walk_order=w), lambda q, r, w: ref.want(q, r, None, metric, w), radii, ("D",))

    def family_E(self):
        ix, nprobe, metric, n_bits = self.ix, min(5, self.case.k), self.case.metric, len(self.model.assignments)
        for name in ("r30", "touched"):
            ref = self.ref(name)
            sem = ref.sem[:n_bits]
            self.topk_family(lambda Q, sel: ix.search_filtered(Q, 10, nprobe, sem, n_bits), lambda q: self.first(ref.probed(q, nprobe), 10), ("E", name))
            self.topk_family(lambda Q, sel: ix.search_exhaustive_filtered(Q, 10, sem, metric, n_bits), lambda q: self.first(ref.exhaustive(q, metric), 10), ("E exhaustive", name))

    def three(self):
        n_bits = len(self.model.assignments)
        refs = [self.ref("r30"), self.ref("touched"), self.ref("empty")]    # (bitmap 2 is empty)
        return refs, [r.sem[:n_bits] for r in refs], n_bits

    def family_F(self):
        refs, filters, n_bits = self.three()
        nprobe = min(5, self.case.k)
        self.topk_family(lambda Q, sel: self.ix.search_filtered_multi(Q, 10, nprobe, filters, (sel % 3).astype(np.uint32), n_bits),
                         lambda q: self.first(refs[q % 3].probed(q, nprobe), 10), ("F",))

    def family_G(self):
        ix, nprobe = self.ix, min(5, self.case.k)
        refs, filters, n_bits = self.three()
        ref = refs[0]
        radii = dict(zip(self.qs, frg.mixed_radii(ref, self.qs, nprobe)))     # the radii of C, taken on the allowed rows
        self.range_family(lambda Q, r, w: ix.range_search_filtered(Q, r, nprobe, filters[0], n_bits, walk_order=w), lambda q, r, w: ref.want(q, r, nprobe, None, w),
                          radii, ("G",))
        b = self.case.b
        r = np.full(b, NONE, dtype=np.float32)
        for q in self.qs:
            r[q] = frg.mixed_radii(refs[q % 3], [q], nprobe)[0]
        fo = np.arange(b, dtype=np.uint32) % 3
        for walk in (False, True):
            got = ix.range_search_filtered_multi(self.Q, r, nprobe, filters, fo, n_bits, walk_order=walk)
            frg.same(got, [refs[q % 3].want(q, r[q], nprobe, None, walk) if q in self.qs else EMPTY for q in range(b)], ("G multi", walk))
            for q in (0, b - 1):
                got = ix.range_search_filtered_multi(self.Q[q], r[q:q + 1], nprobe, filters, fo[q:q + 1], n_bits, walk_order=walk)
                frg.same(got, [refs[q % 3].want(q, r[q], nprobe, None, walk)], ("G multi", walk, "single", q))

    def family_H(self):
        ar = self.ref("r02")
        n_bits = len(self.model.assignments)
        faa.check(ar, 10, 1, self.case.k, 10, ar.sem[:n_bits], n_bits, self.qs)      # out_nprobe against the definition looped on the host
        for q in (0, self.case.b - 1):
            faa.check(ar, 10, 1, self.case.k, 10, ar.sem[:n_bits], n_bits, [q])

    def prepared_topk(self, Q, top_k, nprobe):
        import torch
        Q = np.ascontiguousarray(np.atleast_2d(Q), dtype=np.float32)
        b = Q.shape[0]
        Qd = torch.from_numpy(Q).cuda()
        ids = torch.zeros((b, top_k), dtype=torch.int64, device="cuda"); dist = torch.zeros((b, top_k), device="cuda")
        cnt = torch.zeros(b, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        self.ix.search_prepared_dev(Qd.data_ptr(), self.case.d, b, top_k, nprobe, self.pf, 0, ids.data_ptr(), dist.data_ptr(), cnt.data_ptr())
        torch.cuda.synchronize()
        self.ix.poll(0)
        return ids.cpu().numpy().view(np.uint64), dist.cpu().numpy(), cnt.cpu().numpy().view(np.uint32)

    def prepared_builds(self):
        self.prepared_topk(self.model.values[:1], 1, 1)
        return self.pf.info()["builds"]

    def prepared_range(self, Q, r, nprobe, walk):
        import torch
        Q = np.ascontiguousarray(np.atleast_2d(Q), dtype=np.float32)
        b = Q.shape[0]
        Qd = torch.from_numpy(Q).cuda()
        rd = torch.from_numpy(np.ascontiguousarray(r, dtype=np.float32)).cuda()
        lims = torch.zeros(b + 1, dtype=torch.int64, device="cuda")
        flags = capi.RANGE_WALK_ORDER if walk else 0
        torch.cuda.synchronize()
        total = self.ix.range_search_prepared_dev(Qd.data_ptr(), self.case.d, b, rd.data_ptr(), nprobe, flags, self.pf, 0, lims.data_ptr(), 0, 0, 0)
        ids = torch.zeros(total + 1, dtype=torch.int64, device="cuda"); dist = torch.zeros(total + 1, device="cuda")
        torch.cuda.synchronize()
        assert self.ix.range_search_prepared_dev(Qd.data_ptr(), self.case.d, b, rd.data_ptr(), nprobe, flags, self.pf, 0, lims.data_ptr(), ids.data_ptr(),
                                                 dist.data_ptr(), total) == total
        return lims.cpu().numpy().view(np.uint64), ids.cpu().numpy().view(np.uint64)[:total], dist.cpu().numpy()[:total]

    def family_I(self):
        ref, nprobe = self.ref("prepared"), min(5, self.case.k)
        self.topk_family(lambda Q, sel: self.prepared_topk(Q, 10, nprobe), lambda q: self.first(ref.probed(q, nprobe), 10), ("I",))
        radii = dict(zip(self.qs, frg.mixed_radii(ref, self.qs, nprobe)))
        self.range_family(lambda Q, r, w: self.prepared_range(Q, r, nprobe, w), lambda q, r, w: ref.want(q, r, nprobe, None, w), radii, ("I range",))

    def battery(self, fams):
        case = self.case
        self.Q = mm.step_queries(case, self.model, self.step)
        self.qs = sorted(set(range(min(6, case.b))) | set(range(6, case.b, 5)) | {case.b - 1})     # the aimed queries, every fifth of the rest, the last
        self.refs = {}
        self.family_A()
        for f in fams:
            getattr(self, "family_" + f)()

    def twin(self):
        """after a reload: a second handle uploaded from the Model's fields returns the same bits for A and C"""
        m, case = self.model, self.case
        t = IVFFlatIndex(case.d, metric=case.metric)
        t.num_centroids, t.values, t.centroids, t.assignments = case.k, m.values.copy(), m.centroids.copy(), np.asarray(m.assignments, dtype=np.uint64)
        t._upload()
        gone = [v for v in range(len(m.assignments)) if not m.in_list(v)]
        t.ids = [[v for v, c in enumerate(m.assignments) if c == j] for j in range(case.k)]
        t.remove_batch(gone)
        assert t.ids == m.ids
        nprobe = min(5, case.k)
        ref = self.ref("all")
        r = np.asarray([ref.mth(q, nprobe, 10) for q in range(case.b)], dtype=np.float32)
        for a, b in ((self.ix.search_batch(self.Q, min(10, sum(m.lens())), nprobe), t.search_batch(self.Q, min(10, sum(m.lens())), nprobe)),
                     (self.ix.search_batch(self.Q, 1, 0), t.search_batch(self.Q, 1, 0))):
            assert np.array_equal(a[2], b[2])
            live = np.arange(a[0].shape[1])[None, :] < a[2][:, None]
            assert np.array_equal(a[0][live], b[0][live]) and np.array_equal(bits(a[1])[live], bits(b[1])[live]), "A on a second handle"
        for walk in (False, True):
            a, b = self.ix.range_search(self.Q, r, nprobe, walk_order=walk), t.range_search(self.Q, r, nprobe, walk_order=walk)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(bits(a[2]), bits(b[2])), "C on a second handle"
        t.close()

    # ---- the certificate and head cases --------------------------------------------------------------------------------------------
    def audit(self, label, tight):
        """the certificate case: the audit of tests/test_update_gpu.py on the step's batch (the aimed queries first), and only it -- the
        battery's top_k 200 over lists shorter than that fails certificates by design, and a shadow that fails more than 1/8 of its queries
        retires itself for the handle: nothing would be left to audit"""
        from tests.test_update_gpu import audit
        self.Q = mm.step_queries(self.case, self.model, self.step)
        assert self.ix.shadow_state()["active"], (label, self.ix.shadow_state(), self.ix.prescan_stats())
        audit(self.ix, self.Q, 30, 6, range(0, self.case.b, 5), self.model.ever, label, tight_live=tight)

    def context(self):
        return f"{self.case.id} seed {self.seed:#x} step {self.i}: replay({self.case.id!r}, {self.seed:#x}, {self.i}, log={mm.op_log(self.steps[:self.i + 1])})"

    def run(self, upto=None):
        last = len(self.steps) - 1 if upto is None else upto
        try:
            if self.head:
                self.i, self.step = -1, ("build", dict(aim=self.model.ids[0][:3], touched=self.model.ids[0][:3]))
                assert self.ix.head_state()["valid"], "the int8 head after the build"
                self.battery("")
            updated = False
            for self.i, self.step in enumerate(self.steps[:last + 1]):
                op, a = self.step
                self.device_step(self.step)
                if self.poison:
                    testhooks.poison_slack(self.ix, float("nan"))
                self.mirror_and_state()
                if self.cert:
                    self.audit(a["kind"], op == "compact")
                    continue
                self.battery(mm.FAMILIES if self.i == last or op in ("compact", "reload") else a["fams"])
                if op == "reload":
                    self.twin()
                if self.head:
                    if op == "update" and not updated:
                        updated = True
                        assert not self.ix.head_state()["valid"], "the int8 head after the first update"
                    if op == "compact":
                        assert self.ix.head_state()["valid"], "the int8 head after compact"
        except AssertionError as e:
            raise AssertionError(f"{self.context()} :: {e}") from e
        finally:
            self.close()


def run_plan(case, tmp_path, seed=None, upto=None, **kw):
    t0 = time.time()
    r = Run(case, tmp_path, seed, **kw)
    r.run(upto)
    print(f"mutation fuzz {r.case.id}: {time.time() - t0:.1f} s")


@pytest.mark.parametrize("case_id", mm.SHAPE_IDS)
def test_mutation_plan(case_id, tmp_path):
    run_plan(case_id, tmp_path)


OPTIONS = {
    "f32rows": [("shadow", 0, 1)],
    "memory1": [("memory", 1, 0)],
    "exact_paths": [("prescan", 2, 1), ("coarse", 2, 0)],
    "seg_rows64": [("seg_rows", 64, 0)],
    "chunked": [("add_batch_rows", 64, 131072), ("remove_batch_ids", 7, 1 << 20)],    # an update of more than 64 rows stages twice
    "poisoned_slack": [],
}


@pytest.mark.parametrize("name", list(OPTIONS))
def test_mutation_plan_under_options(name, tmp_path):
    for opt, value, _ in OPTIONS[name]:
        capi.set_option(opt, value)
    try:
        run_plan(mm.OPTION_CASE, tmp_path, poison=name == "poisoned_slack")
    finally:
        for opt, _, default in OPTIONS[name]:
            capi.set_option(opt, default)


def test_mutation_plan_through_device_pointers(tmp_path):
    run_plan(mm.OPTION_CASE, tmp_path, dev=True)


@pytest.mark.parametrize("case_id", ["cert_l2", "cert_cos"])
def test_mutation_plan_certificate(case_id, tmp_path):
    run_plan(case_id, tmp_path, cert=True)


def test_regression_relayout_while_another_list_shrinks(tmp_path):
    """Found by test_mutation_plan[n4097_d16_k2_cos] at step 5 (and by the int8-head case at step 4): an update drains one list into lists
    that outgrow their capacity.  The re-layout planned every list for its length AFTER the call but copied the rows it held BEFORE it, so
    the drained list's tiles were copied -- and then compacted away -- over the storage of the list behind it, whose first rows were gone."""
    run_plan("n4097_d16_k2_cos", tmp_path, seed=0x6EEF, upto=5)


def test_mutation_plan_int8_head(tmp_path):
    run_plan("head", tmp_path, head=True)
