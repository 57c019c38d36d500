"""The condition that keeps tests/test_mutation_fuzz_gpu.py from quietly testing nothing (no GPU): plan + Model of tests/mutation_model.py
for every case of the fuzz, the coverage the fuzz relies on asserted from the Model alone; Model.update / Model.remove against hand-written
micro-cases; a plan generated twice is identical.  A seed that misses a condition is changed in the case table -- the assertions stay."""
import bisect

import numpy as np
import pytest

from tests import mutation_model as mm
from tests.mutation_model import MOVED, SKIPPED, STAYED


def trace(case):
    """the plan replayed on a fresh Model, call by call -> per step a dict of what happened, from the Model alone"""
    model = mm.fresh_model(case)
    steps = mm.plan(case)
    out = []
    for op, a in steps:
        t = dict(op=op, kind=a["kind"], fams=a["fams"], stayed=0, moved=0, skipped=0, calls=[], lens0=model.lens())
        if op == "update":
            for c in a["calls"]:
                place = {v: (model.assignments[v], bisect.bisect_left(model.ids[model.assignments[v]], v)) for v in c["ids"] if model.in_list(v)}
                lens0 = model.lens()
                cl, st, counts = model.update(c["ids"], np.asarray(c["rows"], dtype=np.float32))
                t["stayed"] += counts[0]; t["moved"] += counts[1]; t["skipped"] += counts[2]
                into = {}
                for v, s, c_new in zip(c["ids"], st, cl):
                    if s == MOVED:
                        into[c_new] = into.get(c_new, 0) + 1
                mover_at = {}   # old list -> the smallest old position of a mover
                for v, s in zip(c["ids"], st):
                    if s == MOVED:
                        l, p = place[v]
                        mover_at[l] = min(mover_at.get(l, p), p)
                behind = any(s == STAYED and place[v][0] in mover_at and place[v][1] > mover_at[place[v][0]] for v, s in zip(c["ids"], st))
                t["calls"].append(dict(counts=counts, into=into, lens0=lens0, lens1=model.lens(), stay_behind_mover=behind, relayout=c["relayout"],
                                       lost=set(place[v][0] for v, s in zip(c["ids"], st) if s == MOVED)))
        elif op in ("add", "add_batch"):
            cl, _ = mm.apply(model, (op, a))
            t["clusters"] = cl
        else:
            t["ret"] = mm.apply(model, (op, a))
        t["lens1"] = model.lens()
        t["aim"] = a["aim"]
        t["live"] = set(model.live())
        out.append(t)
    return out


@pytest.mark.parametrize("case_id", list(mm.CASES))
def test_the_plan_covers_what_the_fuzz_relies_on(case_id):
    case = mm.CASES[case_id]
    tr = trace(case)
    assert len(tr) == mm.STEPS
    kinds = [t["kind"] for t in tr]
    for forced in ("update_crowd", "update_drain", "update_refill", "remove_structured", "compact", "reload", "update_stays", "add", "add_batch", "remove_scattered"):
        assert kinds.count(forced) >= 1, forced
    assert sum(t["stayed"] for t in tr) >= 30 and sum(t["moved"] for t in tr) >= 30 and sum(t["skipped"] for t in tr) >= 5
    calls = [c for t in tr for c in t["calls"]]
    if case.many:
        assert any(max(c["into"].values(), default=0) > 64 for c in calls), "no update call with more than 64 movers into one list"
    # a list that reaches length 0 and later becomes non-empty again
    emptied = {}
    refilled = False
    for i, t in enumerate(tr):
        for c in range(case.k):
            if t["lens0"][c] > 0 and t["lens1"][c] == 0:
                emptied.setdefault(c, i)
            if c in emptied and emptied[c] < i and t["lens1"][c] > 0:
                refilled = True
    assert refilled
    up = any(mm.tiles(a) > mm.tiles(b) and b > 0 for c in calls for b, a in zip(c["lens0"], c["lens1"]))
    down = any(mm.tiles(a) < mm.tiles(b) and a > 0 for c in calls for b, a in zip(c["lens0"], c["lens1"]))
    assert up, "no list crosses a multiple of 64 upwards through an update"
    assert down, "no list crosses a multiple of 64 downwards through an update"
    after_movers = [tr[i + 1] for i in range(len(tr) - 1) if tr[i]["op"] == "update" and tr[i]["moved"]]
    assert any(t["op"] == "remove" for t in after_movers)
    assert any(t["op"] == "compact" for t in after_movers)
    # an add_batch directly after an update with movers whose rows go into slack: into a list that update took rows out of
    assert any(tr[i + 1]["op"] == "add_batch" and tr[i]["op"] == "update" and tr[i]["moved"] and
               set(tr[i + 1]["clusters"]) & set().union(*[c["lost"] for c in tr[i]["calls"]]) for i in range(len(tr) - 1))
    r = kinds.index("reload")
    assert any(t["op"] == "update" for t in tr[:r])
    assert any(c["stay_behind_mover"] for c in calls), "no stay behind a mover's old position in one call"
    # both crowd predictions: exactly to capacity (no re-layout), one row more (one re-layout) -- straight after the build or a compact
    i = kinds.index("update_crowd")
    assert i == 0 or kinds[i - 1] == "compact"
    fill, one = tr[i]["calls"]
    tgt = next(iter(fill["into"]))
    assert fill["relayout"] == 0 and one["relayout"] == 1 and fill["counts"][1] == len(fill["into"]) * 0 + sum(fill["into"].values())
    assert fill["into"] == {tgt: mm.capacity(fill["lens0"][tgt]) - fill["lens0"][tgt]} and fill["lens1"][tgt] == mm.capacity(fill["lens0"][tgt])
    assert one["into"] == {tgt: 1} and fill["counts"][0] == fill["counts"][2] == 0
    assert all(l1 <= mm.capacity(l0) for j, (l0, l1) in enumerate(zip(fill["lens0"], fill["lens1"])))   # (no other list overflows)
    # a stays-only call exists (0 re-layouts, no prepared-filter build)
    assert any(t["kind"] == "update_stays" and t["stayed"] >= 10 and t["moved"] == 0 for t in tr)
    # every search family is scheduled at least three times and at least once directly after an update that moved rows
    last = len(tr) - 1
    sched = [mm.FAMILIES if (i == last or t["op"] in ("compact", "reload")) else t["fams"] for i, t in enumerate(tr)]
    for f in mm.FAMILIES:
        assert sum(f in s for s in sched) >= 3, f
        assert any(f in s for s, t in zip(sched, tr) if t["op"] == "update" and t["moved"]), f
    # the aimed queries exist after every step and name live rows
    for t in tr:
        assert 1 <= len(t["aim"]) <= 6 and set(t["aim"]) <= t["live"], t["kind"]


def test_a_plan_generated_twice_is_identical_and_replay_follows_it():
    for case_id in ("n200_d7_k40_cos", "n333_d33_k5_l2"):
        a, b = mm.plan(case_id), mm.plan(case_id)
        assert a == b
        assert mm.plan(case_id, 77) != a
        model, steps = mm.replay(case_id, upto=4, log=mm.op_log(a[:5]))
        assert steps == a[:5]
        whole, _ = mm.replay(case_id)
        assert len(whole.assignments) >= len(model.assignments)
        with pytest.raises(AssertionError):
            mm.replay(case_id, upto=4, log=mm.op_log(a[:4]) + [("compact", 1)])


# ---- Model.update / Model.remove against hand-written micro-cases -----------------------------------------------------------------------
def micro():
    """d = 1, two centroids at -1 and +1 (L2): x < 0 -> list 0, x >= 0 -> ties go to the first minimum"""
    values = np.array([[-1.0], [1.0], [-0.5], [0.5], [-2.0], [2.0], [-0.25]], dtype=np.float32)
    return mm.Model(values, np.array([[-1.0], [1.0]], dtype=np.float32), [0, 1, 0, 1, 0, 1, 0], mm.L2)


def test_model_update_head_insert():
    m = micro()
    assert m.ids == [[0, 2, 4, 6], [1, 3, 5]]
    cl, st, counts = m.update([0], [[3.0]])
    assert (cl, st, counts) == ([1], [MOVED], (0, 1, 0))
    assert m.ids == [[2, 4, 6], [0, 1, 3, 5]] and m.assignments[0] == 1 and m.values[0, 0] == 3.0


def test_model_update_tail_insert_and_a_stay():
    m = micro()
    cl, st, counts = m.update([6, 2], [[0.75], [-0.75]])
    assert (cl, st, counts) == ([1, 0], [MOVED, STAYED], (1, 1, 0))
    assert m.ids == [[0, 2, 4], [1, 3, 5, 6]] and m.values[2, 0] == -0.75 and m.assignments[2] == 0
    assert m.ever.shape[0] == 7 + 2


def test_model_update_middle_insert():
    m = micro()
    cl, st, counts = m.update([2, 5], [[1.5], [-3.0]])
    assert (cl, st, counts) == ([1, 0], [MOVED, MOVED], (0, 2, 0))
    assert m.ids == [[0, 4, 5, 6], [1, 2, 3]]


def test_model_update_skips_an_id_in_no_list():
    m = micro()
    assert m.remove([3, 3, 99]) == 1 and m.remove([3]) == 0
    before = m.values.copy()
    cl, st, counts = m.update([3, 1], [[-4.0], [0.25]])
    assert (cl, st, counts) == ([0, 1], [SKIPPED, STAYED], (1, 0, 1))
    assert m.values[3, 0] == before[3, 0] and m.assignments[3] == 1 and m.ids == [[0, 2, 4, 6], [1, 5]]


def test_model_a_list_emptied_by_update_and_by_remove_and_filled_again():
    m = micro()
    m.update([1, 3, 5], [[-1.0], [-1.0], [-1.0]])
    assert m.ids == [[0, 1, 2, 3, 4, 5, 6], []]
    assert m.add([0.5]) == (1, 7) and m.ids[1] == [7]
    assert m.remove([7, 0]) == 2 and m.ids == [[1, 2, 3, 4, 5, 6], []]
    m.update([4], [[9.0]])
    assert m.ids == [[1, 2, 3, 5, 6], [4]]
    assert m.compact() == 2 * 64
    assert len(m.assignments) == 8 and m.values.shape == (8, 1)
