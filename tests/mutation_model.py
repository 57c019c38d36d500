"""The model and the plan generator of the mutation fuzz (tests/test_mutation_fuzz_gpu.py, tests/test_mutation_model_host.py,
scripts/fuzz_mutations.py).  A helper module, not a test: no GPU, no vers_amd.index -- the oracle and the data generator only.

Model   the reference's five fields (values, centroids, assignments, ids, metric) restated from the oracle alone, with the mutators of the
        C ABI: add / add_batch (the oracle's add rule), remove (retain per list), update (values[v] = x; stay, or delete + bisect.insort;
        status 2 for an id in no list), compact and reload (no change of fields).  `ever` is every row value ever stored.
plan    (case, seed) -> 12 steps of plain Python literals (op, args), the rows included: deterministic, replayable from (case, seed) alone.
replay  (case, seed, upto) -> the Model after steps 0 .. upto and those steps; a failing assertion of the fuzz prints this call.

A plan is seven blocks whose order the seed draws (the crowd block first where the built lists allow it, else straight after compact):
  crowd | update, remove scattered | update, add_batch | drain, add, refill, compact | remove structured | stays | reload
so that every forced kind and every adjacency tests/test_mutation_model_host.py asserts is there by construction; ids, rows, sizes, targets
and the order inside the updates come from numpy.random.default_rng(seed)."""
import bisect
from collections import namedtuple
from functools import lru_cache

import numpy as np

from oracle import c_oracle as co
from tests import datagen as dg
from tests.golden import make_golden as mg

STAYED, MOVED, SKIPPED = 0, 1, 2
L2, COS = 0, 1
FAMILIES = "BCDEFGHI"   # (A runs after every step)
STEPS = 12

# n, d, k, b, build iterations, "an update call with more than 64 movers into one list" is asserted, what the shape reaches
SHAPES = [
    (50, 1, 3, 5, 2, False, "d = 1, ld = 64: one column of data in a 16-byte piece"),
    (200, 7, 40, 17, 3, False, "lists of ~5 rows, empty lists, every list inside one tile"),
    (333, 33, 5, 9, 2, False, "odd d; lists of ~66: one row past a tile"),
    (1000, 65, 64, 33, 2, False, "d one past a 64-column step; b past the MFMA threshold"),
    (1500, 130, 10, 40, 3, True, "lists of ~150: lengths cross 64 / 128 / 192 both ways"),
    (4097, 16, 2, 31, 2, True, "two lists of ~2,000 rows: one block per list with ~32 tiles"),
    (900, 300, 30, 40, 2, False, "ld 320: padding columns of staged and moved rows"),
    (2500, 20, 300, 33, 2, False, "k > rows per tile, most lists under 10 rows, many empty"),
]
Case = namedtuple("Case", "id n d k b metric iters many seed add_m")
CASES = {}
for _n, _d, _k, _b, _it, _many, _ in SHAPES:
    for _m in (L2, COS):
        _id = f"n{_n}_d{_d}_k{_k}_{'cos' if _m else 'l2'}"
        # seed: one per case.  add_m: the add_batch sizes the case draws from (n = 50: the index must grow before a list can be crowded)
        CASES[_id] = Case(_id, _n, _d, _k, _b, _m, _it, _many, 0x5EED + _n + _m, (200,) if _n == 50 else (1, 63, 64, 65, 200))
CASES["cert_l2"] = Case("cert_l2", 3000, 96, 12, 64, L2, 3, True, 0xCE27, (1, 63, 64, 65, 200))
CASES["cert_cos"] = Case("cert_cos", 3000, 96, 12, 64, COS, 3, True, 0xCE28, (1, 63, 64, 65, 200))
CASES["head"] = Case("head", 3000, 320, 12, 40, L2, 3, True, 0x4EAD, (1, 63, 64, 65, 200))
SHAPE_IDS = [i for i in CASES if i.startswith("n")]
OPTION_CASE = "n1500_d130_k10_l2"


def round_up(x, m):
    return (x + m - 1) // m * m


def capacity(length):
    """the storage rule of a build, an upload and compact: what a list may grow to before storage is re-laid-out"""
    return round_up(length + max(8, length // 16), 64)


def tiles(length):
    return (length + 63) // 64


class Model:
    def __init__(self, values, centroids, assignments, metric):
        self.values = np.array(values, dtype=np.float32)
        self.centroids = np.array(centroids, dtype=np.float32)
        self.assignments = [int(a) for a in assignments]
        self.metric = int(metric)
        self.ids = [[] for _ in range(self.centroids.shape[0])]
        for v, c in enumerate(self.assignments):
            self.ids[c].append(v)
        self._ever = [self.values.copy()]

    @property
    def ever(self):
        return np.concatenate(self._ever)

    def lens(self):
        return [len(l) for l in self.ids]

    def live(self):
        return sorted(v for l in self.ids for v in l)

    def in_list(self, v):
        l = self.ids[self.assignments[v]]
        j = bisect.bisect_left(l, v)
        return j < len(l) and l[j] == v

    def cluster(self, x):
        return int(co.add_cluster(self.centroids, np.ascontiguousarray(x, dtype=np.float32), self.metric))

    def add(self, x):
        x = np.asarray(x, dtype=np.float32).reshape(1, -1)
        c, v = self.cluster(x[0]), len(self.assignments)
        self.values = np.concatenate([self.values, x])
        self._ever.append(x.copy())
        self.assignments.append(c)
        self.ids[c].append(v)
        return c, v

    def add_batch(self, X):
        out = [self.add(x) for x in np.asarray(X, dtype=np.float32).reshape(-1, self.values.shape[1])]
        return [c for c, _ in out], [v for _, v in out]

    def remove(self, ids):
        gone = set(int(v) for v in ids)
        left = 0
        for c, l in enumerate(self.ids):
            kept = [v for v in l if v not in gone]
            left += len(l) - len(kept)
            self.ids[c] = kept
        return left

    def update(self, ids, X):
        """-> (clusters, status, (stayed, moved, skipped))"""
        X = np.asarray(X, dtype=np.float32).reshape(-1, self.values.shape[1])
        ids = [int(v) for v in ids]
        assert len(set(ids)) == len(ids) == X.shape[0] and all(0 <= v < len(self.assignments) for v in ids)
        self.values = self.values.copy()
        clusters, status = [], []
        for v, x in zip(ids, X):
            c = self.cluster(x)
            clusters.append(c)
            old = self.assignments[v]
            if not self.in_list(v):
                status.append(SKIPPED)
                continue
            self.values[v] = x
            self._ever.append(x[None].copy())
            if c == old:
                status.append(STAYED)
            else:
                status.append(MOVED)
                self.ids[old].remove(v)
                self.assignments[v] = c
                bisect.insort(self.ids[c], v)
        return clusters, status, tuple(status.count(s) for s in (STAYED, MOVED, SKIPPED))

    def compact(self):
        return sum(capacity(len(l)) for l in self.ids)   # the storage rows afterwards

    def reload(self):
        pass


# ---- the cases' corpora -----------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=4)
def base(case):
    """-> (X, init draws, the oracle's build, own cluster per row of X under the final centroids) as tests/test_fuzz_gpu.py builds"""
    n, d, k = case.n, case.d, case.k
    X = dg.dist_c(n + d, n, d, max(2, k // 2), dg.default_sigma(d))
    if case.metric:  # rows of different lengths: 1 - dot is then not a monotone function of the L2 distance
        X = (X * (0.5 + (np.arange(n) % 5)[:, None] * 0.375)).astype(np.float32)
    init = mg.init_draws(n ^ d, 1, k, n)
    ob = co.build_index(X, k, 1, case.iters, init, metric=case.metric)
    own = np.array([co.add_cluster(ob["centroids"], x, case.metric) for x in X], dtype=np.int64)
    return X, init, ob, own


def fresh_model(case):
    X, _, ob, _ = base(case)
    return Model(X, ob["centroids"], ob["assignments"], case.metric)


def fixed_queries(case):
    return dg.dist_c(case.n + case.d + 1, case.b, case.d, max(2, case.k // 2), dg.default_sigma(case.d))


def step_queries(case, model, step):
    """the batch after a step: exact copies of rows the step touched first, corpus-like queries (fixed per case) behind them"""
    Q = fixed_queries(case).copy()
    aim = step[1]["aim"][:min(6, case.b)]
    if aim:
        Q[:len(aim)] = model.values[aim]
    return Q


# ---- the generator ------------------------------------------------------------------------------------------------------------------------
class _Gen:
    def __init__(self, case, seed):
        self.case, self.rng, self.m = case, np.random.default_rng(seed), fresh_model(case)
        self.X, _, _, self.own = base(case)
        self.steps = []
        self.n_removes = 0
        self.lost = {}          # the last update's movers out per list
        self.drained = None
        self.prev_aim, self.prev_touched = [], []
        self.fam_u, self.fam_o = int(self.rng.integers(8)), int(self.rng.integers(8))
        self._spread = {}
        self._reach = {}

    # -- rows --
    def spread(self, c):
        if c in self._spread:
            return self._spread[c]
        self._spread[c] = s = self.spread_of(c)
        return s

    def spread_of(self, c):
        l = self.m.ids[c]
        if len(l) < 2:
            ls = [j for j in range(self.case.k) if len(self.m.ids[j]) >= 2]
            return float(np.mean([self.spread(j) for j in ls[:8]])) if ls else 0.05
        return float(np.std(self.m.values[l].astype(np.float64) - self.m.centroids[c].astype(np.float64)))

    def noise(self, c, m):
        return (self.rng.standard_normal((m, self.case.d)) * (0.01 * self.spread(c))).astype(np.float32)

    def pool(self, c):
        """rows that belong to list c: its live rows, else the corpus rows whose own cluster it is, else its centroid"""
        if self.m.ids[c]:
            return self.m.values[self.m.ids[c]]
        don = self.X[self.own == c]
        return don if don.shape[0] else self.m.centroids[c][None]

    def near(self, c, m):
        """m rows drawn around list c (a row of its pool plus noise of 1 % of its spread): most of them belong to it"""
        p = self.pool(c)
        return (p[self.rng.integers(p.shape[0], size=m)] + self.noise(c, m)).astype(np.float32)

    def rows_into(self, c, m):
        """up to m rows the oracle's add rule sends to list c: its live rows, the corpus rows whose own cluster it is, its centroid -- plus
        noise, kept when they land there"""
        out = []
        srcs = ([self.m.values[self.m.ids[c]]] if self.m.ids[c] else []) + ([self.X[self.own == c]] if (self.own == c).any() else []) + \
            [self.m.centroids[c][None], self.X, -self.X]     # (any corpus row, either sign: d = 1 has lists only a sign reaches)
        for src in srcs:
            for _ in range(4):
                if len(out) >= m:
                    break
                cand = (src[self.rng.integers(src.shape[0], size=max(m, 8))] + self.noise(c, max(m, 8))).astype(np.float32)
                out += [x for x in cand if self.m.cluster(x) == c]
        return np.asarray(out[:m], dtype=np.float32).reshape(-1, self.case.d)

    def gone(self, m):
        """up to m ids that were issued and are in no list now"""
        g = [v for v in range(len(self.m.assignments)) if not self.m.in_list(v)]
        return [g[i] for i in self.rng.permutation(len(g))[:m]]

    # -- bookkeeping --
    def neighbours(self, v):
        l = self.m.ids[self.m.assignments[v]]
        j = bisect.bisect_left(l, v)
        return [l[i] for i in (j - 1, j + 1) if 0 <= i < len(l)]

    def emit(self, op, args, kind, aim, touched, movers):
        live = set(self.m.live())
        aim = [v for v in dict.fromkeys(int(v) for v in aim) if v in live][:6]
        touched = sorted(set(int(v) for v in touched) & live)
        if not aim:
            aim, touched = self.prev_aim, self.prev_touched
            aim = [v for v in aim if v in live]
            touched = [v for v in touched if v in live]
        if movers:
            off, self.fam_u = self.fam_u, self.fam_u + 3
        else:
            off, self.fam_o = self.fam_o, self.fam_o + 3
        fams = "".join(sorted(FAMILIES[(off + j) % 8] for j in range(3)))
        args = dict(args, kind=kind, aim=aim, touched=touched, fams=fams, moved=bool(movers))
        self.steps.append((op, args))
        self.prev_aim, self.prev_touched = aim, touched
        self._spread = {}

    def do_update(self, kind, calls):
        """calls: [(ids, rows, predicted relayouts or None)]"""
        aim, touched, out, moved_any = [], [], [], False
        self.lost = {}
        for ids, rows, relayout in calls:
            ids = [int(v) for v in ids]
            before = {v: (self.m.assignments[v], self.neighbours(v)) for v in ids if self.m.in_list(v)}
            _, st, counts = self.m.update(ids, rows)
            stays = [v for v, s in zip(ids, st) if s == STAYED]
            movs = [v for v, s in zip(ids, st) if s == MOVED]
            for v in movs:
                self.lost[before[v][0]] = self.lost.get(before[v][0], 0) + 1
            old_nb = [w for v in movs[:2] for w in before[v][1]]
            new_nb = [w for v in movs[:2] for w in self.neighbours(v)]
            aim += stays[:1] + movs[:1] + old_nb[:1] + new_nb[:1] + stays[-1:] + movs[-1:]
            touched += stays + movs + old_nb + new_nb
            moved_any |= counts[1] > 0
            if counts[1] == 0:
                relayout = 0
            out.append(dict(ids=ids, rows=np.asarray(rows, dtype=np.float32).tolist(), relayout=relayout))
        self.emit("update", dict(calls=out), kind, aim, touched, moved_any)

    # -- the kinds --
    def add(self):
        m = int(self.rng.integers(1, 6))
        lists = [c for c in self.lost] or list(range(self.case.k))   # into slack the last update vacated, where there is some
        rows = np.concatenate([self.near(lists[int(self.rng.integers(len(lists)))], 1) for _ in range(m)])
        _, vids = self.m.add_batch(rows)
        self.emit("add", dict(rows=rows.tolist()), "add", vids, vids, False)

    def add_batch(self):
        m = int(self.rng.choice(self.case.add_m))
        half = m // 2
        c = max(self.lost, key=self.lost.get) if self.lost else int(np.argmax(self.m.lens()))
        grow = (self.m.centroids[c][None] + self.rng.standard_normal((m - half, self.case.d)) * self.spread(c)).astype(np.float32)
        corp = dg.dist_c(self.case.n + 7 * len(self.steps), half, self.case.d, max(2, self.case.k // 2), dg.default_sigma(self.case.d)) if half else \
            np.zeros((0, self.case.d), np.float32)
        rows = np.concatenate([corp, grow]).astype(np.float32)
        _, vids = self.m.add_batch(rows)
        self.emit("add_batch", dict(rows=rows.tolist()), "add_batch", [vids[0], vids[-1], vids[len(vids) // 2]], vids, False)

    def do_remove(self, kind, ids):
        gone = set(ids)
        nb = []
        for v in ids:
            if self.m.in_list(v):
                nb += [w for w in self.neighbours(v) if w not in gone]
        self.m.remove(ids)
        self.emit("remove", dict(ids=[int(v) for v in ids]), kind, nb[:3] + nb[-3:], nb, False)

    def remove_scattered(self):
        n_ever = len(self.m.assignments)
        m = max(2, int(n_ever * self.rng.uniform(0.05, 0.20)))
        ids = self.rng.choice(n_ever, m, replace=False).tolist()
        ids.append(ids[0])                                   # one id repeated
        if self.n_removes % 2:
            ids = sorted(ids, reverse=True)                  # descending order every other time
        self.n_removes += 1
        self.do_remove("remove_scattered", ids)

    def remove_structured(self):
        lens = self.m.lens()
        c = int(np.argmax(lens))
        l = self.m.ids[c]
        ids = list(l[64:128]) + [l[0], l[-1]]                # a tile's worth from the middle, the first and the last row
        others = [j for j in range(self.case.k) if j != c and lens[j]]
        if others:
            ids += list(self.m.ids[others[int(self.rng.integers(len(others)))]])   # and on another list, the whole list
        self.do_remove("remove_structured", ids)

    def reach(self, c):
        """rows can be made for list c (of equal centroids the first one wins every row: the others' lists are out of reach)"""
        if c not in self._reach:
            self._reach[c] = self.rows_into(c, 2).shape[0] == 2
        return self._reach[c]

    def others(self, c):
        return [j for j in range(self.case.k) if j != c and self.reach(j)]

    def update_mixed(self):
        n_ever = len(self.m.assignments)
        m = min(n_ever, int(self.rng.integers(20, 401)))
        ids = self.rng.choice(n_ever, m, replace=False).tolist()   # of the ids ever issued, removed ones included
        ids += [v for v in self.gone(8) if v not in ids]
        lens = self.m.lens()
        past = [c for c in range(self.case.k) if lens[c] > 64 and 1 <= lens[c] % 64 <= 30]
        out = []
        if past:   # a list a few rows past a tile loses them (and more): its length crosses a multiple of 64 downwards
            c = past[int(self.rng.integers(len(past)))]
            out = self.m.ids[c][:lens[c] % 64 + 3]
            ids = [v for v in ids if v not in out] + out
        m = len(ids)
        rows = np.zeros((m, self.case.d), dtype=np.float32)
        for i, v in enumerate(ids):
            a = self.m.assignments[v]
            o = self.others(a)
            if (i % 2 == 0 and v not in out) or not o:
                rows[i] = self.m.values[v] + self.noise(a, 1)[0]    # most of these stay
            else:
                rows[i] = self.near(o[int(self.rng.integers(len(o)))], 1)[0]   # most of these move -- into lists emptied earlier too
        self.do_update("update_mixed", [(ids, rows, None)])

    def update_stays(self):
        live = self.m.live()
        ids = self.rng.choice(live, min(len(live), int(self.rng.integers(20, 201))), replace=False).tolist()
        rows = np.stack([self.m.values[v] + self.noise(self.m.assignments[v], 1)[0] for v in ids]).astype(np.float32)
        keep = [i for i, v in enumerate(ids) if self.m.cluster(rows[i]) == self.m.assignments[v]]
        ids, rows = [ids[i] for i in keep], rows[keep]
        g = self.gone(6)                                                   # ids in no list: skipped
        rows = np.concatenate([rows, self.m.values[g]]) if g else rows
        self.do_update("update_stays", [(ids + g, rows, 0)])

    def update_drain(self):
        lens = self.m.lens()
        cand = sorted((j for j in range(self.case.k) if lens[j] and self.reach(j) and (lens[j] > 64 or not self.case.many)), key=lambda j: lens[j])
        if not cand:
            cand = [j for j in range(self.case.k) if lens[j] and self.reach(j)]
        c = cand[int(self.rng.integers(max(1, len(cand) // 2)))]          # one of the shorter lists (of those past a tile, where lists are long)
        ids = list(self.m.ids[c])
        self.rng.shuffle(ids)
        o = self.others(c)
        to = self.rng.integers(len(o), size=len(ids))                      # every row receives a row of another list
        rows = np.zeros((len(ids), self.case.d), dtype=np.float32)
        for t in np.unique(to):
            r = self.rows_into(o[t], int((to == t).sum()))
            assert r.shape[0] == int((to == t).sum()), "drain: too few rows found for a list"
            rows[to == t] = r
        self.drained = c
        self.do_update("update_drain", [(ids, rows, None)])

    def update_refill(self):
        c = self.drained
        m = int(self.rng.integers(65, 91)) if self.case.many else int(self.rng.integers(3, 12))
        rows = self.rows_into(c, m)
        outside = [v for v in self.m.live() if self.m.assignments[v] != c]
        ids = sorted(self.rng.choice(outside, min(len(outside), rows.shape[0]), replace=False).tolist(), reverse=True)
        self.do_update("update_refill", [(ids, rows[:len(ids)], None)])

    def crowd_target(self):
        lens = self.m.lens()
        live = sum(lens)
        for c in sorted((j for j in range(self.case.k) if lens[j] and self.reach(j)), key=lambda j: lens[j]):   # the shortest non-empty list ...
            if capacity(lens[c]) - lens[c] + 1 <= live - lens[c]:                               # ... that the other lists can fill
                return c
        return None

    def update_crowd(self):
        c = self.crowd_target()
        assert c is not None, "crowd: no list can be filled to its capacity"
        need = capacity(len(self.m.ids[c])) - len(self.m.ids[c])
        rows = self.rows_into(c, need + 1)
        assert rows.shape[0] == need + 1, "crowd: too few candidate rows pass the add rule"
        outside = [v for v in self.m.live() if self.m.assignments[v] != c]
        ids = self.rng.choice(outside, need + 1, replace=False).tolist()
        # exactly to capacity: no re-layout; then one row more: one re-layout
        self.do_update("update_crowd", [(ids[:need], rows[:need], 0), (ids[need:], rows[need:], 1)])

    def compact(self):
        self.emit("compact", dict(rows_after=self.m.compact()), "compact", [], [], False)

    def reload(self):
        self.emit("reload", dict(), "reload", [], [], False)

    def run(self):
        blocks = {"rm": [self.update_mixed, self.remove_scattered], "ab": [self.update_mixed, self.add_batch],
                  "dr": [self.update_drain, self.add, self.update_refill, self.compact], "st": [self.remove_structured],
                  "ss": [self.update_stays], "rl": [self.reload]}
        rest = ["ab", "dr", "st", "ss", "rl"]
        # "rm" first: its update follows the crowd (the crowded list shrinks past its tile again) and every later update sees removed ids
        if self.crowd_target() is not None:
            order = ["rm"] + [rest[i] for i in self.rng.permutation(len(rest))]
            seq = [self.update_crowd] + [f for b in order for f in blocks[b]]
        else:   # the index has to grow first: add_batch, then compact and the crowd straight after it
            tail = ["st", "ss", "rl"]
            seq = blocks["ab"] + blocks["dr"] + [self.update_crowd] + blocks["rm"] + [f for i in self.rng.permutation(3) for f in blocks[tail[i]]]
        assert len(seq) == STEPS
        for f in seq:
            f()
        return self.steps


def plan(case, seed=None):
    case = CASES[case] if isinstance(case, str) else case
    return _Gen(case, case.seed if seed is None else seed).run()


def apply(model, step):
    """one step on the Model -> what the device must return for it"""
    op, a = step
    if op in ("add", "add_batch"):
        return model.add_batch(np.asarray(a["rows"], dtype=np.float32))
    if op == "remove":
        return model.remove(a["ids"])
    if op == "update":
        return [model.update(c["ids"], np.asarray(c["rows"], dtype=np.float32)) for c in a["calls"]]
    if op == "compact":
        return model.compact()
    assert op == "reload", op
    return model.reload()


def op_log(steps):
    """the steps without their rows: what a failing assertion prints"""
    out = []
    for op, a in steps:
        if op == "update":
            out.append((a["kind"], [len(c["ids"]) for c in a["calls"]]))
        elif op in ("add", "add_batch"):
            out.append((a["kind"], len(a["rows"])))
        elif op == "remove":
            out.append((a["kind"], len(a["ids"])))
        else:
            out.append((a["kind"], 0))
    return out


def replay(case, seed=None, upto=STEPS - 1, log=None):
    """-> (the Model after steps 0 .. upto, those steps).  log: an op log a failure printed -- asserted to be this plan's."""
    case = CASES[case] if isinstance(case, str) else case
    steps = plan(case, seed)[:upto + 1]
    if log is not None:
        assert [tuple(x) for x in log] == [tuple(x) for x in op_log(steps)], "the op log is not this plan's"
    model = fresh_model(case)
    for s in steps:
        apply(model, s)
    return model, steps
