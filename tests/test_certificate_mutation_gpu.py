"""The list scan's certificate on indexes CHANGED after the build: add_batch into slack, single adds, a re-layout, remove_batch
(scattered ids, a whole tile, the rows that carry the maxima), add_batch into freed slack, another re-layout.

tests/test_certificate_gpu.py audits the derived state one full pass leaves behind (refresh_norms(0, cap_rows)): the per-row |x|^2,
the fp16 shadow rows and the two running maxima the bound charges -- max |x|^2 and the fp16 residual R^2.  The mutation paths produce
the same state another way: per touched tile (row_norms_tiles_kernel, shadow_residual_tiles_kernel, rows_to_f16_tiles_kernel,
tiles_to_rowmajor_kernel), per row (vers_ivf_add), or not at all (remove_batch leaves the maxima where they were).  Comparing search
results with the oracle can miss a wrong derived value; here every dumped val is checked against its bound, the maxima against host
restatements of row_norm_blocked / row_shadow_residual (csrc/prescan.hip.h), and the vals against those of a fresh handle that
holds the same fields."""
import numpy as np
import pytest

from oracle import c_oracle as co
from tests.golden import make_golden as mg
from tests.test_certificate_gpu import bits, corpus, d_ref
from vers_amd import capi, testhooks
from vers_amd.index import IVFFlatIndex

gpu = pytest.mark.gpu   # (per test: the restatements below are checked on the CPU)


# ---- host restatements of the two maxima ---------------------------------------------------------------------------------------
def shadow_of(x):
    """f32(f16(x)): numpy.float16 rounds to nearest even, as the kernel's _Float16 conversion (v_cvt_f16_f32) does"""
    return np.asarray(x, dtype=np.float32).astype(np.float16).astype(np.float32)


def _seq_sum_sq(a):
    """per row: the SEQUENTIAL f32 sum of a[j] * a[j], every product and every add rounded to f32 (numpy multiplies and accumulates f32
    arrays in f32 and has no fused multiply-add; accumulate, unlike reduce, cannot re-associate) -- co.squared_euclidean(a, 0)"""
    a = np.ascontiguousarray(np.atleast_2d(a), dtype=np.float32)
    if a.shape[0] == 0:
        return np.zeros(0, dtype=np.float32)
    return np.add.accumulate((a * a).astype(np.float32), axis=1, dtype=np.float32)[:, -1]


def row_x2(rows):
    """row_norm_blocked per row (the zero padding columns up to ld add nothing: acc + 0 * 0 = acc)"""
    return _seq_sum_sq(rows)


def row_r2(rows):
    """row_shadow_residual per row: x - f32(f16(x)) is exact in f32 (prescan.hip.h), then the same chain"""
    x = np.ascontiguousarray(np.atleast_2d(rows), dtype=np.float32)
    return _seq_sum_sq(x - shadow_of(x))


def xmax2_ref(rows):
    r = row_x2(rows)
    return float(r.max()) if r.size else 0.0


def r2_ref(rows):
    r = row_r2(rows)
    return float(r.max()) if r.size else 0.0


def test_host_restatements_of_the_maxima_against_float64():
    """Hand-made rows: ordinary values, values in fp16's subnormal range (spacing 2^-24 below 2^-14), and values exactly between two
    fp16 numbers (ties go to the even significand).  A sequential f32 chain of m non-negative terms -- one rounding per product, one
    per add -- is within m u (1 + m u) of the exact sum, u = 2^-24; where every operation is exact the helpers must be too."""
    u = 2.0 ** -24
    # the conversion itself: ties to even, gradual underflow
    ties = np.array([1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 2.0 ** -11), 1.5 * 2.0 ** -24, 2.5 * 2.0 ** -24, 0.5 * 2.0 ** -24, 2.0 ** -26,
                     2048 + 1, 2048 + 3], dtype=np.float32)
    want = np.array([1.0, 1 + 2.0 ** -9, -1.0, 2 * 2.0 ** -24, 2 * 2.0 ** -24, 0.0, 0.0, 2048, 2048 + 4], dtype=np.float32)
    assert np.array_equal(shadow_of(ties), want)
    rows = [
        np.array([0.3, -1.7, 0.001, 2.5, -0.049, 7.25, 0.6, -0.11], dtype=np.float32),                      # ordinary
        np.array([3.1e-6, -5.9e-5, 2.0 ** -15 + 2.0 ** -25, 7.7e-7, -1.3e-8, 6.0e-5, 2.0 ** -24, 0.9], dtype=np.float32),   # fp16 subnormals and one ordinary
        ties[:8],                                                                                           # exact ties
        np.array([3.0, 0.0, -4.0, 0.0, 0.0, 0.0, 0.0, 0.0], dtype=np.float32),                              # exact: 25, residual 0
    ]
    R = np.stack(rows)
    m = R.shape[1]
    x64 = R.astype(np.float64)
    s64 = x64.astype(np.float16).astype(np.float64)        # (f64 -> f16 of an f32 value: the same single rounding)
    assert np.array_equal(s64, shadow_of(R).astype(np.float64))
    e_x = (x64 * x64).sum(1)
    e_r = ((x64 - s64) ** 2).sum(1)
    gx, gr = row_x2(R).astype(np.float64), row_r2(R).astype(np.float64)
    assert row_x2(R).dtype == np.float32 and row_r2(R).dtype == np.float32
    assert np.all(np.abs(gx - e_x) <= m * u * (1 + m * u) * e_x), (gx, e_x)
    assert np.all(np.abs(gr - e_r) <= m * u * (1 + m * u) * e_r), (gr, e_r)
    assert gx[3] == 25.0 and gr[3] == 0.0
    # the tie row: each of the first three residuals is exactly 2^-11 in size, whichever neighbour is taken -- the direction is pinned above
    assert row_r2(ties[:3])[0] == np.float32(3 * 2.0 ** -22)
    assert xmax2_ref(R) == float(gx.max()) and r2_ref(R) == float(gr.max()) and xmax2_ref(R[:0]) == 0.0 and r2_ref(R[:0]) == 0.0
    # ... and the oracle's own chain: bit for bit
    zero = np.zeros(m, dtype=np.float32)
    for i in range(R.shape[0]):
        assert np.array_equal(bits(row_x2(R[i])), bits(co.squared_euclidean(R[i], zero))), i
        assert np.array_equal(bits(row_r2(R[i])), bits(co.squared_euclidean(R[i] - shadow_of(R[i]), zero))), i
    # padding columns add nothing
    assert np.array_equal(bits(row_x2(np.concatenate([R, np.zeros((4, 24), np.float32)], axis=1))), bits(row_x2(R)))


# ---- the audit -----------------------------------------------------------------------------------------------------------------
def live_ids(ix):
    return np.sort(np.concatenate([np.asarray(l, dtype=np.int64) for l in ix.ids] + [np.zeros(0, np.int64)]))


def tag(ix, shadow):
    return f"metric {ix.metric} {'fp16 shadow' if shadow else 'f32 rows   '}"


def audit(ix, Q, top_k, nprobe, queries, *, shadow, pristine, label, tight_live=False):
    """One batched search (b >= 32: the matrix-core list scan), then for every query of `queries` what the scan dumped:
    (a) every val inside its bound, (b) only live rows of the probed lists, (c, d, e) the maxima the bound charges against the host
    restatements -- >= over the live rows, <= over every row ever stored; `pristine` (no removal so far): equal to the latter;
    `tight_live`: equal to the former -- and (f) the results against the oracle on the host mirror.
    info["r2"] is the handle's raw f32 maximum of the per-row residual sums (vers_ivf_test_last_vals copies pre_misc[2]; pre_bound
    inflates it on its own), so it is compared as it is."""
    metric = ix.metric
    n_ever = ix.values.shape[0]
    live = live_ids(ix)
    assert live.size > 0
    is_live = np.zeros(n_ever, dtype=bool); is_live[live] = True
    x2 = row_x2(ix.values)
    x_lo, x_hi = float(x2[live].max()), float(x2.max())
    r2 = row_r2(ix.values)
    r_lo, r_hi = float(r2[live].max()), float(r2.max())
    assert np.isfinite(x_hi) and np.isfinite(r_hi)
    asg = ix.assignments.astype(np.int64)
    st0 = ix.prescan_stats()
    ids, dist, cnt = ix.search_batch(Q, top_k, nprobe)
    st1 = ix.prescan_stats()
    assert st1["batches"] > st0["batches"], "the batch did not run the matrix-core list scan"
    out = dict(fallback=st1["fallback_queries"] - st0["fallback_queries"], dumps={}, oracle={}, worst=0.0, n_vals=0, info=None)
    for qi in queries:
        vids, vals, bnd, info = testhooks.last_vals(ix, qi, cap=32768)
        assert 0 < len(vids) < 32768, (label, qi)
        assert info["metric"] == metric and (info["shadow"] != 0) == bool(shadow), (label, qi, info)
        v = vids.astype(np.int64)
        # (b) only live rows, each once, of the nprobe lists the oracle ranks for this query (stable order of the centroid distances)
        assert np.all(v < n_ever) and np.all(is_live[np.minimum(v, n_ever - 1)]), (label, qi, "a removed or unknown vec id was dumped", v[(v >= n_ever) | ~is_live[np.minimum(v, n_ever - 1)]])
        assert np.unique(v).size == v.size, (label, qi, "a row was dumped twice")
        cd = np.array([d_ref(c, Q[qi], metric) for c in ix.centroids], dtype=np.float32)
        probed = np.argsort(cd, kind="stable")[:nprobe]
        assert np.all(np.isin(asg[v], probed)), (label, qi, "a row of a list that was not probed")
        # (a) |val + |q|^2 - D_ref| <= bound (cosine: |1 + val - D_ref|)
        for vid, val, b in zip(v, vals, bnd):
            D = d_ref(ix.values[vid], Q[qi], metric)
            err = abs((1.0 + float(val) - D) if metric else (float(val) + info["qn"] - D))
            assert np.isfinite(b) and b > 0
            assert err <= b, (label, qi, int(vid), float(val), D, err, b)
            out["worst"] = max(out["worst"], err / b)
            out["n_vals"] += 1
        # (c), (d) max |x|^2: exact comparisons, the hook hands the f32 back as a double
        assert x_lo <= info["xmax2"] <= x_hi, (label, qi, x_lo, info["xmax2"], x_hi)
        if pristine:
            assert info["xmax2"] == x_hi, (label, qi, info["xmax2"], x_hi)
        if tight_live:
            assert info["xmax2"] == x_lo, (label, qi, info["xmax2"], x_lo)
        # (e) the fp16 residual maximum, while the shadow feeds the scan
        if info["shadow"] != 0:
            assert r_lo <= info["r2"] <= r_hi, (label, qi, r_lo, info["r2"], r_hi)
            if pristine:
                assert info["r2"] == r_hi, (label, qi, info["r2"], r_hi)
            if tight_live:
                assert info["r2"] == r_lo, (label, qi, info["r2"], r_lo)
        # (f) results: the oracle on the host mirror, bit for bit
        oi, od = co.search_nprobe(ix.values, ix.centroids, ix.ids, Q[qi], top_k, nprobe, metric)
        assert cnt[qi] == len(oi) and np.array_equal(ids[qi, :len(oi)], oi) and np.array_equal(bits(dist[qi, :len(oi)]), bits(od)), (label, qi)
        out["dumps"][qi] = (v, bits(vals).copy())
        out["oracle"][qi] = oi.astype(np.int64)
        out["info"] = info
    print(f"{tag(ix, shadow)} {label:40s}: worst |val - exact| / bound = {out['worst']:.4f} over {out['n_vals']} dumped vals ({out['fallback']} of {Q.shape[0]} queries re-scanned)")
    assert out["n_vals"] > 0 and out["worst"] <= 1.0, (label, out["worst"])
    return out


def same_vals(a, b, label):
    """a, b: audits of the same batch on two handles that hold the same fields.  val = |x|^2 - 2 <x~, q'> depends on the row's shadow
    bits, its xnorm and the query block, not on where the row lies in storage (a tile's rows are separate accumulator rows of the MFMA,
    every row walks its columns in the same order, the list is split between waves by whole tiles): a (query, row) both scans dumped
    has the same val bits.  A query whose certificate held has its true top-k inside the kept candidates on either handle, so only
    queries that went to the exact re-scan may miss ids of the oracle's answer in the intersection."""
    shared, missed = 0, 0
    for qi, (va, ba) in a["dumps"].items():
        vb, bb = b["dumps"][qi]
        common, ia, ib = np.intersect1d(va, vb, return_indices=True)
        diff = ba[ia] != bb[ib]
        assert not diff.any(), (label, qi, "vals differ from a fresh handle's", common[diff][:8], ba[ia][diff][:8], bb[ib][diff][:8])
        shared += common.size
        missed += int(not np.all(np.isin(a["oracle"][qi], common)))
    assert shared > 0, label
    assert missed <= a["fallback"] + b["fallback"], (label, missed, a["fallback"], b["fallback"])
    print(f"{label:40s}: {shared} (query, row) vals equal a fresh handle's bit for bit")


def fresh_handle(ix, tmp_path, removed):
    """the host mirror's fields in a second handle: upload while nothing was removed, load_index of the saved file afterwards"""
    if not removed:
        t = IVFFlatIndex(ix.d, metric=ix.metric)
        t.num_centroids, t.values, t.centroids, t.assignments = ix.num_centroids, ix.values.copy(), ix.centroids.copy(), ix.assignments.copy()
        t.ids = [list(l) for l in ix.ids]
        t._upload()
        return t
    path = str(tmp_path / "mutated.idx")
    ix.save_index(path)
    t = IVFFlatIndex.load_index(path, ix.d, metric=ix.metric)
    assert t.ids == ix.ids
    return t


# ---- rows to add, and where they go ----------------------------------------------------------------------------------------------
def round_up(x, m):
    return (x + m - 1) // m * m


def add_pool(kind, d, seed, m=300):
    """rows of the three unit-norm corpus kinds, interleaved, at the scale of `kind`; every 7th scaled by 3: the maximum norm moves"""
    scale = np.float32(300.0 if kind == "norm_300" else 1.0)
    P = np.concatenate([corpus("dist_c", m, d, seed), corpus("dist_u", m, d, seed + 1), corpus("mixed_subnormal", m, d, seed + 2)])
    P = (P[np.random.default_rng(seed).permutation(3 * m)] * scale).astype(np.float32)
    P[::7] *= np.float32(3.0)
    return P


def pick(ix, pool, budget, want, at_least=None):
    """the first `want` rows of `pool` (no fewer than `at_least`, default `want`) such that list c gets at most budget[c] of them (the
    list add chooses: the oracle's first-minimum centroid) -> (rows, the pool without them)"""
    left = list(budget)
    take = []
    for i, x in enumerate(pool):
        c = co.add_cluster(ix.centroids, x, ix.metric)
        if left[c] > 0:
            left[c] -= 1
            take.append(i)
            if len(take) == want:
                break
    assert len(take) >= (want if at_least is None else at_least), (len(take), want, budget)
    return pool[take], np.delete(pool, take, axis=0)


def around_longest(ix, seed):
    """the construction of test_relayout_one_list_doubled_and_batch_larger_than_index: more than twice the longest list's rows around its
    centroid -- no slack holds them; some scaled by 3.  The noise is the list's own spread around its centroid, not that test's 1e-3:
    hundreds of rows within 1e-3 of one point are near-ties denser than a candidate list's slack for every query that has them among
    its neighbours (measured: 62 to 64 of 64 queries then go to the exact re-scan), and a shadow that fails more than 1/8 of 256
    queries retires itself -- stages 5 to 9 would audit the f32 rows only."""
    sizes = [len(l) for l in ix.ids]
    c = int(np.argmax(sizes))
    rng = np.random.default_rng(seed)
    sigma = float(np.std(ix.values[np.asarray(ix.ids[c], dtype=np.int64)].astype(np.float64) - ix.centroids[c].astype(np.float64)))
    rows = (ix.centroids[c][None, :] + rng.normal(0, sigma, (2 * sizes[c] + 70, ix.d))).astype(np.float32)
    rows[::9] *= np.float32(3.0)
    return rows


def mutate_and_audit(tmp_path, metric, shadow, d, kind, *, n=3000, k=12, b=64, nprobe=6, top_k=30, stages=range(1, 10), poison_after=(), expect_shadow=None,
                     seed=0xC30):
    """The stages of the module docstring on ONE index, the audit after each; fresh-handle comparison after stages 4, 7 and the last."""
    X = corpus(kind, n, d, seed + metric)
    Q = corpus(kind, b, d, seed + 0x10 + metric)
    pool = add_pool(kind, d, seed + 0x20)
    ix = IVFFlatIndex.build_index(k, 1, 3, X, init_indices=mg.init_draws(seed, 1, k, n), metric=metric)
    assert bool(ix.shadow_state()["active"]) == bool(shadow)
    queries = range(0, b, 5)
    removed = False
    last = max(stages)

    def check(label, **kw):
        r = audit(ix, Q, top_k, nprobe, queries, shadow=shadow, pristine=not removed, label=label, **kw)
        if shadow:   # the WIDE candidate lists (four keys per lane, hi-only query blocks)
            audit(ix, Q, 100, nprobe, queries, shadow=shadow, pristine=not removed, label=label + ", wide lists", **kw)
        return r

    def twin(label, r):
        t = fresh_handle(ix, tmp_path, removed)
        rt = audit(t, Q, top_k, nprobe, queries, shadow=shadow, pristine=not removed, label=label + " (fresh handle)")
        same_vals(r, rt, label)
        t.close()

    def poisoned(label):
        for v in (float("inf"), float("nan"), -1.0e30, 1.5e19):
            before = audit(ix, Q, top_k, nprobe, queries, shadow=shadow, pristine=False, label=f"{label}, before slack = {v}")
            testhooks.poison_slack(ix, v)
            after = audit(ix, Q, top_k, nprobe, queries, shadow=shadow, pristine=False, label=f"{label}, slack = {v}")
            assert after["fallback"] == before["fallback"], (label, v, before["fallback"], after["fallback"])

    # 1. build.  Capacities: plan_storage's rule -- checked against the bytes the handle reports
    r = check("1 build")
    if expect_shadow is not None:
        assert r["info"]["shadow"] == expect_shadow, r["info"]
    lens = [len(l) for l in ix.ids]
    caps = [round_up(l + max(8, l // 16), 64) for l in lens]
    rows_bytes = ix.layout_bytes()["rows"]
    assert rows_bytes % (4 * sum(caps)) == 0 and d <= rows_bytes // (4 * sum(caps)) < d + 64, (rows_bytes, caps)
    free = [c - l for c, l in zip(caps, lens)]
    if 2 in stages:   # add_batch of rows that fit the slack: at most half of each list's
        budget = [f // 2 for f in free]
        rows, pool = pick(ix, pool, budget, 150, at_least=24)
        ix.add_batch(rows)
        assert ix.layout_bytes()["rows"] == rows_bytes
        r = check("2 add_batch into slack")
    if 3 in stages:   # 70 single adds, still inside the slack
        budget = [c - len(l) for c, l in zip(caps, ix.ids)]
        rows, pool = pick(ix, pool, budget, 70)
        for x in rows:
            ix.add(x)
        assert ix.layout_bytes()["rows"] == rows_bytes
        r = check("3 single adds")
    if 4 in stages:   # an add_batch that forces a re-layout
        relayouts = capi.add_batch_phases()["relayouts"]
        ix.add_batch(around_longest(ix, 5))
        assert ix.layout_bytes()["rows"] > rows_bytes and capi.add_batch_phases()["relayouts"] >= relayouts + 1
        r = check("4 add_batch with a re-layout")
        twin("4 add_batch with a re-layout", r)
    lens5 = [len(l) for l in ix.ids]
    if 5 in stages:   # scattered ids
        assert ix.remove_batch(np.arange(3, ix.values.shape[0], 17)) > 0
        removed = True
        r = check("5 remove_batch, scattered")
    if 6 in stages:   # a whole tile's worth from the middle of the longest list, then its first and last rows
        c = int(np.argmax([len(l) for l in ix.ids]))
        assert len(ix.ids[c]) >= 192
        assert ix.remove_batch(list(ix.ids[c][64:128])) == 64
        assert ix.remove_batch([ix.ids[c][0], ix.ids[c][-1]]) == 2
        r = check("6 remove_batch, a tile, first, last")
    if 6 in poison_after:
        poisoned("6")
    if 7 in stages:   # add_batch into the freed slack: no more rows per list than it lost
        lost = [l0 - len(l) for l0, l in zip(lens5, ix.ids)]
        rows_bytes7, relayouts = ix.layout_bytes()["rows"], capi.add_batch_phases()["relayouts"]
        rows, pool = pick(ix, pool, lost, 150, at_least=24)
        ix.add_batch(rows)
        assert ix.layout_bytes()["rows"] == rows_bytes7 and capi.add_batch_phases()["relayouts"] == relayouts
        r = check("7 add_batch into freed slack")
        twin("7 add_batch into freed slack", r)
    if 8 in stages:   # the rows that carry the maxima leave: remove_batch does not lower them -- they stay upper bounds, (c) and (e)
        live = live_ids(ix)
        x2, r2 = row_x2(ix.values)[live], row_r2(ix.values)[live]
        gone = np.unique(np.concatenate([live[x2 == x2.max()], live[np.argsort(r2, kind="stable")[-3:]]]))   # (every row that attains max |x|^2)
        assert ix.remove_batch(gone) == gone.size
        r = check("8 remove_batch of the maxima's rows")
        live = live_ids(ix)
        i = r["info"]
        print(f"{tag(ix, shadow)} after 8: max |x|^2 {i['xmax2']:.9g} (live rows {xmax2_ref(ix.values[live]):.9g}): {'re-tightened' if i['xmax2'] == xmax2_ref(ix.values[live]) else 'not re-tightened'}"
              + (f"; R^2 {i['r2']:.9g} (live rows {r2_ref(ix.values[live]):.9g}): {'re-tightened' if i['r2'] == r2_ref(ix.values[live]) else 'not re-tightened'}" if shadow else ""))
    if 9 in stages:   # one more re-layout.  relayout_for ends in the full pass refresh_norms(0, cap_rows), which zeroes the maxima and
        # counts the rows that hold a vector; the batch's own rows then raise them (refresh_tiles): tight on the LIVE rows again
        rows_bytes9 = ix.layout_bytes()["rows"]
        ix.add_batch(around_longest(ix, 6))
        assert ix.layout_bytes()["rows"] > rows_bytes9
        r = check("9 re-layout after removals", tight_live=True)
    if 9 in poison_after:
        poisoned("9")
    if last not in (4, 7):
        twin(f"{last} final state", r)
    ix.close()


KINDS = ("dist_c", "dist_u", "norm_300", "mixed_subnormal")


@gpu
@pytest.mark.parametrize("shadow", [1, 0])
@pytest.mark.parametrize("metric", [capi.METRIC_L2SQ, capi.METRIC_COSDIST])
@pytest.mark.parametrize("d", [96, 300])
def test_certificate_state_after_every_kind_of_mutation(tmp_path, d, metric, shadow):
    """d = 300: ld pads to 320, the padding columns of added and moved rows count.  The four corpus kinds are dealt over the cases."""
    kind = KINDS[(metric + 2 * shadow + (1 if d == 300 else 0)) % 4]
    capi.set_option("shadow", shadow)
    try:
        mutate_and_audit(tmp_path, metric, shadow, d, kind, seed=0xC30 + d)
    finally:
        capi.set_option("shadow", 1)


@gpu
def test_certificate_state_after_mutations_without_the_row_major_copy(tmp_path):
    """memory = 1: the tiles are the only f32 copy, the exact finish gathers its survivors from them"""
    capi.set_option("memory", 1)
    try:
        mutate_and_audit(tmp_path, capi.METRIC_L2SQ, 1, 96, "dist_c", seed=0xC3A)
    finally:
        capi.set_option("memory", 0)


@gpu
def test_certificate_state_after_mutations_hi_only_query_block(tmp_path):
    """d = 1536: the query block of the shadow scan is fp16 hi only; stages 1, 2, 5 and 7.  (At this d the rows scaled by 3 widen the
    window enough that most of the wide batches' queries go to the exact re-scan -- they are audited like the others.  The index sees
    8 batches of 32 = 256 queries: fewer than the shadow's self-retirement check needs, and audit() asserts the shadow still feeds the scan.)"""
    n, d, k, b, nprobe = 2500, 1536, 8, 32, 4
    mutate_and_audit(tmp_path, capi.METRIC_L2SQ, 1, d, "dist_c", n=n, k=k, b=b, nprobe=nprobe, stages=(1, 2, 5, 7), expect_shadow=2, seed=0xC3C)


@gpu
def test_slack_contents_after_removals_and_a_relayout(tmp_path):
    """inf, NaN, -1e30 and 1.5e19 in every storage row that holds no vector -- rows freed by a removal (after stage 6), slack a re-layout
    made (after stage 9): every check of the audit holds and no query more or fewer goes to the exact re-scan than just before"""
    mutate_and_audit(tmp_path, capi.METRIC_L2SQ, 1, 96, "dist_c", poison_after=(6, 9), seed=0xC3D)


# ---- the adversarial case, delivered by add --------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("way", ["add_batch", "single adds", "add_batch into freed slack"])
def test_aligned_shadow_residuals_arrive_after_the_build(way):
    """test_shadow_rounding_errors_aligned_with_the_query with the aligned rows ADDED: the index is built on rows that ARE fp16 numbers
    (R = 0: the shadow term of the bound is 0), then rows whose every element sits 0.49 ulp(fp16) off its fp16 value on the side of the
    query's sign arrive.  R^2 must rise to the new rows' residual; the Cauchy-Schwarz step is attained on them."""
    n, d, k, b, top_k, m = 4096, 128, 8, 32, 10, 512
    rng = np.random.default_rng(0x5AF)
    sgn = rng.choice([-1.0, 1.0], d).astype(np.float32)
    X = ((0.03125 + rng.integers(0, 1024, (n, d)) * 2.0 ** -15) * rng.choice([-1.0, 1.0], (n, d))).astype(np.float32)   # fp16 values in +-[2^-5, 2^-4): ulp 2^-15
    assert np.array_equal(X.astype(np.float16).astype(np.float32), X)
    A = ((0.03125 + rng.integers(0, 1024, (m, d)) * 2.0 ** -15) * rng.choice([-1.0, 1.0], (m, d))).astype(np.float32)
    A = (A + sgn[None, :] * np.float32(0.49 * 2.0 ** -15)).astype(np.float32)                                           # + 0.49 ulp along sgn
    assert not np.any(A.astype(np.float16).astype(np.float32) == A)
    Q = np.tile((sgn / np.sqrt(np.float32(d)))[None, :], (b, 1)).astype(np.float32)
    Q += (1e-3 * rng.standard_normal((b, d))).astype(np.float32)                                                        # distinct queries, still along sgn
    ix = IVFFlatIndex.build_index(k, 1, 2, X, init_indices=mg.init_draws(0x5AF, 1, k, n))
    assert ix.shadow_state()["active"]
    queries = range(0, b, 3)
    r = audit(ix, Q, top_k, k, queries, shadow=1, pristine=True, label=f"fp16-exact rows ({way})")
    assert r["info"]["r2"] == 0.0
    removed = False
    if way == "add_batch":
        ix.add_batch(A)
    elif way == "single adds":
        for x in A:
            ix.add(x)
    else:
        cl = np.array([co.add_cluster(ix.centroids, x) for x in A])
        gone = np.concatenate([np.asarray(l[::3], dtype=np.int64) for l in ix.ids])
        lost = np.array([len(l[::3]) for l in ix.ids])
        assert np.all(np.bincount(cl, minlength=k) <= lost), "the added rows would not fit the freed slack"
        rows_bytes, relayouts = ix.layout_bytes()["rows"], capi.add_batch_phases()["relayouts"]
        assert ix.remove_batch(gone) == gone.size
        removed = True
        ix.add_batch(A)
        assert ix.layout_bytes()["rows"] == rows_bytes and capi.add_batch_phases()["relayouts"] == relayouts
    # the removed rows have no residual: R^2 over every row ever stored is the added rows' either way
    r = audit(ix, Q, top_k, k, queries, shadow=1, pristine=not removed, label=f"aligned residuals by {way}")
    assert r["info"]["r2"] == r2_ref(ix.values) > 0.0, (r["info"]["r2"], r2_ref(ix.values))
    worst, n_added = 0.0, 0
    for qi in queries:
        vids, vals, bnd, info = testhooks.last_vals(ix, qi, cap=32768)
        for vid, val, bd in zip(vids.astype(np.int64), vals, bnd):
            if vid >= n:
                worst = max(worst, abs(float(val) + info["qn"] - d_ref(ix.values[vid], Q[qi], 0)) / bd)
                n_added += 1
    print(f"aligned shadow residuals by {way:26s}: worst |val - exact| / bound = {worst:.4f} over {n_added} vals of added rows")
    assert n_added > 0 and 0.3 < worst <= 1.0, (worst, n_added)
    ix.close()
