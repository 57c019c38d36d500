"""Host-side mirror of vers's IVFFlatIndex (reference: vers/src/indexes/ivfflat.rs) on top of the
C ABI -- the Python stand-in for the Rust `impl Index<N> for IVFFlatIndexHip<N>` shown in
INTEGRATION.md.  Same method names, argument meaning and error behaviour as the reference: the
five fields stay host-owned (for save_index/load_index), the device handle is a cache.

A reference panic surfaces as capi.VersError (status NAN / INSUFFICIENT / EMPTY).
"""
from __future__ import annotations

import ctypes as C
import struct

import numpy as np

from . import capi
from .capi import _ptr, _vp, check, lib


class IVFFlatIndex:
    def __init__(self, d: int, device: int = 0, metric: int = capi.METRIC_L2SQ):
        """metric: METRIC_L2SQ = the reference's IVFFlat; METRIC_COSDIST = 1 - dot (base.rs:153-155) in every distance
        of build / add / search (extension, vers_ivf_set_metric)."""
        self.d = int(d)
        self.device = device
        self.metric = int(metric)
        self._h = _vp()
        check(lib().vers_ivf_create(device, self.d, C.byref(self._h)))
        if self.metric != capi.METRIC_L2SQ:
            check(lib().vers_ivf_set_metric(self._h, self.metric))
        # the reference's fields, in its order (ivfflat.rs:9-15)
        self.num_centroids = 0
        self.values = np.zeros((0, self.d), dtype=np.float32)
        self.centroids = np.zeros((0, self.d), dtype=np.float32)
        self.assignments = np.zeros(0, dtype=np.uint64)
        self.ids = []  # list of python lists of vec ids
        self.cost = np.float32(np.inf)
        self.iterations = None
        self._range_cap = 0  # range_search: the previous call's total, offered as the next call's capacity

    def close(self):
        if self._h:
            lib().vers_ivf_destroy(self._h)
            self._h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- IVFFlatIndex::build_index (ivfflat.rs:102-136) -----------------------------------------
    @classmethod
    def build_index(cls, num_clusters: int, num_attempts: int, max_iterations: int, vectors, init_indices=None,
                    rng=None, device: int = 0, metric: int = capi.METRIC_L2SQ) -> "IVFFlatIndex":
        vectors = np.ascontiguousarray(vectors, dtype=np.float32)
        n, d = vectors.shape
        self = cls(d, device, metric)
        if init_indices is None:
            # initialize_centroids (ivfflat.rs:18-27): k draws WITH replacement per attempt
            rng = rng or np.random.default_rng()
            init_indices = rng.integers(0, max(n, 1), size=num_attempts * num_clusters)
        init = np.ascontiguousarray(np.asarray(init_indices).reshape(-1), dtype=np.uint64)
        assert init.size == num_attempts * num_clusters
        cent = np.zeros((num_clusters, d), dtype=np.float32)
        asg = np.zeros(n, dtype=np.uint64)
        cost = C.c_float(0); kept = C.c_int32(0)
        iters = np.zeros(max(num_attempts, 1), dtype=np.uint64)
        check(lib().vers_ivf_build(self._h, _ptr(vectors), n, 4 * d, num_clusters, num_attempts, max_iterations,
                                   _ptr(init), _ptr(cent), 4 * d, _ptr(asg), C.byref(cost), C.byref(kept), _ptr(iters)))
        self.num_centroids = num_clusters
        self.values = vectors.copy()  # ivfflat.rs:131 vectors.clone()
        self.cost = np.float32(cost.value)
        self.iterations = iters[:num_attempts]
        if kept.value:
            self.centroids, self.assignments = cent, asg
        else:  # nothing beat +inf: empty centroids/assignments (ivfflat.rs:109-110)
            self.centroids = np.zeros((0, d), dtype=np.float32)
            self.assignments = np.zeros(0, dtype=np.uint64)
        self.ids = [[] for _ in range(num_clusters)]
        for vec_id, c in enumerate(self.assignments):  # ivfflat.rs:123-127
            self.ids[int(c)].append(vec_id)
        return self

    # -- Index::add (ivfflat.rs:200-213) ------------------------------------------------------------
    def add(self, embedding, vec_id: int = 0):
        """`vec_id` is accepted and ignored, exactly like the reference (ivfflat.rs:209)."""
        e = np.ascontiguousarray(embedding, dtype=np.float32).reshape(self.d)
        c = C.c_uint64(0); vid = C.c_uint64(0)
        check(lib().vers_ivf_add(self._h, _ptr(e), C.byref(c), C.byref(vid)))
        assert vid.value == len(self.assignments)
        self.values = np.concatenate([self.values, e[None]], axis=0)
        self.assignments = np.concatenate([self.assignments, np.array([c.value], dtype=np.uint64)])
        self.ids[c.value].append(int(vid.value))
        return int(c.value), int(vid.value)

    def add_batch(self, embeddings):
        """`add` for every row of `embeddings` [n][d] in one call (vers_ivf_add_batch): same clusters, vec ids, lists and
        fields as n calls of add.  Returns (clusters, vec_ids) as u64 arrays.  On an error (a NaN distance at row i) the
        rows before it are added and mirrored, then the error is raised."""
        e = np.ascontiguousarray(embeddings, dtype=np.float32).reshape(-1, self.d)
        n = e.shape[0]
        cl = np.zeros(max(n, 1), dtype=np.uint64)
        first = C.c_uint64(0); added = C.c_uint64(0)
        rc = lib().vers_ivf_add_batch(self._h, _ptr(e), n, 4 * self.d, _ptr(cl), C.byref(first), C.byref(added))
        m = int(added.value)
        cl = cl[:m]
        vids = np.arange(first.value, first.value + m, dtype=np.uint64)
        if m:
            assert first.value == len(self.assignments)
            self.values = np.concatenate([self.values, e[:m]], axis=0)
            self.assignments = np.concatenate([self.assignments, cl])
            for c, v in zip(cl.tolist(), vids.tolist()):
                self.ids[c].append(v)
        check(rc)
        return cl, vids

    def add_batch_dev(self, rows_ptr: int, n: int, ld: int, clusters_ptr: int = 0):
        """vers_ivf_add_batch_dev on rows already in HBM ([n][ld] f32); clusters (u64) to clusters_ptr when given.  The host
        fields are NOT mirrored (the rows stay on the device).  Returns (first_vec_id, added)."""
        first = C.c_uint64(0); added = C.c_uint64(0)
        check(lib().vers_ivf_add_batch_dev(self._h, _vp(rows_ptr), n, ld, _vp(clusters_ptr) if clusters_ptr else None, C.byref(first),
                                           C.byref(added)))
        return int(first.value), int(added.value)

    # -- removal (extension; the reference has none): ids[assignments[v]].retain(|&x| x != v) ---------
    def remove_batch(self, vec_ids):
        """Removes the listed vec ids from their inverted lists (vers_ivf_remove_batch): `ids` loses them, `values` and
        `assignments` keep their entries (positions are vec ids).  Any order, repeats allowed, ids already gone are skipped;
        an id >= len(assignments) raises and removes nothing.  Returns the number of rows that left the index."""
        v = np.ascontiguousarray(np.asarray(vec_ids, dtype=np.uint64).reshape(-1))
        removed = C.c_uint64(0)
        check(lib().vers_ivf_remove_batch(self._h, _ptr(v) if v.size else None, v.size, C.byref(removed)))
        gone = set(v.tolist())
        expect = 0
        for c, lst in enumerate(self.ids):
            kept = [x for x in lst if x not in gone]
            expect += len(lst) - len(kept)
            self.ids[c] = kept
        assert removed.value == expect, (removed.value, expect)
        return int(removed.value)

    def remove_batch_dev(self, ids_ptr: int, n: int, comm=None):
        """vers_ivf_remove_batch_dev on a device array of u64 vec ids; comm: the vers_amd.dist.TorchComm of a sharded handle
        (every rank calls with the same ids).  The host fields are NOT mirrored.  Returns the number of rows removed."""
        removed = C.c_uint64(0)
        check(lib().vers_ivf_remove_batch_dev(self._h, _vp(ids_ptr) if n else None, n, comm.ptr() if comm is not None else None,
                                              C.byref(removed)))
        return int(removed.value)

    # -- update (extension; the reference has none): values[v] = x, the row to the list of its first-minimum centroid ----
    def update_batch(self, vec_ids, embeddings):
        """Replaces the vectors stored under `vec_ids` by the rows of `embeddings` (vers_ivf_update_batch); the vec ids are kept.  A row
        whose first-minimum centroid is still its list is overwritten in place; one that changes cluster leaves its list and enters the
        new one at its sorted place by vec id (bisect.insort); an id that is in no list is skipped.  All or nothing: an id >=
        len(assignments), an id twice in the call or a NaN distance raises and changes nothing.  The host mirror follows and the device's
        clusters and status are asserted against it.  Returns (clusters, status): u64 [n], u8 [n] (0 stayed, 1 moved, 2 skipped)."""
        import bisect
        v = np.ascontiguousarray(np.asarray(vec_ids, dtype=np.uint64).reshape(-1))
        e = np.ascontiguousarray(embeddings, dtype=np.float32).reshape(-1, self.d)
        n = v.size
        assert e.shape[0] == n
        cl = np.zeros(max(n, 1), dtype=np.uint64)
        st = np.zeros(max(n, 1), dtype=np.uint8)
        counts = np.zeros(4, dtype=np.uint64)
        check(lib().vers_ivf_update_batch(self._h, _ptr(v) if n else None, _ptr(e) if n else None, n, 4 * self.d, _ptr(cl), _ptr(st), counts.ctypes.data_as(C.POINTER(C.c_uint64))))
        cl, st = cl[:n], st[:n]
        self.values = self.values.copy()
        self.assignments = self.assignments.copy()
        want = np.zeros(n, dtype=np.uint8)
        for i, (vid, c) in enumerate(zip(v.tolist(), cl.tolist())):
            old = int(self.assignments[vid])
            lst = self.ids[old]
            j = bisect.bisect_left(lst, vid)
            if j == len(lst) or lst[j] != vid:
                want[i] = 2
                continue
            self.values[vid] = e[i]
            if c != old:
                want[i] = 1
                del lst[j]
                self.assignments[vid] = c
                bisect.insort(self.ids[c], vid)
        assert np.array_equal(st, want), (st, want)
        assert counts[:3].tolist() == [int((want == s).sum()) for s in (0, 1, 2)], counts
        self.last_update_counts = tuple(int(x) for x in counts)
        return cl, st

    def update_batch_dev(self, ids_ptr: int, rows_ptr: int, n: int, ld: int, clusters_ptr: int = 0, status_ptr: int = 0):
        """vers_ivf_update_batch_dev on device arrays: u64 vec ids, rows [n][ld] f32; clusters (u64) / status (u8) to device memory when
        given.  The host fields are NOT mirrored.  Returns (stayed, moved, skipped, relayouts)."""
        counts = np.zeros(4, dtype=np.uint64)
        check(lib().vers_ivf_update_batch_dev(self._h, _vp(ids_ptr) if n else None, _vp(rows_ptr) if n else None, n, ld,
                                              _vp(clusters_ptr) if clusters_ptr else None, _vp(status_ptr) if status_ptr else None, counts.ctypes.data_as(C.POINTER(C.c_uint64))))
        return tuple(int(x) for x in counts)

    def compact(self):
        """vers_ivf_compact: every list back to the capacity a fresh upload of the current lengths plans, the certificate maxima
        recomputed over the rows the lists hold.  Nothing of the five fields changes (the host mirror is left as it is).  Returns
        (storage rows before, storage rows after)."""
        before, after = C.c_uint64(0), C.c_uint64(0)
        check(lib().vers_ivf_compact(self._h, C.byref(before), C.byref(after)))
        return int(before.value), int(after.value)

    # -- recluster (extension): build_index over the live rows in ascending vec id, the vec ids kept -----------------
    def recluster(self, num_clusters: int, num_attempts: int, max_iterations: int, init_indices=None, rng=None):
        """vers_ivf_recluster: k-means again over the rows that are in some list, taken in ascending vec id (L); `init_indices`
        [num_attempts * num_clusters] are POSITIONS in L (drawn as build_index draws them when None).  When an attempt is kept,
        `centroids`, `assignments` (0 for an id in no list), `ids` and `num_centroids` follow the call's outputs; `values`,
        len(assignments) and the live count do not change.  When none is kept (num_attempts == 0, no finite cost) nothing changes.
        A refusal raises and changes nothing.  Returns (cost, kept, iterations)."""
        n = len(self.assignments)
        live = np.sort(np.fromiter((v for lst in self.ids for v in lst), dtype=np.int64))
        if init_indices is None:
            rng = rng or np.random.default_rng()
            init_indices = rng.integers(0, max(live.size, 1), size=num_attempts * num_clusters)
        init = np.ascontiguousarray(np.asarray(init_indices).reshape(-1), dtype=np.uint64)
        assert init.size == num_attempts * num_clusters
        cent = np.zeros((max(num_clusters, 1), self.d), dtype=np.float32)
        asg = np.zeros(max(n, 1), dtype=np.uint64)
        cost = C.c_float(np.inf); kept = C.c_int32(0)
        iters = np.zeros(max(num_attempts, 1), dtype=np.uint64)
        check(lib().vers_ivf_recluster(self._h, num_clusters, num_attempts, max_iterations, _ptr(init) if init.size else None, _ptr(cent), 4 * self.d,
                                       _ptr(asg), C.byref(cost), C.byref(kept), _ptr(iters)))
        if kept.value:
            asg = asg[:n]
            dead = np.ones(n, dtype=bool)
            dead[live] = False
            assert not asg[dead].any()
            self.num_centroids = int(num_clusters)
            self.centroids, self.assignments = cent[:num_clusters], asg
            self.ids = [[] for _ in range(num_clusters)]
            for v in live.tolist():  # ascending vec id: every list ascending
                self.ids[int(asg[v])].append(v)
            self.cost = np.float32(cost.value)
            self.iterations = iters[:num_attempts]
        return np.float32(cost.value), int(kept.value), iters[:num_attempts]

    def live_count(self):
        live = C.c_uint64(0)
        check(lib().vers_ivf_live_count(self._h, C.byref(live)))
        return int(live.value)

    # -- fetch (extension): the stored vector, its list and whether it is still there, by vec id --------------------
    def fetch(self, vec_ids, want_rows: bool = True, row_stride_floats=None, fill=None):
        """vers_ivf_fetch: for every v of `vec_ids` (any order, repeats allowed) the stored vector, its cluster and a status -- 0 found,
        2 in no list (then the row is zeros and the cluster capi.NO_CLUSTER).  An id >= len(assignments) raises and writes nothing.
        row_stride_floats / fill: the rows come back in a [n, stride] array prefilled with `fill` (columns >= d are never written).
        -> (rows [n, d or stride] f32 or None, clusters [n] u64, status [n] u8); the counts are left in last_fetch_counts."""
        v = np.ascontiguousarray(np.asarray(vec_ids, dtype=np.uint64).reshape(-1))
        n = v.size
        stride = self.d if row_stride_floats is None else int(row_stride_floats)
        rows = np.full((max(n, 1), stride), 0.0 if fill is None else fill, dtype=np.float32) if want_rows else None
        cl = np.zeros(max(n, 1), dtype=np.uint64)
        st = np.zeros(max(n, 1), dtype=np.uint8)
        counts = np.zeros(2, dtype=np.uint64)
        check(lib().vers_ivf_fetch(self._h, _ptr(v) if n else None, n, _ptr(rows) if want_rows else None, 4 * stride, _ptr(cl), _ptr(st),
                                   counts.ctypes.data_as(C.POINTER(C.c_uint64))))
        self.last_fetch_counts = (int(counts[0]), int(counts[1]))
        return (rows[:n] if want_rows else None), cl[:n], st[:n]

    def fetch_dev(self, ids_ptr: int, n: int, rows_ptr: int = 0, ld: int = 0, clusters_ptr: int = 0, status_ptr: int = 0, stream: int = 0):
        """vers_ivf_fetch_dev on device arrays: u64 vec ids in; rows [n][ld] f32, clusters (u64), status (u8) out, each optional.  Queued on
        `stream` and waited for.  Returns (found, in no list)."""
        counts = np.zeros(2, dtype=np.uint64)
        check(lib().vers_ivf_fetch_dev(self._h, _vp(ids_ptr) if n else None, n, _vp(rows_ptr) if rows_ptr else None, ld, _vp(clusters_ptr) if clusters_ptr else None,
                                       _vp(status_ptr) if status_ptr else None, counts.ctypes.data_as(C.POINTER(C.c_uint64)), _vp(stream)))
        return int(counts[0]), int(counts[1])

    def search_by_id(self, vec_ids, top_k: int, nprobe: int = 0, exclude_self: bool = False):
        """search_batch(values[vec_ids], top_k, nprobe) without the queries leaving the device (vers_ivf_search_by_id).  exclude_self
        (nprobe >= 1): each row as on an index from which its own id alone was removed.  An id that is in no list raises."""
        v = np.ascontiguousarray(np.asarray(vec_ids, dtype=np.uint64).reshape(-1))
        b = v.size
        ids = np.zeros((b, max(top_k, 1)), dtype=np.uint64)
        dist = np.zeros((b, max(top_k, 1)), dtype=np.float32)
        cnt = np.zeros(max(b, 1), dtype=np.uint32)
        check(lib().vers_ivf_search_by_id(self._h, _ptr(v) if b else None, b, top_k, nprobe, capi.BYID_EXCLUDE_SELF if exclude_self else 0, _ptr(ids), _ptr(dist),
                                          _ptr(cnt)))
        return ids[:, :top_k], dist[:, :top_k], cnt[:b]

    def search_by_id_dev(self, ids_in_ptr: int, b: int, top_k: int, nprobe: int, ids_ptr: int, dist_ptr: int, cnt_ptr: int, exclude_self: bool = False,
                         stream: int = 0, flags=None):
        """vers_ivf_search_by_id_dev on raw device pointers; after the id check it is search_dev's protocol: poll() reports."""
        f = (capi.BYID_EXCLUDE_SELF if exclude_self else 0) if flags is None else int(flags)
        check(lib().vers_ivf_search_by_id_dev(self._h, _vp(ids_in_ptr) if b else None, b, top_k, nprobe, f, _vp(ids_ptr), _vp(dist_ptr), _vp(cnt_ptr), _vp(stream)))

    # -- the same on handles sharded by cluster: every rank calls with the same ids ------------------------------------
    def fetch_sharded_dev(self, comm, ids_ptr: int, n: int, rows_ptr: int = 0, ld: int = 0, clusters_ptr: int = 0, status_ptr: int = 0, stream: int = 0):
        """vers_ivf_fetch_sharded_dev: fetch_dev on a handle sharded by cluster.  comm: the vers_amd.dist.TorchComm of the handle (None on
        an unsharded one: the call is fetch_dev).  One all_gather tells every rank where each id lives, one per non-empty chunk of
        option "add_batch_rows" requests carries the rows; every rank receives what fetch_dev returns on the unsharded index.
        Returns (found, in no list)."""
        counts = np.zeros(2, dtype=np.uint64)
        check(lib().vers_ivf_fetch_sharded_dev(self._h, comm.ptr() if comm is not None else None, _vp(ids_ptr) if n else None, n, _vp(rows_ptr) if rows_ptr else None, ld,
                                               _vp(clusters_ptr) if clusters_ptr else None, _vp(status_ptr) if status_ptr else None,
                                               counts.ctypes.data_as(C.POINTER(C.c_uint64)), _vp(stream)))
        return int(counts[0]), int(counts[1])

    def update_batch_sharded_dev(self, comm, ids_ptr: int, rows_ptr: int, n: int, ld: int, clusters_ptr: int = 0, status_ptr: int = 0):
        """vers_ivf_update_batch_sharded_dev: update_batch_dev on a handle sharded by cluster.  EVERY rank calls with the same ids and rows
        (comm: the vers_amd.dist.TorchComm of the handle; None on an unsharded one: the call is update_batch_dev); one all_gather tells
        every rank where each id lives, no row crosses ranks.  The host fields are NOT mirrored.  Returns (stayed, moved, skipped,
        this rank's relayouts)."""
        counts = np.zeros(4, dtype=np.uint64)
        check(lib().vers_ivf_update_batch_sharded_dev(self._h, comm.ptr() if comm is not None else None, _vp(ids_ptr) if n else None, _vp(rows_ptr) if n else None, n, ld,
                                                      _vp(clusters_ptr) if clusters_ptr else None, _vp(status_ptr) if status_ptr else None,
                                                      counts.ctypes.data_as(C.POINTER(C.c_uint64))))
        return tuple(int(x) for x in counts)

    def search_by_id_sharded_dev(self, comm, gather_ptr, ids_in_ptr: int, b: int, top_k: int, nprobe: int, ids_ptr: int, dist_ptr: int, cnt_ptr: int,
                                 exclude_self: bool = False, stream: int = 0, flags=None):
        """vers_ivf_search_by_id_sharded_dev: search_by_id_dev on a handle sharded by cluster.  comm (dist.TorchComm) carries the where
        round and the row round that put the query block on every rank, gather_ptr (dist.TorchGather.ptr() or RcclComm.gather_ptr())
        the sharded search behind them; both None on an unsharded handle.  After the id check it is search_sharded_dev's protocol."""
        f = (capi.BYID_EXCLUDE_SELF if exclude_self else 0) if flags is None else int(flags)
        check(lib().vers_ivf_search_by_id_sharded_dev(self._h, comm.ptr() if comm is not None else None, gather_ptr, _vp(ids_in_ptr) if b else None, b, top_k, nprobe, f,
                                                      _vp(ids_ptr), _vp(dist_ptr), _vp(cnt_ptr), _vp(stream)))

    def sync_from_device(self, chunk: int = 1 << 16):
        """Rebuilds the host fields from the handle -- what a process that used the _dev mutators (which do not mirror) needs before
        save_index.  Ids 0 .. n-1 are fetched in chunks: `values[v]` and `assignments[v]` are replaced for every id that is in a list;
        entries of ids in no list keep what the mirror held (nothing observable depends on them), zeros / 0 beyond the mirror's length;
        `ids[c]` = the ascending found ids of cluster c; `centroids` through vers_ivf_get_centroids.  Returns (found, in no list)."""
        n, k, _ = self.info()
        values = np.zeros((n, self.d), dtype=np.float32)
        assignments = np.zeros(n, dtype=np.uint64)
        keep = min(n, len(self.assignments), len(self.values))
        values[:keep] = self.values[:keep]
        assignments[:keep] = self.assignments[:keep]
        found_mask = np.zeros(n, dtype=bool)
        for v0 in range(0, n, max(1, int(chunk))):
            v1 = min(n, v0 + max(1, int(chunk)))
            rows, cl, st = self.fetch(np.arange(v0, v1, dtype=np.uint64))
            ok = st == capi.FETCH_FOUND
            values[v0:v1][ok] = rows[ok]
            assignments[v0:v1][ok] = cl[ok]
            found_mask[v0:v1] = ok
        self.values, self.assignments = values, assignments
        self.num_centroids = int(k)
        self.centroids = self.get_centroids()
        self.ids = [[] for _ in range(int(k))]
        for v in np.flatnonzero(found_mask).tolist():  # ascending vec id: every list ascending
            self.ids[int(assignments[v])].append(v)
        return int(found_mask.sum()), int(n - found_mask.sum())

    # -- Index::search_approximate (ivfflat.rs:153-198) ---------------------------------------------
    def search_approximate(self, query, top_k: int):
        ids, dist, cnt = self.search_batch(np.asarray(query, dtype=np.float32).reshape(1, self.d), top_k, nprobe=0)
        return [(int(i), np.float32(x)) for i, x in zip(ids[0, :cnt[0]], dist[0, :cnt[0]])]

    def search_batch(self, queries, top_k: int, nprobe: int = 0):
        q = np.ascontiguousarray(np.atleast_2d(queries), dtype=np.float32)
        b = q.shape[0]
        ids = np.zeros((b, max(top_k, 1)), dtype=np.uint64)
        dist = np.zeros((b, max(top_k, 1)), dtype=np.float32)
        cnt = np.zeros(b, dtype=np.uint32)
        check(lib().vers_ivf_search(self._h, _ptr(q), 4 * self.d, b, top_k, nprobe, _ptr(ids), _ptr(dist), _ptr(cnt)))
        return ids[:, :top_k], dist[:, :top_k], cnt

    def search_exhaustive(self, queries, top_k: int, metric: int = capi.METRIC_L2SQ):
        q = np.ascontiguousarray(np.atleast_2d(queries), dtype=np.float32)
        b = q.shape[0]
        ids = np.zeros((b, max(top_k, 1)), dtype=np.uint64)
        dist = np.zeros((b, max(top_k, 1)), dtype=np.float32)
        cnt = np.zeros(b, dtype=np.uint32)
        check(lib().vers_ivf_search_exhaustive(self._h, _ptr(q), 4 * self.d, b, top_k, metric, _ptr(ids), _ptr(dist), _ptr(cnt)))
        return ids[:, :top_k], dist[:, :top_k], cnt

    # -- filtered search (extension): a bitmap of allowed vec ids per call = a virtual remove_batch of the others -----
    @staticmethod
    def _filter_words(allowed, n_bits):
        """allowed -> (u64 words, n_bits).  A bool array (allowed[v]; n_bits defaults to its length), an integer array of allowed vec ids
        (n_bits defaults to the largest id + 1), or a ready (words, n_bits) pair as capi.allowed_bitmap packs it."""
        if isinstance(allowed, tuple):
            words, nb = allowed
            return np.ascontiguousarray(words, dtype=np.uint64), int(nb)
        a = np.asarray(allowed)
        if n_bits is None:
            n_bits = a.size if a.dtype == np.bool_ else (int(a.max()) + 1 if a.size else 0)
        return capi.allowed_bitmap(a, n_bits), int(n_bits)

    def search_filtered(self, queries, top_k: int, nprobe: int, allowed, n_bits=None):
        """search_batch(queries, top_k, nprobe) on the index WITHOUT the vec ids `allowed` leaves out (vers_ivf_search_filtered; nprobe >= 1):
        the allowed rows of the min(nprobe, k) nearest lists, ascending (distance, probe rank, list position); the index is not touched.
        -> (ids [b, top_k] u64, dist [b, top_k] f32, count [b] u32); count may be 0."""
        q = np.ascontiguousarray(np.atleast_2d(queries), dtype=np.float32)
        b = q.shape[0]
        words, nb = self._filter_words(allowed, n_bits)
        ids = np.zeros((b, max(top_k, 1)), dtype=np.uint64)
        dist = np.zeros((b, max(top_k, 1)), dtype=np.float32)
        cnt = np.zeros(b, dtype=np.uint32)
        check(lib().vers_ivf_search_filtered(self._h, _ptr(q), 4 * self.d, b, top_k, nprobe, _ptr(words), nb, _ptr(ids), _ptr(dist), _ptr(cnt)))
        return ids[:, :top_k], dist[:, :top_k], cnt

    def search_exhaustive_filtered(self, queries, top_k: int, allowed, metric: int = capi.METRIC_L2SQ, n_bits=None):
        """search_exhaustive over the allowed rows that are in a list now (vers_ivf_search_exhaustive_filtered): ascending (distance, vec id)."""
        q = np.ascontiguousarray(np.atleast_2d(queries), dtype=np.float32)
        b = q.shape[0]
        words, nb = self._filter_words(allowed, n_bits)
        ids = np.zeros((b, max(top_k, 1)), dtype=np.uint64)
        dist = np.zeros((b, max(top_k, 1)), dtype=np.float32)
        cnt = np.zeros(b, dtype=np.uint32)
        check(lib().vers_ivf_search_exhaustive_filtered(self._h, _ptr(q), 4 * self.d, b, top_k, metric, _ptr(words), nb, _ptr(ids), _ptr(dist),
                                                        _ptr(cnt)))
        return ids[:, :top_k], dist[:, :top_k], cnt

    def search_filtered_dev(self, q_ptr: int, ldq: int, b: int, top_k: int, nprobe: int, bits_ptr: int, n_bits: int, ids_ptr: int, dist_ptr: int,
                            cnt_ptr: int, stream: int = 0):
        """vers_ivf_search_filtered_dev on raw device pointers (the bitmap too); queued on `stream`, not synchronised: poll() reports."""
        check(lib().vers_ivf_search_filtered_dev(self._h, _vp(q_ptr), ldq, b, top_k, nprobe, _vp(bits_ptr) if bits_ptr else None, n_bits,
                                                 _vp(ids_ptr), _vp(dist_ptr), _vp(cnt_ptr), _vp(stream)))

    def search_exhaustive_filtered_dev(self, q_ptr: int, ldq: int, b: int, top_k: int, metric: int, bits_ptr: int, n_bits: int, ids_ptr: int,
                                       dist_ptr: int, cnt_ptr: int, stream: int = 0):
        check(lib().vers_ivf_search_exhaustive_filtered_dev(self._h, _vp(q_ptr), ldq, b, top_k, metric, _vp(bits_ptr) if bits_ptr else None, n_bits,
                                                            _vp(ids_ptr), _vp(dist_ptr), _vp(cnt_ptr), _vp(stream)))

    # -- filtered search with a filter per query: query q of the batch uses bitmap filter_of[q] -----
    @staticmethod
    def _filters_words(filters, n_bits):
        """filters -> (u64 [n_filters, stride] words, n_bits).  A sequence of bool arrays / id arrays (n_bits defaults to the largest any of
        them needs) or a ready (words [n_filters, stride], n_bits) pair as capi.allowed_bitmaps packs it."""
        if isinstance(filters, tuple):
            words, nb = filters
            words = np.ascontiguousarray(words, dtype=np.uint64)
            return words.reshape(len(words), -1), int(nb)
        arrs = [np.asarray(a) for a in filters]
        if n_bits is None:
            n_bits = max([a.size if a.dtype == np.bool_ else (int(a.max()) + 1 if a.size else 0) for a in arrs], default=0)
        return capi.allowed_bitmaps(arrs, n_bits), int(n_bits)

    def _filtered_multi(self, fn, queries, top_k, arg, filters, filter_of, n_bits):
        q = np.ascontiguousarray(np.atleast_2d(queries), dtype=np.float32)
        b = q.shape[0]
        words, nb = self._filters_words(filters, n_bits)
        fo = np.ascontiguousarray(np.broadcast_to(np.asarray(filter_of, dtype=np.uint32).reshape(-1), (b,)))
        ids = np.zeros((b, max(top_k, 1)), dtype=np.uint64)
        dist = np.zeros((b, max(top_k, 1)), dtype=np.float32)
        cnt = np.zeros(b, dtype=np.uint32)
        check(fn(self._h, _ptr(q), 4 * self.d, b, top_k, arg, _ptr(words), words.shape[1] if words.size else 0, words.shape[0], nb, _ptr(fo), _ptr(ids),
                 _ptr(dist), _ptr(cnt)))
        return ids[:, :top_k], dist[:, :top_k], cnt

    def search_filtered_multi(self, queries, top_k: int, nprobe: int, filters, filter_of, n_bits=None):
        """One batch whose queries use different filters (vers_ivf_search_filtered_multi; nprobe >= 1): row q is row q of
        search_filtered(queries, top_k, nprobe, filters[filter_of[q]]), bit for bit.  At most capi.FILTER_MAX filters per call.
        -> (ids [b, top_k] u64, dist [b, top_k] f32, count [b] u32); count may be 0."""
        return self._filtered_multi(lib().vers_ivf_search_filtered_multi, queries, top_k, nprobe, filters, filter_of, n_bits)

    def search_exhaustive_filtered_multi(self, queries, top_k: int, filters, filter_of, metric: int = capi.METRIC_L2SQ, n_bits=None):
        """search_exhaustive_filtered with a filter per query (vers_ivf_search_exhaustive_filtered_multi)."""
        return self._filtered_multi(lib().vers_ivf_search_exhaustive_filtered_multi, queries, top_k, metric, filters, filter_of, n_bits)

    def search_filtered_multi_dev(self, q_ptr: int, ldq: int, b: int, top_k: int, nprobe: int, filters_ptr: int, stride_words: int, n_filters: int,
                                  n_bits: int, filter_of_ptr: int, ids_ptr: int, dist_ptr: int, cnt_ptr: int, stream: int = 0):
        """vers_ivf_search_filtered_multi_dev on raw device pointers (bitmaps and filter_of too); queued on `stream`, not synchronised: poll()
        reports.  A filter_of entry at or beyond n_filters selects the empty filter."""
        check(lib().vers_ivf_search_filtered_multi_dev(self._h, _vp(q_ptr), ldq, b, top_k, nprobe, _vp(filters_ptr) if filters_ptr else None, stride_words,
                                                       n_filters, n_bits, _vp(filter_of_ptr) if filter_of_ptr else None, _vp(ids_ptr), _vp(dist_ptr),
                                                       _vp(cnt_ptr), _vp(stream)))

    def search_exhaustive_filtered_multi_dev(self, q_ptr: int, ldq: int, b: int, top_k: int, metric: int, filters_ptr: int, stride_words: int,
                                             n_filters: int, n_bits: int, filter_of_ptr: int, ids_ptr: int, dist_ptr: int, cnt_ptr: int, stream: int = 0):
        check(lib().vers_ivf_search_exhaustive_filtered_multi_dev(self._h, _vp(q_ptr), ldq, b, top_k, metric, _vp(filters_ptr) if filters_ptr else None,
                                                                  stride_words, n_filters, n_bits, _vp(filter_of_ptr) if filter_of_ptr else None,
                                                                  _vp(ids_ptr), _vp(dist_ptr), _vp(cnt_ptr), _vp(stream)))

    # -- adaptive depth: every query probes until min_allowed allowed rows are in reach, between nprobe_min and nprobe_max lists -----
    def search_filtered_adaptive(self, queries, top_k: int, nprobe_min: int, nprobe_max: int, min_allowed: int, allowed, n_bits=None):
        """vers_ivf_search_filtered_adaptive: row q is row q of search_filtered(queries, top_k, P_q, allowed), bit for bit, with P_q the
        smallest depth in [min(nprobe_min, k), min(nprobe_max, k)] whose lists hold min_allowed allowed rows (or the upper end).
        -> (ids [b, top_k] u64, dist [b, top_k] f32, count [b] u32, nprobe [b] u32 = P_q)."""
        q = np.ascontiguousarray(np.atleast_2d(queries), dtype=np.float32)
        b = q.shape[0]
        words, nb = self._filter_words(allowed, n_bits)
        ids = np.zeros((b, max(top_k, 1)), dtype=np.uint64)
        dist = np.zeros((b, max(top_k, 1)), dtype=np.float32)
        cnt = np.zeros(b, dtype=np.uint32)
        npr = np.zeros(b, dtype=np.uint32)
        check(lib().vers_ivf_search_filtered_adaptive(self._h, _ptr(q), 4 * self.d, b, top_k, nprobe_min, nprobe_max, min_allowed, _ptr(words), nb,
                                                      _ptr(ids), _ptr(dist), _ptr(cnt), _ptr(npr)))
        return ids[:, :top_k], dist[:, :top_k], cnt, npr

    def search_filtered_adaptive_dev(self, q_ptr: int, ldq: int, b: int, top_k: int, nprobe_min: int, nprobe_max: int, min_allowed: int, bits_ptr: int,
                                     n_bits: int, ids_ptr: int, dist_ptr: int, cnt_ptr: int, nprobe_ptr: int, stream: int = 0):
        """vers_ivf_search_filtered_adaptive_dev on raw device pointers (nprobe_ptr: u32 [b] or 0); queued on `stream`, not synchronised."""
        check(lib().vers_ivf_search_filtered_adaptive_dev(self._h, _vp(q_ptr), ldq, b, top_k, nprobe_min, nprobe_max, min_allowed,
                                                          _vp(bits_ptr) if bits_ptr else None, n_bits, _vp(ids_ptr), _vp(dist_ptr), _vp(cnt_ptr),
                                                          _vp(nprobe_ptr) if nprobe_ptr else None, _vp(stream)))

    def search_filtered_multi_adaptive(self, queries, top_k: int, nprobe_min: int, nprobe_max: int, min_allowed: int, filters, filter_of, n_bits=None):
        """vers_ivf_search_filtered_multi_adaptive: row q is row q of search_filtered_adaptive with bitmap filters[filter_of[q]].
        -> (ids, dist, count, nprobe)."""
        q = np.ascontiguousarray(np.atleast_2d(queries), dtype=np.float32)
        b = q.shape[0]
        words, nb = self._filters_words(filters, n_bits)
        fo = np.ascontiguousarray(np.broadcast_to(np.asarray(filter_of, dtype=np.uint32).reshape(-1), (b,)))
        ids = np.zeros((b, max(top_k, 1)), dtype=np.uint64)
        dist = np.zeros((b, max(top_k, 1)), dtype=np.float32)
        cnt = np.zeros(b, dtype=np.uint32)
        npr = np.zeros(b, dtype=np.uint32)
        check(lib().vers_ivf_search_filtered_multi_adaptive(self._h, _ptr(q), 4 * self.d, b, top_k, nprobe_min, nprobe_max, min_allowed, _ptr(words),
                                                            words.shape[1] if words.size else 0, words.shape[0], nb, _ptr(fo), _ptr(ids), _ptr(dist),
                                                            _ptr(cnt), _ptr(npr)))
        return ids[:, :top_k], dist[:, :top_k], cnt, npr

    def search_filtered_multi_adaptive_dev(self, q_ptr: int, ldq: int, b: int, top_k: int, nprobe_min: int, nprobe_max: int, min_allowed: int,
                                           filters_ptr: int, stride_words: int, n_filters: int, n_bits: int, filter_of_ptr: int, ids_ptr: int,
                                           dist_ptr: int, cnt_ptr: int, nprobe_ptr: int, stream: int = 0):
        """vers_ivf_search_filtered_multi_adaptive_dev on raw device pointers; a filter_of entry at or beyond n_filters selects the empty filter
        (depth min(nprobe_max, k), count 0)."""
        check(lib().vers_ivf_search_filtered_multi_adaptive_dev(self._h, _vp(q_ptr), ldq, b, top_k, nprobe_min, nprobe_max, min_allowed,
                                                                _vp(filters_ptr) if filters_ptr else None, stride_words, n_filters, n_bits,
                                                                _vp(filter_of_ptr) if filter_of_ptr else None, _vp(ids_ptr), _vp(dist_ptr), _vp(cnt_ptr),
                                                                _vp(nprobe_ptr) if nprobe_ptr else None, _vp(stream)))

    def filter_stats(self):
        """vers_ivf_filter_stats: of the most recent filtered call and over the handle's life -- 64-row tile visits the plan implied, tile
        visits actually loaded, work items skipped before their first load, allowed storage rows."""
        last = (C.c_uint64 * 4)(); tot = (C.c_uint64 * 4)()
        check(lib().vers_ivf_filter_stats(self._h, last, tot))
        keys = ("tiles_planned", "tiles_loaded", "items_skipped", "rows_allowed")
        return dict(last=dict(zip(keys, (int(v) for v in last))), total=dict(zip(keys, (int(v) for v in tot))))

    # -- range search (extension; the reference has search_approximate only) ---------------------------
    def range_search(self, queries, radius, nprobe: int, walk_order: bool = False):
        """Every row of the min(nprobe, k) nearest lists of each query with distance <= radius (vers_ivf_range_search).  radius: a
        scalar or one value per query.  -> (lims [b + 1] u64, ids u64, dist f32), CSR: query q owns [lims[q], lims[q + 1]).  Default
        order: ascending (distance, probe rank, list position) = the head of search_batch(top_k = all, nprobe); walk_order: probe
        rank, then list position.  The first call offers the previous call's total as capacity (0 the first time: a size query);
        a second call follows when that was too small."""
        q = np.ascontiguousarray(np.atleast_2d(queries), dtype=np.float32)
        b = q.shape[0]
        r = np.ascontiguousarray(np.broadcast_to(np.asarray(radius, dtype=np.float32).reshape(-1), (b,)) if np.ndim(radius) else
                                 np.full(b, radius, dtype=np.float32))
        flags = capi.RANGE_WALK_ORDER if walk_order else 0
        lims = np.zeros(b + 1, dtype=np.uint64)
        cap = int(self._range_cap)
        total = C.c_uint64(0)
        while True:
            ids = np.zeros(cap, dtype=np.uint64); dist = np.zeros(cap, dtype=np.float32)
            check(lib().vers_ivf_range_search(self._h, _ptr(q), 4 * self.d, b, _ptr(r), nprobe, flags, _ptr(lims), _ptr(ids) if cap else None,
                                              _ptr(dist) if cap else None, cap, C.byref(total)))
            if total.value <= cap:
                break
            cap = int(total.value)
        self._range_cap = int(total.value)
        return lims, ids[:total.value], dist[:total.value]

    def range_search_dev(self, q_ptr: int, ldq: int, b: int, radius_ptr: int, nprobe: int, flags: int, lims_ptr: int, ids_ptr: int,
                         dist_ptr: int, cap: int, stream: int = 0) -> int:
        """vers_ivf_range_search_dev on raw device pointers; synchronous.  Returns the total: ids / distances were written only when it
        is <= cap."""
        total = C.c_uint64(0)
        check(lib().vers_ivf_range_search_dev(self._h, _vp(q_ptr), ldq, b, _vp(radius_ptr), nprobe, flags, _vp(lims_ptr),
                                              _vp(ids_ptr) if ids_ptr else None, _vp(dist_ptr) if dist_ptr else None, cap, C.byref(total),
                                              _vp(stream)))
        return int(total.value)

    def range_search_exhaustive(self, queries, radius, metric: int = capi.METRIC_L2SQ, walk_order: bool = False):
        """Every row that is in a list now with distance <= radius (vers_ivf_range_search_exhaustive): the ground truth of range_search.
        -> (lims, ids, dist) like range_search, by the same two-call protocol.  Default order: ascending (distance, vec id) = the head of
        search_exhaustive(top_k = all rows); walk_order: ascending cluster, then list position (get_list(0), (1), ... concatenated)."""
        q = np.ascontiguousarray(np.atleast_2d(queries), dtype=np.float32)
        b = q.shape[0]
        r = capi.range_radii(radius, b)
        flags = capi.RANGE_WALK_ORDER if walk_order else 0
        lims = np.zeros(b + 1, dtype=np.uint64)
        cap = int(self._range_cap)
        total = C.c_uint64(0)
        while True:
            ids = np.zeros(cap, dtype=np.uint64); dist = np.zeros(cap, dtype=np.float32)
            check(lib().vers_ivf_range_search_exhaustive(self._h, _ptr(q), 4 * self.d, b, _ptr(r), metric, flags, _ptr(lims),
                                                         _ptr(ids) if cap else None, _ptr(dist) if cap else None, cap, C.byref(total)))
            if total.value <= cap:
                break
            cap = int(total.value)
        self._range_cap = int(total.value)
        return lims, ids[:total.value], dist[:total.value]

    def range_search_exhaustive_dev(self, q_ptr: int, ldq: int, b: int, radius_ptr: int, metric: int, flags: int, lims_ptr: int, ids_ptr: int,
                                    dist_ptr: int, cap: int, stream: int = 0) -> int:
        """vers_ivf_range_search_exhaustive_dev on raw device pointers; synchronous.  Returns the total: ids / distances were written only
        when it is <= cap."""
        total = C.c_uint64(0)
        check(lib().vers_ivf_range_search_exhaustive_dev(self._h, _vp(q_ptr), ldq, b, _vp(radius_ptr), metric, flags, _vp(lims_ptr),
                                                         _vp(ids_ptr) if ids_ptr else None, _vp(dist_ptr) if dist_ptr else None, cap,
                                                         C.byref(total), _vp(stream)))
        return int(total.value)

    # -- filtered range search (extension): range search on the index WITHOUT the vec ids `allowed` leaves out -----
    def _range_filtered(self, fn, queries, radius, arg, allowed, n_bits, walk_order):
        q = np.ascontiguousarray(np.atleast_2d(queries), dtype=np.float32)
        b = q.shape[0]
        r = capi.range_radii(radius, b)
        words, nb = self._filter_words(allowed, n_bits)
        flags = capi.RANGE_WALK_ORDER if walk_order else 0
        lims = np.zeros(b + 1, dtype=np.uint64)
        cap = int(self._range_cap)
        total = C.c_uint64(0)
        while True:
            ids = np.zeros(cap, dtype=np.uint64); dist = np.zeros(cap, dtype=np.float32)
            check(fn(self._h, _ptr(q), 4 * self.d, b, _ptr(r), arg, flags, _ptr(words) if words.size else None, nb, _ptr(lims),
                     _ptr(ids) if cap else None, _ptr(dist) if cap else None, cap, C.byref(total)))
            if total.value <= cap:
                break
            cap = int(total.value)
        self._range_cap = int(total.value)
        return lims, ids[:total.value], dist[:total.value]

    def range_search_filtered(self, queries, radius, nprobe: int, allowed, n_bits=None, walk_order: bool = False):
        """range_search(queries, radius, nprobe) on the index WITHOUT the vec ids `allowed` leaves out (vers_ivf_range_search_filtered): every
        allowed row of the min(nprobe, k) nearest lists with distance <= radius; the index is not touched.  allowed / n_bits as
        search_filtered.  -> (lims, ids, dist) like range_search, by the same two-call protocol."""
        return self._range_filtered(lib().vers_ivf_range_search_filtered, queries, radius, nprobe, allowed, n_bits, walk_order)

    def range_search_exhaustive_filtered(self, queries, radius, allowed, metric: int = capi.METRIC_L2SQ, n_bits=None, walk_order: bool = False):
        """range_search_exhaustive over the allowed rows that are in a list now (vers_ivf_range_search_exhaustive_filtered)."""
        return self._range_filtered(lib().vers_ivf_range_search_exhaustive_filtered, queries, radius, metric, allowed, n_bits, walk_order)

    def range_search_filtered_dev(self, q_ptr: int, ldq: int, b: int, radius_ptr: int, nprobe: int, flags: int, bits_ptr: int, n_bits: int,
                                  lims_ptr: int, ids_ptr: int, dist_ptr: int, cap: int, stream: int = 0) -> int:
        """vers_ivf_range_search_filtered_dev on raw device pointers (the bitmap too); synchronous.  Returns the total: ids / distances were
        written only when it is <= cap."""
        total = C.c_uint64(0)
        check(lib().vers_ivf_range_search_filtered_dev(self._h, _vp(q_ptr), ldq, b, _vp(radius_ptr), nprobe, flags, _vp(bits_ptr) if bits_ptr else None,
                                                       n_bits, _vp(lims_ptr), _vp(ids_ptr) if ids_ptr else None, _vp(dist_ptr) if dist_ptr else None,
                                                       cap, C.byref(total), _vp(stream)))
        return int(total.value)

    def range_search_exhaustive_filtered_dev(self, q_ptr: int, ldq: int, b: int, radius_ptr: int, metric: int, flags: int, bits_ptr: int,
                                             n_bits: int, lims_ptr: int, ids_ptr: int, dist_ptr: int, cap: int, stream: int = 0) -> int:
        """vers_ivf_range_search_exhaustive_filtered_dev on raw device pointers (the bitmap too); synchronous.  Returns the total."""
        total = C.c_uint64(0)
        check(lib().vers_ivf_range_search_exhaustive_filtered_dev(self._h, _vp(q_ptr), ldq, b, _vp(radius_ptr), metric, flags,
                                                                  _vp(bits_ptr) if bits_ptr else None, n_bits, _vp(lims_ptr),
                                                                  _vp(ids_ptr) if ids_ptr else None, _vp(dist_ptr) if dist_ptr else None, cap,
                                                                  C.byref(total), _vp(stream)))
        return int(total.value)

    # -- filtered range search with a filter per query: query q of the batch uses bitmap filter_of[q] -----
    def _range_filtered_multi(self, fn, queries, radius, arg, filters, filter_of, n_bits, walk_order):
        q = np.ascontiguousarray(np.atleast_2d(queries), dtype=np.float32)
        b = q.shape[0]
        r = capi.range_radii(radius, b)
        words, nb = self._filters_words(filters, n_bits)
        fo = np.ascontiguousarray(np.broadcast_to(np.asarray(filter_of, dtype=np.uint32).reshape(-1), (b,)))
        flags = capi.RANGE_WALK_ORDER if walk_order else 0
        lims = np.zeros(b + 1, dtype=np.uint64)
        cap = int(self._range_cap)
        total = C.c_uint64(0)
        while True:
            ids = np.zeros(cap, dtype=np.uint64); dist = np.zeros(cap, dtype=np.float32)
            check(fn(self._h, _ptr(q), 4 * self.d, b, _ptr(r), arg, flags, _ptr(words) if words.size else None, words.shape[1] if words.size else 0,
                     words.shape[0], nb, _ptr(fo), _ptr(lims), _ptr(ids) if cap else None, _ptr(dist) if cap else None, cap, C.byref(total)))
            if total.value <= cap:
                break
            cap = int(total.value)
        self._range_cap = int(total.value)
        return lims, ids[:total.value], dist[:total.value]

    def range_search_filtered_multi(self, queries, radius, nprobe: int, filters, filter_of, n_bits=None, walk_order: bool = False):
        """One range batch whose queries use different filters (vers_ivf_range_search_filtered_multi; nprobe >= 1): query q's segment is
        query q's segment of range_search_filtered(queries, radius, nprobe, filters[filter_of[q]]), bit for bit.  filters / filter_of /
        n_bits as search_filtered_multi.  -> (lims, ids, dist) like range_search, by the same two-call protocol."""
        return self._range_filtered_multi(lib().vers_ivf_range_search_filtered_multi, queries, radius, nprobe, filters, filter_of, n_bits, walk_order)

    def range_search_exhaustive_filtered_multi(self, queries, radius, filters, filter_of, metric: int = capi.METRIC_L2SQ, n_bits=None,
                                               walk_order: bool = False):
        """range_search_exhaustive_filtered with a filter per query (vers_ivf_range_search_exhaustive_filtered_multi)."""
        return self._range_filtered_multi(lib().vers_ivf_range_search_exhaustive_filtered_multi, queries, radius, metric, filters, filter_of, n_bits,
                                          walk_order)

    def range_search_filtered_multi_dev(self, q_ptr: int, ldq: int, b: int, radius_ptr: int, nprobe: int, flags: int, filters_ptr: int,
                                        stride_words: int, n_filters: int, n_bits: int, filter_of_ptr: int, lims_ptr: int, ids_ptr: int, dist_ptr: int,
                                        cap: int, stream: int = 0) -> int:
        """vers_ivf_range_search_filtered_multi_dev on raw device pointers (bitmaps and filter_of too); synchronous.  Returns the total: ids /
        distances were written only when it is <= cap.  A filter_of entry at or beyond n_filters selects the empty filter."""
        total = C.c_uint64(0)
        check(lib().vers_ivf_range_search_filtered_multi_dev(self._h, _vp(q_ptr), ldq, b, _vp(radius_ptr), nprobe, flags,
                                                             _vp(filters_ptr) if filters_ptr else None, stride_words, n_filters, n_bits,
                                                             _vp(filter_of_ptr) if filter_of_ptr else None, _vp(lims_ptr),
                                                             _vp(ids_ptr) if ids_ptr else None, _vp(dist_ptr) if dist_ptr else None, cap,
                                                             C.byref(total), _vp(stream)))
        return int(total.value)

    def range_search_exhaustive_filtered_multi_dev(self, q_ptr: int, ldq: int, b: int, radius_ptr: int, metric: int, flags: int, filters_ptr: int,
                                                   stride_words: int, n_filters: int, n_bits: int, filter_of_ptr: int, lims_ptr: int, ids_ptr: int,
                                                   dist_ptr: int, cap: int, stream: int = 0) -> int:
        """vers_ivf_range_search_exhaustive_filtered_multi_dev on raw device pointers (bitmaps and filter_of too); synchronous.  Returns the total."""
        total = C.c_uint64(0)
        check(lib().vers_ivf_range_search_exhaustive_filtered_multi_dev(self._h, _vp(q_ptr), ldq, b, _vp(radius_ptr), metric, flags,
                                                                        _vp(filters_ptr) if filters_ptr else None, stride_words, n_filters, n_bits,
                                                                        _vp(filter_of_ptr) if filter_of_ptr else None, _vp(lims_ptr),
                                                                        _vp(ids_ptr) if ids_ptr else None, _vp(dist_ptr) if dist_ptr else None, cap,
                                                                        C.byref(total), _vp(stream)))
        return int(total.value)

    # -- device cache -----------------------------------------------------------------------------------
    def _upload(self):
        v = np.ascontiguousarray(self.values, dtype=np.float32)
        c = np.ascontiguousarray(self.centroids, dtype=np.float32)
        a = np.ascontiguousarray(self.assignments, dtype=np.uint64)
        check(lib().vers_ivf_upload(self._h, _ptr(v), v.shape[0], 4 * self.d, _ptr(c), c.shape[0], 4 * self.d, _ptr(a)))

    def info(self):
        n = C.c_uint64(0); k = C.c_uint64(0); m = C.c_uint64(0)
        check(lib().vers_ivf_info(self._h, C.byref(n), C.byref(k), C.byref(m)))
        return n.value, k.value, m.value

    def list_lengths(self):
        _, k, _ = self.info()
        out = np.zeros(max(k, 1), dtype=np.uint64)
        check(lib().vers_ivf_list_lengths(self._h, _ptr(out)))
        return out[:k]

    def last_scan(self):
        ms = C.c_float(0); u = C.c_uint64(0); s = C.c_uint64(0); it = C.c_uint32(0)
        check(lib().vers_ivf_last_scan(self._h, C.byref(ms), C.byref(u), C.byref(s), C.byref(it)))
        return dict(ms=ms.value, union_rows=u.value, streamed_rows=s.value, items=it.value)

    def last_coarse_ms(self):
        a = C.c_float(0); b = C.c_float(0)
        check(lib().vers_ivf_last_coarse_ms(self._h, C.byref(a), C.byref(b)))
        return dict(gemm_ms=a.value, select_ms=b.value)

    def coarse_stats(self):
        a = C.c_uint64(0); b = C.c_uint64(0)
        check(lib().vers_ivf_coarse_stats(self._h, C.byref(a), C.byref(b)))
        return dict(mfma_batches=a.value, fallback_queries=b.value)

    def prescan_stats(self):
        a = C.c_uint64(0); b = C.c_uint64(0)
        check(lib().vers_ivf_prescan_stats(self._h, C.byref(a), C.byref(b)))
        return dict(batches=a.value, fallback_queries=b.value)

    def prune_stats(self):
        """Early abandon of the batched list scan (option "pre_prune"): 64-column steps executed, steps of abandoned tiles that ran
        no math and tiles abandoned -- of the last matrix-core scan and over the handle's life."""
        last = (C.c_uint64 * 3)(); tot = (C.c_uint64 * 3)()
        check(lib().vers_ivf_prune_stats(self._h, last, tot))
        keys = ("steps_executed", "steps_skipped", "tiles_abandoned")
        return dict(last=dict(zip(keys, (int(v) for v in last))), total=dict(zip(keys, (int(v) for v in tot))))

    def head_state(self):
        """The int8 head of the stored rows (option "pre_head"): valid, bytes, columns per row, and the filter's counters of the last
        list scan and over the handle's life."""
        v = C.c_int32(0); nb = C.c_uint64(0); cols = C.c_uint32(0)
        last = (C.c_uint64 * 3)(); tot = (C.c_uint64 * 3)()
        check(lib().vers_ivf_head_state(self._h, C.byref(v), C.byref(nb), C.byref(cols), last, tot))
        keys = ("quads_tested", "quads_dead", "head_steps")
        return dict(valid=bool(v.value), bytes=int(nb.value), cols=int(cols.value), last=dict(zip(keys, (int(x) for x in last))),
                    total=dict(zip(keys, (int(x) for x in tot))))

    def ball_state(self):
        """The sub-cluster balls of the lists (option "pre_ball"): valid, bytes, lists with balls, sub-clusters, and the ball filter's
        counters of the last list scan and over the handle's life."""
        v = C.c_int32(0); nb = C.c_uint64(0); nl = C.c_uint32(0); ns = C.c_uint64(0)
        last = (C.c_uint64 * 2)(); tot = (C.c_uint64 * 2)()
        check(lib().vers_ivf_ball_state(self._h, C.byref(v), C.byref(nb), C.byref(nl), C.byref(ns), last, tot))
        keys = ("units_tested", "units_dead")
        return dict(valid=bool(v.value), bytes=int(nb.value), lists_with_balls=int(nl.value), subclusters=int(ns.value),
                    last=dict(zip(keys, (int(x) for x in last))), total=dict(zip(keys, (int(x) for x in tot))))

    def last_finish_ms(self):
        ms = C.c_float(0)
        check(lib().vers_ivf_last_finish_ms(self._h, C.byref(ms)))
        return ms.value

    def layout_bytes(self):
        r = C.c_uint64(0); s_ = C.c_uint64(0); m = C.c_uint64(0)
        check(lib().vers_ivf_layout_bytes(self._h, C.byref(r), C.byref(s_), C.byref(m)))
        return dict(rows=r.value, shadow=s_.value, rowmajor=m.value)

    def shadow_state(self):
        a = C.c_int32(0); b = C.c_uint64(0)
        check(lib().vers_ivf_shadow_state(self._h, C.byref(a), C.byref(b)))
        return dict(active=bool(a.value), bytes=int(b.value))

    def scan_times(self, reset: bool = True):
        ms = np.zeros(1024, dtype=np.float32); n = C.c_uint32(0)   # (a ring of 64 per workspace; one workspace per stream in flight)
        check(lib().vers_ivf_scan_times(self._h, _ptr(ms), 1024, C.byref(n), 1 if reset else 0))
        return ms[:n.value].copy()

    def get_list(self, cluster: int):
        ln = C.c_uint64(0)
        check(lib().vers_ivf_get_list(self._h, cluster, None, 0, None, 0, C.byref(ln)))
        rows = np.zeros((ln.value, self.d), dtype=np.float32); ids = np.zeros(ln.value, dtype=np.uint64)
        check(lib().vers_ivf_get_list(self._h, cluster, _ptr(rows), 4 * self.d, _ptr(ids), ln.value, C.byref(ln)))
        return rows, ids

    def get_centroids(self):
        _, k, _ = self.info()
        c = np.zeros((k, self.d), dtype=np.float32)
        check(lib().vers_ivf_get_centroids(self._h, _ptr(c), 4 * self.d))
        return c

    # device-resident entry points (bench.py): torch tensors are passed as raw pointers
    def build_dev(self, rows_ptr: int, n: int, num_clusters: int, num_attempts: int, max_iterations: int, init_indices,
                  want_fields: bool = False):
        """build_index on rows already in HBM.  want_fields: also bring `centroids` and `assignments` (the reference's
        fields, ivfflat.rs:11-13) back to the host -- what upload_dev / save_index need."""
        init = np.ascontiguousarray(np.asarray(init_indices).reshape(-1), dtype=np.uint64)
        cost = C.c_float(0); kept = C.c_int32(0)
        iters = np.zeros(max(num_attempts, 1), dtype=np.uint64)
        ld = (self.d + 3) // 4 * 4
        cent = np.zeros((num_clusters, self.d), dtype=np.float32) if want_fields else None
        asg = np.zeros(max(n, 1), dtype=np.uint64) if want_fields else None
        check(lib().vers_ivf_build_dev(self._h, _vp(rows_ptr), n, ld, num_clusters, num_attempts, max_iterations, _ptr(init),
                                       _ptr(cent) if want_fields else None, 4 * self.d if want_fields else 0,
                                       _ptr(asg) if want_fields else None, C.byref(cost), C.byref(kept), _ptr(iters)))
        self.num_centroids = num_clusters
        self.cost = np.float32(cost.value); self.iterations = iters[:num_attempts]
        if want_fields and kept.value:
            self.centroids, self.assignments = cent, asg[:n]
        return bool(kept.value)

    def upload_dev(self, rows_ptr: int, n: int, ld: int, centroids_ptr: int, k: int, c_ld: int, assignments_ptr: int):
        """Device cache from DEVICE-resident fields (vers_ivf_upload_dev): rows [n][ld] f32, centroids [k][c_ld] f32,
        assignments [n] u64.  With set_shard only the lists LPT deals to this rank are stored."""
        check(lib().vers_ivf_upload_dev(self._h, _vp(rows_ptr), n, ld, _vp(centroids_ptr), k, c_ld, _vp(assignments_ptr)))
        self.num_centroids = k

    # Streamed rebuild of the device cache (vers_ivf_upload_begin / _chunk / _end): the reference's load_index -> search
    # sequence (base.rs:45-58, utils.rs:140-148) for an index no single GPU holds -- fields arrive in chunks, a sharded
    # handle keeps only its own lists, nothing of n_total rows is ever allocated.
    def upload_begin(self, centroids, list_lengths, n_total: int):
        c = np.ascontiguousarray(centroids, dtype=np.float32).reshape(-1, self.d)
        ll = np.ascontiguousarray(list_lengths, dtype=np.uint64)
        assert ll.shape[0] == c.shape[0]
        check(lib().vers_ivf_upload_begin(self._h, _ptr(c), c.shape[0], 4 * self.d, _ptr(ll), n_total))
        self.num_centroids = c.shape[0]

    def upload_chunk(self, rows, assignments, first_vec_id: int):
        v = np.ascontiguousarray(rows, dtype=np.float32).reshape(-1, self.d)
        a = np.ascontiguousarray(assignments, dtype=np.uint64)
        assert a.shape[0] == v.shape[0]
        check(lib().vers_ivf_upload_chunk(self._h, _ptr(v), 4 * self.d, _ptr(a), first_vec_id, v.shape[0]))

    def upload_chunk_dev(self, rows_ptr: int, ld: int, assignments_ptr: int, first_vec_id: int, n: int):
        check(lib().vers_ivf_upload_chunk_dev(self._h, _vp(rows_ptr), ld, _vp(assignments_ptr), first_vec_id, n))

    def upload_end(self):
        check(lib().vers_ivf_upload_end(self._h))

    def search_dev(self, q_ptr: int, ldq: int, b: int, top_k: int, nprobe: int, ids_ptr: int, dist_ptr: int, cnt_ptr: int,
                   stream: int = 0):
        check(lib().vers_ivf_search_dev(self._h, _vp(q_ptr), ldq, b, top_k, nprobe, _vp(ids_ptr), _vp(dist_ptr), _vp(cnt_ptr),
                                        _vp(stream)))

    def search_exhaustive_dev(self, q_ptr: int, ldq: int, b: int, top_k: int, metric: int, ids_ptr: int, dist_ptr: int,
                              cnt_ptr: int, stream: int = 0):
        check(lib().vers_ivf_search_exhaustive_dev(self._h, _vp(q_ptr), ldq, b, top_k, metric, _vp(ids_ptr), _vp(dist_ptr),
                                                   _vp(cnt_ptr), _vp(stream)))

    # -- sharding by cluster, one process per GPU -----------------------------------------------------------
    def set_shard(self, rank: int, world: int):
        check(lib().vers_ivf_set_shard(self._h, rank, world))

    def build_sharded_dev(self, rows_ptr: int, n_local: int, ld: int, row_begin: int, n_total: int, num_clusters: int,
                          num_attempts: int, max_iterations: int, init_indices, comm, want_assignments: bool = False):
        """build_index over a ROW-SHARDED corpus (vers_ivf_build_sharded_dev): this process holds rows
        [row_begin, row_begin + n_local) of n_total in HBM; `comm` is a vers_amd.dist.TorchComm (RCCL on the GPUs).
        Bit-identical to the single-process build; afterwards the handle holds the lists LPT deals to comm.rank."""
        init = np.ascontiguousarray(np.asarray(init_indices).reshape(-1), dtype=np.uint64)
        cost = C.c_float(0); kept = C.c_int32(0)
        iters = np.zeros(max(num_attempts, 1), dtype=np.uint64)
        asg = np.zeros(max(n_local, 1), dtype=np.uint64) if want_assignments else None
        check(lib().vers_ivf_build_sharded_dev(self._h, _vp(rows_ptr), n_local, ld, row_begin, n_total, num_clusters, num_attempts,
                                               max_iterations, _ptr(init), comm.ptr(), _ptr(asg) if want_assignments else None,
                                               C.byref(cost), C.byref(kept), _ptr(iters)))
        self.num_centroids = num_clusters
        self.cost = np.float32(cost.value); self.iterations = iters[:num_attempts]
        if want_assignments:
            self.local_assignments = asg[:n_local]
        return bool(kept.value)

    def search_sharded_dev(self, gather_ptr, q_ptr: int, ldq: int, b: int, top_k: int, nprobe: int, ids_ptr: int, dist_ptr: int,
                           cnt_ptr: int, stream: int = 0):
        """search_approximate over lists sharded by cluster, end to end on `stream` (vers_ivf_search_sharded_dev): partial
        search -> ONE all-gather (gather_ptr: vers_amd.rccl.RcclComm.gather_ptr() = ncclAllGather on the stream, or
        dist.TorchGather.ptr()) -> merge.  No host synchronisation."""
        check(lib().vers_ivf_search_sharded_dev(self._h, gather_ptr, _vp(q_ptr), ldq, b, top_k, nprobe, _vp(ids_ptr), _vp(dist_ptr),
                                                _vp(cnt_ptr), _vp(stream)))

    def search_exhaustive_sharded_dev(self, gather_ptr, q_ptr: int, ldq: int, b: int, top_k: int, metric: int, ids_ptr: int,
                                      dist_ptr: int, cnt_ptr: int, stream: int = 0):
        check(lib().vers_ivf_search_exhaustive_sharded_dev(self._h, gather_ptr, _vp(q_ptr), ldq, b, top_k, metric, _vp(ids_ptr),
                                                           _vp(dist_ptr), _vp(cnt_ptr), _vp(stream)))

    def owners(self):
        _, k, _ = self.info()
        o = np.zeros(max(k, 1), dtype=np.uint8)
        check(lib().vers_ivf_owners(self._h, _ptr(o)))
        return o[:k]

    def coarse_ahead_dev(self, q_ptr: int, ldq: int, b: int, nprobe: int, stream: int = 0):
        """Stage and rank the NEXT batch's queries on the handle's side stream while the current batch is scanned
        (vers_ivf_coarse_ahead_dev); the following search of the same query block picks the result up."""
        check(lib().vers_ivf_coarse_ahead_dev(self._h, _vp(q_ptr), ldq, b, nprobe, _vp(stream)))

    def search_exhaustive_partial_dev(self, q_ptr: int, ldq: int, b: int, top_k: int, metric: int, keys_ptr: int, ids_ptr: int,
                                      stream: int = 0):
        """Brute force over this rank's rows as (key, vec_id) pairs for merge_partials_dev (rows shard with the lists)."""
        check(lib().vers_ivf_search_exhaustive_partial_dev(self._h, _vp(q_ptr), ldq, b, top_k, metric, _vp(keys_ptr), _vp(ids_ptr),
                                                           _vp(stream)))

    def search_partial_dev(self, q_ptr: int, ldq: int, b: int, top_k: int, nprobe: int, keys_ptr: int, ids_ptr: int,
                           stream: int = 0):
        check(lib().vers_ivf_search_partial_dev(self._h, _vp(q_ptr), ldq, b, top_k, nprobe, _vp(keys_ptr), _vp(ids_ptr),
                                                _vp(stream)))

    @staticmethod
    def merge_partials_dev(keys_ptr: int, ids_ptr: int, rank_stride: int, world: int, b: int, top_k: int, nprobe: int,
                           out_ids_ptr: int, out_dist_ptr: int, out_cnt_ptr: int, stream: int = 0):
        check(lib().vers_topk_merge_dev(_vp(keys_ptr), _vp(ids_ptr), rank_stride, world, b, top_k, nprobe, _vp(out_ids_ptr),
                                        _vp(out_dist_ptr), _vp(out_cnt_ptr), _vp(stream)))

    # -- range search on handles sharded by cluster ------------------------------------------------------------
    def range_search_partial_dev(self, q_ptr: int, ldq: int, b: int, radius_ptr: int, nprobe: int, flags: int, lims_ptr: int, keys_ptr: int,
                                 ids_ptr: int, cap: int, stream: int = 0, exhaustive_metric=None) -> int:
        """This rank's part of a range search as CSR of (key, vec id) pairs for merge_range_partials_dev
        (vers_ivf_range_search_partial_dev; exhaustive_metric given: vers_ivf_range_search_exhaustive_partial_dev over this rank's rows,
        `nprobe` unused).  Synchronous.  Returns the LOCAL total: keys / ids were written only when it is <= cap."""
        total = C.c_uint64(0)
        if exhaustive_metric is None:
            check(lib().vers_ivf_range_search_partial_dev(self._h, _vp(q_ptr), ldq, b, _vp(radius_ptr), nprobe, flags, _vp(lims_ptr),
                                                          _vp(keys_ptr) if keys_ptr else None, _vp(ids_ptr) if ids_ptr else None, cap,
                                                          C.byref(total), _vp(stream)))
        else:
            check(lib().vers_ivf_range_search_exhaustive_partial_dev(self._h, _vp(q_ptr), ldq, b, _vp(radius_ptr), exhaustive_metric, flags,
                                                                     _vp(lims_ptr), _vp(keys_ptr) if keys_ptr else None,
                                                                     _vp(ids_ptr) if ids_ptr else None, cap, C.byref(total), _vp(stream)))
        return int(total.value)

    @staticmethod
    def merge_range_partials_dev(keys_ptr: int, ids_ptr: int, rank_stride: int, rank_lims_ptr: int, world: int, b: int, flags: int,
                                 out_lims_ptr: int, out_ids_ptr: int, out_dist_ptr: int, stream: int = 0):
        """vers_range_merge_dev: `world` partials (rank r's arrays at r * rank_stride elements, its limits at rank_lims[r]) -> the CSR result;
        queued on `stream`, not synchronised."""
        check(lib().vers_range_merge_dev(_vp(keys_ptr) if keys_ptr else None, _vp(ids_ptr) if ids_ptr else None, rank_stride, _vp(rank_lims_ptr),
                                         world, b, flags, _vp(out_lims_ptr), _vp(out_ids_ptr) if out_ids_ptr else None,
                                         _vp(out_dist_ptr) if out_dist_ptr else None, _vp(stream)))

    def range_search_sharded_dev(self, comm, q_ptr: int, ldq: int, b: int, radius_ptr: int, nprobe: int, flags: int, lims_ptr: int,
                                 ids_ptr: int, dist_ptr: int, cap: int, stream: int = 0) -> int:
        """Range search over lists sharded by cluster, end to end (vers_ivf_range_search_sharded_dev): every rank calls with the same
        arguments and the same cap; comm: the vers_amd.dist.TorchComm of the sharded handle (None on an unsharded one).  Returns the
        GLOBAL total: ids / distances were written only when it is <= cap."""
        total = C.c_uint64(0)
        check(lib().vers_ivf_range_search_sharded_dev(self._h, comm.ptr() if comm is not None else None, _vp(q_ptr), ldq, b, _vp(radius_ptr),
                                                      nprobe, flags, _vp(lims_ptr), _vp(ids_ptr) if ids_ptr else None,
                                                      _vp(dist_ptr) if dist_ptr else None, cap, C.byref(total), _vp(stream)))
        return int(total.value)

    def range_search_exhaustive_sharded_dev(self, comm, q_ptr: int, ldq: int, b: int, radius_ptr: int, metric: int, flags: int, lims_ptr: int,
                                            ids_ptr: int, dist_ptr: int, cap: int, stream: int = 0) -> int:
        """The exhaustive twin of range_search_sharded_dev (vers_ivf_range_search_exhaustive_sharded_dev); default order only."""
        total = C.c_uint64(0)
        check(lib().vers_ivf_range_search_exhaustive_sharded_dev(self._h, comm.ptr() if comm is not None else None, _vp(q_ptr), ldq, b,
                                                                 _vp(radius_ptr), metric, flags, _vp(lims_ptr),
                                                                 _vp(ids_ptr) if ids_ptr else None, _vp(dist_ptr) if dist_ptr else None, cap,
                                                                 C.byref(total), _vp(stream)))
        return int(total.value)

    # -- filtered search on handles sharded by cluster (vers_hip.h: partials, vers_adaptive_t, the _filtered_sharded_dev calls) -----------
    # filt = (filters_ptr, stride_words, n_filters, n_bits, filter_of_ptr): the _multi form; filter_of_ptr 0 = one bitmap for the batch.
    # adaptive = None (plain depth) or (nprobe_min, min_allowed, allowed_len_ptr, out_nprobe_ptr) with `nprobe` the call's nprobe_max.
    @staticmethod
    def _filt(filt):
        fp, stride, nf, n_bits, fo = filt
        return (_vp(fp) if fp else None, stride, nf, n_bits, _vp(fo) if fo else None)

    @staticmethod
    def _adaptive(adaptive):
        if adaptive is None:
            return None, None
        nprobe_min, min_allowed, alen_ptr, np_ptr = adaptive
        ad = capi.Adaptive(nprobe_min, min_allowed, alen_ptr if alen_ptr else None, np_ptr if np_ptr else None)
        return ad, C.byref(ad)

    def filter_allowed_len_dev(self, filters_ptr: int, stride_words: int, n_filters: int, n_bits: int, out_len_ptr: int, stream: int = 0):
        """u32 [n_filters][k] on the device: the rows of every list THIS handle stores that each bitmap allows, 0 for lists of other ranks
        (vers_ivf_filter_allowed_len_dev); the ranks' arrays add up to the global counts an adaptive partial takes."""
        check(lib().vers_ivf_filter_allowed_len_dev(self._h, _vp(filters_ptr) if filters_ptr else None, stride_words, n_filters, n_bits,
                                                    _vp(out_len_ptr), _vp(stream)))

    def search_filtered_partial_dev(self, q_ptr: int, ldq: int, b: int, top_k: int, nprobe: int, filt, keys_ptr: int, ids_ptr: int,
                                    adaptive=None, stream: int = 0):
        """This rank's part of a probed filtered search as (key, vec id) pairs for merge_partials_dev (vers_ivf_search_filtered_partial_dev)."""
        ad, adp = self._adaptive(adaptive)
        check(lib().vers_ivf_search_filtered_partial_dev(self._h, _vp(q_ptr), ldq, b, top_k, nprobe, *self._filt(filt), adp, _vp(keys_ptr), _vp(ids_ptr),
                                                         _vp(stream)))

    def search_exhaustive_filtered_partial_dev(self, q_ptr: int, ldq: int, b: int, top_k: int, metric: int, filt, keys_ptr: int, ids_ptr: int,
                                               stream: int = 0):
        check(lib().vers_ivf_search_exhaustive_filtered_partial_dev(self._h, _vp(q_ptr), ldq, b, top_k, metric, *self._filt(filt), _vp(keys_ptr),
                                                                    _vp(ids_ptr), _vp(stream)))

    def search_filtered_sharded_dev(self, gather_ptr, q_ptr: int, ldq: int, b: int, top_k: int, nprobe: int, filt, ids_ptr: int, dist_ptr: int,
                                    cnt_ptr: int, adaptive=None, stream: int = 0):
        """Probed filtered search over lists sharded by cluster, end to end on `stream` (vers_ivf_search_filtered_sharded_dev); gather_ptr as
        search_sharded_dev's (None on an unsharded handle).  adaptive: two gathers, allowed_len_ptr must be 0."""
        ad, adp = self._adaptive(adaptive)
        check(lib().vers_ivf_search_filtered_sharded_dev(self._h, gather_ptr, _vp(q_ptr), ldq, b, top_k, nprobe, *self._filt(filt), adp, _vp(ids_ptr),
                                                         _vp(dist_ptr), _vp(cnt_ptr), _vp(stream)))

    def search_exhaustive_filtered_sharded_dev(self, gather_ptr, q_ptr: int, ldq: int, b: int, top_k: int, metric: int, filt, ids_ptr: int,
                                               dist_ptr: int, cnt_ptr: int, stream: int = 0):
        check(lib().vers_ivf_search_exhaustive_filtered_sharded_dev(self._h, gather_ptr, _vp(q_ptr), ldq, b, top_k, metric, *self._filt(filt),
                                                                    _vp(ids_ptr), _vp(dist_ptr), _vp(cnt_ptr), _vp(stream)))

    def range_search_filtered_partial_dev(self, q_ptr: int, ldq: int, b: int, radius_ptr: int, nprobe: int, flags: int, filt, lims_ptr: int,
                                          keys_ptr: int, ids_ptr: int, cap: int, stream: int = 0, exhaustive_metric=None) -> int:
        """range_search_partial_dev behind a filter (vers_ivf_range_search_filtered_partial_dev / _exhaustive_filtered_partial_dev).  Returns
        the LOCAL total: keys / ids were written only when it is <= cap."""
        total = C.c_uint64(0)
        fn = lib().vers_ivf_range_search_filtered_partial_dev if exhaustive_metric is None else lib().vers_ivf_range_search_exhaustive_filtered_partial_dev
        check(fn(self._h, _vp(q_ptr), ldq, b, _vp(radius_ptr), nprobe if exhaustive_metric is None else exhaustive_metric, flags, *self._filt(filt),
                 _vp(lims_ptr), _vp(keys_ptr) if keys_ptr else None, _vp(ids_ptr) if ids_ptr else None, cap, C.byref(total), _vp(stream)))
        return int(total.value)

    def range_search_filtered_sharded_dev(self, comm, q_ptr: int, ldq: int, b: int, radius_ptr: int, nprobe: int, flags: int, filt, lims_ptr: int,
                                          ids_ptr: int, dist_ptr: int, cap: int, stream: int = 0, exhaustive_metric=None) -> int:
        """range_search_sharded_dev behind a filter (vers_ivf_range_search_filtered_sharded_dev / _exhaustive_filtered_sharded_dev): every rank
        calls with the same arguments, bitmaps and cap.  Returns the GLOBAL total."""
        total = C.c_uint64(0)
        fn = lib().vers_ivf_range_search_filtered_sharded_dev if exhaustive_metric is None else lib().vers_ivf_range_search_exhaustive_filtered_sharded_dev
        check(fn(self._h, comm.ptr() if comm is not None else None, _vp(q_ptr), ldq, b, _vp(radius_ptr),
                 nprobe if exhaustive_metric is None else exhaustive_metric, flags, *self._filt(filt), _vp(lims_ptr), _vp(ids_ptr) if ids_ptr else None,
                 _vp(dist_ptr) if dist_ptr else None, cap, C.byref(total), _vp(stream)))
        return int(total.value)

    def range_search_exhaustive_filtered_partial_dev(self, q_ptr: int, ldq: int, b: int, radius_ptr: int, metric: int, flags: int, filt, lims_ptr: int,
                                                     keys_ptr: int, ids_ptr: int, cap: int, stream: int = 0) -> int:
        return self.range_search_filtered_partial_dev(q_ptr, ldq, b, radius_ptr, 0, flags, filt, lims_ptr, keys_ptr, ids_ptr, cap, stream, exhaustive_metric=metric)

    def range_search_exhaustive_filtered_sharded_dev(self, comm, q_ptr: int, ldq: int, b: int, radius_ptr: int, metric: int, flags: int, filt, lims_ptr: int,
                                                     ids_ptr: int, dist_ptr: int, cap: int, stream: int = 0) -> int:
        return self.range_search_filtered_sharded_dev(comm, q_ptr, ldq, b, radius_ptr, 0, flags, filt, lims_ptr, ids_ptr, dist_ptr, cap, stream,
                                                      exhaustive_metric=metric)

    # -- prepared filters (vers_hip.h): masks kept across calls, refreshed when rows move ------------------------------------------------
    def prepare_filter(self, filters, n_bits: int) -> "PreparedFilter":
        """A PreparedFilter from host bitmaps: u64 [n_filters][stride_words] (one row per bitmap; a 1-d array is one bitmap), copied by the
        library (vers_ivf_filter_prepare)."""
        f = np.ascontiguousarray(np.atleast_2d(np.asarray(filters, dtype=np.uint64)))
        out = _vp(None)
        check(lib().vers_ivf_filter_prepare(self._h, _ptr(f) if f.size else None, f.shape[1], f.shape[0], n_bits, C.byref(out)))
        return PreparedFilter(self, out.value)

    def prepare_filter_dev(self, filters_ptr: int, stride_words: int, n_filters: int, n_bits: int) -> "PreparedFilter":
        """The same from bitmaps on the device (vers_ivf_filter_prepare_dev)."""
        out = _vp(None)
        check(lib().vers_ivf_filter_prepare_dev(self._h, _vp(filters_ptr) if filters_ptr else None, stride_words, n_filters, n_bits, C.byref(out)))
        return PreparedFilter(self, out.value)

    @staticmethod
    def _pf(pf):
        return _vp(pf.ptr if isinstance(pf, PreparedFilter) else pf)

    def search_prepared_dev(self, q_ptr: int, ldq: int, b: int, top_k: int, nprobe: int, pf, filter_of_ptr: int, ids_ptr: int, dist_ptr: int,
                            cnt_ptr: int, adaptive=None, stream: int = 0):
        """search_filtered_sharded_dev (no exchange) with a PreparedFilter in the bitmaps' place (vers_ivf_search_prepared_dev)."""
        ad, adp = self._adaptive(adaptive)
        check(lib().vers_ivf_search_prepared_dev(self._h, _vp(q_ptr), ldq, b, top_k, nprobe, self._pf(pf), _vp(filter_of_ptr) if filter_of_ptr else None, adp,
                                                 _vp(ids_ptr), _vp(dist_ptr), _vp(cnt_ptr), _vp(stream)))

    def search_exhaustive_prepared_dev(self, q_ptr: int, ldq: int, b: int, top_k: int, metric: int, pf, filter_of_ptr: int, ids_ptr: int,
                                       dist_ptr: int, cnt_ptr: int, stream: int = 0):
        check(lib().vers_ivf_search_exhaustive_prepared_dev(self._h, _vp(q_ptr), ldq, b, top_k, metric, self._pf(pf),
                                                            _vp(filter_of_ptr) if filter_of_ptr else None, _vp(ids_ptr), _vp(dist_ptr), _vp(cnt_ptr), _vp(stream)))

    def range_search_prepared_dev(self, q_ptr: int, ldq: int, b: int, radius_ptr: int, nprobe: int, flags: int, pf, filter_of_ptr: int,
                                  lims_ptr: int, ids_ptr: int, dist_ptr: int, cap: int, stream: int = 0, exhaustive_metric=None) -> int:
        """range_search_filtered_sharded_dev (no exchange) with a PreparedFilter (vers_ivf_range_search_prepared_dev / _exhaustive_prepared_dev).
        Returns the total."""
        total = C.c_uint64(0)
        fn = lib().vers_ivf_range_search_prepared_dev if exhaustive_metric is None else lib().vers_ivf_range_search_exhaustive_prepared_dev
        check(fn(self._h, _vp(q_ptr), ldq, b, _vp(radius_ptr), nprobe if exhaustive_metric is None else exhaustive_metric, flags, self._pf(pf),
                 _vp(filter_of_ptr) if filter_of_ptr else None, _vp(lims_ptr), _vp(ids_ptr) if ids_ptr else None, _vp(dist_ptr) if dist_ptr else None, cap,
                 C.byref(total), _vp(stream)))
        return int(total.value)

    def range_search_exhaustive_prepared_dev(self, q_ptr: int, ldq: int, b: int, radius_ptr: int, metric: int, flags: int, pf, filter_of_ptr: int,
                                             lims_ptr: int, ids_ptr: int, dist_ptr: int, cap: int, stream: int = 0) -> int:
        return self.range_search_prepared_dev(q_ptr, ldq, b, radius_ptr, 0, flags, pf, filter_of_ptr, lims_ptr, ids_ptr, dist_ptr, cap, stream,
                                              exhaustive_metric=metric)

    def poll(self, stream: int = 0):
        check(lib().vers_ivf_poll(self._h, _vp(stream)))

    # -- Index::save_index / load_index (base.rs:31-58) ---------------------------------------------
    def save_index(self, file_path: str):
        write_index_file(file_path, self.num_centroids, self.values, self.centroids, self.assignments, self.ids)

    @classmethod
    def load_index(cls, file_path: str, d: int, device: int = 0, metric: int = capi.METRIC_L2SQ) -> "IVFFlatIndex":
        """`d` plays the role of the const generic N of IVFFlatIndex<N>.  (The file has no metric field -- the
        reference has no metric switch -- so a cosine-distance index is reloaded with metric=METRIC_COSDIST.)"""
        f = read_index_file(file_path, d)
        self = cls(d, device, metric)
        self.num_centroids, self.values, self.centroids = f["num_centroids"], f["values"], f["centroids"]
        self.assignments, self.ids = f["assignments"], f["ids"]
        self._upload()
        # vers_ivf_upload implies ids[c] = every position with assignments == c; positions missing from the file's lists were
        # removed before it was saved and leave the device cache again (none in a file the reference wrote)
        in_list = np.zeros(len(self.assignments), dtype=bool)
        for lst in self.ids:
            in_list[np.asarray(lst, dtype=np.int64)] = True
        gone = np.flatnonzero(~in_list).astype(np.uint64)
        if gone.size and len(self.centroids):
            removed = C.c_uint64(0)
            check(lib().vers_ivf_remove_batch(self._h, _ptr(gone), gone.size, C.byref(removed)))
            assert removed.value == gone.size, (removed.value, gone.size)
        return self


class PreparedFilter:
    """A vers_filter_t of one IVFFlatIndex: bitmaps the library copied and the masks it keeps for them.  Close it before (or let it go with)
    the index; the index frees the objects still alive when it is closed."""
    INFO = ("n_filters", "n_bits", "device_bytes", "builds", "tail_refreshes", "hits", "fresh", "reserved")

    def __init__(self, index: IVFFlatIndex, ptr: int):
        self.index, self.ptr = index, ptr

    def refresh(self, stream: int = 0):
        """Brings the masks up to date now, on `stream`, so that the next search finds them fresh (vers_ivf_filter_refresh)."""
        check(lib().vers_ivf_filter_refresh(self.index._h, _vp(self.ptr), _vp(stream)))

    def info(self) -> dict:
        out = np.zeros(8, dtype=np.uint64)
        check(lib().vers_ivf_filter_info(self.index._h, _vp(self.ptr), _ptr(out)))
        return dict(zip(self.INFO, map(int, out)))

    def close(self):
        if self.ptr and self.index._h:
            check(lib().vers_ivf_filter_destroy(self.index._h, _vp(self.ptr)))
        self.ptr = 0


# The index file of Index::save_index (base.rs:31-43): bincode 1.3.3 with default options over the five fields of
# IVFFlatIndex<N> in declaration order (ivfflat.rs:9-15) -- little endian, fixed-width integers, usize and every
# length as u64, a struct is its fields back to back without tags or names, Vec<T> = u64 length + items,
# Vector<N>([f32; N]) through serde_arrays = N raw f32 WITHOUT a length (a fixed-size array is a tuple to serde), and
# no padding: the 256-byte alignment of Vector<N> exists in memory only.  (bincode / serde_arrays sources are not
# vendored in the reference: layout restated from their published format -- "parity unpinned" for this row, see
# DESIGN.md; tests/test_index_file.py pins these rules byte by byte and against the C++ host mirror.)
def write_index_file(file_path, num_centroids, values, centroids, assignments, ids):
    with open(file_path, "wb") as f:
        f.write(struct.pack("<Q", int(num_centroids)))
        for mat in (values, centroids):
            m = np.ascontiguousarray(mat, dtype="<f4")
            f.write(struct.pack("<Q", m.shape[0])); f.write(m.tobytes())
        a = np.ascontiguousarray(assignments, dtype="<u8")
        f.write(struct.pack("<Q", a.size)); f.write(a.tobytes())
        f.write(struct.pack("<Q", len(ids)))
        for lst in ids:
            l = np.asarray(lst, dtype="<u8")
            f.write(struct.pack("<Q", l.size)); f.write(l.tobytes())


def read_index_file(file_path, d: int) -> dict:
    """The five fields; raises IOError("Deserialization error: ...") like base.rs:52-57 on a short or oversized file."""
    with open(file_path, "rb") as f:
        buf = f.read()
    off = 0

    def u64():
        nonlocal off
        if off + 8 > len(buf):
            raise IOError("Deserialization error: unexpected end of file")
        (v,) = struct.unpack_from("<Q", buf, off); off += 8
        return v

    def take(dtype, count):
        nonlocal off
        nbytes = count * np.dtype(dtype).itemsize
        if off + nbytes > len(buf):
            raise IOError("Deserialization error: unexpected end of file")
        a = np.frombuffer(buf, dtype=dtype, count=count, offset=off).copy(); off += nbytes
        return a

    out = {"num_centroids": u64()}
    out["values"] = take("<f4", u64() * d).reshape(-1, d)
    out["centroids"] = take("<f4", u64() * d).reshape(-1, d)
    out["assignments"] = take("<u8", u64())
    out["ids"] = [list(map(int, take("<u8", u64()))) for _ in range(u64())]
    return out
