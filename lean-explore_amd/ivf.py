"""IVFFlatIndex — the IVF-flat index the reference ships and searches
(``faiss.IndexIVFFlat(IndexFlatIP(d), d, nlist, METRIC_INNER_PRODUCT)`` with ``index.nprobe = 64``, reference
src/lean_explore/extract/index.py:95-116, search/engine.py:247-250), served by libleansearch's ``ls_ivf``
(include/leansearch_ivf.h): the probed lists of a query are the top ``nprobe`` rows of the exact search over the
centroids, and the result is the exact subset search over the rows of those lists - scores bit-identical to the flat
scan's, ties by original row. ``nprobe >= nlist`` equals :class:`FlatIPIndex`. Opt-in; a subset-search result by
definition, not a bit-for-bit copy of faiss (which leaves tie and summation order open).

All arithmetic of a search happens in the library; this class owns the handle, buffers rows until the first search (as
``FlatIPIndex`` does) and runs the Lloyd iterations of ``train`` (assignment by the library's exact k = 1 search, mean
update on the host). ``build_on_device=True`` / ``train(on_device=True)`` run both steps as one kernel each on rows kept
in HBM (include/leansearch_ivf_build.h) and compute the lists of ``add`` with one launch per upload step: the same
centroids and lists, bit for bit. ``add`` on an index that was already searched merges the new rows into its lists on
the GPU (include/leansearch_ivf_add.h): the result is the index built from all rows at once. ``remove_ids`` drops rows
the same way (include/leansearch_ivf_remove.h): the lists are compacted on the GPU, the survivors renumbered densely, and
the result is the index built from the survivors - so an update is ``remove_ids(stale)`` followed by ``add(fresh)``.

``metric="l2"`` (include/leansearch_ivf_l2.h; faiss's ``IndexIVFFlat(IndexFlatL2(d), d, nlist)``): the probed lists are the
``nprobe`` nearest centroids under the exact squared distance, the result is the flat L2 subset search over their rows -
distances bit-identical to :class:`FlatL2Index`, smallest first, ties by original row, padding ``(+FLT_MAX, -1)``.
fp32 or fp16 rows; everything above (``train``, the device build, ``add``, ``remove_ids``, subsets, ``range_search``)
works under it.
"""

from __future__ import annotations

import ctypes
from typing import Any

import numpy as np

from . import native
from .index import _DTYPE_NAMES, _METRIC_NAMES, FlatIPIndex, FlatL2Index, _dtype_code, _metric_code, switch_refusal

MAX_POINTS_PER_CENTROID = 256  # training rows sampled per centroid at most (faiss's ClusteringParameters default)
MAX_NLIST_ON_DEVICE = 8191  # the device build's bound (leansearch_ivf_build.h: nlist < 8192)


class _Trainer:
    """``ls_ivf_trainer``: the training rows in HBM, one assignment kernel and one means kernel per call."""

    def __init__(self, x: np.ndarray, nlist: int, device: int, l2: bool = False):
        self.n, self.d, self.nlist = x.shape[0], x.shape[1], int(nlist)
        self._h = ctypes.c_void_p()
        lib = native.load()
        create = lib.ls_ivf_trainer_create_l2 if l2 else lib.ls_ivf_trainer_create  # (l2: assign under L2)
        native.check(create(ctypes.byref(self._h), native.addr(x), self.n, self.d, self.nlist, int(device)))

    def assign(self, cent: np.ndarray) -> np.ndarray:
        """List of every training row (int64 [n]) under the library's exact k = 1 search over ``cent``."""
        cent = np.ascontiguousarray(cent, dtype=np.float32)
        a = np.zeros(self.n, dtype=np.int32)
        native.check(native.load().ls_ivf_trainer_assign(self._h, native.addr(cent), native.addr(a), None))
        return a.astype(np.int64)

    def means(self) -> np.ndarray:
        """float64 [nlist, d] of the last ``assign``: the mean of every list's rows (added in ascending row order); a
        list without rows keeps its centroid."""
        out = np.zeros((self.nlist, self.d), dtype=np.float64)
        native.check(native.load().ls_ivf_trainer_means(self._h, native.addr(out)))
        return out

    def last_kernel_ms(self) -> tuple[float, float]:
        """(assignment kernel ms, means kernel ms) of the most recent of each."""
        a, m = ctypes.c_float(), ctypes.c_float()
        native.check(native.load().ls_ivf_trainer_last_kernel_ms(self._h, ctypes.byref(a), ctypes.byref(m)))
        return a.value, m.value

    def close(self) -> None:
        if self._h is not None and self._h.value:
            native.load().ls_ivf_trainer_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class IVFFlatIndex:
    supports_fused_normalize = True  # search(..., normalize=True) fuses faiss.normalize_L2 (both stages use that query)

    def __init__(self, d: int, nlist: int, dtype: Any = "f32", device: int = 0, build_on_device: bool = False,
                 small_batch: bool = False, metric: Any = "ip"):
        """``small_batch=True`` (fp32 rows, off by default; ``ls_ivf_set_small_batch``): groups of 2..16 queries of a
        search share one centroid search, one pass over the union of the lists they probe and one selection launch -
        the same results, bit for bit. ``metric="l2"``: squared-distance search (fp32 or fp16 rows, no small batches;
        both refused with ValueError before a device is touched)."""
        if d <= 0:
            raise ValueError("d must be positive")
        if int(nlist) < 1:
            raise ValueError("nlist must be at least 1")
        if build_on_device and int(nlist) > MAX_NLIST_ON_DEVICE:
            raise ValueError(f"build_on_device serves nlist < {MAX_NLIST_ON_DEVICE + 1}, got {int(nlist)}")
        self.build_on_device = bool(build_on_device)
        self.d, self.nlist = int(d), int(nlist)
        self._dtype = _dtype_code(dtype)
        # ("sq8": the rows are stored as an sq8 index trained on them - the step a flat sq8 index of the same rows has)
        if self._dtype not in _DTYPE_NAMES:
            raise ValueError(f"unsupported storage dtype {dtype!r} (use 'f32', 'f16', 'sq8' or 'bf16')")
        self._metric = _metric_code(metric)
        if self._metric == native.LS_METRIC_L2 and self._dtype == native.LS_DTYPE_SQ8:
            raise ValueError("metric='l2' needs dtype='f32' or 'f16' (sq8 codes serve the inner product only)")
        if self._metric == native.LS_METRIC_L2 and self._dtype == native.LS_DTYPE_BF16:
            raise ValueError("metric='l2' needs dtype='f32' or 'f16' (bf16 rows serve the inner product only)")
        self.device = int(device)
        self.nprobe = 1  # faiss's default
        self.is_trained = False
        self._centroids: np.ndarray | None = None
        self._quantizer: FlatIPIndex | None = None
        self._pending: list[np.ndarray] = []
        self._assign: list[np.ndarray] | None = None  # explicit lists of the pending rows (an index file's), or None
        self._names_lists = False  # of a built index: its adds named their lists (what _assign says before the build)
        self._ntotal = 0
        self._handle: ctypes.c_void_p | None = None
        self._handle_gen = 0  # bumped by close(): an IVFSubset of a closed handle is invalid
        self.small_batch = False
        self.set_small_batch(small_batch)

    def set_small_batch(self, enable: bool) -> None:
        """Switch the small-batch pass (``ls_ivf_set_small_batch``) on or off; kept when the device object is rebuilt.
        fp16 / sq8 rows refuse it (ValueError, before any device is touched); switching it off is always allowed."""
        enable = bool(enable)
        if enable and (refusal := switch_refusal("ivf", self._metric, self._dtype)):
            raise ValueError(refusal)
        if self._handle is not None:
            native.check(native.load().ls_ivf_set_small_batch(self._handle, 1 if enable else 0))
        self.small_batch = enable

    @property
    def metric(self) -> str:
        """``"ip"`` or ``"l2"``: fixed when the index is made."""
        return _METRIC_NAMES[self._metric]

    @property
    def _l2(self) -> bool:
        return self._metric == native.LS_METRIC_L2

    def last_passes(self) -> tuple[int, int]:
        """(union passes the most recent search launched, the sum of their union sizes in rows)."""
        p, r = ctypes.c_int32(), ctypes.c_int64()
        native.check(native.load().ls_ivf_last_passes(self._ensure_built(), ctypes.byref(p), ctypes.byref(r)))
        return p.value, r.value

    # ------------------------------------------------------------------ centroids
    def set_centroids(self, c: np.ndarray) -> None:
        c = np.ascontiguousarray(c, dtype=np.float32)
        if c.shape != (self.nlist, self.d):
            raise ValueError(f"centroids must be [{self.nlist}, {self.d}] float32, got {c.shape}")
        if self._handle is not None:
            raise ValueError("the device index is built: its centroids are fixed")
        if self._quantizer is not None:
            self._quantizer.close()
        self._centroids, self._quantizer, self.is_trained = c.copy(), None, True

    @property
    def centroids(self) -> np.ndarray:
        if self._centroids is None:
            raise ValueError("the index is not trained (train or set_centroids first)")
        return self._centroids

    @property
    def quantizer(self) -> FlatIPIndex:
        """A FlatIPIndex of the centroids - a FlatL2Index on an L2 index - (faiss's ``index.quantizer``): an independent
        handle of the same rows as the one the library probes with."""
        if self._quantizer is None:
            q = (FlatL2Index if self._l2 else FlatIPIndex)(self.d, dtype="f32", device=self.device)
            q.add(self.centroids)
            self._quantizer = q
        return self._quantizer

    def _nearest(self, cent: np.ndarray, x: np.ndarray) -> np.ndarray:
        """List of every row of x under the library's exact k = 1 search over ``cent`` (ties: lowest list)."""
        q = (FlatL2Index if self._l2 else FlatIPIndex).from_array(cent, dtype="f32", device=self.device)
        try:
            _, I = q.search(x, 1)
        finally:
            q.close()
        a = I[:, 0].copy()
        a[a < 0] = 0
        return a

    def train(self, x: np.ndarray, niter: int = 10, seed: int = 1234, on_device: bool | None = None) -> None:
        """Lloyd iterations under the index's metric: assign (exact k = 1 search on the GPU), then every centroid
        becomes the mean of its rows (float64 on the host). At most 256 training rows per centroid, sampled with
        ``seed``; an empty cluster is re-seeded with a row of the largest cluster (the one that scores lowest against
        that cluster's centroid; ``metric="l2"``: the one FARTHEST from it - the largest float64 squared distance,
        lowest row among equals). The same seed gives the same centroids. ``on_device=True`` (the default of an index
        made with ``build_on_device=True``): the sampled rows stay in HBM and both steps are one kernel each
        (``ls_ivf_trainer``); the same centroids, bit for bit."""
        if on_device is None:
            on_device = self.build_on_device
        if on_device and self.nlist > MAX_NLIST_ON_DEVICE:
            raise ValueError(f"train(on_device=True) serves nlist < {MAX_NLIST_ON_DEVICE + 1}, got {self.nlist}")
        x = np.ascontiguousarray(x, dtype=np.float32)
        if x.ndim != 2 or x.shape[1] != self.d:
            raise ValueError(f"train expects [n, {self.d}] float32")
        if x.shape[0] < self.nlist:
            raise ValueError(f"train needs at least nlist = {self.nlist} rows, got {x.shape[0]}")
        rng = np.random.default_rng(seed)
        cap = MAX_POINTS_PER_CENTROID * self.nlist
        if x.shape[0] > cap:
            x = x[np.sort(rng.choice(x.shape[0], cap, replace=False))]
        cent = x[np.sort(rng.choice(x.shape[0], self.nlist, replace=False))].copy()
        trainer = _Trainer(np.ascontiguousarray(x), self.nlist, self.device, l2=self._l2) if on_device else None

        def assign_and_reseed(cent, update):
            """One assignment; `update`: centroids become the means of their rows. Empty clusters are re-seeded:
            the largest cluster (lowest list number among equals) gives up the row that scores lowest against its own
            centroid (lowest row among equals), which becomes the empty cluster's centroid - under the inner product a
            scaled copy of a centroid would take either all of its rows or none. Returns (centroids, empties found)."""
            a = trainer.assign(cent) if trainer is not None else self._nearest(cent, x)
            order = np.argsort(a, kind="stable")
            counts = np.bincount(a, minlength=self.nlist).astype(np.int64)
            starts = np.concatenate(([0], np.cumsum(counts)[:-1]))
            new = cent.astype(np.float64)
            if update and trainer is not None:
                new = trainer.means()  # (a list without rows: its centroid, as above)
            elif update:
                full = np.flatnonzero(counts)
                new[full] = np.add.reduceat(x[order], starts[full], axis=0, dtype=np.float64) / counts[full, None]
            empty = np.flatnonzero(counts == 0)
            left = counts.copy()
            taken: dict[int, int] = {}
            for e in empty:
                big = int(np.argmax(np.where(counts > 0, left, -1)))  # (never a cluster that was itself just re-seeded)
                members = order[starts[big]:starts[big] + counts[big]]
                if self._l2:  # farthest first: the largest float64 squared distance to its own centroid
                    score = -((x[members].astype(np.float64) - new[big][None, :]) ** 2).sum(axis=1)
                else:
                    score = x[members].astype(np.float64) @ new[big]
                rank = np.lexsort((members, score))  # lowest score first, lowest row among equals
                j = taken.get(big, 0)
                taken[big] = j + 1
                new[e] = x[members[rank[min(j, rank.size - 1)]]]
                left[e] = left[big] // 2
                left[big] -= left[e]
            return new.astype(np.float32), int(empty.size)

        try:
            for _ in range(int(niter)):
                cent, _ = assign_and_reseed(cent, True)
            for _ in range(4):  # the centroids moved after the last assignment: make sure no list is left without a row
                cent, n_empty = assign_and_reseed(cent, False)
                if not n_empty:
                    break
        finally:
            if trainer is not None:
                trainer.close()
        self.set_centroids(cent)

    # ------------------------------------------------------------------ rows
    def add(self, x: np.ndarray, assign: np.ndarray | None = None) -> None:
        """index.add(x): buffered until the first search builds the device object; on a built index the rows are merged
        into its lists in HBM (``ls_ivf_add``: the index equals the one built from all rows at once, existing
        :class:`IVFSubset` objects stay valid). ``assign`` (int [n], optional) names every row's list instead of the
        default (largest inner product with the centroids - smallest distance on an L2 index -, ties lowest); either every add names its lists or none
        does, before and after the build."""
        if not self.is_trained:
            raise ValueError("the index is not trained (train or set_centroids first)")
        x = np.ascontiguousarray(x, dtype=np.float32)
        if x.ndim != 2 or x.shape[1] != self.d:
            raise ValueError(f"add expects [n, {self.d}] float32")
        names = self._names_lists if self._handle is not None else self._assign is not None
        if (assign is not None) != names and self._ntotal:
            raise ValueError("either every add names its lists or none does")
        if assign is not None:
            assign = np.ascontiguousarray(assign, dtype=np.int32).reshape(-1)
            if assign.shape[0] != x.shape[0] or (assign.size and (assign.min() < 0 or assign.max() >= self.nlist)):
                raise ValueError(f"assign must name a list in [0, {self.nlist}) for each of the {x.shape[0]} rows")
        if self._handle is not None:
            return self._add_built(x, assign)
        if assign is not None:
            self._assign = (self._assign or []) + [assign]
        if x.shape[0] == 0:
            return
        self._pending.append(x)
        self._ntotal += x.shape[0]

    def _add_built(self, x: np.ndarray, assign: np.ndarray | None) -> None:
        """``add`` on a built index: one ``ls_ivf_add`` (all or nothing: on an error the index is as it was)."""
        if x.shape[0] == 0:
            return
        lib = native.load()
        named = assign is not None
        if assign is None and self.build_on_device:
            # the lists ls_ivf_add would compute itself, by one launch per upload step (as _ensure_built does)
            assign = np.zeros(x.shape[0], dtype=np.int32)
            native.check(self._assign_fn(lib)(native.addr(x), x.shape[0], self.d, native.addr(self.centroids), self.nlist,
                                              native.addr(assign), self.device))
        native.check(lib.ls_ivf_add(self._handle, native.addr(x), x.shape[0],
                                    native.addr(assign) if assign is not None else None))
        if not self._ntotal:
            self._names_lists = named  # (the first rows of an index built empty decide)
        self._ntotal += x.shape[0]

    def remove_ids(self, sel) -> int:
        """index.remove_ids(sel): drop the selected rows and return how many were dropped. ``sel`` is what ``subset()``
        accepts: a bool mask [ntotal], an int array of row ids (out-of-range ids select nothing) or a faiss-style
        selector. Survivors are renumbered densely, as ``faiss.IndexFlat.remove_ids`` renumbers: old row ``r`` becomes
        ``r - (removed rows below r)``, so a positional id map loses the same positions. On a built index this is one
        ``ls_ivf_remove`` (all or nothing; the lists are compacted in HBM and the index equals the one built from the
        survivors; existing :class:`IVFSubset` objects stay valid and cover their surviving rows). Before the build
        the buffered rows, and the buffered lists where the adds named them, are edited on the host."""
        from .id_selectors import to_bitmap

        if not self.is_trained:
            raise ValueError("the index is not trained (train or set_centroids first)")
        bm = np.ascontiguousarray(to_bitmap(sel, self._ntotal), dtype=np.uint8).reshape(-1)
        if self._handle is not None:
            removed = ctypes.c_int64()
            native.check(native.load().ls_ivf_remove(self._handle, native.addr(bm) if bm.size else None, bm.size,
                                                     ctypes.byref(removed)))
            self._ntotal -= removed.value
            return int(removed.value)
        gone = np.zeros(self._ntotal, dtype=bool)  # (bits at r >= ntotal are ignored, rows past a short bitmap are kept)
        bits = np.unpackbits(bm, bitorder="little")[:self._ntotal].astype(bool)
        gone[:bits.size] = bits
        removed = int(gone.sum())
        if not removed:
            return 0
        keep = ~gone
        rows = np.concatenate(self._pending, axis=0)
        self._pending = [np.ascontiguousarray(rows[keep])] if keep.any() else []
        if self._assign is not None:
            # (an index emptied by the removal is as it was before its first add: that add decides again)
            self._assign = [np.concatenate(self._assign)[keep]] if keep.any() else None
        self._ntotal -= removed
        return removed

    def _assign_fn(self, lib):
        """The stateless assignment of the index's metric: ``ls_ivf_assign`` or ``ls_ivf_assign_l2``."""
        return lib.ls_ivf_assign_l2 if self._l2 else lib.ls_ivf_assign

    def _ensure_built(self) -> ctypes.c_void_p:
        if self._handle is not None:
            return self._handle
        lib = native.load()
        cent = self.centroids
        corpus = (np.concatenate(self._pending, axis=0) if self._pending else np.zeros((0, self.d), np.float32))
        assign = None
        if self._assign is not None and corpus.shape[0]:
            assign = np.ascontiguousarray(np.concatenate(self._assign), dtype=np.int32)
        elif self.build_on_device and corpus.shape[0]:
            # the lists ls_ivf_create would compute itself (n / 8 launches), by one launch per upload step
            assign = np.zeros(corpus.shape[0], dtype=np.int32)
            native.check(self._assign_fn(lib)(native.addr(corpus), corpus.shape[0], self.d, native.addr(cent), self.nlist,
                                              native.addr(assign), self.device))
        h = ctypes.c_void_p()
        create = lib.ls_ivf_create_l2 if self._l2 else lib.ls_ivf_create
        native.check(create(ctypes.byref(h), corpus.ctypes.data if corpus.size else None, corpus.shape[0],
                            self.d, self._dtype, cent.ctypes.data, self.nlist,
                            assign.ctypes.data if assign is not None else None, self.device))
        self._handle = h
        self._names_lists = self._assign is not None
        if self.small_batch:
            native.check(lib.ls_ivf_set_small_batch(h, 1))
        self._pending, self._assign = [], None  # the rows live in HBM now
        return h

    @property
    def ntotal(self) -> int:
        return self._ntotal

    @property
    def storage_dtype(self) -> str:
        return _DTYPE_NAMES[self._dtype]

    @property
    def bf16_inexact(self) -> int:
        """Elements of a bf16 index whose stored value differs from the float32 handed in (NaN never counts), over every
        row ever added (ls_ivf_bf16_inexact; removal does not lower it). Builds the device object if need be."""
        if self._dtype != native.LS_DTYPE_BF16:
            raise ValueError("bf16_inexact: the index does not store bf16 rows")
        out = ctypes.c_int64()
        native.check(native.load().ls_ivf_bf16_inexact(self._ensure_built(), ctypes.byref(out)))
        return int(out.value)

    def reconstruct_n(self, row0: int = 0, count: int | None = None) -> np.ndarray:
        """Rows [row0, row0 + count) as float32 [count, d], in add order: the buffered rows before the device object
        exists, afterwards read back from HBM (``ls_ivf_reconstruct``; fp16 / sq8 storage: the stored values)."""
        row0 = int(row0)
        count = self._ntotal - row0 if count is None else int(count)
        if row0 < 0 or count < 0 or row0 + count > self._ntotal:
            raise ValueError(f"reconstruct_n({row0}, {count}) is outside the {self._ntotal} rows of the index")
        if self._handle is None:
            rows = (np.concatenate(self._pending, axis=0) if self._pending else np.zeros((0, self.d), np.float32))
            return rows[row0:row0 + count].copy()
        out = np.zeros((count, self.d), dtype=np.float32)
        native.check(native.load().ls_ivf_reconstruct(self._handle, row0, count, native.addr(out)))
        return out

    def list_sizes(self) -> np.ndarray:
        out = np.zeros(self.nlist, dtype=np.int64)
        native.check(native.load().ls_ivf_list_sizes(self._ensure_built(), out.ctypes.data))
        return out

    def assignment(self) -> np.ndarray:
        """The list of every row (int32 [ntotal])."""
        out = np.zeros(self._ntotal, dtype=np.int32)
        native.check(native.load().ls_ivf_assignment(self._ensure_built(), out.ctypes.data if out.size else None))
        return out

    # ------------------------------------------------------------------ search
    def subset(self, sel) -> "IVFSubset":
        """Upload a row subset once (ls_ivf_subset_create): ``sel`` is a bool mask [ntotal], an int array of ORIGINAL
        row ids or a faiss-style selector (``faiss_compat.IDSelectorRange`` / ``IDSelectorBatch`` /
        ``IDSelectorBitmap``). Search it with ``search(x, k, params=subset)``."""
        from .id_selectors import to_bitmap

        if isinstance(sel, IVFSubset):
            if sel.index is not self:
                raise ValueError("the IVFSubset belongs to another index")
            return sel
        bm = np.ascontiguousarray(to_bitmap(sel, self._ntotal), dtype=np.uint8)
        h = self._ensure_built()
        sid, rows = ctypes.c_int32(), ctypes.c_int64()
        native.check(native.load().ls_ivf_subset_create(h, native.addr(bm) if bm.size else None, bm.size,
                                                        ctypes.byref(sid), ctypes.byref(rows)))
        return IVFSubset(self, sid.value, rows.value)

    def search_subset(self, x: np.ndarray, k: int, sel, *, nprobe: int | None = None, normalize: bool = False
                      ) -> tuple[np.ndarray, np.ndarray]:
        """The one-shot form: ``subset(sel)``, one search, ``close()``. An :class:`IVFSubset` is searched as it is."""
        x, k, nprobe = self._checked(x, k, self.nprobe if nprobe is None else nprobe)
        if x.shape[0] == 0 and not isinstance(sel, IVFSubset):
            return self._search(x, k, nprobe, normalize, None)  # nq = 0: nothing is uploaded
        sub = self.subset(sel)
        try:
            return self._search(x, k, nprobe, normalize, sub)
        finally:
            if sub is not sel:
                sub.close()

    def search(self, x: np.ndarray, k: int, *, normalize: bool = False, params=None
               ) -> tuple[np.ndarray, np.ndarray]:
        """index.search(x, k) over the rows of the ``nprobe`` probed lists (``params.nprobe``, faiss's
        ``SearchParametersIVF``, overrides the attribute for this call). Returns (D float32 [nq, k], I int64 [nq, k])
        best first under (score desc, original row asc); unfilled slots are (-FLT_MAX, -1). An L2 index returns squared
        distances, smallest first, ties by original row, unfilled slots (+FLT_MAX, -1). ``params.sel`` - or
        ``params`` itself - may be an :class:`IVFSubset` of this index (``subset(sel)``): the search then returns the
        selected rows of the probed lists only. A raw selector or mask is refused here: upload it with ``subset()``,
        or use ``search_subset()``."""
        nprobe, sub = self.nprobe, None
        if params is not None:
            sel = getattr(params, "sel", None)
            if sel is not None:
                if not isinstance(sel, IVFSubset):
                    raise ValueError("IVFFlatIndex.search takes an IVFSubset of this index as its selector, not a raw "
                                     f"selector or mask ({type(sel).__name__}): upload it once with subset(sel), or use "
                                     "search_subset(x, k, sel)")
                if sel.index is not self:
                    raise ValueError("the IVFSubset belongs to another index")
                sub = sel
            nprobe = getattr(params, "nprobe", nprobe)
        return self._search(x, k, nprobe, normalize, sub)

    def range_search(self, x: np.ndarray, radius: float, *, normalize: bool = False, params=None
                     ) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """index.range_search(x, radius) over the rows of the ``nprobe`` probed lists (ls_ivf_range_search,
        include/leansearch_range.h): every such row whose score is strictly above ``radius`` (an L2 index: whose squared distance is
        strictly below ``radius``; ``D`` holds distances). ``params`` is handled
        exactly as in :meth:`search` (``params.nprobe``; an :class:`IVFSubset` of this index as ``params.sel`` or as
        ``params`` itself restricts the result to its rows). Returns ``(lims, D, I)`` as faiss does: ``lims`` uint64
        [nq + 1]; query ``i`` owns ``D[lims[i]:lims[i + 1]]`` (float32, the flat scan's bits) and
        ``I[lims[i]:lims[i + 1]]`` (int64 original rows, ASCENDING). ``nprobe >= nlist`` equals
        ``FlatIPIndex.range_search`` of the same rows. The arrays are copies."""
        from .index import _empty_range_result, take_range_result

        nprobe, sub = self.nprobe, None
        if params is not None:
            sel = getattr(params, "sel", None)
            if sel is not None:
                if not isinstance(sel, IVFSubset):
                    raise ValueError("IVFFlatIndex.range_search takes an IVFSubset of this index as its selector, not a "
                                     f"raw selector or mask ({type(sel).__name__}): upload it once with subset(sel)")
                if sel.index is not self:
                    raise ValueError("the IVFSubset belongs to another index")
                sub = sel
            nprobe = getattr(params, "nprobe", nprobe)
        x, _, nprobe = self._checked(x, 1, nprobe)
        nq = x.shape[0]
        if nq == 0:
            return _empty_range_result()
        sid = sub.id if sub is not None else 0  # (raises for a closed subset, before anything is built)
        h = self._handle if self._handle is not None else self._ensure_built()
        lib = native.load()
        flags = native.LS_FLAG_NORMALIZE if normalize else 0
        res = ctypes.c_void_p()
        if sub is not None:
            rc = lib.ls_ivf_range_search_subset(h, sid, native.addr(x), nq, float(radius), nprobe, flags, ctypes.byref(res))
        else:
            rc = lib.ls_ivf_range_search(h, native.addr(x), nq, float(radius), nprobe, flags, ctypes.byref(res))
        native.check(rc)
        return take_range_result(lib, res)

    def _checked(self, x, k, nprobe):
        """The arguments of a search, checked and converted (before anything reaches the device)."""
        nprobe = int(nprobe)
        if nprobe < 1:
            raise ValueError("nprobe must be at least 1")
        if type(x) is not np.ndarray or x.dtype != np.float32 or not x.flags.c_contiguous:
            x = np.ascontiguousarray(x, dtype=np.float32)
        if x.ndim != 2 or x.shape[1] != self.d:
            raise ValueError(f"search expects [nq, {self.d}] float32, got {x.shape}")
        k = int(k)
        if k <= 0:
            raise ValueError("k must be positive")
        return x, k, nprobe

    def _search(self, x, k, nprobe, normalize, sub) -> tuple[np.ndarray, np.ndarray]:
        x, k, nprobe = self._checked(x, k, nprobe)
        nq = x.shape[0]
        D = np.empty((nq, k), dtype=np.float32)
        I = np.empty((nq, k), dtype=np.int64)
        if nq == 0:
            return D, I
        sid = sub.id if sub is not None else 0  # (raises for a closed subset, before anything is built)
        h = self._handle if self._handle is not None else self._ensure_built()
        addr = native.addr
        flags = native.LS_FLAG_NORMALIZE if normalize else 0
        if sub is not None:
            rc = native.load().ls_ivf_search_subset(h, sid, addr(x), nq, k, nprobe, flags, addr(D), addr(I))
        else:
            rc = native.load().ls_ivf_search(h, addr(x), nq, k, nprobe, flags, addr(D), addr(I))
        if rc:
            native.check(rc)
        return D, I

    # ------------------------------------------------------------------ instrumentation
    def set_profiling(self, enabled: bool) -> None:
        native.check(native.load().ls_ivf_set_profiling(self._ensure_built(), 1 if enabled else 0))

    def last_kernel_ms(self) -> tuple[float, float, int]:
        """(coarse ms, fine ms, queries served by the second launch) of the most recent search."""
        a, b, r = ctypes.c_float(), ctypes.c_float(), ctypes.c_int32()
        native.check(native.load().ls_ivf_last_kernel_ms(self._ensure_built(), ctypes.byref(a), ctypes.byref(b),
                                                         ctypes.byref(r)))
        return a.value, b.value, r.value

    def last_add_kernel_ms(self) -> tuple[float, int]:
        """(merge kernel ms, bytes it read and wrote) of the most recent ``add`` on the built index, with profiling
        on; zeros otherwise."""
        ms, nbytes = ctypes.c_float(), ctypes.c_int64()
        native.check(native.load().ls_ivf_add_last_kernel_ms(self._ensure_built(), ctypes.byref(ms), ctypes.byref(nbytes)))
        return ms.value, nbytes.value

    def last_remove_kernel_ms(self) -> tuple[float, int]:
        """(row-compaction kernel ms, bytes it read and wrote) of the most recent ``remove_ids`` on the built index,
        with profiling on; zeros otherwise."""
        ms, nbytes = ctypes.c_float(), ctypes.c_int64()
        native.check(native.load().ls_ivf_remove_last_kernel_ms(self._ensure_built(), ctypes.byref(ms),
                                                                ctypes.byref(nbytes)))
        return ms.value, nbytes.value

    def close(self) -> None:
        if self._handle is not None:
            native.load().ls_ivf_destroy(self._handle)  # (frees the handle's subsets with it)
            self._handle = None
            self._handle_gen += 1
        if self._quantizer is not None:
            self._quantizer.close()
            self._quantizer = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class IVFSubset:
    """A row subset uploaded once to its IVF index (``IVFFlatIndex.subset``): pass it as ``params.sel``, or as
    ``params`` itself, to search the selected rows of the probed lists without another upload. Holds its index; freed
    by ``close()``, by garbage collection, or with the index's handle (after which it is invalid). It covers the rows
    that existed when it was made: an ``add`` on the built index leaves it valid and does not extend it (the flat
    index's rule), so a subset never goes stale. A ``remove_ids`` on the built index leaves it valid too: afterwards it
    covers exactly its surviving rows under their new numbers (``rows`` and ``list_sizes()`` follow; it may become
    empty, and a search of it then returns all padding)."""

    def __init__(self, index: IVFFlatIndex, sid: int, rows: int):
        self.index = index
        self._id = sid
        self._gen = index._handle_gen
        self._rows = int(rows)  # selected rows when it was made (what a closed subset still reports)

    @property
    def rows(self) -> int:
        """Selected rows now: a ``remove_ids`` on the index may have taken some away."""
        if self.valid:
            self._rows = int(self.list_sizes().sum())
        return self._rows

    @property
    def valid(self) -> bool:
        return self._id is not None and self.index._handle is not None and self.index._handle_gen == self._gen

    @property
    def id(self) -> int:
        if not self.valid:
            raise ValueError("this IVFSubset was closed, or its index was closed")
        return self._id

    @property
    def sel(self) -> "IVFSubset":  # lets an IVFSubset stand where faiss expects SearchParameters
        return self

    def list_sizes(self) -> np.ndarray:
        """Selected rows of every list (int64 [nlist])."""
        out = np.zeros(self.index.nlist, dtype=np.int64)
        native.check(native.load().ls_ivf_subset_list_sizes(self.index._handle, self.id, out.ctypes.data))
        return out

    def close(self) -> None:
        if self.valid:
            native.check(native.load().ls_ivf_subset_destroy(self.index._handle, self._id))
        self._id = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
