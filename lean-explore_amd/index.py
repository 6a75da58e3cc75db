"""FlatIPIndex — the faiss-shaped object the local search backend holds.

It offers exactly the members the reference uses on its FAISS index
(reference src/lean_explore/search/engine.py:247-250 and tests/extract/index_test.py:172-173):
``search(x, k) -> (D, I)``, ``ntotal``, ``d``, ``add(x)``; it has no ``nprobe`` attribute (the
reference sets it only ``if hasattr(index, "nprobe")``, engine.py:247). All arithmetic happens in
libleansearch.so on the MI355X; this class only owns the handle and marshals numpy / torch
buffers across the C ABI.
"""

from __future__ import annotations

import ctypes
from typing import Any, Callable, NamedTuple

import numpy as np

from . import native

_DTYPES = {"f32": native.LS_DTYPE_F32, "float32": native.LS_DTYPE_F32,
           "f16": native.LS_DTYPE_F16, "float16": native.LS_DTYPE_F16,
           "sq8": native.LS_DTYPE_SQ8,  # (never "int8": the rows handed in stay float32; lean_explore_amd/sq8.py)
           "bf16": native.LS_DTYPE_BF16, "bfloat16": native.LS_DTYPE_BF16}  # (include/leansearch_bf16.h; bf16.py)
_DTYPE_NAMES = {native.LS_DTYPE_F32: "f32", native.LS_DTYPE_F16: "f16", native.LS_DTYPE_SQ8: "sq8",
                native.LS_DTYPE_BF16: "bf16"}


def _dtype_code(dtype: Any) -> int:
    if isinstance(dtype, int):
        return dtype
    try:
        return _DTYPES[str(np.dtype(dtype)) if not isinstance(dtype, str) else dtype]
    except (KeyError, TypeError):
        raise ValueError(f"unsupported storage dtype {dtype!r} (use 'f32', 'f16', 'sq8' or 'bf16')") from None


_METRICS = {"ip": native.LS_METRIC_INNER_PRODUCT, "inner_product": native.LS_METRIC_INNER_PRODUCT,
            "l2": native.LS_METRIC_L2}
_METRIC_NAMES = {native.LS_METRIC_INNER_PRODUCT: "ip", native.LS_METRIC_L2: "l2"}


def _metric_code(metric: Any) -> int:
    try:
        if isinstance(metric, str):
            return _METRICS[metric.lower()]
        return _METRICS[_METRIC_NAMES[int(metric)]]  # (the LS_METRIC_* numbers, which are faiss's METRIC_*)
    except (KeyError, TypeError, ValueError):
        raise ValueError(f"unsupported metric {metric!r} (use 'ip' or 'l2')") from None


class _Switch(NamedTuple):
    symbol: str  # the C setter
    rule: Callable[[bool, int, bool], "str | None"]  # (L2 metric, dtype code, devices=[...] given) -> why enabling is refused
    on_handle: Callable[[bool, int], bool]  # (L2 metric, dtype code) -> a built handle of this kind is told of every set


def _first(*rules: tuple[Any, str]) -> str | None:
    return next((text for applies, text in rules if applies), None)


_F32, _F16, _SQ8, _BF16 = native.LS_DTYPE_F32, native.LS_DTYPE_F16, native.LS_DTYPE_SQ8, native.LS_DTYPE_BF16
# The small-batch switches: what each serves and the words it is refused with otherwise - the first rule
# that applies is the one raised. Switching one off is never refused here. The flat index's four in the order they are
# checked and applied to a handle, then the IVF index's.
SWITCHES: dict[str, _Switch] = {
    "f16": _Switch("ls_set_f16_small_batch", lambda l2, dt, placed: _first(
        (l2, "f16_small_batch: an L2 index serves every query alone by the scan"),
        (dt == _BF16, "f16_small_batch needs dtype='f16' (the index stores bf16 rows: every bf16 query is served alone by the scan)"),
        (dt == _SQ8, "f16_small_batch needs dtype='f16' (every sq8 query is served alone by the scan)"),
        (dt != _F16, "f16_small_batch needs dtype='f16' (small fp32 batches already share a pass)")),
        lambda l2, dt: dt == _F16),
    "sq8": _Switch("ls_set_sq8_small_batch", lambda l2, dt, placed: _first(
        (l2, "sq8_small_batch: an L2 index stores no sq8 codes and serves every query alone by the scan"),
        (dt == _BF16, "sq8_small_batch needs dtype='sq8' (the index stores bf16 rows: every bf16 query is served alone by the scan)"),
        (dt != _SQ8, "sq8_small_batch needs dtype='sq8'")),
        lambda l2, dt: dt == _SQ8),
    "subset": _Switch("ls_set_subset_small_batch", lambda l2, dt, placed: _first(
        (l2, "subset_small_batch: an L2 index serves every query alone by the row-list scan"),
        (dt == _BF16, "subset_small_batch needs dtype='f32' (the index stores bf16 rows: their subset searches launch per query)"),
        (dt != _F32, "subset_small_batch needs dtype='f32' (fp16 and sq8 subset searches launch per query)"),
        (placed, "subset_small_batch serves an index on one device (no devices=[...])")),
        lambda l2, dt: True),
    "l2": _Switch("ls_set_l2_small_batch", lambda l2, dt, placed: _first(
        (not l2, "l2_small_batch needs metric='l2' (an inner-product index has its own small-batch options)"),
        (dt == _SQ8, "l2_small_batch needs dtype='f32' or 'f16' (there is no sq8 L2 index)"),
        (dt == _BF16, "l2_small_batch needs dtype='f32' or 'f16' (there is no L2 index of bf16 rows)"),
        (placed, "l2_small_batch serves an index on one device (no devices=[...])")),
        lambda l2, dt: l2),
    "ivf": _Switch("ls_ivf_set_small_batch", lambda l2, dt, placed: _first(
        (l2, "small_batch serves the inner product: every L2 query is served alone (ls_ivf_set_small_batch)"),
        (dt == _BF16, "small_batch serves fp32 rows: the index stores bf16 rows (ls_ivf_set_small_batch)"),
        (dt != _F32, f"small_batch serves fp32 rows, not {_DTYPE_NAMES.get(dt)!r} (ls_ivf_set_small_batch)")),
        lambda l2, dt: True),
}
_FLAT_SWITCHES = ("f16", "sq8", "subset", "l2")


def switch_refusal(name: str, metric: Any, dtype: Any, placed: bool = False) -> str | None:
    """Why switch ``name`` cannot be on for this metric and storage dtype (``placed``: over ``devices=[...]``); None: served."""
    return SWITCHES[name].rule(_metric_code(metric) == native.LS_METRIC_L2, _dtype_code(dtype), placed)


def normalize_L2(x: np.ndarray, device: int = 0) -> None:
    """In-place row L2 normalisation of a C-contiguous float32 [nq, d] array.

    Counterpart of ``faiss.normalize_L2`` (reference search/engine.py:242): returns None,
    rows with zero norm are left unchanged.
    """
    if not isinstance(x, np.ndarray) or x.dtype != np.float32 or x.ndim != 2 \
            or not x.flags.c_contiguous:
        raise ValueError("normalize_L2 expects a C-contiguous float32 array of shape [nq, d]")
    lib = native.load()
    native.check(lib.ls_normalize_l2(x.ctypes.data, x.shape[0], x.shape[1], device))


def _empty_range_result() -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    return np.zeros(1, np.uint64), np.zeros(0, np.float32), np.zeros(0, np.int64)


def take_range_result(lib, res: ctypes.c_void_p) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(lims uint64 [nq + 1], D float32, I int64) copied out of an ``ls_range_result``, which is freed."""
    try:
        nq = int(lib.ls_range_nq(res))
        lims = np.ctypeslib.as_array((ctypes.c_int64 * (nq + 1)).from_address(lib.ls_range_lims(res))).astype(np.uint64)
        total = int(lims[-1])
        if not total:
            return lims, np.zeros(0, np.float32), np.zeros(0, np.int64)
        D = np.ctypeslib.as_array((ctypes.c_float * total).from_address(lib.ls_range_scores(res))).copy()
        I = np.ctypeslib.as_array((ctypes.c_int64 * total).from_address(lib.ls_range_rows(res))).copy()
        return lims, D, I
    finally:
        lib.ls_range_free(res)


def _device_list(devices: Any) -> list[int] | None:
    """``None`` -> single device; ``"all"`` -> every visible GPU; else a list of ordinals."""
    if devices is None:
        return None
    if isinstance(devices, str):
        if devices.strip().lower() == "all":
            return list(range(native.device_count()))
        devices = [int(t) for t in devices.replace(",", " ").split()]
    out = [int(t) for t in devices]
    if not out:
        raise ValueError("devices must name at least one GPU")
    return out


class FlatIPIndex:
    """Exact inner-product index resident in HBM: one GPU, or — ``devices=[...]`` — row-sharded
    over several GPUs of the node inside this one process (ls_create_sharded: concurrent local
    top-k, one RCCL all-gather of the packed results, merge on ``devices[0]``; bit-identical
    to the single-GPU answer). The reference's backend is one process holding one index
    (reference mcp/server.py:147-151), so this is how `Service.search()` uses a whole node."""

    supports_fused_normalize = True  # search(..., normalize=True) fuses faiss.normalize_L2
    _default_metric = "ip"

    def __init__(self, d: int, dtype: Any = "f32", device: int = 0, base: int = 0,
                 devices: Any = None, replicate: bool = False, f16_small_batch: bool = False,
                 sq8_step: Any = None, sq8_small_batch: bool = False, subset_small_batch: bool = False,
                 metric: Any = None, l2_small_batch: bool = False):
        if d <= 0:
            raise ValueError("d must be positive")
        self.d = int(d)
        self._dtype = _dtype_code(dtype)
        # metric="l2" (include/leansearch_l2.h): search and range_search return SQUARED distances, smallest first,
        # padding (+FLT_MAX, -1); f32 or f16 rows on one device, every query served alone by the scan
        self._metric = self._check_metric(self._default_metric if metric is None else metric, devices)
        # dtype="sq8" (include/leansearch_sq8.h; not faiss's QT_8bit): int8 codes in HBM, one float32 step per
        # dimension - `sq8_step` [d], or trained from the rows present when the handle is built (sq8.train_step)
        self._sq8_step = self._check_sq8(sq8_step, devices)
        # dtype="bf16" (include/leansearch_bf16.h): bfloat16 rows in HBM, float32 query - exact for rows that are already
        # bf16-valued (bf16_inexact == 0); inner product on one device, every query served alone by the scan
        if self._dtype == native.LS_DTYPE_BF16 and devices is not None:
            raise ValueError("a bf16 index cannot be sharded or replicated (devices=...): bf16 rows are served on one device")
        # The small-batch switches (SWITCHES), all off by default: several queries share ONE corpus pass.
        # f16_small_batch: 1..32 on the f16 matrix cores - a query's bits then do not depend on its company, but differ
        # (within the fp16 tolerance) from the default path's. sq8_small_batch (2..16 over the codes), subset_small_batch
        # (2..16 of a subset search) and l2_small_batch (groups of 8 / 4 / 1): the same bits either way.
        asked = dict(zip(_FLAT_SWITCHES, (f16_small_batch, sq8_small_batch, subset_small_batch, l2_small_batch)))
        # (the order refusals have always come in: f16, sq8, a `devices` that names no GPU, subset, l2)
        self._on = {name: self._check_switch(name, asked[name], devices is not None) for name in ("f16", "sq8")}
        self.devices = _device_list(devices)
        self._on.update((name, self._check_switch(name, asked[name], devices is not None)) for name in ("subset", "l2"))
        # replicate=True: every device of `devices` holds the WHOLE corpus and synchronous searches
        # are dealt round-robin to the replicas (ls_create_replicated) instead of row shards
        self.replicate = bool(replicate)
        if self.replicate and not self.devices:
            raise ValueError("replicate=True needs devices=[...]")
        self.device = int(self.devices[0]) if self.devices else int(device)
        self._base = int(base)
        self._handle: ctypes.c_void_p | None = None
        # rows added before the first search: uploaded (and released) when the handle is built.
        # No host copy outlives that: later add() calls append in HBM (ls_add), host_corpus()
        # reads the rows back (ls_reconstruct).
        self._pending: list[np.ndarray] = []
        self._ntotal = 0
        self._device_built = False             # built straight from device memory
        self.is_trained = True
        self._handle_gen = 0                   # bumped when the handle is dropped: its RowSubsets die with it

    def _check_metric(self, metric: Any, devices: Any) -> int:
        code = _metric_code(metric)
        if code == native.LS_METRIC_L2:
            if self._dtype == native.LS_DTYPE_SQ8:
                raise ValueError("metric='l2' needs dtype='f32' or 'f16' (sq8 codes serve the inner product only)")
            if self._dtype == native.LS_DTYPE_BF16:
                raise ValueError("metric='l2' needs dtype='f32' or 'f16' (bf16 rows serve the inner product only)")
            if devices is not None:
                raise ValueError("an L2 index cannot be sharded or replicated (devices=...)")
        return code

    @property
    def metric(self) -> str:
        """``"ip"`` or ``"l2"``: fixed when the index is made."""
        return _METRIC_NAMES[self._metric]

    def _check_sq8(self, step: Any, devices: Any) -> np.ndarray | None:
        if self._dtype != native.LS_DTYPE_SQ8:
            if step is not None:
                raise ValueError("sq8_step needs dtype='sq8'")
            return None
        if devices is not None:
            raise ValueError("an sq8 index cannot be sharded or replicated (devices=...): every shard would train "
                             "its own step")
        if step is None:
            return None
        step = np.ascontiguousarray(step, dtype=np.float32)
        if step.shape != (self.d,) or not (np.isfinite(step).all() and (step > 0).all()):
            raise ValueError(f"sq8_step must be [{self.d}] float32, every entry finite and > 0")
        return step

    def _check_switch(self, name: str, enable: bool, placed: bool) -> bool:
        if enable and (refusal := SWITCHES[name].rule(self._metric == native.LS_METRIC_L2, self._dtype, placed)):
            raise ValueError(refusal)
        return bool(enable)

    def _set_switch(self, name: str, enable: bool) -> None:
        """Kept across a rebuild of the handle; a built handle of the switch's kind is told at once."""
        self._on[name] = self._check_switch(name, enable, self.devices is not None)
        if self._handle is not None and SWITCHES[name].on_handle(self._metric == native.LS_METRIC_L2, self._dtype):
            self._apply_switch(self._handle, name)

    def _apply_switch(self, h: ctypes.c_void_p, name: str) -> None:
        native.check(getattr(native.load(), SWITCHES[name].symbol)(h, int(self._on[name])))

    def _apply_to_handle(self, h: ctypes.c_void_p) -> None:
        """A fresh handle takes the base and the switches that are on."""
        lib = native.load()
        if self._base:
            native.check(lib.ls_set_base(h, self._base))
        for name in _FLAT_SWITCHES:
            if self._on[name]:
                self._apply_switch(h, name)

    f16_small_batch = property(lambda self: self._on["f16"])
    sq8_small_batch = property(lambda self: self._on["sq8"])
    subset_small_batch = property(lambda self: self._on["subset"])
    l2_small_batch = property(lambda self: self._on["l2"], lambda self, enable: self._set_switch("l2", enable))

    def set_f16_small_batch(self, enable: bool) -> None:
        """Switch the fp16 small-batch pass on or off (ls_set_f16_small_batch); kept across a rebuild of the handle."""
        self._set_switch("f16", enable)

    def set_sq8_small_batch(self, enable: bool) -> None:
        """Switch the sq8 small-batch pass on or off (ls_set_sq8_small_batch); kept across a rebuild of the handle."""
        self._set_switch("sq8", enable)

    def set_subset_small_batch(self, enable: bool) -> None:
        """Switch the subset pass on or off (ls_set_subset_small_batch); kept across a rebuild of the handle."""
        self._set_switch("subset", enable)

    def set_l2_small_batch(self, enable: bool) -> None:
        """Switch the L2 query groups on or off (ls_set_l2_small_batch); kept across a rebuild of the handle."""
        self._set_switch("l2", enable)

    # ------------------------------------------------------------------ construction
    @classmethod
    def from_array(cls, corpus: np.ndarray, dtype: Any = "f32", device: int = 0,
                   base: int = 0, devices: Any = None, replicate: bool = False,
                   f16_small_batch: bool = False, sq8_step: Any = None,
                   sq8_small_batch: bool = False, subset_small_batch: bool = False,
                   metric: Any = None, l2_small_batch: bool = False) -> "FlatIPIndex":
        corpus = np.asarray(corpus)
        if corpus.ndim != 2:
            raise ValueError("corpus must be [n, d]")
        ix = cls(corpus.shape[1], dtype=dtype, device=device, base=base, devices=devices,
                 replicate=replicate, f16_small_batch=f16_small_batch, sq8_step=sq8_step,
                 sq8_small_batch=sq8_small_batch, subset_small_batch=subset_small_batch, metric=metric,
                 l2_small_batch=l2_small_batch)
        ix.add(corpus)
        ix._ensure_built()
        return ix

    @classmethod
    def from_device_tensor(cls, corpus, dtype: Any = "f32", base: int = 0,
                           f16_small_batch: bool = False,
                           sq8_small_batch: bool = False,  # (sq8: the step is trained from the rows)
                           subset_small_batch: bool = False, metric: Any = None,
                           l2_small_batch: bool = False) -> "FlatIPIndex":
        """Build from a torch float32 CUDA tensor [n, d] without a host round trip."""
        import torch

        if not (isinstance(corpus, torch.Tensor) and corpus.is_cuda and corpus.dim() == 2
                and corpus.dtype == torch.float32 and corpus.is_contiguous()):
            raise ValueError("expected a contiguous float32 CUDA tensor [n, d]")
        ix = cls(corpus.shape[1], dtype=dtype, device=corpus.device.index or 0, base=base,
                 f16_small_batch=f16_small_batch, sq8_small_batch=sq8_small_batch,
                 subset_small_batch=subset_small_batch, metric=metric, l2_small_batch=l2_small_batch)
        lib = native.load()
        h = ctypes.c_void_p()
        torch.cuda.synchronize(corpus.device)
        create = lib.ls_create_l2_from_device if ix._metric == native.LS_METRIC_L2 else lib.ls_create_from_device
        native.check(create(ctypes.byref(h), corpus.data_ptr(), corpus.shape[0], ix.d, ix._dtype, ix.device))
        ix._handle = h
        ix._ntotal = int(corpus.shape[0])
        ix._device_built = True
        ix._apply_to_handle(h)
        return ix

    @classmethod
    def from_device_blocks(cls, blocks: list, dtype: Any = "f32", base: int = 0,
                           f16_small_batch: bool = False) -> "FlatIPIndex":
        """Row-sharded index from per-device float32 CUDA tensors ``blocks[g]`` of shape
        [rows_g, d] (block g stays on its own GPU; global rows are numbered block after block).
        Multi-GB synthetic shards never cross the host (ls_create_sharded_from_device)."""
        import torch

        if not blocks:
            raise ValueError("need at least one block")
        d = int(blocks[0].shape[1])
        for b in blocks:
            if not (isinstance(b, torch.Tensor) and b.is_cuda and b.dim() == 2 and b.shape[1] == d
                    and b.dtype == torch.float32 and b.is_contiguous()):
                raise ValueError("every block must be a contiguous float32 CUDA tensor [rows, d]")
        devs = [b.device.index or 0 for b in blocks]
        ix = cls(d, dtype=dtype, base=base, devices=devs, f16_small_batch=f16_small_batch)
        n = len(blocks)
        ptrs = (ctypes.c_void_p * n)(*[b.data_ptr() for b in blocks])
        rows = (ctypes.c_int64 * n)(*[int(b.shape[0]) for b in blocks])
        ids = (ctypes.c_int32 * n)(*devs)
        for b in blocks:
            torch.cuda.synchronize(b.device)
        h = ctypes.c_void_p()
        lib = native.load()
        native.check(lib.ls_create_sharded_from_device(ctypes.byref(h), ptrs, rows, d, ix._dtype, ids, n))
        ix._handle = h
        ix._ntotal = int(sum(int(b.shape[0]) for b in blocks))
        ix._device_built = True
        ix._apply_to_handle(h)
        return ix

    def shards(self) -> list[tuple[int, int, int]]:
        """(device, first global row, rows) of every shard; [] for a single-device index."""
        h = self._ensure_built()
        lib = native.load()
        out = []
        for g in range(int(lib.ls_shard_count(h))):
            dev, row0, rows = ctypes.c_int32(), ctypes.c_int64(), ctypes.c_int64()
            native.check(lib.ls_shard_info(h, g, ctypes.byref(dev), ctypes.byref(row0),
                                           ctypes.byref(rows)))
            out.append((dev.value, row0.value, rows.value))
        return out

    def exchange_info(self) -> dict:
        """What the exchange step of a sharded handle does on this node (ls_shard_exchange_info):
        transport, RCCL version / failure text, enqueue workers, peer-access matrix. {} for a
        single-device index."""
        import json

        h = self._ensure_built()
        lib = native.load()
        if int(lib.ls_shard_count(h)) == 0:
            return {}
        buf = ctypes.create_string_buffer(8192)
        need = int(lib.ls_shard_exchange_info(h, buf, len(buf)))
        if need < 0:
            native.check(need)
        return json.loads(buf.value.decode())

    def add(self, x: np.ndarray) -> None:
        """index.add(x) (reference extract/index.py:116): append float32 rows. On a built index
        the stored rows stay in HBM and only the new ones are uploaded (ls_add)."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        if x.ndim != 2 or x.shape[1] != self.d:
            raise ValueError(f"add expects [n, {self.d}] float32")
        if x.shape[0] == 0:
            return
        if self._handle is not None:
            native.check(native.load().ls_add(self._handle, x.ctypes.data, x.shape[0]))
        else:
            self._pending.append(x)
        self._ntotal += x.shape[0]

    def remove_ids(self, sel) -> int:
        """index.remove_ids(sel): drop the selected rows and return how many were dropped. ``sel`` is what ``subset()``
        accepts: a bool mask [ntotal], an int array of row ids (duplicates fine, out-of-range ids select nothing) or a
        faiss-style selector. Survivors are renumbered densely, as ``faiss.IndexFlat.remove_ids`` renumbers: old row
        ``r`` becomes ``r - (removed rows below r)``, so a positional id map loses the same positions. On a built index
        this is one ``ls_remove``: the stored rows are compacted in place in HBM (no second copy, nothing crosses PCIe),
        the index equals the one built from the survivors, and existing :class:`RowSubset` objects stay valid and cover
        their surviving rows. Before the build the buffered rows are edited on the host."""
        from .id_selectors import to_bitmap

        bm = np.ascontiguousarray(to_bitmap(sel, self._ntotal), dtype=np.uint8).reshape(-1)
        if self._handle is not None:
            removed = ctypes.c_int64()
            native.check(native.load().ls_remove(self._handle, native.addr(bm) if bm.size else None, bm.size,
                                                 ctypes.byref(removed)))
            self._ntotal -= removed.value
            return int(removed.value)
        if self._device_built:
            raise ValueError("remove_ids: the index's handle was dropped")
        gone = np.zeros(self._ntotal, dtype=bool)  # (bits at r >= ntotal are ignored, rows past a short bitmap are kept)
        bits = np.unpackbits(bm, bitorder="little")[:self._ntotal].astype(bool)
        gone[:bits.size] = bits
        removed = int(gone.sum())
        if not removed:
            return 0
        keep = ~gone
        rows = np.concatenate(self._pending, axis=0)
        self._pending = [np.ascontiguousarray(rows[keep])] if keep.any() else []
        self._ntotal -= removed
        return removed

    def remove_stats(self) -> tuple[int, int, float, int]:
        """(moved_rows, slabs, move_ms, move_bytes) of the most recent ``remove_ids`` on the built index
        (ls_remove_last): rows that changed place, staging slabs used and - with ``set_profiling(True)`` - the time
        of the row moves on the GPU and the bytes they read + wrote."""
        moved, slabs, ms, nbytes = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_float(), ctypes.c_int64()
        native.check(native.load().ls_remove_last(self._ensure_built(), ctypes.byref(moved), ctypes.byref(slabs),
                                                  ctypes.byref(ms), ctypes.byref(nbytes)))
        return int(moved.value), int(slabs.value), float(ms.value), int(nbytes.value)

    def set_remove_slab_rows(self, rows: int) -> None:
        """Rows per staging slab of the following ``remove_ids`` calls (ls_remove_set_slab_rows); 0 = automatic (as
        many stored rows as fit 256 MiB). A test and tuning hook: the result does not depend on it."""
        native.check(native.load().ls_remove_set_slab_rows(self._ensure_built(), int(rows)))

    def _drop_handle(self) -> None:
        if self._handle is not None:
            self._handle_gen += 1
            native.load().ls_destroy(self._handle)
            self._handle = None

    def _ensure_built(self) -> ctypes.c_void_p:
        if self._handle is not None:
            return self._handle
        lib = native.load()
        if len(self._pending) > 1:
            self._pending = [np.concatenate(self._pending, axis=0)]
        corpus = self._pending[0] if self._pending else np.zeros((0, self.d), np.float32)
        h = ctypes.c_void_p()
        if self.devices is not None:
            ids = (ctypes.c_int32 * len(self.devices))(*self.devices)
            create = lib.ls_create_replicated if self.replicate else lib.ls_create_sharded
            native.check(create(
                ctypes.byref(h), corpus.ctypes.data if corpus.size else None, corpus.shape[0],
                self.d, self._dtype, ids, len(self.devices)))
        elif self._dtype == native.LS_DTYPE_SQ8:
            native.check(lib.ls_create_sq8(ctypes.byref(h), corpus.ctypes.data if corpus.size else None, corpus.shape[0],
                                           self.d, None if self._sq8_step is None else self._sq8_step.ctypes.data,
                                           self.device))
        else:
            create = lib.ls_create_l2 if self._metric == native.LS_METRIC_L2 else lib.ls_create
            native.check(create(ctypes.byref(h), corpus.ctypes.data if corpus.size else None,
                                corpus.shape[0], self.d, self._dtype, self.device))
        self._handle = h
        self._pending = []  # the rows live in HBM now
        self._apply_to_handle(h)
        return h

    # ------------------------------------------------------------------ properties
    @property
    def ntotal(self) -> int:
        return self._ntotal

    @property
    def storage_dtype(self) -> str:
        return _DTYPE_NAMES[self._dtype]

    @property
    def sq8_step(self) -> np.ndarray:
        """The per-dimension step of an sq8 index, float32 [d] (ls_sq8_step): the one given, or the one trained from
        the rows when the handle was built (building it if need be)."""
        if self._dtype != native.LS_DTYPE_SQ8:
            raise ValueError("sq8_step: the index does not store sq8 codes")
        out = np.empty(self.d, dtype=np.float32)
        native.check(native.load().ls_sq8_step(self._ensure_built(), out.ctypes.data))
        return out

    def codes(self, row0: int = 0, count: int | None = None) -> np.ndarray:
        """The stored int8 codes of rows [row0, row0 + count) of an sq8 index, [count, d] (ls_sq8_codes)."""
        if self._dtype != native.LS_DTYPE_SQ8:
            raise ValueError("codes(): the index does not store sq8 codes")
        h = self._ensure_built()
        count = self._ntotal - int(row0) if count is None else int(count)
        out = np.empty((max(count, 0), self.d), dtype=np.int8)
        native.check(native.load().ls_sq8_codes(h, int(row0), count, out.ctypes.data if out.size else None))
        return out

    @property
    def bf16_inexact(self) -> int:
        """Elements of a bf16 index whose stored value differs from the float32 handed in (NaN never counts), over every
        row ever added (ls_bf16_inexact; removal does not lower it). 0: the index holds exactly what it was given."""
        if self._dtype != native.LS_DTYPE_BF16:
            raise ValueError("bf16_inexact: the index does not store bf16 rows")
        out = ctypes.c_int64()
        native.check(native.load().ls_bf16_inexact(self._ensure_built(), ctypes.byref(out)))
        return int(out.value)

    def bf16_rows(self, row0: int = 0, count: int | None = None) -> np.ndarray:
        """The stored bits of rows [row0, row0 + count) of a bf16 index, uint16 [count, d] (ls_bf16_rows)."""
        if self._dtype != native.LS_DTYPE_BF16:
            raise ValueError("bf16_rows(): the index does not store bf16 rows")
        h = self._ensure_built()
        count = self._ntotal - int(row0) if count is None else int(count)
        out = np.empty((max(count, 0), self.d), dtype=np.uint16)
        native.check(native.load().ls_bf16_rows(h, int(row0), count, out.ctypes.data if out.size else None))
        return out

    @property
    def base(self) -> int:
        return self._base

    def host_corpus(self) -> np.ndarray:
        """The stored rows as float32 [ntotal, d], read back from HBM (index.reconstruct_n);
        an fp16 index returns the rounded values, an sq8 index the decoded codes. Before the first search the rows have not been
        uploaded yet and are returned as added."""
        if self._handle is None and not self._device_built:
            if len(self._pending) > 1:
                self._pending = [np.concatenate(self._pending, axis=0)]
            return self._pending[0] if self._pending else np.zeros((0, self.d), np.float32)
        h = self._ensure_built()
        out = np.empty((self._ntotal, self.d), dtype=np.float32)
        if self._ntotal:
            native.check(native.load().ls_reconstruct(h, 0, self._ntotal, out.ctypes.data))
        return out

    def reconstruct_n(self, row0: int = 0, count: int | None = None) -> np.ndarray:
        """index.reconstruct_n(row0, count): rows [row0, row0 + count) as float32 [count, d] - the stored values (an fp16
        index: rounded; sq8: decoded; bf16: ``bf16.decode`` of the stored bits, exact) once the handle is built."""
        row0 = int(row0)
        count = self._ntotal - row0 if count is None else int(count)
        if row0 < 0 or count < 0 or row0 + count > self._ntotal:
            raise ValueError(f"reconstruct_n({row0}, {count}) is outside the {self._ntotal} rows of the index")
        if self._handle is None and not self._device_built:
            return np.array(self.host_corpus()[row0:row0 + count], dtype=np.float32)
        out = np.empty((count, self.d), dtype=np.float32)
        if count:
            native.check(native.load().ls_reconstruct(self._ensure_built(), row0, count, out.ctypes.data))
        return out

    # ------------------------------------------------------------------ search
    def subset(self, sel) -> "RowSubset":
        """Upload a row subset once (ls_subset_create): ``sel`` is a bool mask [ntotal], an int array of row ids or
        a faiss-style selector (``faiss_compat.IDSelectorRange`` / ``IDSelectorBatch`` / ``IDSelectorBitmap``)."""
        from .id_selectors import to_bitmap

        if isinstance(sel, RowSubset):
            if sel.index is not self:
                raise ValueError("the RowSubset belongs to another index")
            return sel
        bm = to_bitmap(sel, self._ntotal)
        h = self._ensure_built()
        sid, rows = ctypes.c_int32(), ctypes.c_int64()
        native.check(native.load().ls_subset_create(h, native.addr(bm) if bm.size else None, bm.size,
                                                    ctypes.byref(sid), ctypes.byref(rows)))
        return RowSubset(self, sid.value, rows.value)

    def search(self, x: np.ndarray, k: int, *, normalize: bool = False, params=None
               ) -> tuple[np.ndarray, np.ndarray]:
        """index.search(x, k) (reference search/engine.py:250).

        x: float32 [nq, d]. Returns (D float32 [nq, k], I int64 [nq, k]) best first under
        (score desc, row asc); unfilled slots are (-FLT_MAX, -1). An L2 index (``metric="l2"``) returns squared
        distances, best first under (distance asc, row asc); unfilled slots are (+FLT_MAX, -1). ``params.sel`` (faiss's
        ``SearchParameters(sel=...)``) restricts the search to a row subset: a :class:`RowSubset`
        of this index (nothing uploaded), or any selector / mask (a subset for this call only).
        """
        if params is not None and getattr(params, "sel", None) is not None:
            return self._search_subset(x, k, normalize, params.sel)
        # (this wrapper is ~2 us of a 62 us call: no conversion call for the usual float32 row-major
        # query, no helper objects for the three pointers - native.addr)
        if type(x) is not np.ndarray or x.dtype != np.float32 or not x.flags.c_contiguous:
            x = np.ascontiguousarray(x, dtype=np.float32)
        if x.ndim != 2 or x.shape[1] != self.d:
            raise ValueError(f"search expects [nq, {self.d}] float32, got {x.shape}")
        k = int(k)
        if k <= 0:
            raise ValueError("k must be positive")
        h = self._handle if self._handle is not None else self._ensure_built()
        nq = x.shape[0]
        D = np.empty((nq, k), dtype=np.float32)
        I = np.empty((nq, k), dtype=np.int64)
        flags = native.LS_FLAG_NORMALIZE if normalize else 0
        fast = native.fast_search()
        if fast is not None:  # csrc/lsfast.c: the same ls_search, bound without ctypes' argument conversion
            rc = fast[0].search(fast[1], h.value, x, nq, k, flags, D, I)
        else:
            addr = native.addr
            rc = native.load().ls_search(h, addr(x), nq, k, flags, addr(D), addr(I))
        if rc:
            native.check(rc)
        return D, I

    def _search_subset(self, x, k: int, normalize: bool, sel) -> tuple[np.ndarray, np.ndarray]:
        x = np.ascontiguousarray(x, dtype=np.float32)
        if x.ndim != 2 or x.shape[1] != self.d:
            raise ValueError(f"search expects [nq, {self.d}] float32, got {x.shape}")
        k = int(k)
        if k <= 0:
            raise ValueError("k must be positive")
        nq = x.shape[0]
        D = np.empty((nq, k), dtype=np.float32)
        I = np.empty((nq, k), dtype=np.int64)
        if nq == 0:
            return D, I
        sub = self.subset(sel)
        try:
            flags = native.LS_FLAG_NORMALIZE if normalize else 0
            native.check(native.load().ls_search_subset(self._handle, sub.id, native.addr(x), nq, k, flags,
                                                        native.addr(D), native.addr(I)))
        finally:
            if sub is not sel:
                sub.close()
        return D, I

    def range_search(self, x: np.ndarray, radius: float, *, normalize: bool = False, params=None
                     ) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """index.range_search(x, radius): every row whose score is strictly above ``radius`` (ls_range_search,
        include/leansearch_range.h).

        x: float32 [nq, d]. Returns ``(lims, D, I)`` as faiss does: ``lims`` uint64 [nq + 1], and query ``i`` owns
        ``D[lims[i]:lims[i + 1]]`` (float32 scores, bit for bit the single-query scan's) and ``I[lims[i]:lims[i + 1]]``
        (int64 rows + base, ASCENDING - faiss leaves the order open). NaN and -FLT_MAX scores are never returned;
        ``radius=-inf`` returns every other row, ``+inf`` or NaN none. An L2 index returns every row whose squared
        distance is strictly BELOW ``radius`` and D holds distances (``+inf``: every valid row; ``<= 0``, NaN: none). ``params.sel`` works as in :meth:`search`: a
        :class:`RowSubset` of this index, or any selector / mask (a subset for this call only). The arrays are copies.
        A sharded or replicated index refuses the call (ValueError).
        """
        x = np.ascontiguousarray(x, dtype=np.float32)
        if x.ndim != 2 or x.shape[1] != self.d:
            raise ValueError(f"range_search expects [nq, {self.d}] float32, got {x.shape}")
        sel = getattr(params, "sel", None) if params is not None else None
        nq = x.shape[0]
        if nq == 0:
            return _empty_range_result()
        flags = native.LS_FLAG_NORMALIZE if normalize else 0
        res = ctypes.c_void_p()
        lib = native.load()
        if sel is None:
            h = self._handle if self._handle is not None else self._ensure_built()
            native.check(lib.ls_range_search(h, native.addr(x), nq, float(radius), flags, ctypes.byref(res)))
            return take_range_result(lib, res)
        sub = self.subset(sel)
        try:
            native.check(lib.ls_range_search_subset(self._handle, sub.id, native.addr(x), nq, float(radius), flags,
                                                    ctypes.byref(res)))
            return take_range_result(lib, res)
        finally:
            if sub is not sel:
                sub.close()

    def search_device(self, q, k: int, out_scores=None, out_indices=None, *,
                      normalize: bool = False, asynchronous: bool = False,
                      pipeline: bool = False, inorder: bool = False, stream=None):
        """Search with torch CUDA tensors (queries and results stay in HBM).

        q: float32 CUDA tensor [nq, d]. Work is queued on ``stream`` (default: torch's current
        stream). Returns (scores float32 [nq, k], indices int64 [nq, k]) CUDA tensors.
        ``asynchronous``: queue and return, results ordered on the stream. For ANY batched call
        (the speculative MFMA paths: nq > 16 on an fp16 index, nq > 32 on an fp32 index) call
        :meth:`check` before trusting them: it repairs the rare query the speculative threshold
        short-changed, re-writing its rows of the output tensors (keep those alive until then;
        ``q`` may be reused at once in stream order). On a sharded index (``devices=[...]``) ``q``
        and the outputs live on ``devices[0]``.
        ``pipeline``: queue on the index's internal lanes so consecutive calls overlap; results
        are valid only after :meth:`check` (scan-path launches write no score vectors: a query whose
        selection could not prove its result complete is served again in place there). ``inorder``
        (LS_FLAG_INORDER): the caller consumes pipelined scan-path results on the GPU before
        :meth:`check`; launches then keep their score vectors and are exact in the lanes' order.
        """
        if self._metric == native.LS_METRIC_L2:
            raise ValueError("search_device: an L2 index answers through search() / range_search() (host arrays)")
        import torch

        if not (q.is_cuda and q.dtype == torch.float32 and q.dim() == 2 and q.is_contiguous()
                and q.shape[1] == self.d):
            raise ValueError(f"search_device expects a contiguous float32 CUDA tensor [nq, {self.d}]")
        nq = q.shape[0]
        if out_scores is None:
            out_scores = torch.empty((nq, k), dtype=torch.float32, device=q.device)
        if out_indices is None:
            out_indices = torch.empty((nq, k), dtype=torch.int64, device=q.device)
        h = self._ensure_built()
        s = stream if stream is not None else torch.cuda.current_stream(q.device)
        flags = (native.LS_FLAG_NORMALIZE if normalize else 0) | \
                (native.LS_FLAG_ASYNC if asynchronous else 0) | \
                (native.LS_FLAG_PIPELINE if pipeline else 0) | \
                (native.LS_FLAG_INORDER if inorder else 0)
        native.check(native.load().ls_search_device(h, q.data_ptr(), nq, int(k), flags,
                                                    out_scores.data_ptr(), out_indices.data_ptr(),
                                                    s.cuda_stream))
        return out_scores, out_indices

    def export_flags(self, dst, stream=None) -> None:
        """Copy the per-query verification flags (uint32/int32 CUDA tensor [nq]) of the most
        recent search queued on this index, in stream order (see ls_export_flags)."""
        import torch

        if not (dst.is_cuda and dst.dim() == 1 and dst.element_size() == 4 and dst.is_contiguous()):
            raise ValueError("export_flags expects a contiguous 32-bit CUDA tensor [nq]")
        s = stream if stream is not None else torch.cuda.current_stream(dst.device)
        native.check(native.load().ls_export_flags(self._ensure_built(), dst.data_ptr(),
                                                   dst.shape[0], s.cuda_stream))

    def check(self, stream=None) -> None:
        """Synchronise and validate async searches (see ls_check)."""
        import torch

        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        native.check(native.load().ls_check(self._ensure_built(), s.cuda_stream))

    # ------------------------------------------------------------------ instrumentation
    def set_profiling(self, enabled: bool) -> None:
        native.check(native.load().ls_set_profiling(self._ensure_built(), 1 if enabled else 0))

    def last_kernel_ms(self) -> tuple[float, float]:
        a, b = ctypes.c_float(), ctypes.c_float()
        native.check(native.load().ls_last_kernel_ms(self._ensure_built(), ctypes.byref(a),
                                                     ctypes.byref(b)))
        return a.value, b.value

    def debug_option(self, which: int, value: int) -> None:
        native.check(native.load().ls_debug_option(self._ensure_built(), which, value))

    def debug_counter(self, which: int) -> int:
        return int(native.load().ls_debug_counter(self._ensure_built(), which))

    def debug_scores(self) -> np.ndarray:
        """Score vector S of the most recent per-query scan (test hook)."""
        out = np.empty(self._ntotal, dtype=np.float32)
        native.check(native.load().ls_debug_read_scores(self._ensure_built(), out.ctypes.data,
                                                        out.size))
        return out

    def close(self) -> None:
        self._drop_handle()

    def __del__(self):
        try:
            self._drop_handle()
        except Exception:
            pass


class FlatL2Index(FlatIPIndex):
    """``FlatIPIndex(..., metric="l2")`` under faiss's name for it: exact squared-distance search
    (include/leansearch_l2.h). The metric is fixed; everything else is the parent's."""

    _default_metric = "l2"

    def _check_metric(self, metric: Any, devices: Any) -> int:
        code = super()._check_metric(metric, devices)
        if code != native.LS_METRIC_L2:
            raise ValueError("FlatL2Index is an L2 index (use FlatIPIndex for the inner product)")
        return code


class RowSubset:
    """A row subset uploaded once to its index (``FlatIPIndex.subset``): pass it as ``params.sel`` to search it
    without another upload. Holds its index; freed by ``close()``, by garbage collection, or with the index's
    handle (after which it is invalid)."""

    def __init__(self, index: FlatIPIndex, sid: int, rows: int):
        self.index = index
        self._id = sid
        self._gen = index._handle_gen
        self._rows = int(rows)  # selected rows, as last known

    @property
    def rows(self) -> int:
        """The rows the subset covers now (ls_subset_rows: ``remove_ids`` on the index shrinks it); the last known
        count once the subset is closed or its index's handle is gone."""
        if self.valid:
            rows = ctypes.c_int64()
            native.check(native.load().ls_subset_rows(self.index._handle, self._id, ctypes.byref(rows)))
            self._rows = int(rows.value)
        return self._rows

    @property
    def valid(self) -> bool:
        return self._id is not None and self.index._handle is not None and self.index._handle_gen == self._gen

    @property
    def id(self) -> int:
        if not self.valid:
            raise ValueError("this RowSubset was closed, or its index's handle was dropped")
        return self._id

    @property
    def sel(self) -> "RowSubset":  # lets a RowSubset stand where faiss expects SearchParameters
        return self

    def close(self) -> None:
        if self.valid:
            native.check(native.load().ls_subset_destroy(self.index._handle, self._id))
        self._id = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
