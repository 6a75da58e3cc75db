"""Row selectors with faiss's semantics (``faiss.IDSelectorRange`` / ``IDSelectorBatch`` / ``IDSelectorBitmap``,
``faiss.SearchParameters(sel=...)``) and their conversion to the bitmap ``ls_subset_create`` takes: row ``r`` is
selected iff ``(bitmap[r >> 3] >> (r & 7)) & 1``. Host-side only; the search itself runs in libleansearch.
"""

from __future__ import annotations

import numpy as np


def _swig_pair(args: tuple, what: str) -> np.ndarray:
    """``(array)`` or faiss's swig-style ``(n, array)`` -> the first n entries of the array."""
    if len(args) == 1:
        return np.asarray(args[0])
    if len(args) == 2:
        n = int(args[0])
        a = np.asarray(args[1]).reshape(-1)
        if n < 0 or n > a.size:
            raise ValueError(f"{what}: n = {n} does not fit an array of {a.size}")
        return a[:n]
    raise ValueError(f"{what} takes (array) or (n, array)")


class IDSelectorRange:
    """Rows ``imin <= r < imax``."""

    def __init__(self, imin: int, imax: int):
        self.imin, self.imax = int(imin), int(imax)

    def bitmap(self, ntotal: int) -> np.ndarray:
        mask = np.zeros(ntotal, dtype=bool)
        lo, hi = max(self.imin, 0), min(self.imax, ntotal)
        if lo < hi:
            mask[lo:hi] = True
        return _pack(mask)


class IDSelectorBatch:
    """The rows named in ``ids`` (unsorted and duplicated ids allowed; out-of-range ids select nothing)."""

    def __init__(self, *args):
        ids = _swig_pair(args, "IDSelectorBatch")
        if ids.size and not np.issubdtype(ids.dtype, np.integer):
            raise ValueError("IDSelectorBatch expects integer ids")
        self.ids = ids.astype(np.int64).reshape(-1)

    def bitmap(self, ntotal: int) -> np.ndarray:
        return _pack(mask_from_ids(self.ids, ntotal))


class IDSelectorBitmap:
    """faiss's bitmap: row ``r`` selected iff ``r >> 3 < n`` and bit ``r & 7`` of byte ``r >> 3`` is set."""

    def __init__(self, *args):
        bm = _swig_pair(args, "IDSelectorBitmap")
        if bm.dtype != np.uint8:
            raise ValueError("IDSelectorBitmap expects a uint8 bitmap")
        self.bitmap_bytes = np.ascontiguousarray(bm.reshape(-1))

    def bitmap(self, ntotal: int) -> np.ndarray:
        return self.bitmap_bytes  # bits past ntotal are ignored, a short bitmap selects nothing past its end


class SearchParameters:
    """``faiss.SearchParameters(sel=...)``."""

    def __init__(self, sel=None):
        self.sel = sel


class SearchParametersIVF(SearchParameters):
    """``faiss.SearchParametersIVF(sel=..., nprobe=...)``: every row is searched exactly, nprobe is kept only."""

    def __init__(self, sel=None, nprobe: int = 1):
        super().__init__(sel)
        self.nprobe = int(nprobe)


def _pack(mask: np.ndarray) -> np.ndarray:
    return np.packbits(mask.astype(bool, copy=False), bitorder="little")


def mask_from_ids(ids, ntotal: int) -> np.ndarray:
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    mask = np.zeros(ntotal, dtype=bool)
    ok = ids[(ids >= 0) & (ids < ntotal)]
    mask[ok] = True
    return mask


def to_bitmap(sel, ntotal: int) -> np.ndarray:
    """A selector, a bool mask ``[ntotal]`` or an integer array of row ids -> uint8 bitmap bytes."""
    if hasattr(sel, "bitmap") and callable(sel.bitmap):
        return np.ascontiguousarray(sel.bitmap(ntotal), dtype=np.uint8)
    a = np.asarray(sel)
    if a.dtype == bool:
        if a.shape != (ntotal,):
            raise ValueError(f"a bool mask must have shape ({ntotal},), got {a.shape}")
        return _pack(a)
    if a.ndim == 1 and (a.size == 0 or np.issubdtype(a.dtype, np.integer)):
        return _pack(mask_from_ids(a, ntotal))
    raise ValueError("a row selection is a faiss-style selector, a bool mask [ntotal] or an int array of row ids")
