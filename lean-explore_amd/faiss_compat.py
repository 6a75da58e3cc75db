"""The slice of the `faiss` module surface that LeanExplore's local backend uses
(reference src/lean_explore/search/engine.py:156-159,240-250), served by the HIP library:

    import lean_explore_amd.faiss_compat as faiss
    index = faiss.read_index(path); faiss.normalize_L2(x); D, I = index.search(x, k)

Index files. `write_index` / `read_index` speak FAISS's own container for flat indexes (fourcc ``IxFI``
inner product, ``IxF2`` L2: `IndexFlatL2`) and `read_index` also accepts the IVF-flat container the reference ships
(fourcc ``IwFl``, reference src/lean_explore/extract/index.py:103-104,173): the inverted lists are
scattered back to add order and searched exactly (what IVF approximates) - or, with ``ivf=True``, kept
together with the file's centroids and searched as IVF (`lean_explore_amd.ivf.IVFFlatIndex`: probe ``nprobe``
lists, scan only their rows; a subset-search result by this library's definitions, not a copy of faiss's bits).
`write_index` of such an index writes ``IwFl`` back (centroids, lists, ``nprobe``): the file the reference's engine loads.
The byte layout is
restated from upstream faiss's index_write.cpp; no faiss-written file exists in this image, so it
is checked by writer/reader round trips only — UNVERIFIED against real faiss files.
"""

from __future__ import annotations

import struct
from pathlib import Path

import numpy as np

from . import native
from .index import FlatIPIndex, FlatL2Index, _dtype_code, normalize_L2, switch_refusal  # noqa: F401  (re-exported)
from .ivf import IVFFlatIndex
from .id_selectors import (IDSelectorBatch, IDSelectorBitmap, IDSelectorRange,  # noqa: F401  (re-exported)
                        SearchParameters, SearchParametersIVF)

METRIC_INNER_PRODUCT = 0
METRIC_L2 = 1
# faiss.ScalarQuantizer.QT_* (only QT_8bit is served, by the library's own sq8 codes)
QT_8bit, QT_4bit, QT_8bit_uniform, QT_4bit_uniform, QT_fp16, QT_8bit_direct, QT_6bit = range(7)


class IndexFlatIP(FlatIPIndex):
    """faiss.IndexFlatIP(d) (reference extract/index.py:103). ``subset_small_batch=True``: groups of 2..16 queries of a
    search with ``SearchParameters(sel=...)`` share one pass over the selected rows (same results, bit for bit;
    FlatIPIndex(subset_small_batch=True)). ``remove_ids(sel)`` drops rows (``ls_remove``: the stored rows are compacted
    in place in HBM) and returns their number; the survivors are renumbered densely, as ``faiss.IndexFlat.remove_ids``
    renumbers them (old row ``r`` becomes ``r`` minus the removed rows below it). ``write_index`` afterwards writes the
    survivors."""

    def __init__(self, d: int, dtype="f32", device: int = 0, subset_small_batch: bool = False):
        super().__init__(d, dtype=dtype, device=device, subset_small_batch=subset_small_batch)


class IndexFlatL2(FlatL2Index):
    """faiss.IndexFlatL2(d): exact squared-distance search (include/leansearch_l2.h). ``search`` returns squared L2
    distances, smallest first, ties by row, padding ``(+FLT_MAX, -1)``; ``range_search(x, radius)`` every row with
    distance ``< radius``, rows ascending. ``add``, ``remove_ids``, ``SearchParameters(sel=...)`` as on
    :class:`IndexFlatIP`. fp32 or fp16 rows on one device; ``write_index`` writes fourcc ``IxF2``.
    ``l2_small_batch=True``: the queries of a ``search`` go out in groups of 8 / 4 / 1 that share one corpus pass (same
    results, bit for bit; FlatL2Index(l2_small_batch=True), include/leansearch_l2_batch.h)."""

    def __init__(self, d: int, dtype="f32", device: int = 0, l2_small_batch: bool = False):
        super().__init__(d, dtype=dtype, device=device, l2_small_batch=l2_small_batch)


def IndexFlat(d: int, metric: int = METRIC_L2, dtype="f32", device: int = 0, l2_small_batch: bool = False):
    """faiss.IndexFlat(d, metric): an :class:`IndexFlatIP` or an :class:`IndexFlatL2` (faiss's default metric;
    ``l2_small_batch`` is the L2 index's option)."""
    if metric == METRIC_INNER_PRODUCT:
        if l2_small_batch:  # (IndexFlatIP has no such keyword; the words are this function's, about its own argument)
            raise ValueError("l2_small_batch needs METRIC_L2")
        return IndexFlatIP(d, dtype=dtype, device=device)
    if metric == METRIC_L2:
        return IndexFlatL2(d, dtype=dtype, device=device, l2_small_batch=l2_small_batch)
    raise ValueError("only METRIC_INNER_PRODUCT and METRIC_L2 are supported")


class IndexIVFFlat(FlatIPIndex):
    """faiss.IndexIVFFlat(quantizer, d, nlist, metric) as the reference's index builder drives it
    (reference src/lean_explore/extract/index.py:103-116: construct, ``train``, ``add``;
    ``nprobe`` is set by the engine, search/engine.py:247-248). There is nothing to train: the
    rows are searched exactly, i.e. the answer IVF approximates; ``nlist`` / ``nprobe`` are kept
    as plain attributes. ``write_index`` stores it in the flat container. ``remove_ids(sel)`` on this flat-backed
    default drops rows in place in HBM (``ls_remove``) and renumbers the survivors densely, as
    ``faiss.IndexFlat.remove_ids`` renumbers them.

    ``ivf=True`` (opt-in) returns an :class:`~lean_explore_amd.ivf.IVFFlatIndex` instead, which honours ``train``,
    ``nprobe`` and ``SearchParametersIVF(nprobe=)``; with ``build_on_device=True`` its ``train`` and the lists of its
    ``add`` are computed by the GPU build kernels (same centroids and lists), and ``write_index`` writes ``IwFl``.
    ``add`` after a search merges the rows into the built lists on the GPU (``ls_ivf_add``): same index as one build.
    ``remove_ids(sel)`` drops rows (``ls_ivf_remove``: the lists are compacted on the GPU) and returns their number.
    The survivors are RENUMBERED densely, as ``faiss.IndexFlat.remove_ids`` renumbers them (old row ``r`` becomes ``r``
    minus the removed rows below it) - the ids are not kept as ``faiss.IndexIVFFlat.remove_ids`` keeps them: here an id
    is a row position. ``write_index`` / ``read_index(path, ivf=True)`` round-trip the compacted index.
    ``ivf_small_batch=True`` (fp32 rows): groups of 2..16 queries of a search share one pass over the lists they probe
    (same results, bit for bit; IVFFlatIndex(small_batch=True))."""

    def __new__(cls, quantizer=None, d: int = 0, nlist: int = 0, metric: int = METRIC_INNER_PRODUCT,
                dtype="f32", device: int = 0, ivf: bool = False, build_on_device: bool = False,
                ivf_small_batch: bool = False):
        if build_on_device and not ivf:
            raise ValueError("build_on_device builds an IVF index: pass ivf=True")
        if ivf_small_batch and not ivf:
            raise ValueError("ivf_small_batch is an option of the IVF index: pass ivf=True")
        if ivf:
            if metric != METRIC_INNER_PRODUCT:
                raise ValueError("only METRIC_INNER_PRODUCT is supported")
            # (not a cls instance: __init__ is skipped)
            return IVFFlatIndex(d, nlist, dtype=dtype, device=device, build_on_device=build_on_device,
                                small_batch=ivf_small_batch)
        return super().__new__(cls)

    def __init__(self, quantizer, d: int, nlist: int, metric: int = METRIC_INNER_PRODUCT,
                 dtype="f32", device: int = 0, ivf: bool = False, build_on_device: bool = False,
                 ivf_small_batch: bool = False):
        if metric != METRIC_INNER_PRODUCT:
            raise ValueError("only METRIC_INNER_PRODUCT is supported")
        super().__init__(d, dtype=dtype, device=device)
        self.quantizer, self.nlist, self.nprobe, self.is_trained = quantizer, int(nlist), 1, False

    def train(self, x: np.ndarray) -> None:
        self.is_trained = True


def IndexIVFFlatL2(quantizer=None, d: int = 0, nlist: int = 0, dtype="f32", device: int = 0,
                   build_on_device: bool = False) -> IVFFlatIndex:
    """faiss.IndexIVFFlat(faiss.IndexFlatL2(d), d, nlist) - faiss's default IVF index - as an
    :class:`~lean_explore_amd.ivf.IVFFlatIndex` with ``metric="l2"`` (include/leansearch_ivf_l2.h): ``train``, ``add``,
    ``nprobe`` / ``SearchParametersIVF(nprobe=)``, ``search`` (squared distances, smallest first, padding
    ``(+FLT_MAX, -1)``), ``range_search``, ``remove_ids``, subsets. fp32 or fp16 rows. ``quantizer`` is accepted for the
    call's shape only: the index keeps its own exact L2 quantiser. ``write_index`` writes ``IwFl`` with ``METRIC_L2`` and
    a nested ``IxF2`` quantiser; ``read_index(path, ivf=True)`` reads it back."""
    return IVFFlatIndex(d, nlist, dtype=dtype, device=device, build_on_device=build_on_device, metric="l2")


class IndexScalarQuantizer(FlatIPIndex):
    """The shape of ``faiss.IndexScalarQuantizer(d, faiss.ScalarQuantizer.QT_8bit, faiss.METRIC_INNER_PRODUCT)``: a
    thin alias of ``FlatIPIndex(d, dtype="sq8")``. NOT faiss's QT_8bit arithmetic (unsigned affine codes, faiss's own
    decode): the codes are the library's signed symmetric sq8 codes (lean_explore_amd/sq8.py), parity with faiss is
    unpinned. ``train(x)`` fixes the step from ``x``; without it the step is trained from the rows added before
    the first search. ``sq8_small_batch=True``: 2..16 queries share one pass over the codes (same results, bit for
    bit; FlatIPIndex(sq8_small_batch=True)). ``remove_ids(sel)`` drops rows (``ls_remove``: the stored codes are moved
    in place in HBM, never re-encoded, and the step stays) and renumbers the survivors densely, as
    ``faiss.IndexFlat.remove_ids`` renumbers them."""

    def __init__(self, d: int, qtype: int = QT_8bit, metric: int = METRIC_INNER_PRODUCT, device: int = 0,
                 sq8_small_batch: bool = False):
        if qtype != QT_8bit:
            raise ValueError("only QT_8bit is supported (served by the library's sq8 codes)")
        if metric != METRIC_INNER_PRODUCT:
            raise ValueError("only METRIC_INNER_PRODUCT is supported")
        super().__init__(d, dtype="sq8", device=device, sq8_small_batch=sq8_small_batch)
        self.is_trained = False

    def train(self, x: np.ndarray) -> None:
        from . import sq8

        if self._handle is not None:
            raise ValueError("the device index is built: its step is fixed")
        x = np.ascontiguousarray(x, dtype=np.float32)
        if x.ndim != 2 or x.shape[1] != self.d:
            raise ValueError(f"train expects [n, {self.d}] float32")
        self._sq8_step = sq8.train_step(x)
        self.is_trained = True


def get_num_gpus() -> int:
    """faiss.get_num_gpus(): 0, so callers take their CPU-index code path (extract/index.py:106);
    the rows go to HBM when the index is first searched either way."""
    return 0


# ------------------------------------------------------------------ container format helpers
def _fourcc(s: str) -> int:
    return struct.unpack("<I", s.encode("ascii"))[0]


def _write_header(f, d: int, ntotal: int, metric: int) -> None:
    # write_index_header: d (int32), ntotal (int64), two dummy int64 (1 << 20), is_trained (u8),
    # metric_type (int32)
    f.write(struct.pack("<iqqqBi", d, ntotal, 1 << 20, 1 << 20, 1, metric))


def _read_header(f) -> tuple[int, int, int]:
    d, ntotal, _, _, _, metric = struct.unpack("<iqqqBi", f.read(4 + 8 + 8 + 8 + 1 + 4))
    if metric > 1:
        f.read(4)  # metric_arg
    return d, ntotal, metric


def _read_vector(f, dtype, what: str) -> np.ndarray:
    (count,) = struct.unpack("<Q", f.read(8))
    itemsize = np.dtype(dtype).itemsize
    raw = f.read(count * itemsize)
    if len(raw) != count * itemsize:
        raise ValueError(f"truncated index file while reading {what}")
    return np.frombuffer(raw, dtype=dtype, count=count)


def _read_flat_payload(f) -> tuple[int, np.ndarray]:
    d, ntotal, _ = _read_header(f)
    xb = _read_vector(f, "<f4", "flat storage")  # count is in floats (xb / codes/4)
    if xb.size != d * ntotal:
        raise ValueError("flat index: storage size does not match d * ntotal")
    return d, xb.reshape(ntotal, d).astype(np.float32, copy=True)


def write_index(index: FlatIPIndex, path: str | Path, *, allow_lossy: bool = False) -> None:
    """faiss.write_index for a flat index: container ``IxFI`` (inner product) or ``IxF2`` with ``METRIC_L2`` in the
    header (an L2 index: ``FlatIPIndex(metric="l2")``, :class:`IndexFlatL2`).

    A built fp16 index holds only the ROUNDED rows in HBM (no host copy is kept), so the file
    would not round-trip the float32 embeddings that were added and would score differently in
    the reference's faiss: refused unless ``allow_lossy=True``.

    A bf16 index writes its decoded rows; that needs ``allow_lossy=True`` only when ``bf16_inexact != 0`` (with 0 the
    file holds exactly what was added).

    An :class:`~lean_explore_amd.ivf.IVFFlatIndex` is written as ``IwFl`` (see ``_write_ivf_flat``)."""
    if isinstance(index, IVFFlatIndex):
        return _write_ivf_flat(index, path, allow_lossy)
    if getattr(index, "storage_dtype", "f32") == "sq8" and not allow_lossy:
        raise ValueError("write_index on an sq8 index would write the decoded 8-bit rows (as a flat IxFI file), not "
                         "the float32 embeddings that were added; pass allow_lossy=True to do that")
    if (getattr(index, "storage_dtype", "f32") == "f16" and getattr(index, "_handle", None) is not None
            and not allow_lossy):
        raise ValueError("write_index on a built fp16 index would write fp16-rounded rows, not the "
                         "float32 embeddings that were added; pass allow_lossy=True to do that, or "
                         "write the index before the first search / from an f32 index")
    if getattr(index, "storage_dtype", "f32") == "bf16":
        # the decoded rows (f32): exactly what was added when every added value was bf16-valued (bf16_inexact == 0)
        if index.bf16_inexact != 0 and not allow_lossy:
            raise ValueError(f"write_index on a bf16 index that rounded {index.bf16_inexact} of the added values would "
                             "write the bf16-rounded rows, not the float32 embeddings that were added; pass "
                             "allow_lossy=True to do that")
    if getattr(index, "storage_dtype", "f32") == "sq8":
        index._ensure_built()  # (the decoded rows: what a search of this index scores)
    corpus = np.ascontiguousarray(index.host_corpus(), dtype="<f4")
    l2 = getattr(index, "metric", "ip") == "l2"
    with open(path, "wb") as f:
        f.write(struct.pack("<I", _fourcc("IxF2" if l2 else "IxFI")))
        _write_header(f, index.d, corpus.shape[0], METRIC_L2 if l2 else METRIC_INNER_PRODUCT)
        f.write(struct.pack("<Q", corpus.size))
        f.write(corpus.tobytes())


def _write_ivf_flat(index: IVFFlatIndex, path: str | Path, allow_lossy: bool) -> None:
    """faiss.write_index for an IVF-flat index (container ``IwFl``), the layout ``_read_ivf_flat`` parses: header,
    nlist, nprobe, the nested ``IxFI`` quantiser holding the centroids (an L2 index: ``METRIC_L2`` in both headers and a
    nested ``IxF2`` quantiser), direct map type 0 with an empty
    vector, ``ilar`` / nlist / 4 d, ``full`` list sizes, then per non-empty list its rows and its int64 ids ascending.
    Rows and lists come from the buffers while the index is unbuilt and every ``add`` named its lists; otherwise the
    index is built first and read back (``assignment()``, ``reconstruct_n``). fp16 / sq8 storage holds other values
    than the float32 rows that were added: refused unless ``allow_lossy=True``; so is bf16 storage, but only where
    ``bf16_inexact != 0`` (with 0 the file holds exactly what was added)."""
    if not index.is_trained:
        raise ValueError("write_index: the IVF index is not trained (train or set_centroids first)")
    if index.storage_dtype == "bf16" and not allow_lossy and index.bf16_inexact == 0:
        pass  # (every added value was bf16-valued: the stored rows ARE the rows that were added)
    elif index.storage_dtype != "f32" and not allow_lossy:
        raise ValueError(f"write_index on an IVF index of {index.storage_dtype} rows would write the stored values, not "
                         "the float32 embeddings that were added; pass allow_lossy=True to do that")
    d, nlist = index.d, index.nlist
    centroids = np.ascontiguousarray(index.centroids, dtype="<f4")
    if index._handle is None and (index._assign is not None or index.ntotal == 0) and index.storage_dtype == "f32":
        corpus = index.reconstruct_n(0, index.ntotal)  # (the buffered rows)
        assign = (np.concatenate(index._assign).astype(np.int32) if index._assign else np.zeros(0, np.int32))
    else:
        assign = index.assignment()  # (builds the device index)
        corpus = index.reconstruct_n(0, index.ntotal)
    corpus = np.ascontiguousarray(corpus, dtype="<f4")
    l2 = index.metric == "l2"
    metric = METRIC_L2 if l2 else METRIC_INNER_PRODUCT
    with open(path, "wb") as f:
        f.write(struct.pack("<I", _fourcc("IwFl")))
        _write_header(f, d, corpus.shape[0], metric)
        f.write(struct.pack("<QQ", nlist, int(index.nprobe)))
        f.write(struct.pack("<I", _fourcc("IxF2" if l2 else "IxFI")))
        _write_header(f, d, nlist, metric)
        f.write(struct.pack("<Q", nlist * d))
        f.write(centroids.tobytes())
        f.write(struct.pack("<b", 0))  # direct map: none
        f.write(struct.pack("<Q", 0))
        f.write(struct.pack("<I", _fourcc("ilar")))
        f.write(struct.pack("<QQ", nlist, 4 * d))
        f.write(struct.pack("<I", _fourcc("full")))
        f.write(struct.pack("<Q", nlist))
        f.write(np.bincount(assign, minlength=nlist).astype("<u8").tobytes())
        order = np.argsort(assign, kind="stable")  # list after list, ascending row inside a list
        starts = np.concatenate(([0], np.cumsum(np.bincount(assign, minlength=nlist)))).astype(np.int64)
        for li in range(nlist):
            ids = order[starts[li]:starts[li + 1]].astype("<i8")
            if ids.size:
                f.write(corpus[ids].tobytes())
                f.write(ids.tobytes())


def read_index(path: str | Path, dtype="f32", device: int = 0, devices=None,
               replicate: bool = False, f16_small_batch: bool = False, ivf: bool = False,
               sq8_small_batch: bool = False, ivf_small_batch: bool = False, l2_small_batch: bool = False):
    """faiss.read_index (reference search/engine.py:159) -> exact HIP index (``devices``: row-sharded
    over several GPUs inside this process). A top-level ``IxF2`` file gives an :class:`IndexFlatL2` (one device, none
    of the inner product's small-batch options; ``l2_small_batch=True`` switches its query groups on, and is refused
    for every other container). ``ivf=True`` (``IwFl`` files only, one device): an
    :class:`~lean_explore_amd.ivf.IVFFlatIndex` with the file's centroids (the nested quantiser's rows), the file's
    lists and the file's ``nprobe`` - an L2 one (``metric == "l2"``) where the file's header says ``METRIC_L2``;
    ``ivf_small_batch=True`` switches its small-batch pass on (fp32 rows, inner product). Without ``ivf=True`` an L2
    ``IwFl`` file is refused: its rows would be searched under the wrong metric."""
    path = Path(path)
    if ivf_small_batch and not ivf:
        raise ValueError("ivf_small_batch is an option of the IVF index: pass ivf=True")
    if ivf_small_batch and (refusal := switch_refusal("ivf", "ip", dtype)):  # (the file's metric: asked below)
        raise ValueError(f"ivf_small_batch: {refusal}")
    if ivf and (devices is not None or replicate or f16_small_batch or sq8_small_batch):
        raise ValueError("read_index(ivf=True) builds a single-device IVF index (no devices / replicate / "
                         "f16_small_batch / sq8_small_batch)")
    with open(path, "rb") as f:
        (cc,) = struct.unpack("<I", f.read(4))
        if l2_small_batch and cc != _fourcc("IxF2"):
            raise ValueError(f"{path}: l2_small_batch is an option of a flat L2 (IxF2) index")
        if cc == _fourcc("IxFI"):
            if ivf:
                raise ValueError(f"{path}: a flat (IxFI) file has no centroids or lists to search as IVF")
            d, corpus = _read_flat_payload(f)
        elif cc == _fourcc("IxF2"):
            if ivf:
                raise ValueError(f"{path}: a flat (IxF2) file has no centroids or lists to search as IVF")
            if devices is not None or replicate or f16_small_batch or sq8_small_batch:
                raise ValueError(f"{path}: an L2 (IxF2) index is built on one device, without devices / replicate / "
                                 "f16_small_batch / sq8_small_batch")
            d, corpus = _read_flat_payload(f)
            index = IndexFlatL2(d, dtype=dtype, device=device, l2_small_batch=l2_small_batch)
            if corpus.shape[0]:
                index.add(corpus)
            return index
        elif cc == _fourcc("IwFl"):
            if ivf:
                d, corpus, centroids, assign, nprobe, metric = _read_ivf_flat(f, keep_lists=True, any_metric=True)
                if ivf_small_batch and (refusal := switch_refusal("ivf", metric, dtype)):  # (an L2 file: the caller's keyword)
                    raise ValueError(f"{path}: ivf_small_batch: {refusal}")
                index = IVFFlatIndex(d, centroids.shape[0], dtype=dtype, device=device, small_batch=ivf_small_batch,
                                     metric="l2" if metric == METRIC_L2 else "ip")
                index.set_centroids(centroids)
                index.add(corpus, assign=assign)
                index.nprobe = max(int(nprobe), 1)
                return index
            d, corpus = _read_ivf_flat(f)
        else:
            tag = struct.pack("<I", cc).decode("ascii", "replace")
            raise ValueError(f"{path}: unsupported index container {tag!r} "
                             "(expected IxFI flat-IP, IxF2 flat-L2 or IwFl IVF-flat)")
    index = FlatIPIndex(d, dtype=dtype, device=device, devices=devices, replicate=replicate,
                        f16_small_batch=f16_small_batch, sq8_small_batch=sq8_small_batch)
    if corpus.shape[0]:
        index.add(corpus)
    return index


def _read_ivf_flat(f, keep_lists: bool = False, any_metric: bool = False):
    """IndexIVFFlat: ivf header, nested quantizer, direct map, ArrayInvertedLists (``ilar``). Returns (d, rows in add
    order), and with ``keep_lists`` also (centroids [nlist, d], list of every row int32 [ntotal], nprobe).
    ``any_metric`` (with ``keep_lists``): the header may say ``METRIC_L2`` too, and the metric is returned last."""
    d, ntotal, metric = _read_header(f)
    if metric != METRIC_INNER_PRODUCT and not (keep_lists and any_metric and metric == METRIC_L2):
        raise ValueError("IVF index is not an inner-product index")
    nlist, _nprobe = struct.unpack("<QQ", f.read(16))
    (qcc,) = struct.unpack("<I", f.read(4))  # nested coarse quantizer: its rows are the centroids
    if qcc not in (_fourcc("IxFI"), _fourcc("IxF2")):
        raise ValueError("IVF index: unsupported coarse quantizer container")
    qd, centroids = _read_flat_payload(f)
    if keep_lists and (qd != d or centroids.shape[0] != nlist):
        raise ValueError("IVF index: the coarse quantizer does not hold nlist centroids of dimension d")
    (dm_type,) = struct.unpack("<b", f.read(1))  # direct map
    _read_vector(f, "<i8", "direct map")
    if dm_type == 2:
        raise ValueError("IVF index: hashtable direct maps are not supported")
    (lcc,) = struct.unpack("<I", f.read(4))
    if lcc != _fourcc("ilar"):
        raise ValueError("IVF index: unsupported inverted-list container")
    nl, code_size = struct.unpack("<QQ", f.read(16))
    if nl != nlist or code_size != 4 * d:
        raise ValueError("IVF index: inverted lists do not match the header")
    (list_type,) = struct.unpack("<I", f.read(4))
    sizes = np.zeros(nlist, dtype=np.int64)
    raw = _read_vector(f, "<u8", "list sizes")
    if list_type == _fourcc("full"):
        sizes[:] = raw
    elif list_type == _fourcc("sprs"):
        sizes[raw[0::2].astype(np.int64)] = raw[1::2]
    else:
        raise ValueError("IVF index: unknown list-size encoding")
    corpus = np.zeros((ntotal, d), dtype=np.float32)
    seen = np.zeros(ntotal, dtype=bool)
    assign = np.zeros(ntotal, dtype=np.int32)
    for li, n in enumerate(sizes):
        n = int(n)
        if n == 0:
            continue
        codes = np.frombuffer(f.read(n * code_size), dtype="<f4").reshape(n, d)
        ids = np.frombuffer(f.read(n * 8), dtype="<i8")
        corpus[ids] = codes  # ids are the add-order row numbers (index.add without ids)
        seen[ids] = True
        assign[ids] = li
    if not seen.all():
        raise ValueError("IVF index: inverted lists do not cover every row")
    if keep_lists:
        if any_metric:
            return d, corpus, centroids, assign, int(_nprobe), metric
        return d, corpus, centroids, assign, int(_nprobe)
    return d, corpus
