"""bfloat16 storage (include/leansearch_bf16.h, LS_DTYPE_BF16) restated on the host, numpy only.

``encode`` is the library's encode kernel bit for bit (round to nearest even; NaN keeps its sign and top payload bits and
is made quiet; finite values above the largest bf16 become +-inf; subnormals and -0 are kept), ``decode`` is the exact
widening ``bits << 16``. The tests hold the GPU's stored rows to these; the product does not need them.
"""

from __future__ import annotations

import numpy as np


def encode(x) -> np.ndarray:
    """float32 array -> bfloat16 bit patterns, uint16, same shape."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    nan = (u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    rounded = (u.astype(np.uint64) + 0x7FFF + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint64(16)
    return np.where(nan, (u >> np.uint32(16)) | np.uint32(0x0040), rounded.astype(np.uint32)).astype(np.uint16)


def decode(bits) -> np.ndarray:
    """bfloat16 bit patterns (uint16) -> the float32 values they stand for, exactly."""
    b = np.ascontiguousarray(bits, dtype=np.uint16)
    return (b.astype(np.uint32) << np.uint32(16)).view(np.float32)


def inexact(x) -> int:
    """Elements of ``x`` that encode() changes (NaN never counts): what ``bf16_inexact`` reports for rows ``x``."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    return int(((decode(encode(x)).view(np.uint32) != x.view(np.uint32)) & ~np.isnan(x)).sum())
