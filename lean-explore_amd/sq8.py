"""The sq8 storage dtype restated on the host in numpy (include/leansearch_sq8.h).

``train_step`` / ``encode`` / ``decode`` are the definition of the step, the codes and the reconstructed rows: the
library's kernels must agree with them bit for bit (tests/test_sq8_gpu.py). Signed symmetric int8 codes with one float32
step per dimension - NOT faiss's ``QT_8bit`` (unsigned affine codes).
"""

from __future__ import annotations

import numpy as np


def train_step(x: np.ndarray) -> np.ndarray:
    """step[i] = max |x[:, i]| over the finite values / 127 (float32 division); 1 where that maximum is 0."""
    x = np.asarray(x, dtype=np.float32)
    if x.ndim != 2:
        raise ValueError("train_step expects [n, d]")
    a = np.where(np.isfinite(x), np.abs(x), np.float32(0)).astype(np.float32)
    amax = a.max(axis=0) if x.shape[0] else np.zeros(x.shape[1], np.float32)
    step = (amax / np.float32(127.0)).astype(np.float32)
    return np.where(amax > 0, step, np.float32(1.0)).astype(np.float32)


def encode(x: np.ndarray, step: np.ndarray) -> np.ndarray:
    """c = clamp(rint(x / step), -127, 127) in float32 (ties to even); NaN -> 0, +-inf -> +-127. int8 [n, d]."""
    x = np.asarray(x, dtype=np.float32)
    step = np.asarray(step, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        r = np.rint((x / step).astype(np.float32))
    r = np.where(np.isnan(x), np.float32(0), np.clip(r, np.float32(-127), np.float32(127)))
    return r.astype(np.int8)


def decode(codes: np.ndarray, step: np.ndarray) -> np.ndarray:
    """(float)c * step: one float32 multiply. float32 [n, d]."""
    return (np.asarray(codes).astype(np.float32) * np.asarray(step, dtype=np.float32)).astype(np.float32)
