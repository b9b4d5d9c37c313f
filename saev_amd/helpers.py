"""Looking at learned features: top-k helpers with the names, signatures and result shapes of the reference's ``saev.helpers``
(``NumpyTopK``, ``np_topk``, ``csr_topk``).

``csr_topk(arr, k=..., axis=0)`` answers "which k tokens fire latent j hardest" from the saved sparse ``token_acts.npz``.  It
streams the CSR's ``indptr`` / ``indices`` / ``data`` to the HIP device in row blocks and runs the exact per-latent select of
``saev_latent_topk_update`` (engine.LatentTopK); there is no CPU path for it.  ``axis=1`` and ``np_topk`` are small
vectorised numpy on the host.

Among equal values ``axis=0`` keeps the lower row (value descending, row ascending).  The reference's indices follow no fixed rule
there; its values are the same.
"""

from __future__ import annotations

import typing as tp

import numpy as np

# a row block grows past ``batch_size`` rows until it holds about this many stored entries: large enough that the launches of an
# update are noise, small enough that a block and its workspace stay a few tens of megabytes
_BLOCK_ENTRIES = 1 << 22
_MAX_ENTRIES = 2**31 - 1


class NumpyTopK(tp.NamedTuple):
    values: np.ndarray
    indices: np.ndarray


def _descending(a: np.ndarray) -> np.ndarray:
    """Positions along the last axis from the largest value to the smallest, equal values in ascending position (NaN counts as
    largest, as in torch).  Nothing is negated, so unsigned, boolean and the most negative integers order correctly: the
    stable ascending order of the mirrored axis, mirrored back."""
    n = a.shape[-1]
    mirrored = np.argsort(a[..., ::-1], axis=-1, kind="stable")
    return (n - 1) - mirrored[..., ::-1]


def np_topk(arr: np.ndarray, k: int, axis: int | None = None) -> NumpyTopK:
    """``torch.topk`` for numpy: the k largest elements along ``axis`` (None: of the flattened array), descending; among equal
    values the lower index comes first."""
    arr = np.asarray(arr)
    if arr.ndim == 0:
        raise ValueError("np_topk takes an array of at least one dimension")
    lines = arr.reshape(-1) if axis is None else np.moveaxis(arr, axis, -1)  # (an axis out of range raises numpy's AxisError)
    if not 0 <= k <= lines.shape[-1]:
        raise ValueError(f"k = {k} is out of range for {lines.shape[-1]} elements")
    picked = _descending(lines)[..., :k]
    values = np.take_along_axis(lines, picked, axis=-1)
    if axis is None:
        return NumpyTopK(values=values, indices=picked)
    return NumpyTopK(values=np.moveaxis(values, -1, axis), indices=np.moveaxis(picked, -1, axis))


def _csr_parts(arr):
    import scipy.sparse

    if not (scipy.sparse.issparse(arr) and arr.format == "csr"):
        raise TypeError(f"csr_topk takes a scipy CSR array or matrix, got {type(arr).__name__}")
    if arr.ndim != 2:
        raise ValueError(f"csr_topk takes a 2-D CSR array, got shape {arr.shape}")
    return np.asarray(arr.indptr), np.asarray(arr.indices), np.asarray(arr.data)


def _topk_axis1(arr, k: int) -> NumpyTopK:
    """Per row: the k largest among the row's stored entries and its implicit zeros, which carry index 0.  A row without stored
    entries stays all zero.  k may not exceed the number of columns."""
    indptr, indices, data = _csr_parts(arr)
    n_rows, n_cols = arr.shape
    if not 0 <= k <= n_cols:
        raise ValueError(f"k = {k} is out of range for rows of {n_cols} columns")
    values = np.zeros((n_rows, k), dtype=data.dtype)
    columns = np.zeros((n_rows, k), dtype=np.int64)
    stored = np.diff(indptr).astype(np.int64)
    if k == 0 or data.size == 0:
        return NumpyTopK(values=values, indices=columns)
    # a row has n_cols - stored implicit zeros and at most k of them can place: one table line per row holds its stored
    # entries, then that many zeros, then -inf up to the table's width
    zeros = np.minimum(k, n_cols - stored)
    width = int((stored + zeros).max())
    slot = np.arange(width)[None, :]
    line_v = np.where(slot < (stored + zeros)[:, None], 0.0, -np.inf)
    line_c = np.zeros((n_rows, width), dtype=np.int64)
    row_of = np.repeat(np.arange(n_rows), stored)
    at = np.arange(data.size) - indptr[:-1].astype(np.int64)[row_of]
    line_v[row_of, at] = data
    line_c[row_of, at] = indices
    best = _descending(line_v)[:, :k]
    filled = stored > 0
    values[filled] = np.take_along_axis(line_v, best, axis=1)[filled].astype(data.dtype)
    columns[filled] = np.take_along_axis(line_c, best, axis=1)[filled]
    return NumpyTopK(values=values, indices=columns)


def _topk_axis0(arr, k: int, batch_size: int, device=None) -> NumpyTopK:
    import torch

    from .engine import LatentTopK

    indptr, indices, data = _csr_parts(arr)
    n_rows, n_cols = arr.shape
    if batch_size < 1:
        raise ValueError(f"batch_size must be positive, got {batch_size}")
    if not torch.cuda.is_available():
        raise RuntimeError("saev_amd csr_topk(axis=0) runs on a HIP device only (there is no CPU path)")
    data32 = data.astype(np.float32, copy=False)
    if data32.dtype != data.dtype and not np.array_equal(data32.astype(data.dtype), data):
        raise ValueError("csr_topk(axis=0) selects in float32: the values of this array do not survive the conversion")
    if n_cols == 0 or n_rows == 0:
        return NumpyTopK(values=np.zeros((k, n_cols), dtype=data.dtype), indices=np.zeros((k, n_cols), dtype=np.int64))
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    acc = LatentTopK(n_cols, k, device)
    indptr = indptr.astype(np.int64, copy=False)
    r0 = 0
    while r0 < n_rows:
        # at least batch_size rows; more while the block stays under the entry budget
        grown = int(np.searchsorted(indptr, indptr[r0] + _BLOCK_ENTRIES, side="right")) - 1
        r1 = min(n_rows, max(r0 + batch_size, grown))
        p0, p1 = int(indptr[r0]), int(indptr[r1])
        if p1 - p0 > _MAX_ENTRIES:
            raise ValueError(f"rows {r0}..{r1} hold {p1 - p0} entries: more than one update takes; lower batch_size")
        if p1 > p0:
            acc.add_csr(torch.from_numpy(indptr[r0:r1 + 1] - p0).to(device), torch.from_numpy(indices[p0:p1].astype(np.int32, copy=False)).to(device),
                        torch.from_numpy(np.ascontiguousarray(data32[p0:p1])).to(device), row_base=r0)
        r0 = r1
    got = acc.read()
    return NumpyTopK(values=got.values.numpy().astype(data.dtype, copy=False), indices=got.indices.numpy())


def csr_topk(arr, *, k: int, axis: int = 0, batch_size: int = 1024) -> NumpyTopK:
    """Top k values of a scipy CSR array along ``axis``.

    ``axis=0``: for every column the k largest stored nonzero values over all rows and the rows they sit in, shape (k, n_cols),
    descending; columns with fewer than k stored nonzeros are padded with value 0 and index 0.  Runs on the HIP device
    (1 <= k <= 64); ``batch_size`` is the least number of rows per block and never changes the result.
    ``axis=1``: for every row the k largest values and their columns, shape (n_rows, k), on the host.
    """
    if axis == 0:
        return _topk_axis0(arr, k, batch_size)
    if axis == 1:
        return _topk_axis1(arr, k)
    raise ValueError(f"csr_topk selects along axis 0 (per column) or 1 (per row), not {axis}")
