"""The contract of the per-latent top-k (include/saev_amd.h: LATENT TOP-K) restated in numpy, shared by the tests of the kernels
and by tools/gen_golden_latent_topk.py, which checks it against the reference before it records fixture G21.

For each latent: its entries (value != 0, latent in [0, S)) ordered by value descending, then row ascending; the first k."""

import numpy as np


def restate(rows, cols, vals, n_cols: int, k: int):
    """(values (k, S) float32, indices (k, S) int64, counts (S) int64) of the entries (rows[i], cols[i], vals[i])."""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1)
    cols = np.asarray(cols, dtype=np.int64).reshape(-1)
    vals = np.asarray(vals, dtype=np.float32).reshape(-1)
    on = (vals != 0) & (cols >= 0) & (cols < n_cols)
    rows, cols, vals = rows[on], cols[on], vals[on]
    order = np.lexsort((rows, -vals, cols))  # by latent, inside it by value descending, among equal values by row ascending
    rows, cols, vals = rows[order], cols[order], vals[order]
    per = np.bincount(cols, minlength=n_cols).astype(np.int64)
    start = np.concatenate([[0], np.cumsum(per)[:-1]])
    rank = np.arange(cols.size) - start[cols]
    top = rank < k
    values = np.zeros((k, n_cols), dtype=np.float32)
    indices = np.zeros((k, n_cols), dtype=np.int64)
    values[rank[top], cols[top]] = vals[top]
    indices[rank[top], cols[top]] = rows[top]
    return values, indices, np.minimum(per, k)


def restate_csr(indptr, indices, data, n_cols: int, k: int, row_base: int = 0):
    indptr = np.asarray(indptr, dtype=np.int64)
    rows = np.repeat(np.arange(indptr.size - 1, dtype=np.int64), np.diff(indptr)) + row_base
    return restate(rows, indices, data, n_cols, k)


def restate_padded(idx, val, n_cols: int, k: int, row_nnz=None, keep=None, row_base: int = 0):
    """Padded code rows idx / val (n, cap): the first min(row_nnz, cap) slots of every kept row."""
    idx, val = np.asarray(idx), np.asarray(val)
    n, cap = idx.shape
    on = np.ones((n, cap), dtype=bool)
    if row_nnz is not None:
        on &= np.arange(cap)[None, :] < np.asarray(row_nnz)[:, None]
    if keep is not None:
        on &= np.asarray(keep).astype(bool)[:, None]
    rows = np.broadcast_to(np.arange(n, dtype=np.int64)[:, None] + row_base, (n, cap))
    return restate(rows[on], idx[on], val[on], n_cols, k)
