"""The contract of the per-latent histograms and quantiles (include/saev_amd.h: LATENT HISTOGRAM), restated in
numpy with integers only: the key map, the entries, the three levels, the count tables, the windowed histogram, and the three
locate steps with the zero block in closed form.  The CPU tests check it against np.histogram and np.quantile on the dense matrix;
the GPU tests compare the kernels with it table by table and bit by bit."""

import numpy as np

BINS0, BINS, T_STRIDE = 4096, 1024, 16
NO_PREFIX = 0xFFFFFFFF


def key_of(v):
    u = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)
    return np.where(u >> 31 != 0, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def value_of(key):
    k = np.ascontiguousarray(key, dtype=np.uint32)
    return np.where(k >> 31 != 0, k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)


def entries_of(indptr, indices, data, S, keep=None):
    """(latent, key) of every entry of a CSR matrix and its number of kept rows."""
    indptr = np.asarray(indptr, dtype=np.int64)
    n = indptr.size - 1
    rows = np.repeat(np.arange(n), np.diff(indptr))
    indices, data = np.asarray(indices)[indptr[0]:indptr[-1]].astype(np.int64), np.asarray(data, dtype=np.float32)[indptr[0]:indptr[-1]]
    keep = np.ones(n, dtype=bool) if keep is None else np.asarray(keep, dtype=bool)
    on = (data != 0) & (indices >= 0) & (indices < S) & keep[rows]
    return indices[on], key_of(data[on]), int(keep.sum())


def padded_to_csr(idx, val, row_nnz=None):
    n, cap = idx.shape
    nnz = np.full(n, cap) if row_nnz is None else np.minimum(np.asarray(row_nnz), cap)
    live = np.arange(cap)[None, :] < nnz[:, None]
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(nnz, out=indptr[1:])
    return indptr, idx[live], val[live]


def counts0_of(lat, key, S):
    return np.bincount(lat * BINS0 + (key >> 20).astype(np.int64), minlength=S * BINS0).reshape(S, BINS0)


def histogram(counts0, lo_exp=-16, hi_exp=16):
    lo, hi = 2048 + 8 * (lo_exp + 127), 2048 + 8 * (hi_exp + 127)
    counts = np.concatenate([counts0[:, 2048:lo].sum(1, keepdims=True), counts0[:, lo:hi], counts0[:, hi:].sum(1, keepdims=True)], axis=1)
    edges = ((np.arange(lo, hi + 1, dtype=np.int64) - 2048) << 20).astype(np.uint32).view(np.float32)
    return counts, counts0[:, :2048].sum(1), edges


def ranks_of(M, q):
    """floor(h), ceil(h), h - floor(h) of h = (M - 1) q, one fp64 product."""
    h = np.float64(M - 1) * np.float64(q)
    f = np.floor(h)
    return int(f), int(np.ceil(h)), h - f


def _find(c, r):
    """The bin of counts c holding rank r, and the rank left inside it."""
    ends = np.cumsum(c)
    b = int(np.searchsorted(ends, r, side="right"))
    return b, int(r - (ends[b] - c[b]))


def select(lat, key, S, q, over, n_rows):
    """The three passes.  Returns a dict: counts0; per level l in 0..2 ``prefix{l}``, ``rank{l}``, ``resolved`` (S, 2 Q) as the
    locate step leaves them, ``counts1`` / ``counts2`` (S, 2 Q, 1024); lower, higher (float32), linear (float64), count (int64)."""
    Q = len(q)
    T = 2 * Q
    lat = np.asarray(lat, dtype=np.int64)
    out = {"counts0": counts0_of(lat, key, S)}
    prefix = np.full((S, T), NO_PREFIX, dtype=np.int64)
    rank = np.zeros((S, T), dtype=np.int64)
    resolved = np.zeros((S, T), dtype=np.int32)
    count = np.zeros(S, dtype=np.int64)
    frac = np.zeros((S, Q))
    for j in range(S):
        c = out["counts0"][j]
        entries, n_neg = int(c.sum()), int(c[:2048].sum())
        zeros = max(n_rows - entries, 0) if over == "rows" else 0
        M = count[j] = entries + zeros
        for t in range(T):
            if M == 0:
                resolved[j, t] = 2
                continue
            lo, hi, frac[j, t // 2] = ranks_of(M, q[t // 2])
            r = hi if t & 1 else lo
            if n_neg <= r < n_neg + zeros:
                resolved[j, t] = 1
            elif r < n_neg:
                prefix[j, t], rank[j, t] = _find(c, r)
            else:
                b, rank[j, t] = _find(c[2048:], r - n_neg - zeros)
                prefix[j, t] = 2048 + b
    out.update(prefix0=prefix.copy(), rank0=rank.copy(), resolved=resolved)
    for level in (1, 2):
        mine = (key >> (20 if level == 1 else 10)).astype(np.int64)
        digit = ((key >> 10) & 1023 if level == 1 else key & 1023).astype(np.int64)
        table = np.zeros((S, T, BINS), dtype=np.int64)
        for t in range(T):
            on = prefix[lat, t] == mine
            np.add.at(table, (lat[on], t, digit[on]), 1)
        for j, t in zip(*np.nonzero(resolved == 0)):
            d, rank[j, t] = _find(table[j, t], rank[j, t])
            prefix[j, t] = (prefix[j, t] << 10) | d
        out[f"counts{level}"] = table
        out[f"prefix{level}"], out[f"rank{level}"] = prefix.copy(), rank.copy()
    vals = np.where(resolved == 1, np.float32(0), value_of(np.where(resolved == 0, prefix, 0).astype(np.uint32)))
    lower, higher = vals[:, 0::2].astype(np.float32), vals[:, 1::2].astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        lo64, hi64 = lower.astype(np.float64), higher.astype(np.float64)
        linear = np.where(lower == higher, lo64, lo64 + frac * (hi64 - lo64))
    empty = (count == 0)[:, None] & np.ones((1, Q), dtype=bool)
    out.update(lower=np.where(empty, np.float32(np.nan), lower), higher=np.where(empty, np.float32(np.nan), higher),
               linear=np.where(empty, np.nan, linear), count=count)
    return out


def dense_of(indptr, indices, data, S, keep=None):
    """The dense (kept rows, S) float32 matrix np.quantile is run on (entries only: latents outside [0, S) are dropped)."""
    indptr = np.asarray(indptr, dtype=np.int64)
    n = indptr.size - 1
    rows = np.repeat(np.arange(n), np.diff(indptr))
    indices, data = np.asarray(indices).astype(np.int64), np.asarray(data, dtype=np.float32)
    on = (indices >= 0) & (indices < S)
    dense = np.zeros((n, S), dtype=np.float32)
    dense[rows[on], indices[on]] = data[on]
    return dense if keep is None else dense[np.asarray(keep, dtype=bool)]
