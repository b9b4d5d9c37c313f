"""The contract of the single-op forward entries (include/saev_amd.h, "single ops": saev_topk_dense, saev_decode_sparse,
saev_scatter_dense, saev_gather_rows), restated on the host in numpy: the select on the bit patterns, the decode in fp64 with the
bound of its own fp32 chain.  A module, not a test file."""

import numpy as np

U = 2.0 ** -24


def keys(h) -> np.ndarray:
    """The select's total order: uint32 keys, a larger key wins.  bits ^ 0xFFFFFFFF where the sign bit is set, else
    bits | 0x80000000: +NaN above +inf, a sign-bit NaN below -inf, -0.0 < +0.0."""
    bits = np.ascontiguousarray(h, dtype=np.float32).view(np.uint32)
    return np.where(bits & np.uint32(0x80000000), bits ^ np.uint32(0xFFFFFFFF), bits | np.uint32(0x80000000)).astype(np.uint32)


def from_keys(k) -> np.ndarray:
    """The float32 whose key is k (the inverse of `keys`)."""
    k = np.asarray(k, dtype=np.uint32)
    bits = np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), k ^ np.uint32(0xFFFFFFFF)).astype(np.uint32)
    return bits.view(np.float32)


def select(h, k: int, mask=None):
    """(idx int32, val float32), (n, k) each: per row the k eligible latents (mask word != 0) of largest key, ties to the lower
    latent index, written in ascending latent order with the bits of h; slots past the number of eligible latents hold -1 / 0."""
    h = np.ascontiguousarray(h, dtype=np.float32)
    one = h.ndim == 1
    h2 = h[None] if one else h
    n, S = h2.shape
    assert 1 <= k <= S
    cand = np.arange(S) if mask is None else np.nonzero(np.asarray(mask) != 0)[0]
    idx = np.full((n, k), -1, dtype=np.int32)
    val = np.zeros((n, k), dtype=np.float32)
    key = keys(h2)
    for b in range(n):
        # stable sort of the negated keys: equal keys stay in ascending index order
        order = cand[np.argsort(-key[b, cand].astype(np.int64), kind="stable")][:k]
        order = np.sort(order)
        idx[b, :len(order)] = order
        val[b, :len(order)] = h2[b, order]
    return (idx[0], val[0]) if one else (idx, val)


def decode(idx, val, W_dec, b_dec, prefixes):
    """x_hats[b, p] = b_dec + sum over the entries with 0 <= idx < prefixes[p] of val * W_dec[idx] in fp64 (duplicates add up).
    Returns (x_hats, mag, m): mag[b, p, d] = |b_dec_d| + sum |val_j| |W_dec[idx_j, d]| over the entries used, m[b, p] their number."""
    idx = np.asarray(idx)
    val = np.asarray(val, dtype=np.float64)
    W = np.asarray(W_dec, dtype=np.float64)
    b = np.asarray(b_dec, dtype=np.float64)
    n, k = idx.shape
    P, D = len(prefixes), W.shape[1]
    out = np.empty((n, P, D))
    mag = np.empty((n, P, D))
    m = np.empty((n, P), dtype=np.int64)
    rows = W[np.clip(idx, 0, W.shape[0] - 1)]  # (n, k, D)
    for p, cut in enumerate(prefixes):
        use = ((idx >= 0) & (idx < int(cut))).astype(np.float64)
        out[:, p] = b + np.einsum("nk,nkd->nd", val * use, rows)
        mag[:, p] = np.abs(b) + np.einsum("nk,nkd->nd", np.abs(val) * use, np.abs(rows))
        m[:, p] = use.sum(axis=1)
    return out, mag, m


def decode_tolerance(mag, m):
    """(2 m + 2) 2^-24 mag + m 2^-149.  The kernel forms acc += v * w once per code in fp32 starting from b_dec: one rounding per
    code if the product is contracted into an fma, two if not; every partial sum is bounded by mag.  2 m u covers either form to
    first order, the two further units the higher-order terms of (1 + u)^(2m) (m <= 2^20) and the fp64 restatement; one smallest
    subnormal per code for results that round in the subnormal range."""
    m = np.asarray(m, dtype=np.float64)[..., None]
    return (2 * m + 2) * U * mag + m * 2.0 ** -149


def scatter(idx, val, S: int) -> np.ndarray:
    """Dense (n, S) float32 of the codes; entries outside [0, S) are dropped."""
    idx = np.asarray(idx)
    val = np.asarray(val, dtype=np.float32)
    f = np.zeros((idx.shape[0], S), dtype=np.float32)
    for b in range(idx.shape[0]):
        ok = (idx[b] >= 0) & (idx[b] < S)
        f[b, idx[b, ok]] = val[b, ok]
    return f


def gather(pool, rows) -> np.ndarray:
    return np.asarray(pool)[np.asarray(rows)]
