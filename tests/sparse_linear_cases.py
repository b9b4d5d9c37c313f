"""Designs shared by the CPU and GPU tests of SPARSE LINEAR: fixture G27 and its classifier designs, pooling CSRs with the edge cases
in known places, classification designs at any shape, and the closed form of the intercept-only optimum."""

import pathlib

import numpy as np
import scipy.sparse

import sparse_linear_restatement as R

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden"
N_CLS = 4  # classifier designs of G27


def golden():
    with np.load(GOLDEN / "g27_sparse_linear.npz") as z:
        return {k: z[k] for k in z.files}


def cls_design(g, i):
    """(X float32 by the restatement's max pooling of the stored tokens, y, K) of classifier design i."""
    n, tpi, s, k = (int(v) for v in g[f"cls{i}_shape"])
    x = R.pool_images(g[f"cls{i}_indptr"], g[f"cls{i}_indices"], g[f"cls{i}_data"], n, tpi, s, "max")
    return x, g[f"cls{i}_y"], k


def pool_design(n_img, tpi, s, seed):
    """(indptr, indices, data) of signed codes with, in image 0, latent 0 stored in all tpi patches with negative values only (the
    largest is -1) and latent s - 1 (if s > 1) in the first tpi - 1 patches with negative values only; image 1 is empty, and so is
    every third patch of image 2."""
    rng = np.random.default_rng(seed)
    per_row = max(1, min(s // 2, 20))
    cols = np.sort(rng.integers(0, s, size=(n_img * tpi, per_row)), axis=1)
    first = np.concatenate([np.ones((len(cols), 1), dtype=bool), cols[:, 1:] != cols[:, :-1]], axis=1)  # a column once per row
    rows = np.repeat(np.arange(n_img * tpi, dtype=np.int64), per_row).reshape(cols.shape)[first]
    cols = cols[first].astype(np.int64)
    vals = (rng.standard_normal(len(rows)) * 3).astype(np.float32)
    vals[vals == 0] = 1.0
    img, patch = rows // tpi, rows % tpi
    keep = ~((img == 0) & ((cols == 0) | (cols == s - 1))) & (img != 1) & ~((img == 2) & (patch % 3 == 0))
    rows, cols, vals = rows[keep], cols[keep], vals[keep]
    p = np.arange(tpi)
    rows, cols, vals = np.concatenate([rows, p]), np.concatenate([cols, np.zeros(tpi, np.int64)]), np.concatenate([vals, (-1.0 - p % 5).astype(np.float32)])
    if s > 1:
        q = p[:-1]
        rows, cols, vals = np.concatenate([rows, q]), np.concatenate([cols, np.full(len(q), s - 1)]), np.concatenate([vals, (-2.0 - q % 3).astype(np.float32)])
    m = scipy.sparse.csr_matrix((vals, (rows, cols)), shape=(n_img * tpi, s))
    m.sort_indices()
    assert m.has_canonical_format and m.nnz == len(vals)
    return m.indptr.astype(np.int64), m.indices.astype(np.int32), m.data.astype(np.float32)


def make_design(n, s, k, seed, codes=8):
    """(X float32 (n, s), y) of gamma codes with latents 3c .. 3c + 2 (mod s) stronger on class c; every class occurs."""
    rng = np.random.default_rng(seed)
    y = rng.integers(0, k, size=n)
    y[:k] = np.arange(k)
    x = np.where(rng.random((n, s)) < min(1.0, codes / s), rng.gamma(2.0, 1.0, size=(n, s)), 0.0).astype(np.float32)
    for j in range(3):
        on = rng.random(n) < 0.7
        col = (3 * y + j) % s
        x[on, col[on]] = np.maximum(x[on, col[on]], rng.gamma(4.0, 1.0, size=int(on.sum())).astype(np.float32))
    return x, y


def c_keeping_features(x, y, factor=4.0):
    """C at which the largest |g| at W = 0 (intercepts at the class priors) is ``factor``: above 1 features enter, below 1 the
    optimum is W = 0."""
    classes, yi = R.class_indices(y)
    k = len(classes)
    prior = np.bincount(yi, minlength=k) / len(yi)
    r0 = (prior[1] - (yi == 1))[:, None] if k == 2 else prior[None, :] - np.eye(k)[yi]
    gmax = float(np.abs(r0.T @ np.asarray(x, dtype=np.float64)).max())
    return factor / gmax if gmax > 0 else 1.0


def closed_form_intercepts(y):
    """(the intercepts of the optimum when W = 0: log(n_1 / n_0) for two classes, log(n_k / n) minus its mean otherwise;
    min_k p_k (1 - p_k))."""
    classes, yi = R.class_indices(y)
    counts = np.bincount(yi, minlength=len(classes)).astype(np.float64)
    p = counts / len(yi)
    b = np.asarray([np.log(counts[1] / counts[0])]) if len(classes) == 2 else np.log(p) - np.log(p).mean()
    return b, float((p * (1 - p)).min())
