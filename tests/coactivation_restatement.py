"""The contract of saev_coactivation (include/saev_amd.h: COACTIVATION) restated on the CPU: firing sets from the stored entries, the
supports and intersection counts as a scipy int64 product of the two 0/1 matrices, and the two orders written with Python ints
(which cannot overflow, so the 64-bit cross-products of the header are exact here by construction).  No GPU, no library."""

from __future__ import annotations

import functools

import numpy as np
import scipy.sparse

JACCARD, CONTAINMENT = "jaccard", "containment"


def firing(csr, thr: float):
    """The 0/1 int64 CSR matrix of the STORED entries with value > thr (an entry that is not stored never fires, whatever thr)."""
    csr = scipy.sparse.csr_matrix(csr)
    keep = csr.data.astype(np.float32) > np.float32(thr)
    rows = np.repeat(np.arange(csr.shape[0]), np.diff(csr.indptr))
    out = scipy.sparse.csr_matrix((np.ones(int(keep.sum()), dtype=np.int64), (rows[keep], csr.indices[keep])), shape=csr.shape)
    assert out.nnz == 0 or out.data.max() == 1, "rows must be canonical (no column twice in a row)"
    return out


def supports(fire) -> np.ndarray:
    return np.asarray(fire.sum(axis=0)).reshape(-1).astype(np.int64)


def intersections(fire_a, fire_b):
    """I(a, b) as an (Sa, Sb) int64 CSR matrix: ((A > t_a).T @ (B > t_b))."""
    return scipy.sparse.csr_matrix(fire_a.T.astype(np.int64) @ fire_b.astype(np.int64))


def before(measure: str, n_a: int, i1: int, nb1: int, b1: int, i2: int, nb2: int, b2: int) -> bool:
    """Does partner b1 rank before partner b2 for a latent of support n_a?  Python ints throughout."""
    n_a, i1, nb1, b1, i2, nb2, b2 = (int(v) for v in (n_a, i1, nb1, b1, i2, nb2, b2))
    if measure == JACCARD:
        u1, u2 = n_a + nb1 - i1, n_a + nb2 - i2
        left, right = i1 * u2, i2 * u1
        return left > right if left != right else b1 < b2
    if measure == CONTAINMENT:
        if i1 != i2:
            return i1 > i2
        if nb1 != nb2:
            return nb1 < nb2
        return b1 < b2
    raise ValueError(measure)


def rank(measure: str, n_a: int, cands: list[tuple[int, int, int]]) -> list[tuple[int, int, int]]:
    """(I, n_b, b) triples with I >= 1, best first."""
    def cmp(p, q):
        return -1 if before(measure, n_a, *p, *q) else 1 if before(measure, n_a, *q, *p) else 0
    return sorted(cands, key=functools.cmp_to_key(cmp))


def match(A, B=None, *, thr_a: float = 0.0, thr_b: float = 0.0, measure: str = JACCARD, top_m: int = 1) -> dict:
    """What ``engine.coactivation_match`` must return, as numpy arrays: index and intersection (Sa, top_m) int32, support_a, support_b
    int32, jaccard and containment (Sa, top_m) float64 (NaN at index -1), mutual (Sa) bool and reverse_index (Sb) int32."""
    self_mode = B is None
    fa = firing(A, thr_a)
    fb = fa if self_mode else firing(B, thr_b)
    n_a, n_b = supports(fa), supports(fb)
    inter = intersections(fa, fb)
    index, isect = _top(inter, n_a, n_b, measure, top_m, self_mode)
    if self_mode:
        rev = index[:, 0].copy()
    else:
        rev = _top(scipy.sparse.csr_matrix(inter.T), n_b, n_a, measure, 1, False)[0][:, 0]
    ok = index >= 0
    nb_of = n_b[np.maximum(index, 0)]
    with np.errstate(divide="ignore", invalid="ignore"):
        jac = np.where(ok, isect.astype(np.float64) / (n_a[:, None] + nb_of - isect).astype(np.float64), np.nan)
        con = np.where(ok, isect.astype(np.float64) / n_a[:, None].astype(np.float64), np.nan)
    best = index[:, 0]
    mutual = (best >= 0) & (rev[np.maximum(best, 0)] == np.arange(len(best)))
    return dict(index=index, intersection=isect, support_a=n_a.astype(np.int32), support_b=n_b.astype(np.int32), jaccard=jac, containment=con,
                mutual=mutual, reverse_index=rev.astype(np.int32))


def _top(inter, n_a, n_b, measure, top_m, self_mode):
    Sa = inter.shape[0]
    index = np.full((Sa, top_m), -1, dtype=np.int32)
    isect = np.zeros((Sa, top_m), dtype=np.int32)
    for a in range(Sa):
        cols = inter.indices[inter.indptr[a]:inter.indptr[a + 1]]
        vals = inter.data[inter.indptr[a]:inter.indptr[a + 1]]
        cands = [(int(i), int(n_b[b]), int(b)) for i, b in zip(vals, cols) if i >= 1 and not (self_mode and b == a)]
        for r, (i, _, b) in enumerate(rank(measure, int(n_a[a]), cands)[:top_m]):
            index[a, r], isect[a, r] = b, i
    return index, isect
