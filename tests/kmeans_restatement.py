"""Numpy restatement of one mini-batch k-means step as saev_amd.baselines.MiniBatchKMeans defines it (include/saev_amd.h: K-MEANS):
fp32 state, every DECISION (nearest centre, empties, pairs under the tolerance, farthest points) taken exactly in fp64 with ties to
the lower index, every UPDATE in fp32 in the reference's order of operations.  tools/gen_golden_kmeans.py holds it to the
reference's centres bit for bit; the tests hold the HIP path to the same fixtures."""

import dataclasses

import numpy as np


def tol(D: int) -> float:
    """Relative error of the fp32 difference-form squared distance: one rounding per difference, one per square, at most D - 1
    per sum over non-negative terms."""
    return (D + 3) * 2.0 ** -24


def dist2_64(X: np.ndarray, C: np.ndarray, block: int = 256) -> np.ndarray:
    """(n, k) squared distances in fp64, difference form."""
    X64, C64 = X.astype(np.float64), C.astype(np.float64)
    out = np.empty((X.shape[0], C.shape[0]))
    for i in range(0, X.shape[0], block):
        d = X64[i:i + block, None, :] - C64[None, :, :]
        out[i:i + block] = np.einsum("nkd,nkd->nk", d, d)
    return out


def r_fp32(X: np.ndarray, C: np.ndarray) -> np.ndarray:
    """(n, k) the kernels' refined value bit for bit: fp32, k ascending, a subtraction, a product and an addition per k."""
    s = np.zeros((X.shape[0], C.shape[0]), dtype=np.float32)
    for k in range(X.shape[1]):
        d = X[:, None, k] - C[None, :, k]
        s = s + d * d
    return s


@dataclasses.dataclass
class State:
    k: int
    collapse_tol: float
    centers: np.ndarray | None = None
    counts: np.ndarray | None = None
    n_steps: int = 0


@dataclasses.dataclass
class StepLog:
    assign: np.ndarray     # (n,) the fp64 argmin against the centres before the update
    inertia64: float       # the fp64 mean of the fp64 minima
    losers: np.ndarray     # (k,) bool, on the updated centres
    n_empty: int
    centers_before: np.ndarray  # the centres the assignment was taken against
    centers_updated: np.ndarray  # the centres the pair test (and the farthest points) were taken against
    counts_updated: np.ndarray


def step(st: State, batch: np.ndarray, draws: list) -> StepLog:
    """One partial_fit.  ``draws`` is consumed from the front: the initial permutation (only when the first batch has at least k
    rows), then the replacement rows of a step with empty clusters."""
    X = np.ascontiguousarray(batch, dtype=np.float32)
    n = X.shape[0]
    if st.centers is None:
        if n >= st.k:
            st.centers = X[np.asarray(draws.pop(0))[:st.k]].copy()
        else:
            st.centers = np.tile(X, (-(-st.k // n), 1))[:st.k].copy()
        st.counts = np.zeros(st.k, dtype=np.float32)
    before = st.centers.copy()
    d2 = dist2_64(X, st.centers)
    assign = d2.argmin(axis=1)
    counts_b = np.bincount(assign, minlength=st.k).astype(np.float32)
    sums = np.zeros_like(st.centers)
    np.add.at(sums, assign, X)  # unbuffered, in row order: a one-thread index_add_
    prev = st.counts.copy()
    empty = (prev == 0) & (counts_b == 0)
    if empty.any():
        counts_b[empty] = 1.0
        sums[empty] = X[np.asarray(draws.pop(0))]
    st.counts = prev + counts_b
    m = counts_b > 0
    st.centers[m] = (st.centers[m] * prev[m, None] + sums[m]) / st.counts[m, None]
    inertia = float(d2[np.arange(n), assign].mean())
    losers = collapsed(st.centers, st.counts, st.collapse_tol)
    updated, counts_updated = st.centers.copy(), st.counts.copy()
    if losers.any():
        need = int(losers.sum())
        cand = X if n >= need else np.tile(X, (-(-need // n), 1))
        far = np.sqrt(dist2_64(cand, st.centers).max(axis=1))
        pick = np.argsort(-far, kind="stable")[:need]
        st.centers[losers] = cand[pick]
        st.counts[losers] = 0.0
    st.n_steps += 1
    return StepLog(assign=assign, inertia64=inertia, losers=losers, n_empty=int(empty.sum()), centers_before=before,
                   centers_updated=updated, counts_updated=counts_updated)


def collapsed(centers: np.ndarray, counts: np.ndarray, tol_: float) -> np.ndarray:
    """The loser mask: for every pair i < j closer than tol_ (fp64), i if counts[i] <= counts[j] else j."""
    k = centers.shape[0]
    losers = np.zeros(k, dtype=bool)
    if k < 2:
        return losers
    close = np.triu(np.sqrt(dist2_64(centers, centers)) < tol_, 1)
    i, j = np.nonzero(close)
    losers[np.where(counts[i] <= counts[j], i, j)] = True
    return losers
