"""Numpy restatement of one mini-batch k-means step as saev_amd.baselines.MiniBatchKMeans defines it (include/saev_amd.h: K-MEANS):
fp32 state, every DECISION (nearest centre, empties, pairs under the tolerance, farthest points) taken exactly in fp64 with ties to
the lower index, every UPDATE in fp32 in the reference's order of operations.  tools/gen_golden_kmeans.py holds it to the
reference's centres bit for bit; the tests hold the HIP path to the same fixtures.

The second half restates the CANDIDATE RULE of the fp16 filter ("The bound") with torch ops in fp64 and fp32, so
that it runs on the CPU in the host tests and on the device beside the fp64 distances in the GPU tests: filter_values gives s~
and E of every pair, candidate_bracket / collapsed_bracket the two counts between which a correct device filter must report."""

import dataclasses

import numpy as np
import torch


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


# ---- the candidate rule of the fp16 filter -----------------------------------------------------------------
# Everything the rule is made of is a function of the inputs alone except the fp32 MFMA sum of the image dot product, which the
# device forms in an order of its own.  The restatement forms that dot product in fp64 (exact to about 2^-53) and carries the
# accumulation term the bound already states, coh_gamma(Dp) (rn.x + rn.y)_x (rn.x + rn.y)_c on the cosine, as the half-width
# delta_ij = 2 nx nc x that term of an interval around s~_ij.  Two fp32 sums are taken in the library's fixed order, because a last
# bit there moves an fp16 image element and with it s~ by more than delta: the centring vector (rows far from the origin have
# |mu| >> |x - mu|, so one ulp of mu is 1e-3 of x') and the norm the unit row is divided by.

IMG_SCALE = 8192.0            # 2^13: the image is fp16(2^13 u)
F16_MIN_NORMAL = 2.0 ** -14   # images below it are flushed to zero
MU_CHUNKS = 64


def filter_tol(D: int) -> float:
    """tau of km_pair: 1.001 (D + 3) 2^-24."""
    return 1.001 * (D + 3) * 2.0 ** -24


def padded(D: int) -> int:
    return (D + 63) // 64 * 64


def coh_gamma(Dp: int) -> np.float32:
    """The accumulation term of the cosine bound for images padded to Dp: 2 x 1.05 Dp 2^-22, evaluated in fp32."""
    return np.float32(2.0) * np.float32(1.05) * np.float32(Dp) * np.float32(2.0 ** -22)


def centring_vector(C: torch.Tensor) -> torch.Tensor:
    """mu, the fp32 mean of the centres in the library's fixed order: up to 64 chunks of ceil(k / 64) consecutive centres, each
    summed from 0 in ascending order, the partial sums added in ascending order, one division by k; 0 where that is not finite."""
    k, D = C.shape
    per = -(-k // MU_CHUNKS)
    chunks = -(-k // per)
    pad = torch.zeros(chunks * per, D, dtype=torch.float32, device=C.device)
    pad[:k] = C
    pad = pad.view(chunks, per, D)
    part = torch.zeros(chunks, D, dtype=torch.float32, device=C.device)
    for r in range(per):
        part = part + pad[:, r]
    tot = torch.zeros(D, dtype=torch.float32, device=C.device)
    for b in range(chunks):
        tot = tot + part[b]
    mu = tot / torch.tensor(float(k), dtype=torch.float32, device=C.device)
    return torch.where(mu.abs() <= 3.0e38, mu, torch.zeros_like(mu))


def _prepare_norm(Wc: torch.Tensor) -> torch.Tensor:
    """prepare's fp32 norm of each row: 64 partial sums (partial l takes the column quads l, l + 64, ... in ascending order, one
    fused multiply-add per element: the product is exact in fp64 and the sum is rounded once to fp32, up to a double rounding
    of probability 2^-29), added pairwise at distances 32, 16, ..., 1, then a square root."""
    S, D = Wc.shape
    M = -(-(D // 4) // 64)
    pad = torch.zeros(S, M * 256, dtype=torch.float32, device=Wc.device)
    pad[:, :D] = Wc
    v = pad.view(S, M, 64, 4).double()
    ss = torch.zeros(S, 64, dtype=torch.float32, device=Wc.device)
    for m in range(M):
        for e in range(4):
            ss = (v[:, m, :, e] * v[:, m, :, e] + ss.double()).float()
    w = 64
    while w > 1:
        w //= 2
        ss = ss[:, :w] + ss[:, w:2 * w]
    return ss[:, 0].sqrt()


@dataclasses.dataclass
class FilterRows:
    """What the bound needs of one operand, row by row."""
    sq: torch.Tensor    # (S,) fp64 ||w'||^2, summed in fp64
    rt: torch.Tensor    # (S,) fp64 its square root
    nrm: torch.Tensor   # (S,) fp32 prepare's norm of w', the divisor of the unit row
    rnx: torch.Tensor   # (S,) fp32 ||u||, rounded up by 1 + 2^-20
    rny: torch.Tensor   # (S,) fp32 ||d|| 2^-13, rounded up by 1 + 2^-20, d = 2^13 u - image
    img: torch.Tensor   # (S, D) fp64 the fp16 image's values
    has_image: torch.Tensor  # (S,) bool: the unit row is finite (false for a centred row that is exactly zero)


def filter_rows(W: torch.Tensor, mu: torch.Tensor) -> FilterRows:
    Wc = W - mu                                   # x' = fl32(x - mu)
    sq = (Wc.double() ** 2).sum(dim=1)
    nrm = _prepare_norm(Wc)
    u = Wc / nrm[:, None]                         # fl32(x' / n)
    s = u * IMG_SCALE                             # (exact)
    h = s.half()
    h = torch.where(h.float().abs() < F16_MIN_NORMAL, torch.zeros_like(h), h)
    d = s - h.float()
    up = torch.tensor(1.0 + 2.0 ** -20, dtype=torch.float32, device=W.device)
    rnx = (u.double() ** 2).sum(dim=1).sqrt().float() * up
    rny = ((d.double() ** 2).sum(dim=1).sqrt() * (1.0 / IMG_SCALE)).float() * up
    return FilterRows(sq=sq, rt=sq.sqrt(), nrm=nrm, rnx=rnx, rny=rny, img=h.double(), has_image=(u.abs() <= 3.0e38).all(dim=1))


def _pairs(x: FilterRows, c: FilterRows, D: int, rows: slice):
    """(s~, E, delta) of the pairs (rows of x) x (all of c), fp64: km_pair with the exact image dot product."""
    gam = coh_gamma(padded(D))
    ct = (x.img[rows] @ c.img.T) * 2.0 ** -26
    ax, ay = x.rnx[rows, None], x.rny[rows, None]
    bx, by = c.rnx[None, :], c.rny[None, :]
    gam_t = torch.tensor(float(gam), dtype=torch.float32, device=ct.device)
    acc_term = gam_t * (ax + ay) * (bx + by)      # fp32, in coh_pair_bound's order
    ecos32 = 1.02 * ((ay * bx + ax * by + ay * by) + acc_term) + 1e-30  # (fp32 tensors: the constants are taken as fp32)
    P = x.nrm[rows, None].double() * c.nrm[None, :].double()
    ecos = ecos32.double() + 1.25e-7 * ax.double() * bx.double()
    ss = x.sq[rows, None] + c.sq[None, :]
    st = ss - 2.0 * P * ct
    E1 = 2.0 * P * ecos + 1e-12 * ss
    up2 = (st + E1).clamp_min(0.0)
    up = up2.sqrt() * (1.0 + 1e-12)
    rho = 5.97e-8 * (x.rt[rows, None] + c.rt[None, :])
    dl = rho * (2.0 * up + rho)
    E = (E1 + dl + filter_tol(D) * (up2 + dl)) * (1.0 + 1e-9) + 1e-30
    delta = 2.0 * P * float(gam) * (ax.double() + ay.double()) * (bx.double() + by.double())
    return st, E, delta


def _row_blocks(n: int, k: int):
    step = max(1, 2 ** 21 // max(k, 1))
    return [slice(i, min(n, i + step)) for i in range(0, n, step)]


def filter_values(X: torch.Tensor, C: torch.Tensor):
    """(s~, E), both (n, k) fp64: the filter's approximation of the refined value r_ij and its bound E_ij >= |s~_ij - r_ij|."""
    mu = centring_vector(C)
    x, c = filter_rows(X, mu), filter_rows(C, mu)
    out = [_pairs(x, c, X.shape[1], rows)[:2] for rows in _row_blocks(X.shape[0], C.shape[0])]
    return torch.cat([o[0] for o in out]), torch.cat([o[1] for o in out])


def candidate_brackets(X: torch.Tensor, C: torch.Tensor) -> dict:
    """{farthest: (sure, maybe)} for both directions from one preparation: see candidate_bracket."""
    mu = centring_vector(C)
    x, c = filter_rows(X, mu), filter_rows(C, mu)
    assert bool(x.has_image.all()) and bool(c.has_image.all()), "a centred row without a unit image: the filter does not answer"
    count = {False: [0, 0], True: [0, 0]}
    for rows in _row_blocks(X.shape[0], C.shape[0]):
        st, E, delta = _pairs(x, c, X.shape[1], rows)
        for farthest in (False, True):
            g = st if farthest else -st
            L_hi = (g - E + delta).max(dim=1, keepdim=True).values
            L_lo = (g - E - delta).max(dim=1, keepdim=True).values
            count[farthest][0] += int((g + E - delta >= L_hi).sum())
            count[farthest][1] += int((g + E + delta >= L_lo).sum())
    return {f: tuple(v) for f, v in count.items()}


def candidate_bracket(X: torch.Tensor, C: torch.Tensor, farthest: bool):
    """(sure, maybe): with g = -s (nearest) or s (farthest), the pairs with g~ + E - delta >= max_j (g~ - E + delta) and those with
    g~ + E + delta >= max_j (g~ - E - delta).  The device's s~ lies within delta of the restated one, so a correct filter reports
    sure <= candidates <= maybe."""
    return candidate_brackets(X, C)[bool(farthest)]


def collapsed_bracket(C: torch.Tensor, tol_: float):
    """(sure, maybe) for the collapsed pass: the pairs i < j with s~ + delta - E < tol^2 and those with s~ - delta - E < tol^2."""
    mu = centring_vector(C)
    x = filter_rows(C, mu)
    assert bool(x.has_image.all()), "a centred row without a unit image: the filter does not answer"
    k = C.shape[0]
    thr2 = float(np.float32(tol_)) ** 2
    j = torch.arange(k, device=C.device)[None, :]
    sure = maybe = 0
    for rows in _row_blocks(k, k):
        st, E, delta = _pairs(x, x, C.shape[1], rows)
        upper = torch.arange(rows.start, rows.stop, device=C.device)[:, None] < j
        sure += int((upper & (st + delta - E < thr2)).sum())
        maybe += int((upper & (st - delta - E < thr2)).sum())
    return sure, maybe
