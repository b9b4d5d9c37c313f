"""The contract of the per-latent logistic probes (include/saev_amd.h: PROBE1D) restated in fp64 numpy, shared by the tests of the
kernels, by the CPU tests that hold it against fixture G23 (recorded from the reference), and by tools/gen_golden_probe1d.py.

Written from the contract, pair by pair: the event sums, one solver iteration, the slab-wise loop, and the evaluation.  Sums are
accumulated in extended precision, so that their own error stays far below the bands they are compared in."""

import dataclasses
import math

import numpy as np

EPS, LAM_MIN, LAM_MAX, FALLBACK = 1e-8, 1e-12, 1e12, 1e-3
INACTIVE, CLIPPED, SINGULAR, FALLBACK_FLAG, EMPTY, GROWN, SHRUNK = 1, 2, 4, 8, 16, 32, 64
SUM_NAMES = ("mu", "g1", "s", "sv", "svv", "loss", "y")


@dataclasses.dataclass(frozen=True)
class Hyper:
    ridge: float = 1e-8
    tol: float = 1e-6
    max_iter: int = 200
    lam_init: float = 1e-3
    lam_shrink: float = 0.1
    lam_grow: float = 10.0
    delta_logit: float = 6.0
    class_slab_size: int = 8


def prepare(indptr, indices, data, n_latents):
    """Latent-major events: (starts, rows, vals, qx); inside a latent the rows ascend (a stable sort of the stored entries)."""
    indptr = np.asarray(indptr, dtype=np.int64)
    indices = np.asarray(indices, dtype=np.int64)
    data = np.asarray(data, dtype=np.float32)
    rows_csr = np.repeat(np.arange(indptr.size - 1, dtype=np.int64), np.diff(indptr))
    order = np.argsort(indices, kind="stable")
    counts = np.bincount(indices, minlength=n_latents)
    starts = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    rows, vals = rows_csr[order].astype(np.int32), data[order]
    qx = np.ones(n_latents)
    for j in np.flatnonzero(counts):
        v = vals[starts[j]:starts[j + 1]].astype(np.float64)
        qx[j] = max(math.sqrt(math.fsum(v * v) / counts[j]), 1e-6)
    return starts, rows, vals, qx


def labels_matrix(y, n_classes):
    """N x C bool from class ids (one-hot implied) or from a 0/1 matrix."""
    y = np.asarray(y)
    if y.ndim == 1:
        out = np.zeros((y.size, n_classes), dtype=bool)
        out[np.arange(y.size), y.astype(np.int64)] = True
        return out
    assert y.shape[1] == n_classes and np.isin(y, (0, 1)).all()
    return y.astype(bool)


def pack_bits(ymat):
    n, c = ymat.shape
    words = (c + 31) // 32
    padded = np.zeros((n, words * 32), dtype=np.uint64)
    padded[:, :c] = ymat
    return (padded.reshape(n, words, 32) << np.arange(32, dtype=np.uint64)).sum(axis=2).astype(np.uint32)


def _sigmoid_parts(z):
    e = np.exp(-np.abs(z))
    hi = 1.0 / (1.0 + e)
    return e, hi, e * hi  # exp(-|z|), sigma(|z|), sigma(-|z|)


def _segment_sums(terms, starts):
    """(S, C) sums and sums of magnitudes of the (nnz, C) terms over the latents' segments, in extended precision."""
    n_latents = starts.size - 1
    out = np.zeros((n_latents, terms.shape[1]), dtype=np.longdouble)
    mag = np.zeros_like(out)
    full = np.flatnonzero(np.diff(starts))
    if full.size:
        ext = terms.astype(np.longdouble)
        out[full] = np.add.reduceat(ext, starts[full], axis=0)
        mag[full] = np.add.reduceat(np.abs(ext), starts[full], axis=0)
    return out.astype(np.float64), mag.astype(np.float64)


def _event_logits(starts, vals, b, w):
    lat = np.repeat(np.arange(starts.size - 1), np.diff(starts))
    v = vals.astype(np.float64)[:, None]
    return b[lat] + w[lat] * v, v


def event_sums(starts, rows, vals, ymat, b, w):
    """The seven event sums of every pair at the given (b, w): (sums, magnitudes), each (S, 7, C)."""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        z, v = _event_logits(starts, vals, b, w)
        y = ymat[rows]
        e, hi, lo = _sigmoid_parts(z)
        mu = np.where(z >= 0, hi, lo)
        om = np.where(z >= 0, lo, hi)
        s = hi * lo
        loss = np.where(y, np.maximum(-z, 0), np.maximum(z, 0)) + np.log1p(e)
        terms = (mu, np.where(y, -om, mu) * v, s, s * v, s * v * v, loss, y.astype(np.float64))
        both = [_segment_sums(t, starts) for t in terms]
    return np.stack([a for a, _ in both], axis=1), np.stack([m for _, m in both], axis=1)


def base_intercept(pos, n):
    pi = np.clip(np.asarray(pos, dtype=np.float64) / n, EPS, 1 - EPS)
    return np.log(pi / (1 - pi))


def init_state(n_latents, pos, n, hp):
    c = len(pos)
    nan = np.full((n_latents, c), np.nan)
    return dict(b=np.tile(base_intercept(pos, n), (n_latents, 1)), w=np.zeros((n_latents, c)), lam=np.full((n_latents, c), hp.lam_init),
                prev_pred=nan.copy(), prev_loss=nan.copy(), clipped=np.zeros((n_latents, c), dtype=bool))


def _sigma(z):
    _, hi, lo = _sigmoid_parts(z)
    return np.where(z >= 0, hi, lo)


def update(sums, state, counts, qx, pos, n, hp):
    """One solver iteration of every pair from its event sums: (new state, info)."""
    with np.errstate(all="ignore"):
        b, w, lam = state["b"], state["w"], state["lam"].copy()
        n = float(n)
        pi = (np.asarray(pos, dtype=np.float64) / n)[None, :]
        base = base_intercept(pos, n)[None, :]
        nnz = np.asarray(counts, dtype=np.float64)[:, None]
        empty = np.broadcast_to(nnz == 0, b.shape)
        qx_sq = np.broadcast_to((qx * qx)[:, None], b.shape)
        qxr = np.sqrt(qx_sq)
        mu0 = np.clip(_sigma(b), EPS, 1 - EPS)
        s0 = mu0 * (1 - mu0)
        zf = np.maximum(n - nnz, 0.0) / n
        g0 = sums[:, 0] / n + zf * mu0 - pi
        g0 = g0 + hp.ridge * (b - base)
        g1 = sums[:, 1] / n + hp.ridge * w
        h0 = sums[:, 2] / n + zf * s0 + hp.ridge
        h1 = sums[:, 3] / n
        h2 = sums[:, 4] / n + hp.ridge
        pos_zero = np.minimum(np.maximum(pi - sums[:, 6] / n, 0.0), zf)
        neg_zero = zf - pos_zero
        zero_loss = -(pos_zero * np.log(mu0) + neg_zero * np.log1p(-np.minimum(mu0, 1 - EPS)))
        loss = sums[:, 5] / n + zero_loss + 0.5 * hp.ridge * (w * w + (b - base) * (b - base))
        g0 = np.where(empty, 0.0, g0)
        g1 = np.where(empty, 0.0, g1)
        lam = np.where(empty, hp.lam_init, lam)

        flags = np.zeros(b.shape, dtype=np.int32)
        prev = np.isfinite(state["prev_pred"]) & np.isfinite(state["prev_loss"])
        rho = (state["prev_loss"] - loss) / np.maximum(state["prev_pred"], 1e-18)
        grow = prev & ((rho <= 0.25) | state["clipped"])
        shrink = prev & (rho >= 0.75) & ~state["clipped"]
        lam = np.where(shrink, lam * hp.lam_shrink, lam)
        lam = np.where(grow, lam * hp.lam_grow, lam)
        lam = np.where(prev, np.clip(lam, LAM_MIN, LAM_MAX), lam)
        flags |= np.where(shrink, SHRUNK, 0) | np.where(grow, GROWN, 0)

        success = np.maximum(np.abs(g0), np.abs(g1)) <= hp.tol
        flags |= np.where(success, INACTIVE, 0)
        db, dw, pred = np.zeros_like(b), np.zeros_like(b), np.zeros_like(b)
        clipped = np.zeros(b.shape, dtype=bool)
        tries = np.zeros(b.shape, dtype=np.int32)
        for _ in range(5):
            active = ~success
            tries += active
            h0e, h2e = h0 + lam, h2 + lam * qx_sq
            det = h0e * h2e - h1 * h1
            valid = np.abs(det) > 1e-18
            ds = np.where(valid, det, 1.0)
            dbt = np.where(valid, (h2e * g0 - h1 * g1) / ds, 0.0)
            dwt = np.where(valid, (h0e * g1 - h1 * g0) / ds, 0.0)
            flags |= np.where(active & ~valid, SINGULAR, 0)
            qd = qxr * dwt
            norm = np.sqrt(dbt * dbt + qd * qd)
            clip = norm > hp.delta_logit
            scale = np.where(clip, hp.delta_logit / (norm + 1e-18), 1.0)
            dbt, dwt = dbt * scale, dwt * scale
            predt = g0 * dbt + g1 * dwt - 0.5 * (h0 * (dbt * dbt) + 2.0 * h1 * dbt * dwt + h2 * (dwt * dwt))
            ok = active & np.isfinite(predt) & (predt > 0)
            db, dw, pred, clipped = np.where(ok, dbt, db), np.where(ok, dwt, dw), np.where(ok, predt, pred), np.where(ok, clip, clipped)
            lam = np.where(active & ~ok, np.clip(lam * hp.lam_grow, LAM_MIN, LAM_MAX), lam)
            success = success | ok
        failed = ~success
        qg = np.maximum(qxr, 1e-12) * g1
        gs = np.sqrt(g0 * g0 + qg * qg)
        alpha = np.where(gs > 0, (FALLBACK * hp.delta_logit) / (gs + 1e-18), 0.0)
        db, dw = np.where(failed, -alpha * g0, db), np.where(failed, -alpha * g1, dw)
        pred = np.where(failed, np.nan, pred)
        clipped = clipped | failed
        flags |= np.where(failed, FALLBACK_FLAG, 0) | np.where(clipped, CLIPPED, 0)
        lam = np.clip(lam, LAM_MIN, LAM_MAX)
        nb, nw = b - db, w - dw
        nb, nw = np.where(empty, base, nb), np.where(empty, 0.0, nw)
        lam = np.where(empty, hp.lam_init, lam)
        db, dw = np.where(empty, 0.0, db), np.where(empty, 0.0, dw)
        pred = np.where(empty, np.nan, pred)
        clipped = clipped & ~empty
        flags = np.where(empty, (flags & ~CLIPPED) | EMPTY, flags)
        grad = np.maximum(np.abs(g0), np.abs(g1 / np.maximum(qxr, 1e-12)))
    new = dict(b=nb, w=nw, lam=lam, prev_pred=pred, prev_loss=loss, clipped=clipped)
    info = dict(db=db, dw=dw, pred=pred, lam=lam, flags=flags, tries=tries, grad=grad, g0=g0, g1=g1, h0=h0, h1=h1, h2=h2, loss=loss)
    return new, info


def fit(indptr, indices, data, n_latents, y, n_classes, hp):
    """The whole fit: (intercept, coef, n_iter per class, qx), fp64."""
    starts, rows, vals, qx = prepare(indptr, indices, data, n_latents)
    ymat = labels_matrix(y, n_classes)
    n = ymat.shape[0]
    pos = ymat.sum(axis=0)
    counts = np.diff(starts)
    state = init_state(n_latents, pos, n, hp)
    n_iter = np.zeros(n_classes, dtype=np.int32)
    slabs = [(c0, min(c0 + hp.class_slab_size, n_classes)) for c0 in range(0, n_classes, hp.class_slab_size)]
    running = [True] * len(slabs)
    for _ in range(hp.max_iter):
        if not any(running):
            break
        sums, _ = event_sums(starts, rows, vals, ymat, state["b"], state["w"])
        new, info = update(sums, state, counts, qx, pos, n, hp)
        for i, (c0, c1) in enumerate(slabs):
            if not running[i]:
                continue
            for k in state:
                state[k][:, c0:c1] = new[k][:, c0:c1]
            n_iter[c0:c1] += 1
            if np.all(info["grad"][:, c0:c1] <= hp.tol):
                running[i] = False
    return state["b"], state["w"], n_iter, qx


def _softplus(x):
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def evaluate(indptr, indices, data, n_latents, y, n_classes, b, w, threshold=0.5):
    """(loss, tp, fp, tn, fn, loss magnitudes): fp64 (S, C); the counts are exact integers."""
    starts, rows, vals, _ = prepare(indptr, indices, data, n_latents)
    ymat = labels_matrix(y, n_classes)
    n = float(ymat.shape[0])
    with np.errstate(over="ignore", under="ignore"):
        z, _ = _event_logits(starts, vals, b, w)
        yy = ymat[rows]
        e, hi, lo = _sigmoid_parts(z)
        mu = np.where(z >= 0, hi, lo)
        loss_nz, loss_mag = _segment_sums(np.where(yy, np.maximum(-z, 0), np.maximum(z, 0)) + np.log1p(e), starts)
        pred = mu > threshold
        pos_nz = _segment_sums(yy.astype(np.float64), starts)[0]
        tp_nz = _segment_sums((pred & yy).astype(np.float64), starts)[0]
        fp_nz = _segment_sums((pred & ~yy).astype(np.float64), starts)[0]
        nnz = np.diff(starts).astype(np.float64)[:, None]
        n_zero = n - nnz
        pos_zero = np.minimum(np.maximum(ymat.sum(axis=0)[None, :] - pos_nz, 0.0), n_zero)
        neg_zero = n_zero - pos_zero
        zp, zn = pos_zero * _softplus(-b), neg_zero * _softplus(b)
        loss = (loss_nz + zp + zn) / n
        pz = _sigma(b) > threshold
    tp = tp_nz + np.where(pz, pos_zero, 0.0)
    fp = fp_nz + np.where(pz, neg_zero, 0.0)
    fn = (pos_nz - tp_nz) + np.where(pz, 0.0, pos_zero)
    tn = (nnz - pos_nz - fp_nz) + np.where(pz, 0.0, neg_zero)
    return loss, tp, fp, tn, fn, (loss_mag + zp + zn) / n
