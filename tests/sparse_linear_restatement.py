"""A numpy restatement of the SPARSE LINEAR contract (include/saev_amd.h) that the tests and the fixture generator
lean on: the pooling of a token CSR to image rows, the objective, gradient and KKT residual of the L1-penalised logistic regression
in float64, and a plain float64 FISTA with backtracking and function-value restart that follows the library's decisions (its sums
are numpy's, so its bits are not the library's).  No device, no scikit-learn."""

import numpy as np


# ---------------------------------------------------------------- pooling --------------------------------------------------------------

def pool_images(indptr, indices, data, n_images, tpi, n_latents, agg):
    """(n_images, n_latents) float32: per image and latent the maximum of the tpi dense values (an implicit 0 competes where the latent
    is stored in fewer than tpi patches), or the float32 sum of the stored values in patch order divided once by float32(tpi)."""
    indptr = np.asarray(indptr, dtype=np.int64)
    indices = np.asarray(indices)
    data = np.asarray(data, dtype=np.float32)
    out = np.zeros((n_images, n_latents), dtype=np.float32)
    for i in range(n_images):
        acc = np.zeros(n_latents, dtype=np.float32) if agg == "mean" else np.full(n_latents, -np.inf, dtype=np.float32)
        cnt = np.zeros(n_latents, dtype=np.int64)
        for p in range(tpi):
            lo, hi = indptr[i * tpi + p], indptr[i * tpi + p + 1]
            c, v = indices[lo:hi], data[lo:hi]
            if agg == "mean":
                acc[c] = acc[c] + v  # (distinct columns within a row: one float32 addition each)
            else:
                acc[c] = np.maximum(acc[c], v)
                cnt[c] += 1
        out[i] = acc / np.float32(tpi) if agg == "mean" else np.where(cnt < tpi, np.maximum(acc, np.float32(0)), acc)
    return out


# ---------------------------------------------------------------- the problem ----------------------------------------------------------

def class_indices(y):
    """(classes, index of each y in classes)."""
    classes, inv = np.unique(np.asarray(y), return_inverse=True)
    return classes, inv.astype(np.int64)


def _loss_and_resid(Z, yi, K):
    """(sum of the rows' losses, r = p - onehot) from the logits Z (n, coef_rows)."""
    if K == 2:
        v = Z[:, 0]
        t = np.where(yi == 1, 1.0, -1.0)
        e = np.exp(-np.abs(v))
        p = np.where(v >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
        return float((np.maximum(-t * v, 0.0) + np.log1p(e)).sum()), (p - (yi == 1))[:, None]
    m = Z.max(axis=1, keepdims=True)
    lse = m[:, 0] + np.log(np.exp(Z - m).sum(axis=1))
    r = np.exp(Z - lse[:, None])
    r[np.arange(len(yi)), yi] -= 1.0
    return float((lse - Z[np.arange(len(yi)), yi]).sum()), r


def objective(X, yi, K, W, b, C):
    """F(W, b) = C * sum_i loss_i + ||W||_1 in float64."""
    X = np.asarray(X, dtype=np.float64)
    loss, _ = _loss_and_resid(X @ np.asarray(W, dtype=np.float64).T + np.asarray(b, dtype=np.float64), yi, K)
    return C * loss + float(np.abs(W).sum())


def gradient(X, yi, K, W, b, C):
    """(g = C dLoss/dW, g_b = C dLoss/db) in float64."""
    X = np.asarray(X, dtype=np.float64)
    _, r = _loss_and_resid(X @ np.asarray(W, dtype=np.float64).T + np.asarray(b, dtype=np.float64), yi, K)
    return C * (r.T @ X), C * r.sum(axis=0)


def kkt_terms(W, g, g_b):
    """The stopping rule: |g + sign(w)| where w != 0, max(|g| - 1, 0) where w == 0, |g_b| for an intercept; the largest of them."""
    res = np.where(W != 0, np.abs(g + np.sign(W)), np.maximum(np.abs(g) - 1.0, 0.0))
    return max(float(res.max()), float(np.abs(g_b).max()))


def kkt_residual(X, yi, K, W, b, C):
    return kkt_terms(np.asarray(W), *gradient(X, yi, K, W, b, C))


def gradient_rounding(X, n, K, C):
    """(n + K + 4) 2^-52 C max_j sum_i |x_ij|: the rounding of one gradient element's float64 sum."""
    return (n + K + 4) * 2.0 ** -52 * C * float(np.abs(np.asarray(X, dtype=np.float64)).sum(axis=0).max())


def objective_rounding(X, W, b, C, F):
    """A bound on the rounding of objective(): the n + S K non-negative terms summed in float64 (each partial sum at most F), and the
    dot products inside the logits (an error of at most (S + 2) 2^-52 (|x_i| . |w_k| + |b_k|) each) through the loss, which is
    2-Lipschitz in the largest error of a row's logits."""
    X, W = np.abs(np.asarray(X, dtype=np.float64)), np.abs(np.asarray(W, dtype=np.float64))
    n, S = X.shape
    logits = float((X @ W.T + np.abs(np.asarray(b))).max(axis=1).sum())
    return 2.0 ** -52 * ((n + S * W.shape[0] + 8) * abs(F) + 2.0 * C * (S + 2) * logits)


def ranked_support(W):
    """The non-zero features in the order of argsort(-sum |coef_|, stable)."""
    imp = np.abs(np.asarray(W)).sum(axis=0)
    order = np.argsort(-imp, kind="stable")
    return order[imp[order] > 0]


# ---------------------------------------------------------------- the solver -----------------------------------------------------------

def fista(X, y, C, kkt_tol=1e-4, max_iter=5000):
    """dict(coef, intercept, classes, n_iter, kkt, objective, converged, L) of FISTA with backtracking on L (start 1, doubling) and
    function-value restart; the KKT residual is evaluated at the extrapolated point y, which is returned when it is within kkt_tol."""
    X = np.asarray(X, dtype=np.float64)
    classes, yi = class_indices(y)
    K = len(classes)
    if K < 2:
        raise ValueError("fewer than two classes")
    n, S = X.shape
    R = 1 if K == 2 else K
    X1 = np.concatenate([X, np.ones((n, 1))], axis=1)  # the intercept is column S
    W = np.zeros((R, S + 1))
    Wp = W.copy()
    Z, Zp = np.zeros((n, R)), np.zeros((n, R))
    L, t, beta, F = 1.0, 1.0, 0.0, C * n * np.log(K)
    need, it, done = True, 0, False
    g = fy = l1y = kkt = None
    pen = np.ones(S + 1)
    pen[S] = 0.0
    while it < max_iter:
        it += 1
        Y = W + beta * (W - Wp)
        if need:
            loss_y, r = _loss_and_resid(Z + beta * (Z - Zp), yi, K)
            g, fy = C * (r.T @ X1), C * loss_y
            l1y = float(np.abs(Y[:, :S]).sum())
            kkt = kkt_terms(Y[:, :S], g[:, :S], g[:, S])
        if kkt <= kkt_tol:
            done = True
            break
        U = Y - g / L
        Wn = np.where(pen > 0, np.sign(U) * np.maximum(np.abs(U) - 1.0 / L, 0.0), U)
        Zn = X1 @ Wn.T
        fn = C * _loss_and_resid(Zn, yi, K)[0]
        d = Wn - Y
        if not fn <= fy + float((g * d).sum()) + 0.5 * L * float((d * d).sum()) + 1e-12 * abs(fy):
            L, need = 2.0 * L, False
            continue
        need = True
        Fn = fn + float(np.abs(Wn[:, :S]).sum())
        if beta != 0.0 and Fn > F:
            t, beta = 1.0, 0.0
            continue
        tn = 0.5 * (1.0 + np.sqrt(1.0 + 4.0 * t * t))
        beta, t, F = (t - 1.0) / tn, tn, Fn
        Wp, W, Zp, Z = W, Wn, Z, Zn
    out = W + beta * (W - Wp) if done else W
    coef, b = out[:, :S].copy(), out[:, S].copy()
    if K > 2:
        b -= b.mean()
    return dict(coef=coef, intercept=b, classes=classes, n_iter=it, kkt=kkt_residual(X, yi, K, coef, b, C), objective=objective(X, yi, K, coef, b, C),
                converged=done, L=L)
