"""The exactness check of a TopK encode that the GPU tests share: every row against an fp64 product."""

import torch


def assert_topk_exact(x, idx, val, W_enc, b_enc, what=""):
    """x (b, d), codes idx / val (b, k), W_enc (d, s), b_enc (s), all on one device.  On EVERY row, in slabs of 512, against
    h = x W_enc + b_enc in fp64: (a) each emitted value is the pre-activation at its emitted latent and (b) nothing left out
    exceeds the smallest kept value -- both to the rounding of a d-term fp32 dot product,
    tol_b = 8 * 2^-24 * ||x_b|| * max_s ||W_enc[:, s]||.  (b) and not set equality with the fp64 top-k: where the k-th and
    (k+1)-th pre-activation of a row lie closer than tol_b, a correct fp32 result may keep either.
    Returns the worst value error and the worst cut excess, in units of tol_b."""
    b = x.shape[0]
    st_idx = idx.long()
    W, be = W_enc.double(), b_enc.double()
    wmax = W.norm(dim=0).max().item()
    worst_val = worst_cut = 0.0
    for lo in range(0, b, 512):
        rows = slice(lo, min(b, lo + 512))
        h = x[rows].double() @ W + be
        tol = 8.0 * 2.0 ** -24 * x[rows].double().norm(dim=1) * wmax
        err = (h.gather(1, st_idx[rows]) - val[rows].double()).abs().amax(dim=1)
        worst_val = max(worst_val, (err / tol).max().item())
        assert (err <= tol).all(), f"{what}rows {lo}..: value error {err.max().item():.3e} > tol {tol.min().item():.3e}"
        kth = val[rows].min(dim=1).values.double()
        over = h.scatter(1, st_idx[rows], float("-inf")).amax(dim=1) - kth
        worst_cut = max(worst_cut, (over / tol).max().item())
        assert (over <= tol).all(), f"{what}rows {lo}..: a left-out pre-activation exceeds the smallest kept one by {over.max().item():.3e}"
        del h
    return worst_val, worst_cut
