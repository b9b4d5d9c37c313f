"""The PROBE AP contract of include/saev_amd.h restated in numpy / Python floats, and the same sums at high precision.

``pair_groups`` turns one latent's sorted events, one class and one (w, b) into the pair's tie groups in rank order: the score
s(a) = fl(fl(w a) + b) of every event in the score's dtype (numpy rounds each operation on its own), the events walked by descending
value for w >= 0 and by ascending value for w < 0, the zero block of Z rows put in at a = 0 with score b, and maximal runs of equal
score (``==``, so +0 == -0) closed into groups -- which is where the zero block merges with neighbours whose score rounds to b.
Each group is (t, n, R, r, in_zero) with LATENT AP's meaning of t, n, R, r.  The terms, dH, the order of addition and the bound are
those of tests/latent_ap_restatement.py: ``term_f64`` in Python floats as the device forms them, ``ExactTerms`` at 80 digits."""

from __future__ import annotations

import decimal

import numpy as np

from latent_ap_restatement import ExactTerms, bound, dh, sorted_events, term_f64, ulps32  # noqa: F401  (re-exported for the tests)

DTYPES = {0: np.float32, 1: np.float64}


def score(w, a, b, dtype):
    """fl(fl(w a) + b) in ``dtype``; a is float32 and converts exactly."""
    with np.errstate(over="ignore", invalid="ignore"):
        return (np.asarray(a, dtype=np.float32).astype(dtype) * dtype(w) + dtype(b)).astype(dtype)


def pair_groups(val, is_c, n_rows, pos_c, w, b, dtype):
    """(groups, tp, pred_pos) of one pair.  ``val``: the latent's events by descending value; ``is_c``: whether the event's row is
    of the class.  groups: a list of (t, n, R, r, holds_zero_block) in rank order."""
    m = len(val)
    z = n_rows - m
    order = np.arange(m) if w >= 0 else np.arange(m)[::-1]
    v, k = val[order], is_c[order].astype(np.int64)
    first = int((v > 0).sum()) if w >= 0 else int((v < 0).sum())  # events walked before the zero block
    s_ev = score(w, v, b, dtype)
    if z > 0:
        s = np.concatenate([s_ev[:first], score(w, np.zeros(1, np.float32), b, dtype), s_ev[first:]])
        rows = np.concatenate([np.ones(first, np.int64), [z], np.ones(m - first, np.int64)])
        of_c = np.concatenate([k[:first], [pos_c - int(k.sum())], k[first:]])
        zero_at = first
    else:
        s, rows, of_c, zero_at = s_ev, np.ones(m, np.int64), k, -1
    heads = np.flatnonzero(np.concatenate([[True], s[1:] != s[:-1]]))
    n_g, r_g = np.add.reduceat(rows, heads), np.add.reduceat(of_c, heads)
    t_g = np.concatenate([[0], np.cumsum(n_g)[:-1]])
    R_g = np.concatenate([[0], np.cumsum(r_g)[:-1]])
    zero_g = int(np.searchsorted(heads, zero_at, side="right")) - 1 if zero_at >= 0 else -1
    groups = [(int(t), int(n), int(R), int(r), i == zero_g) for i, (t, n, R, r) in enumerate(zip(t_g, n_g, R_g, r_g))]
    above = s > 0
    return groups, int(of_c[above].sum()), int(rows[above].sum())


def _walk(indptr, indices, data, n_rows, n_latents, cls, n_classes, w, b, term, zero, add):
    cls = np.asarray(cls).astype(np.int64)
    assert cls.shape == (n_rows,) and cls.min() >= -1 and cls.max() < n_classes
    w, b = np.asarray(w), np.asarray(b)
    assert w.dtype == b.dtype and w.dtype in (np.float32, np.float64) and w.shape == b.shape == (n_latents, n_classes)
    dtype = w.dtype.type
    pos = np.bincount(cls[cls >= 0], minlength=n_classes).astype(np.int64)
    starts, _, val, rows = sorted_events(indptr, indices, data, n_latents)
    sums = np.full((n_latents, n_classes), zero, dtype=object)
    void = ~(np.isfinite(w) & np.isfinite(b))
    n_ev, tp, pred = (np.zeros((n_latents, n_classes), dtype=np.int64) for _ in range(3))
    reach = dict(merged=0, collapsed=0, inf_ties=0, zero_first=0, zero_inside=0)
    for j in range(n_latents):
        v, cl = val[starts[j]:starts[j + 1]], cls[rows[starts[j]:starts[j + 1]]]
        for c in range(n_classes):
            n_ev[j, c] = int((cl == c).sum())
            if void[j, c]:
                continue
            groups, tp[j, c], pred[j, c] = pair_groups(v, cl == c, n_rows, int(pos[c]), w[j, c], b[j, c], dtype)
            acc = zero
            for t, n, R, r, _ in groups:
                if r > 0:
                    acc = add(acc, term(t, n, R, r))
            sums[j, c] = acc
            z = n_rows - len(v)
            zg = [g for g in groups if g[4]]
            reach["merged"] += bool(zg and zg[0][1] > z and w[j, c] != 0)
            reach["collapsed"] += bool(len(groups) == 1 and len(v) > 1 and w[j, c] != 0)
            reach["zero_first"] += bool(zg and zg[0][0] == 0 and len(groups) > 1)
            reach["zero_inside"] += bool(zg and zg[0][0] > 0 and zg[0][0] + zg[0][1] < n_rows)
            reach["inf_ties"] += bool(np.isinf(score(w[j, c], v, b[j, c], dtype)).sum() > 1)
    return sums, pos, n_ev, tp, pred, void, reach


def _finish(sums, pos, void, to_float):
    ap = np.zeros(sums.shape, dtype=np.float64)
    for j in range(sums.shape[0]):
        for c in range(sums.shape[1]):
            ap[j, c] = np.nan if void[j, c] else to_float(sums[j, c], int(pos[c])) if pos[c] > 0 else 0.0
    return ap


def probe_ap(indptr, indices, data, n_rows, n_latents, cls, n_classes, w, b):
    """dict(ap (S, C) float64, pos, n_ev, tp, pred_pos, reach): the contract in fp64, in the device's order."""
    sums, pos, n_ev, tp, pred, void, reach = _walk(indptr, indices, data, n_rows, n_latents, cls, n_classes, w, b, term_f64, 0.0, lambda x, y: x + y)
    return dict(ap=_finish(sums, pos, void, lambda s, p: float(s) / float(p)), pos=pos, n_ev=n_ev, tp=tp, pred_pos=pred, reach=reach)


def exact_ap(indptr, indices, data, n_rows, n_latents, cls, n_classes, w, b):
    """The same with the terms and sums at 80 digits, rounded once to float64."""
    terms = ExactTerms(n_rows)
    sums, pos, n_ev, tp, pred, void, reach = _walk(indptr, indices, data, n_rows, n_latents, cls, n_classes, w, b, terms, decimal.Decimal(0), terms.ctx.add)
    return dict(ap=_finish(sums, pos, void, lambda s, p: float(terms.ctx.divide(s, decimal.Decimal(p)))), pos=pos, n_ev=n_ev, tp=tp, pred_pos=pred,
                reach=reach)


def top_rows(indptr, indices, data, n_latents, k):
    """(S, k) int64: the rows of every latent's first k events in (value descending, row ascending) order, 0 behind the last."""
    starts, _, _, rows = sorted_events(indptr, indices, data, n_latents)
    out = np.zeros((n_latents, k), dtype=np.int64)
    for j in range(n_latents):
        got = rows[starts[j]:starts[j + 1]][:k]
        out[j, :len(got)] = got
    return out
