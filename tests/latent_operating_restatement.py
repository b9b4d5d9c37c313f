"""The LATENT OPERATING POINTS contract of include/saev_amd.h restated in numpy with Python integers and explicit loops.

  ``operating``     per latent the dense column (a row without an event, or with a stored +-0.0, has activation +0) and per task the
                    distinct values of the INCLUDED rows in descending order (``np.unique``); every value is a candidate with
                    TP(v) / FP(v) = the positives / negatives with a >= v, after "predict nothing" (theta = +Inf, TP = FP = 0).  A
                    candidate replaces the best so far only when it is strictly better on the integers, so ties stay with the
                    higher threshold.
  ``by_subsets``    the DEFINITION on tiny inputs: all 2^n subsets of a task's included rows as the predicted set, those a threshold
                    can realise kept, scored with ``fractions.Fraction``.
  ``by_roc_curve``  the same argmax from ``sklearn.metrics.roc_curve(drop_intermediate=False)``.

``operating`` returns the entry's outputs: ``f1``, ``youden`` (S x T float64, formed with the contract's expressions), ``f1_thr``,
``j_thr`` (S x T float32), ``f1_tp``, ``f1_fp``, ``j2``, ``j_tp``, ``j_fp`` (S x T int64), ``n_pos``, ``n_neg`` (T) and ``pos`` (C)."""

from __future__ import annotations

import itertools
from fractions import Fraction

import numpy as np

from latent_auroc_restatement import _row_roles, task_counts

PAIRS_INT = ("f1_tp", "f1_fp", "j2", "j_tp", "j_fp")
PAIRS_F64 = ("f1", "youden")
PAIRS_F32 = ("f1_thr", "j_thr")


def f1_of(tp, fp, n_pos):
    """(2.0 * TP) / (double)(TP + FP + n_pos), one division; NaN when n_pos = 0."""
    return (2.0 * float(tp)) / float(tp + fp + n_pos) if n_pos > 0 else np.nan


def youden_of(j2, n_pos, n_neg):
    """(double)j2 / ((double)n_pos * (double)n_neg); NaN when n_pos n_neg = 0."""
    return float(j2) / (float(n_pos) * float(n_neg)) if n_pos > 0 and n_neg > 0 else np.nan


def best_points(values, is_pos, n_pos, n_neg):
    """The two winners of one (latent, task): ``values`` float32 activations of the included rows, ``is_pos`` their side.  Returns
    ((TP, FP, theta) of the best F1, (J2, TP, FP, theta) of the best J) in Python integers and floats."""
    uniq, inverse = np.unique(values, return_inverse=True)
    p_at = np.bincount(inverse.reshape(-1), weights=is_pos, minlength=len(uniq)).astype(np.int64)
    q_at = np.bincount(inverse.reshape(-1), weights=~is_pos, minlength=len(uniq)).astype(np.int64)
    best_f, best_j = (0, 0, float("inf")), (0, 0, 0, float("inf"))
    tp = fp = 0
    for v, p, q in zip(uniq[::-1].tolist(), p_at[::-1].tolist(), q_at[::-1].tolist()):
        tp, fp = tp + p, fp + q
        if tp * (best_f[0] + best_f[1] + n_pos) > best_f[0] * (tp + fp + n_pos):
            best_f = (tp, fp, v)
        j2 = tp * n_neg - fp * n_pos
        if j2 > best_j[0]:
            best_j = (j2, tp, fp, v)
    assert (tp, fp) == (n_pos, n_neg)
    return best_f, best_j


def operating(indptr, indices, data, n_rows, n_latents, cls, roles):
    """The entry's outputs (see the head of the file).  The latents without a stored entry share one all-zero column: it is worked
    through once."""
    roles = np.asarray(roles, dtype=np.uint8)
    n_tasks = roles.shape[0]
    row_role = _row_roles(cls, roles)
    n_pos, n_neg, pos = task_counts(cls, roles)
    shape = (n_latents, n_tasks)
    out = {k: np.zeros(shape, dtype=np.int64) for k in PAIRS_INT}
    out.update({k: np.full(shape, np.nan) for k in PAIRS_F64})
    out.update({k: np.full(shape, np.inf, dtype=np.float32) for k in PAIRS_F32})
    indptr = np.asarray(indptr, dtype=np.int64)
    p0, p1 = int(indptr[0]), int(indptr[-1])
    ev_rows = np.repeat(np.arange(n_rows), np.diff(indptr))
    ev_cols, ev_vals = np.asarray(indices)[p0:p1], np.asarray(data, dtype=np.float32)[p0:p1]
    order = np.argsort(ev_cols, kind="stable")
    starts = np.searchsorted(ev_cols[order], np.arange(n_latents + 1))
    included = [np.flatnonzero(row_role[t] > 0) for t in range(n_tasks)]
    sides = [row_role[t][included[t]] == 2 for t in range(n_tasks)]

    def column(j, col):
        for t in range(n_tasks):
            np_t, nn_t = int(n_pos[t]), int(n_neg[t])
            (tp, fp, thr), (j2, jtp, jfp, jthr) = best_points(col[included[t]], sides[t], np_t, nn_t)
            out["f1_tp"][j, t], out["f1_fp"][j, t], out["f1_thr"][j, t] = tp, fp, thr
            out["j2"][j, t], out["j_tp"][j, t], out["j_fp"][j, t], out["j_thr"][j, t] = j2, jtp, jfp, jthr
            out["f1"][j, t], out["youden"][j, t] = f1_of(tp, fp, np_t), youden_of(j2, np_t, nn_t)

    empty = np.flatnonzero(np.diff(starts) == 0)
    if len(empty):
        column(empty[0], np.zeros(n_rows, dtype=np.float32))
        for k in out:
            out[k][empty[1:]] = out[k][empty[0]]
    for j in np.flatnonzero(np.diff(starts) > 0):
        col = np.zeros(n_rows, dtype=np.float32)
        at = order[starts[j]:starts[j + 1]]
        col[ev_rows[at]] = ev_vals[at]
        column(j, col + np.float32(0))  # -0.0 -> +0.0
    out["n_pos"], out["n_neg"], out["pos"] = n_pos, n_neg, pos
    return out


def _pick(cands, score):
    """The first candidate that attains the maximum of ``score``: the candidates come in descending threshold order."""
    best = cands[0]
    for c in cands[1:]:
        if score(c) > score(best):
            best = c
    return best


def by_subsets(values, is_pos):
    """((TP, FP, theta) best F1, (J2, TP, FP, theta) best J) of one pair by the definition: every subset of the rows as the predicted
    set; a subset is realisable when some theta has {a >= theta} equal to it, i.e. when it is empty or holds every row at or above its
    lowest value.  The realisable subsets are nested, so "the higher threshold" among equals is the smaller subset.  n <= 12."""
    values, is_pos = np.asarray(values, dtype=np.float32), np.asarray(is_pos, dtype=bool)
    n = len(values)
    assert n <= 12
    n_pos, n_neg = int(is_pos.sum()), int((~is_pos).sum())
    cands = []
    for mask in itertools.product((False, True), repeat=n):
        m = np.array(mask, dtype=bool)
        theta = float(values[m].min()) if m.any() else float("inf")
        if m.any() and not np.array_equal(m, values >= np.float32(theta)):
            continue
        cands.append((int((m & is_pos).sum()), int((m & ~is_pos).sum()), theta, int(m.sum())))
    cands.sort(key=lambda c: c[3])
    assert len({c[3] for c in cands}) == len(cands)
    f = _pick(cands, lambda c: Fraction(2 * c[0], c[0] + c[1] + n_pos) if c[0] + c[1] + n_pos else Fraction(0))
    # (J is defined with both sides present; without one of them J2 is 0 for every candidate and "predict nothing" stays)
    j = _pick(cands, lambda c: Fraction(c[0], n_pos) - Fraction(c[1], n_neg) if n_pos and n_neg else Fraction(0))
    return (f[0], f[1], f[2]), (j[0] * n_neg - j[1] * n_pos, j[0], j[1], j[2])


def by_roc_curve(values, is_pos):
    """The same from ``sklearn.metrics.roc_curve(drop_intermediate=False)``: its leading ``inf`` is "predict nothing" and its
    thresholds descend, so the first index that attains the maximum is the tie rule.  Needs both sides present and finite values."""
    from sklearn.metrics import roc_curve

    values, is_pos = np.asarray(values, dtype=np.float32), np.asarray(is_pos, dtype=bool)
    n_pos, n_neg = int(is_pos.sum()), int((~is_pos).sum())
    fpr, tpr, thr = roc_curve(is_pos, values, drop_intermediate=False)
    tp, fp = np.rint(tpr * n_pos).astype(np.int64).tolist(), np.rint(fpr * n_neg).astype(np.int64).tolist()
    cands = [(a, b, float(np.float32(th))) for a, b, th in zip(tp, fp, thr.tolist())]
    assert cands[0][:2] == (0, 0) and cands[0][2] == float("inf")
    f = _pick(cands, lambda c: Fraction(2 * c[0], c[0] + c[1] + n_pos))
    j = _pick(cands, lambda c: c[0] * n_neg - c[1] * n_pos)
    return (f[0], f[1], f[2]), (j[0] * n_neg - j[1] * n_pos, j[0], j[1], j[2])
