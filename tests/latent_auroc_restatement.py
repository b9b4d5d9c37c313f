"""The LATENT AUROC contract of include/saev_amd.h restated in numpy with Python integers, three ways:

  ``one_walk``   the contract's form: one forward walk of a latent's events in (value descending, row ascending) order as if the rows
                 without an event were absent, then the closed-form correction  2 q0 Ppos + p0 q0 + 2 p0 Qneg.
  ``by_pairs``   the DEFINITION: every (positive, negative) pair of a dense column counted, 2 when the positive's activation is
                 strictly larger, 1 when the two are equal.  O(n^2): for small designs.
  ``by_ranks``   U2 = 2 (rank sum of the positives) - n_pos (n_pos + 1) from ``scipy.stats.rankdata``'s average ranks (the
                 reference's formulation), vectorised: for the larger designs.

All three return the entry's outputs: ``u2``, ``fire_pos``, ``fire_neg`` (S x T, Python integers in int64 arrays), ``n_pos``,
``n_neg`` (T), ``sum_pos``, ``sum_neg`` (S x T float64: the role's event values added one at a time in walk order, from +0),
``auroc`` (``auroc_of``) and ``n_ev_pos`` / ``n_ev_neg`` (S x T: how many values each sum received)."""

from __future__ import annotations

import math

import numpy as np
from scipy.stats import rankdata

from latent_ap_restatement import sorted_events


def task_counts(cls, roles):
    """(n_pos (T), n_neg (T), pos (C)) of one class per row (-1: none) and a T x C role matrix."""
    roles = np.asarray(roles)
    cls = np.asarray(cls)
    pos = np.bincount(cls[cls >= 0], minlength=roles.shape[1]).astype(np.int64)
    return (pos[None, :] * (roles == 2)).sum(axis=1), (pos[None, :] * (roles == 1)).sum(axis=1), pos


def auroc_of(u2, n_pos, n_neg):
    """u2 / (2.0 * n_pos * n_neg) in fp64, every operation rounded on its own; NaN where n_pos n_neg = 0."""
    out = np.full(u2.shape, np.nan)
    for t in range(u2.shape[1]):
        if n_pos[t] > 0 and n_neg[t] > 0:
            den = (2.0 * float(n_pos[t])) * float(n_neg[t])
            out[:, t] = [float(int(u)) / den for u in u2[:, t]]
    return out


def _row_roles(cls, roles):
    """(T x N) role of every row in every task; a row of class -1 has role 0."""
    roles = np.asarray(roles, dtype=np.uint8)
    table = np.concatenate([np.zeros((roles.shape[0], 1), dtype=np.uint8), roles], axis=1)
    return table[:, np.asarray(cls, dtype=np.int64) + 1]


def _sequential_sum(values):
    """values[0] + values[1] + ... in fp64 from +0, one addition at a time (np.add.accumulate is sequential)."""
    with np.errstate(invalid="ignore", over="ignore"):
        return float(np.add.accumulate(np.concatenate([[0.0], values.astype(np.float64)]))[-1])


def _empty(s, t):
    z = lambda dt: np.zeros((s, t), dtype=dt)  # noqa: E731
    return dict(u2=z(np.int64), fire_pos=z(np.int64), fire_neg=z(np.int64), sum_pos=z(np.float64), sum_neg=z(np.float64), n_ev_pos=z(np.int64),
                n_ev_neg=z(np.int64), abs_pos=z(np.float64), abs_neg=z(np.float64), fsum_pos=z(np.float64), fsum_neg=z(np.float64))


def _finish(out, cls, roles):
    out["n_pos"], out["n_neg"], out["pos"] = task_counts(cls, roles)
    out["auroc"] = auroc_of(out["u2"], out["n_pos"], out["n_neg"])
    return out


def _sums(out, j, t, val, r):
    """The per-role sums and supports of latent j, task t from its events in walk order (val) and their roles (r)."""
    for name, role in (("pos", 2), ("neg", 1)):
        v = val[r == role]
        out[f"sum_{name}"][j, t] = _sequential_sum(v)
        out[f"n_ev_{name}"][j, t] = len(v)
        out[f"fire_{name}"][j, t] = int((v > 0).sum())
        finite = v[np.isfinite(v)].astype(np.float64)
        out[f"abs_{name}"][j, t] = math.fsum(np.abs(finite).tolist())
        out[f"fsum_{name}"][j, t] = math.fsum(finite.tolist()) if len(finite) == len(v) else np.nan


def one_walk(indptr, indices, data, n_rows, n_latents, cls, roles):
    """The contract's walk, literally, in Python integers."""
    roles = np.asarray(roles, dtype=np.uint8)
    n_tasks = roles.shape[0]
    starts, _, val, rows = sorted_events(indptr, indices, data, n_latents)
    row_role = _row_roles(cls, roles)
    n_pos, n_neg, _ = task_counts(cls, roles)
    out = _empty(n_latents, n_tasks)
    for j in range(n_latents):
        v_j, r_j = val[starts[j]:starts[j + 1]], rows[starts[j]:starts[j + 1]]
        for t in range(n_tasks):
            role = row_role[t, r_j]
            p = q = P = Qev = Ppos = Qneg = U2 = 0
            cur, open_ = None, False
            for v, r in zip(v_j.tolist(), role.tolist()):
                if open_ and v != cur:
                    U2 += q * (2 * P + p)
                    P += p
                    p = q = 0
                cur, open_ = v, True
                isp, isn = int(r == 2), int(r == 1)
                p += isp
                q += isn
                Qev += isn
                if v > 0:
                    Ppos += isp
                else:
                    Qneg += isn
            if open_:
                U2 += q * (2 * P + p)
                P += p
            p0, q0 = int(n_pos[t]) - P, int(n_neg[t]) - Qev
            U2 += 2 * q0 * Ppos + p0 * q0 + 2 * p0 * Qneg
            assert 0 <= U2 <= 2 * int(n_pos[t]) * int(n_neg[t])
            out["u2"][j, t] = U2
            _sums(out, j, t, v_j, role)
            assert out["fire_pos"][j, t] == Ppos and out["fire_neg"][j, t] == Qev - Qneg
    return _finish(out, cls, roles)


def dense_columns(indptr, indices, data, n_rows, n_latents):
    """(n_rows, n_latents) float32: the stored values, 0 elsewhere (a stored +-0.0 is the same activation as no entry)."""
    dense = np.zeros((n_rows, n_latents), dtype=np.float32)
    indptr = np.asarray(indptr, dtype=np.int64)
    rows = np.repeat(np.arange(n_rows), np.diff(indptr))
    p0, p1 = int(indptr[0]), int(indptr[-1])
    dense[rows, np.asarray(indices)[p0:p1]] = np.asarray(data, dtype=np.float32)[p0:p1]
    return dense + np.float32(0)  # -0.0 -> +0.0


def by_pairs(indptr, indices, data, n_rows, n_latents, cls, roles):
    """u2 by the definition: S x T Python integers, every pair counted."""
    roles = np.asarray(roles, dtype=np.uint8)
    dense = dense_columns(indptr, indices, data, n_rows, n_latents)
    row_role = _row_roles(cls, roles)
    u2 = np.zeros((n_latents, roles.shape[0]), dtype=np.int64)
    for t in range(roles.shape[0]):
        pos, neg = dense[row_role[t] == 2], dense[row_role[t] == 1]
        for j in range(n_latents):
            a, b = pos[:, j][:, None], neg[:, j][None, :]
            u2[j, t] = 2 * int((a > b).sum()) + int((a == b).sum())
    return u2


def by_ranks(indptr, indices, data, n_rows, n_latents, cls, roles):
    """The entry's outputs with u2 from average ranks; the sums and supports from the sorted events, vectorised."""
    roles = np.asarray(roles, dtype=np.uint8)
    n_tasks = roles.shape[0]
    starts, _, val, rows = sorted_events(indptr, indices, data, n_latents)
    row_role = _row_roles(cls, roles)
    n_pos, n_neg, _ = task_counts(cls, roles)
    out = _empty(n_latents, n_tasks)
    for j in range(n_latents):
        v_j, r_j = val[starts[j]:starts[j + 1]], rows[starts[j]:starts[j + 1]]
        col = np.zeros(n_rows, dtype=np.float32)
        col[r_j] = v_j
        for t in range(n_tasks):
            inc = row_role[t] > 0
            if n_pos[t] > 0 and n_neg[t] > 0:
                twice = np.round(2 * rankdata(col[inc])).astype(np.int64)  # average ranks are multiples of 1 / 2
                out["u2"][j, t] = int(twice[row_role[t][inc] == 2].sum()) - int(n_pos[t]) * (int(n_pos[t]) + 1)
            _sums(out, j, t, v_j, row_role[t, r_j])
    return _finish(out, cls, roles)


def mean_bound(n, abs_sum):
    """|fp32 mean of n fp32 values, summed in fp32 in any order - their exact mean| <= (n + 2) 2^-24 (sum |a|) / n: (n - 1) additions
    and one division, each within 2^-24 relative, and the cast of the fp64 result this is compared with."""
    return (n + 2) * 2.0 ** -24 * abs_sum / np.maximum(n, 1)
