"""The LATENT AP contract of include/saev_amd.h restated in numpy / Python floats, and the same sums at high precision.

One walker (``_walk``) turns a CSR matrix and one class per row into the tie groups of every latent -- its distinct positive values
descending, the zero group in closed form, its distinct negative values descending -- and hands (t, n, R, r) of every (group, class)
with r > 0 to a term function, adding the terms of a pair in group order.  Two term functions:

  ``term_f64``    the library's arithmetic in Python floats (IEEE fp64, every operation rounded on its own): the direct sum up to
                  DIRECT_MAX rows, the closed form with H_{t+n} - H_t from log1p and the differences of the asymptotic terms above
  ``ExactTerms``  ``decimal`` at 80 significant digits: the closed form with harmonic numbers from a table.  H_m <= 23 and a
                  difference is at least 1 / N > 1e-10, so a difference of two entries keeps more than 65 digits.

``sorted_events`` is the one answer of the library's sort: the events by (latent, value descending, row ascending).
"""

from __future__ import annotations

import decimal
import math

import numpy as np

DIRECT_MAX = 8  # saev_latent_ap_layout.direct_max (tests/test_latent_ap_host_cpu.py compares)
H_SMALL = 32


def value_key(v: np.ndarray) -> np.ndarray:
    """The workspace's key: ~k(v), k the order-preserving uint32 image of an fp32 value (ascending key = descending value)."""
    b = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)
    k = np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000))
    return (~k).astype(np.uint32)


def sorted_events(indptr, indices, data, n_latents):
    """(starts (S + 1), latent, value, row) of the events sorted by (latent, value descending, row ascending)."""
    indptr = np.asarray(indptr, dtype=np.int64)
    n, p0 = len(indptr) - 1, int(indptr[0])
    nnz = int(indptr[-1]) - p0
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr))
    lat = np.asarray(indices)[p0:p0 + nnz].astype(np.int64)
    val = np.asarray(data, dtype=np.float32)[p0:p0 + nnz]
    keep = val != 0
    rows, lat, val = rows[keep], lat[keep], val[keep]
    order = np.lexsort((rows, value_key(val), lat))
    rows, lat, val = rows[order], lat[order], val[order]
    starts = np.searchsorted(lat, np.arange(n_latents + 1)).astype(np.int64)
    return starts, lat, val, rows


def _walk(indptr, indices, data, n_rows, n_latents, cls, n_classes, term, zero, add=lambda a, b: a + b):
    """ap numerators (S x C array of whatever ``term`` returns, summed in group order), pos (C), events per pair (S x C)."""
    cls = np.asarray(cls).astype(np.int64)
    assert cls.shape == (n_rows,) and cls.min() >= -1 and cls.max() < n_classes
    pos = np.bincount(cls[cls >= 0], minlength=n_classes).astype(np.int64)
    starts, _, val, rows = sorted_events(indptr, indices, data, n_latents)
    sums = np.full((n_latents, n_classes), zero, dtype=object)
    n_ev = np.zeros((n_latents, n_classes), dtype=np.int64)
    for j in range(n_latents):
        v, cl = val[starts[j]:starts[j + 1]], cls[rows[starts[j]:starts[j + 1]]]
        m = len(v)
        total = np.bincount(cl[cl >= 0], minlength=n_classes)
        n_ev[j] = total
        heads = np.flatnonzero(np.concatenate([[True], v[1:] != v[:-1]])) if m else np.zeros(0, dtype=np.int64)
        ends = np.concatenate([heads[1:], [m]]).astype(np.int64)
        n_pos_ev = int((v > 0).sum())
        R = np.zeros(n_classes, dtype=np.int64)
        acc = sums[j]

        def zero_group(t):
            z = n_rows - m
            if z > 0:
                r = pos - total
                for c in np.flatnonzero(r > 0):
                    acc[c] = add(acc[c], term(t, z, int(R[c]), int(r[c])))
                R[:] += r

        done = False
        for h, e in zip(heads, ends):
            if not done and h >= n_pos_ev:
                zero_group(int(h))
                done = True
            t = int(h) + (n_rows - m if done else 0)
            g = cl[h:e]
            g = g[g >= 0]
            if len(g) == 1:
                c = int(g[0])
                acc[c] = add(acc[c], term(t, int(e - h), int(R[c]), 1))
                R[c] += 1
            elif len(g):
                r = np.bincount(g, minlength=n_classes)
                for c in np.flatnonzero(r):
                    acc[c] = add(acc[c], term(t, int(e - h), int(R[c]), int(r[c])))
                R += r
        if not done:
            zero_group(m)
    return sums, pos, n_ev


# ---------------------------------------------------------------- fp64, as the library ----------------------------------------------------

def dh_asym(t: float, n: float) -> float:
    m = t + n
    it, im = 1.0 / t, 1.0 / m
    it2, im2 = it * it, im * im
    it4, im4 = it2 * it2, im2 * im2
    corr = -((im4 * im4) * im2 - (it4 * it4) * it2) / 132.0
    corr = corr + (im4 * im4 - it4 * it4) / 240.0
    corr = corr - (im4 * im2 - it4 * it2) / 252.0
    corr = corr + (im4 - it4) / 120.0
    corr = corr + (n * (t + m)) * (it2 * im2) / 12.0
    corr = corr - n / ((2.0 * t) * m)
    return math.log1p(n / t) + corr


def dh(t: int, n: int) -> float:
    """H_{t+n} - H_t as the library forms it."""
    hi = t + n
    if t >= H_SMALL:
        return dh_asym(float(t), float(n))
    direct = 0.0
    for p in range(min(hi, H_SMALL), t, -1):
        direct = direct + 1.0 / float(p)
    if hi <= H_SMALL:
        return direct
    return direct + dh_asym(float(H_SMALL), float(hi - H_SMALL))


def term_f64(t: int, n: int, R: int, r: int) -> float:
    if r == 0:
        return 0.0
    if n == 1:
        return float(r * (R + 1)) / float(t + 1)
    rn = float(r) / float(n)
    a = float(r - 1) / float(n - 1)
    if n <= DIRECT_MAX:
        s = 0.0
        for q in range(n):
            s = s + (rn * (float(R + 1) + float(q) * a)) / float(t + 1 + q)
        return s
    return rn * ((float(R + 1) - a * float(t + 1)) * dh(t, n) + a * float(n))


def latent_ap(indptr, indices, data, n_rows, n_latents, cls, n_classes):
    """(ap (S, C) float64, pos (C) int64, events per pair (S, C) int64): the contract in fp64."""
    sums, pos, n_ev = _walk(indptr, indices, data, n_rows, n_latents, cls, n_classes, term_f64, 0.0)
    sums = sums.astype(np.float64)
    ap = np.where(pos > 0, sums / np.maximum(pos, 1).astype(np.float64), 0.0)
    return ap, pos, n_ev


def best(ap):
    """(best_ap, best_class): the row maximum and the lowest column that attains it."""
    k = np.argmax(ap, axis=1)
    return ap[np.arange(ap.shape[0]), k], k.astype(np.int32)


# ---------------------------------------------------------------- high precision ----------------------------------------------------------

class ExactTerms:
    """term(g, c) at 80 significant digits (the closed form holds for every n >= 2; for n = 1 it is r (R + 1) / (t + 1))."""

    def __init__(self, n_rows: int):
        self.ctx = decimal.Context(prec=80)
        one = decimal.Decimal(1)
        h = [decimal.Decimal(0)]
        for p in range(1, n_rows + 1):
            h.append(self.ctx.add(h[-1], self.ctx.divide(one, decimal.Decimal(p))))
        self.h = h

    def __call__(self, t, n, R, r):
        D, c = decimal.Decimal, self.ctx
        if n == 1:
            return c.divide(D(r * (R + 1)), D(t + 1))
        a = c.divide(D(r - 1), D(n - 1))
        d = c.subtract(self.h[t + n], self.h[t])
        inner = c.add(c.multiply(c.subtract(D(R + 1), c.multiply(a, D(t + 1))), d), c.multiply(a, D(n)))
        return c.divide(c.multiply(D(r), inner), D(n))


def exact_ap(indptr, indices, data, n_rows, n_latents, cls, n_classes):
    """(ap (S, C): the exact value rounded once to float64, pos, events per pair)."""
    terms = ExactTerms(n_rows)
    sums, pos, n_ev = _walk(indptr, indices, data, n_rows, n_latents, cls, n_classes, terms, decimal.Decimal(0), terms.ctx.add)
    ap = np.zeros(sums.shape, dtype=np.float64)
    for j in range(sums.shape[0]):
        for c in range(sums.shape[1]):
            if pos[c] > 0 and sums[j, c] != 0:
                ap[j, c] = float(terms.ctx.divide(sums[j, c], decimal.Decimal(int(pos[c]))))
    return ap, pos, n_ev


def bound(n_ev):
    """|ap - exact| <= (n_{j,c} + 2) 2^-49: a pair has n_{j,c} + 1 terms of at most about 16 roundings of 2^-53 each, every piece of
    a term being at most 1 in AP units."""
    return (n_ev.astype(np.float64) + 2.0) * 2.0 ** -49


def ulps32(a, b):
    """Distance of two float32 arrays of non-negative values in units of the last place."""
    a = np.ascontiguousarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    b = np.ascontiguousarray(b, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.abs(a - b)
