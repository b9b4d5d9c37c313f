"""The contract of the latent edits and of the class firing counts (include/saev_amd.h: LATENT EDITS, CLASS FIRING COUNTS),
restated on the host: the edit in fp64 from coefficients that reproduce the kernel's fp32 values, the counts on integers.
A module, not a test file."""

import fractions
import pathlib

import numpy as np

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden"

SET, SCALE, ADD, IF_ACTIVE = 0, 1, 2, 4
U = 2.0 ** -24


def round_f32(r: fractions.Fraction) -> np.float32:
    """The float32 nearest to the exact rational r (ties to even): rounded ONCE, not through fp64."""
    c = np.float32(float(r))
    if not np.isfinite(c):
        return c
    best, best_err = c, abs(fractions.Fraction(float(c)) - r)
    for nb in (np.nextafter(c, np.float32(-np.inf)), np.nextafter(c, np.float32(np.inf))):
        if not np.isfinite(nb):
            continue
        err = abs(fractions.Fraction(float(nb)) - r)
        if err < best_err or (err == best_err and (int(np.float32(nb).view(np.uint32)) & 1) == 0 and (int(np.float32(best).view(np.uint32)) & 1) == 1):
            best, best_err = np.float32(nb), err
    return np.float32(best)


def coefficient(f: np.float32, op: int, value: np.float32):
    """c_e as the kernel forms it in fp32, or None when the edit is skipped."""
    f, value = np.float32(f), np.float32(value)
    if (op & IF_ACTIVE) and f == 0:
        return None
    kind = op & 3
    with np.errstate(all="ignore"):
        if kind == SET:
            c = np.float32(value - f)  # one fp32 subtraction
        elif kind == SCALE:
            if np.isfinite(f) and np.isfinite(value):
                c = round_f32(fractions.Fraction(float(value)) * fractions.Fraction(float(f)) - fractions.Fraction(float(f)))  # fmaf: exact, rounded once
            else:
                c = np.float32(value * f - f)
        else:
            c = value
    return None if c == 0 else np.float32(c)


def latent_value(idx_row, val_row, nnz: int, latent: int) -> np.float32:
    for s in range(nnz):
        if int(idx_row[s]) == latent:
            return np.float32(val_row[s])
    return np.float32(0)


def intervene(x, W, idx, val, row_nnz, edits, n_groups: int, row_group=None, row_keep=None):
    """``edits``: (latent, op, value, group) tuples.  Returns a dict: ``out`` fp64 (n, D) -- rows without a remaining edit hold x
    exactly --, ``mag`` fp64 (n, D) = |x| + sum |c_e| |W[l_e]|, ``m`` (n) applied edits per row, ``rows_changed`` (n_edits) int64,
    ``coef`` per row the list of (latent, c_e)."""
    x = np.asarray(x, dtype=np.float32)
    W = np.asarray(W, dtype=np.float32)
    n, D = x.shape
    cap = idx.shape[1] if idx.ndim == 2 else 0
    lists = [[] for _ in range(n_groups + 1)]
    for i, (latent, op, value, group) in enumerate(edits):
        lists[group + 1].append((i, latent, op, np.float32(value)))
    out = x.astype(np.float64)
    mag = np.abs(x).astype(np.float64)
    m = np.zeros(n, dtype=np.int64)
    changed = np.zeros(len(edits), dtype=np.int64)
    coef = [[] for _ in range(n)]
    for b in range(n):
        if row_keep is not None and not row_keep[b]:
            continue
        todo = list(lists[0])
        if row_group is not None and 0 <= int(row_group[b]) < n_groups:
            todo += lists[int(row_group[b]) + 1]
        nnz = cap if row_nnz is None else min(max(int(row_nnz[b]), 0), cap)
        for i, latent, op, value in todo:
            c = coefficient(latent_value(idx[b], val[b], nnz, latent), op, value)
            if c is None:
                continue
            with np.errstate(all="ignore"):
                out[b] += np.float64(c) * W[latent].astype(np.float64)
                mag[b] += abs(np.float64(c)) * np.abs(W[latent]).astype(np.float64)
            m[b] += 1
            changed[i] += 1
            coef[b].append((latent, c))
    return dict(out=out, mag=mag, m=m, rows_changed=changed, coef=coef)


def _coefficients_fast(f: np.ndarray, op: int, value: np.float32):
    """``coefficient`` on a vector of f: (c float32, applies bool).  SCALE forms value * f exactly in fp64 (48 bits) and
    checks with an error-free two-sum that the fp64 subtraction of f was exact too, so that the conversion to float32 is
    the one rounding of fmaf; an element that fails the check goes through ``coefficient``."""
    f = np.asarray(f, dtype=np.float32)
    value = np.float32(value)
    kind = op & 3
    with np.errstate(all="ignore"):
        if kind == SET:
            c = (value - f).astype(np.float32)
        elif kind == SCALE:
            p = np.float64(value) * f.astype(np.float64)
            b = -f.astype(np.float64)
            s = p + b
            bb = s - p
            exact = ((p - (s - bb)) + (b - bb) == 0) & np.isfinite(s)
            c = s.astype(np.float32)
            for i in np.nonzero(~exact)[0]:
                ci = coefficient(f[i], SCALE, value)
                c[i] = 0 if ci is None else ci
        else:
            c = np.full(f.shape, value, dtype=np.float32)
    applies = c != 0
    if op & IF_ACTIVE:
        applies &= f != 0
    return c, applies


def intervene_fast(x, W, idx, val, row_nnz, edits, n_groups: int, row_group=None, row_keep=None):
    """``intervene`` with the rows of an edit taken together: the same arguments, and ``out``, ``mag``, ``m`` and
    ``rows_changed`` equal to its on the bits (every row receives its edits in the same order -- the global list, then its
    group's, the caller's order inside a list -- through the same fp64 operations).  ``coef`` is replaced by ``applied``:
    for every edit that was applied anywhere, the rows it was applied to.  A list no row belongs to costs nothing."""
    x = np.asarray(x, dtype=np.float32)
    W = np.asarray(W, dtype=np.float32)
    n, D = x.shape
    cap = idx.shape[1] if idx.ndim == 2 else 0
    keep = np.ones(n, dtype=bool) if row_keep is None else np.asarray(row_keep).astype(bool)
    group = np.full(n, -1, dtype=np.int64) if row_group is None else np.asarray(row_group).astype(np.int64)
    group = np.where((group >= 0) & (group < n_groups), group, -1)
    nnz = np.full(n, cap, dtype=np.int64) if row_nnz is None else np.clip(np.asarray(row_nnz).astype(np.int64), 0, cap)
    live = np.arange(cap)[None, :] < nnz[:, None]
    edit_group = np.array([e[3] for e in edits], dtype=np.int64).reshape(-1)
    by_list = np.argsort(edit_group, kind="stable")  # the global list first, the caller's order kept inside a list
    lo = np.searchsorted(edit_group[by_list], np.arange(-1, n_groups), side="left")
    hi = np.searchsorted(edit_group[by_list], np.arange(-1, n_groups), side="right")
    out = x.astype(np.float64)
    mag = np.abs(x).astype(np.float64)
    m = np.zeros(n, dtype=np.int64)
    changed = np.zeros(len(edits), dtype=np.int64)
    applied = {}
    for g in [-1] + sorted(set(group[keep & (group >= 0)].tolist())):
        rows = np.nonzero(keep if g == -1 else keep & (group == g))[0]
        if rows.size == 0:
            continue
        for i in by_list[lo[g + 1]:hi[g + 1]]:
            latent, op, value, _ = edits[i]
            if cap:
                match = (idx[rows] == latent) & live[rows]
                f = np.where(match.any(axis=1), val[rows, np.argmax(match, axis=1)], np.float32(0)).astype(np.float32)
            else:
                f = np.zeros(rows.size, dtype=np.float32)
            c, applies = _coefficients_fast(f, op, np.float32(value))
            r, c = rows[applies], c[applies].astype(np.float64)
            if r.size == 0:
                continue
            with np.errstate(all="ignore"):
                out[r] += c[:, None] * W[latent].astype(np.float64)[None, :]
                mag[r] += np.abs(c)[:, None] * np.abs(W[latent]).astype(np.float64)[None, :]
            m[r] += 1
            changed[i] = r.size
            applied[int(i)] = r
    return dict(out=out, mag=mag, m=m, rows_changed=changed, applied=applied)


def tolerance(mag, m):
    """(m + 1) u / (1 - (m + 1) u) * (|x_d| + sum |c_e| |W_l_e,d|) + m 2^-149, u = 2^-24: the fmaf chain of m links starting
    from x (each link rounds once; gamma_{m+1} also covers the fp64 evaluation of the restatement itself), plus one smallest
    subnormal per link for results that round in the subnormal range."""
    m = np.asarray(m, dtype=np.float64)[:, None]
    g = (m + 1) * U / (1 - (m + 1) * U)
    return g * mag + m * 2.0 ** -149


# ---- class firing counts -----------------------------------------------------------------------------------------------------------


def fire_counts(idx, val, row_nnz, labels, keep, S: int, C: int, thr):
    """hist (C, T, S), pos (T, S), n_rows_c (C) as int64, entry by entry."""
    thr = np.asarray(thr, dtype=np.float32)
    T = len(thr)
    n = idx.shape[0]
    cap = idx.shape[1]
    hist = np.zeros((C, T, S), dtype=np.int64)
    pos = np.zeros((T, S), dtype=np.int64)
    n_rows_c = np.zeros(C, dtype=np.int64)
    for b in range(n):
        c = int(labels[b])
        if not 0 <= c < C or (keep is not None and not keep[b]):
            continue
        n_rows_c[c] += 1
        nnz = cap if row_nnz is None else min(max(int(row_nnz[b]), 0), cap)
        for j in range(nnz):
            s, v = int(idx[b, j]), np.float32(val[b, j])
            if not 0 <= s < S:
                continue
            m = int(np.sum(v > thr))  # strict; NaN > t is False
            if m >= 1:
                hist[c, m - 1, s] += 1
                pos[m - 1, s] += 1
    return hist, pos, n_rows_c


def fire_counts_fast(idx, val, row_nnz, labels, keep, S: int, C: int, thr):
    """``fire_counts`` with one ``bincount`` per result: the same arguments, the same three int64 arrays."""
    thr = np.asarray(thr, dtype=np.float32)
    T = len(thr)
    idx = np.asarray(idx)
    val = np.asarray(val, dtype=np.float32)
    n, cap = idx.shape
    labels = np.asarray(labels).astype(np.int64)
    ok = (labels >= 0) & (labels < C)
    if keep is not None:
        ok &= np.asarray(keep).astype(bool)
    n_rows_c = np.bincount(labels[ok], minlength=C).astype(np.int64)
    nnz = np.full(n, cap, dtype=np.int64) if row_nnz is None else np.clip(np.asarray(row_nnz).astype(np.int64), 0, cap)
    with np.errstate(invalid="ignore"):
        m = (val[:, :, None] > thr[None, None, :]).sum(axis=2)  # strict; NaN > t is False
    use = ok[:, None] & (np.arange(cap)[None, :] < nnz[:, None]) & (idx >= 0) & (idx < S) & (m >= 1)
    b, j = np.nonzero(use)
    s, bin_ = idx[b, j].astype(np.int64), m[b, j].astype(np.int64) - 1
    hist = np.bincount((labels[b] * T + bin_) * S + s, minlength=C * T * S).astype(np.int64).reshape(C, T, S)
    pos = np.bincount(bin_ * S + s, minlength=T * S).astype(np.int64).reshape(T, S)
    return hist, pos, n_rows_c


def fire_counts_dense(f_dense, labels, keep, C: int, thr):
    """Brute force on a dense (n, S) matrix whose zeros are the absent entries: TP / POS per threshold directly
    (TP[c, t, s] = #{rows of class c with f > thr_t}), as the reference's boolean masks count them."""
    thr = np.asarray(thr, dtype=np.float32)
    f = np.asarray(f_dense, dtype=np.float32)
    labels = np.asarray(labels)
    ok = (labels >= 0) & (labels < C)
    if keep is not None:
        ok &= np.asarray(keep, dtype=bool)
    fires = f[None, :, :] > thr[:, None, None]  # (T, n, S)
    POS = (fires & ok[None, :, None]).sum(axis=1)
    TP = np.stack([(fires & (ok & (labels == c))[None, :, None]).sum(axis=1) for c in range(C)])
    n_rows_c = np.array([(ok & (labels == c)).sum() for c in range(C)], dtype=np.int64)
    return TP.astype(np.int64), POS.astype(np.int64), n_rows_c


def suffix(hist, pos):
    """TP (C, T, S) and POS (T, S) from the bins: sums over u >= t."""
    return np.flip(np.cumsum(np.flip(hist, axis=1), axis=1), axis=1), np.flip(np.cumsum(np.flip(pos, axis=0), axis=0), axis=0)


def f1_from_counts(TP, POS, n_rows_c, mask=None):
    """f1 (C, S) float32 and best_t (C, S) uint8 by the contract's arithmetic: integers exact, each converted to float32 once, one
    fp32 addition of 1e-10, one fp32 division; the maximum over t with ties to the lowest t; masked latents -1 (best_t 0)."""
    FP = POS[None] - TP
    FN = n_rows_c[:, None, None] - TP
    num = (2 * TP).astype(np.float32)
    den = (2 * TP + FP + FN).astype(np.float32) + np.float32(1e-10)
    f = (num / den).astype(np.float32)  # (C, T, S)
    best_t = np.argmax(f, axis=1).astype(np.uint8)  # first maximum = lowest t
    best = np.max(f, axis=1)
    if mask is not None:
        mask = np.asarray(mask, dtype=bool)
        best = np.where(mask[None, :], best, np.float32(-1)).astype(np.float32)
        best_t = np.where(mask[None, :], best_t, 0).astype(np.uint8)
    return best, best_t


# ---- helpers the CPU and the GPU tests share ---------------------------------------------------------------------------------------


def codes_of(f_x: np.ndarray):
    """A dense (n, S) matrix as padded rows: (idx, val, row_nnz), -1 / 0 past a row's entries."""
    nz = f_x != 0
    cap = max(int(nz.sum(axis=1).max()), 1)
    idx = np.full((len(f_x), cap), -1, dtype=np.int32)
    val = np.zeros((len(f_x), cap), dtype=np.float32)
    for b in range(len(f_x)):
        cols = np.nonzero(nz[b])[0]
        idx[b, :len(cols)], val[b, :len(cols)] = cols, f_x[b, cols]
    return idx, val, nz.sum(axis=1).astype(np.int32)


def g30_case(kind: str):
    """Fixture G30 (tools/gen_golden_interventions.py) for "topk" or "relu", with the edits as tuples and the reference's dense
    f_x as padded rows."""
    with np.load(GOLDEN / "g30_interventions.npz") as z:
        g = {k[len(kind) + 1:]: z[k] for k in z.files if k.startswith(kind + "_")}
        g["n_groups"] = int(z["n_groups"])
    g["edits"] = [(int(a), int(b), float(c), int(d)) for a, b, c, d in zip(g["edit_latent"], g["edit_op"], g["edit_value"], g["edit_group"])]
    g["idx"], g["val"], g["row_nnz"] = codes_of(g["f_x"])
    return g


def triple_loop(orig, mod, classes):
    """compute_class_results by its definition: (class, n_orig, n_changed, n_other, n_other_changed, {new class: count})."""
    out = []
    for c in classes:
        om = orig == c
        changed = (mod != orig) & om
        dist = {}
        for new in classes:
            if new != c:
                k = int(((mod == new) & changed).sum())
                if k > 0:
                    dist[new] = k
        out.append((c, int(om.sum()), int(changed.sum()), int((~om).sum()), int(((mod != orig) & ~om).sum()), dist))
    return out
