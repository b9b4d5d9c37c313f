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
