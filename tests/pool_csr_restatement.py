"""POOL CSR (include/saev_amd.h) restated in plain numpy and Python: per image a row that starts from "absent"; a loop
over the image's stored entries, in storage order, keeps for every latent the maximum of the values above the latent's threshold,
the lowest patch attaining it and the number of entries that passed; the row's columns are then emitted in ascending order.  Values
are compared as the float32 numbers they are (a Python float holds every float32 exactly), so ``a > thr`` is the kernel's comparison:
strict, false for a NaN threshold, false for every finite value at +Inf."""

import numpy as np

ERR_COLUMN, ERR_VALUE, ERR_INDPTR, ERR_THRESHOLD = 1, 2, 3, 4
ARRAYS = ("indptr", "indices", "data", "patch", "count")


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint32) if x.dtype == np.float32 else x


def thr_list(thr, s):
    """The threshold of every latent as Python floats, from one number or a (s,) float32 vector."""
    if np.ndim(thr) == 0:
        return [float(np.float32(thr))] * s
    thr = np.asarray(thr)
    assert thr.dtype == np.float32 and thr.shape == (s,)
    return thr.tolist()


def restate(indptr, indices, data, n_images, t, s, thr=0.0, **_):
    assert indptr.dtype == np.int64 and indices.dtype == np.int32 and data.dtype == np.float32 and len(indptr) == n_images * t + 1
    thr = thr_list(thr, s)
    ptr, cols, vals = indptr.tolist(), indices.tolist(), data.tolist()
    out_ptr, out_cols, out_vals, out_patch, out_count = [0], [], [], [], []
    for i in range(n_images):
        row = {}  # latent -> [maximum, lowest patch attaining it, entries that passed]; absent until an entry passes
        for p in range(t):
            for e in range(ptr[i * t + p], ptr[i * t + p + 1]):
                l, a = cols[e], vals[e]
                if not a > thr[l]:
                    continue
                held = row.get(l)
                if held is None:
                    row[l] = [a, p, 1]
                else:
                    if a > held[0]:  # patches ascend in the loop: an equal value keeps the earlier patch
                        held[0], held[1] = a, p
                    held[2] += 1
        for l in sorted(row):
            out_cols.append(l)
            out_vals.append(row[l][0])
            out_patch.append(row[l][1])
            out_count.append(row[l][2])
        out_ptr.append(len(out_cols))
    return dict(indptr=np.asarray(out_ptr, dtype=np.int64), indices=np.asarray(out_cols, dtype=np.int32), data=np.asarray(out_vals, dtype=np.float32),
                patch=np.asarray(out_patch, dtype=np.int32), count=np.asarray(out_count, dtype=np.int32))


def error_word(indptr, indices, data, s, thr=0.0):
    """The largest error code of the input: 0 for a good one."""
    code = 0
    if ((indices < 0) | (indices >= s)).any():
        code = max(code, ERR_COLUMN)
    if not np.isfinite(data).all():
        code = max(code, ERR_VALUE)
    if indptr[0] < 0 or (np.diff(indptr) < 0).any() or indptr[-1] > len(indices):
        code = max(code, ERR_INDPTR)
    if np.ndim(thr) == 1 and (np.asarray(thr) < 0).any():
        code = max(code, ERR_THRESHOLD)
    return code


def workspace_bytes(n_images, s, range_len):
    """saev_pool_csr_workspace_bytes as the header documents it."""
    r256 = lambda b: -(-max(b, 1) // 256) * 256  # noqa: E731
    units = n_images * -(-s // range_len)
    return r256(8 * (units + 1)) + r256(8 * -(-units // 4096))
