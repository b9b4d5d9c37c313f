"""The contract of LATENT EXEMPLARS (include/saev_amd.h) restated in numpy with explicit loops, for the tests: one
latent at a time densified to an (n_images, T) array of event values, its maximum and FIRST argmax per image, ``np.lexsort`` on
(image, -M) and (image, M) inside each group, ``np.setdiff1d`` for the silent images.  Nothing here is shared with the library."""

import numpy as np

ERR_GROUP, ERR_LATENT, ERR_IMAGE = 1, 2, 3
LISTS = ("top_val", "top_img", "top_patch", "bot_val", "bot_img", "bot_patch", "silent_img")
ARRAYS = ("n_group_images", "n_fire") + LISTS


def bits(x):
    """A float32 array as its int32 bit patterns (+0.0 and -0.0 differ, a NaN equals itself); integer arrays pass through."""
    x = np.ascontiguousarray(x)
    return x.view(np.int32) if x.dtype == np.float32 else x


def error_word(indices, s, groups, g):
    bad_latent = ((indices < 0) | (indices >= s)).any()
    bad_group = ((groups < -1) | (groups >= g)).any()
    return ERR_LATENT if bad_latent else ERR_GROUP if bad_group else 0


def events(indptr, indices, data, t, s, groups, thr):
    """(row, latent, value) of the entries that are events."""
    rows = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
    with np.errstate(invalid="ignore"):
        hit = (data > np.float32(thr)) & (indices >= 0) & (indices < s) & (groups[rows // t] >= 0)
    return rows[hit], indices[hit], data[hit]


def restate(indptr, indices, data, *, n_images, t, s, groups, g, k, thr=0.0):
    groups = np.asarray(groups)
    members = [np.flatnonzero(groups == q) for q in range(g)]
    out = dict(n_group_images=np.array([len(m) for m in members], dtype=np.int64), n_fire=np.zeros((s, g), dtype=np.int32))
    for name in LISTS:
        out[name] = np.zeros((s, g, k), dtype=np.float32) if name.endswith("val") else np.full((s, g, k), -1, dtype=np.int32)
    for q in range(g):  # a latent without events: every member is silent
        out["silent_img"][:, q, :min(k, len(members[q]))] = members[q][:k]
    rows, lats, vals = events(indptr, indices, data, t, s, groups, thr)
    order = np.argsort(lats, kind="stable")
    rows, lats, vals = rows[order], lats[order], vals[order]
    cuts = np.flatnonzero(np.diff(lats)) + 1
    for r, j, v in zip(np.split(rows, cuts), np.split(lats, cuts), np.split(vals, cuts)):
        if len(r) == 0:
            continue
        j = int(j[0])
        dense = np.full((n_images, t), -np.inf, dtype=np.float32)
        fires = np.zeros(n_images, dtype=bool)
        dense[r // t, r % t] = v
        fires[r // t] = True
        M, P = dense.max(axis=1), dense.argmax(axis=1)  # argmax: the first of equal values
        for q in range(g):
            f = members[q][fires[members[q]]]
            out["n_fire"][j, q] = len(f)
            for end, key in (("top", -M[f]), ("bot", M[f])):
                chosen = f[np.lexsort((f, key))][:k]
                out[end + "_val"][j, q, :len(chosen)] = M[chosen]
                out[end + "_img"][j, q, :len(chosen)] = chosen
                out[end + "_patch"][j, q, :len(chosen)] = P[chosen]
            silent = np.setdiff1d(members[q], f)[:k]
            out["silent_img"][j, q] = -1
            out["silent_img"][j, q, :len(silent)] = silent
    return out


def patch_rows(indptr, indices, data, t, latents, images):
    """(*shape, t) float32: the stored value of the latent in every row of the image (the first stored one), 0.0 where there is none
    and for image -1."""
    latents, images = np.asarray(latents), np.asarray(images)
    out = np.zeros(latents.shape + (t,), dtype=np.float32)
    for at in np.ndindex(latents.shape):
        if images[at] < 0:
            continue
        for p in range(t):
            row = int(images[at]) * t + p
            for e in range(indptr[row], indptr[row + 1]):
                if indices[e] == latents[at]:
                    out[at + (p,)] = data[e]
                    break
    return out
