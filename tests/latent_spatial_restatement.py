"""The contract of LATENT SPATIAL (include/saev_amd.h) restated in numpy, the slow and obvious way: per image and
latent a dense boolean (gh, gw) array of the firing positions, explicit loops over its cells for the pairs, and the float64 sums
formed one term at a time in ascending row order.  The GPU tests demand EQUALITY with it -- on the bits for the sums.

Nothing here is shared with the kernels: no latent-major list, no neighbour search, no chunks."""

import numpy as np

ERR_GROUP, ERR_LATENT = 1, 2
INTEGERS = ("n_events", "n_images_fire", "pairs_h", "pairs_v", "sum_m2", "overlap")


def error_word(indices, n_latents, groups, n_groups):
    """What the device's error word must hold: 0, or the largest code met."""
    err = 0
    if ((groups < -1) | (groups >= n_groups)).any():
        err = max(err, ERR_GROUP)
    if ((indices < 0) | (indices >= n_latents)).any():
        err = max(err, ERR_LATENT)
    return err


def restate(indptr, indices, data, *, n_images, gh, gw, s, groups, g, thr=0.0, **_):
    """Every output of the entry as a dict of numpy arrays (count_map and sum_map as (S, G, T))."""
    T = gh * gw
    assert len(indptr) == n_images * T + 1 and len(groups) == n_images
    thr = np.float32(thr)
    out = {k: np.zeros((s, g), dtype=np.int64) for k in INTEGERS}
    out["moments"] = np.zeros((s, g, 5), dtype=np.float64)
    out["count_map"] = np.zeros((s, g, T), dtype=np.int32)
    out["sum_map"] = np.zeros((s, g, T), dtype=np.float64)
    out["n_group_images"] = np.bincount(groups[groups >= 0], minlength=g).astype(np.int64)
    mom, cmap, smap = out["moments"], out["count_map"], out["sum_map"]
    with np.errstate(all="ignore"):
        for i in range(n_images):  # ascending images, and inside an image ascending positions: ascending rows
            grp = int(groups[i])
            if grp < 0:
                continue
            ptr = indptr[i * T:(i + 1) * T + 1]
            lo, hi = int(ptr[0]), int(ptr[-1])
            if lo == hi:
                continue
            pos = np.repeat(np.arange(T), np.diff(ptr))
            cols, vals = indices[lo:hi], data[lo:hi].astype(np.float32)
            for j in np.unique(cols):
                fire = np.zeros((gh, gw), dtype=bool)
                value = np.zeros((gh, gw), dtype=np.float32)
                for p, v in zip(pos[cols == j], vals[cols == j]):
                    if v > thr:  # NaN compares false
                        fire[p // gw, p % gw] = True
                        value[p // gw, p % gw] = v
                m = 0
                for p in np.flatnonzero(fire.reshape(-1)):
                    r, c = int(p) // gw, int(p) % gw
                    m += 1
                    if c + 1 < gw and fire[r, c + 1]:
                        out["pairs_h"][j, grp] += 1
                    if r + 1 < gh and fire[r + 1, c]:
                        out["pairs_v"][j, grp] += 1
                    v = np.float64(value[r, c])
                    mom[j, grp, 0] = mom[j, grp, 0] + v
                    mom[j, grp, 1] = mom[j, grp, 1] + v * np.float64(r)
                    mom[j, grp, 2] = mom[j, grp, 2] + v * np.float64(c)
                    mom[j, grp, 3] = mom[j, grp, 3] + v * np.float64(r * r)
                    mom[j, grp, 4] = mom[j, grp, 4] + v * np.float64(c * c)
                    cmap[j, grp, p] += 1
                    smap[j, grp, p] = smap[j, grp, p] + v
                if m:
                    out["n_events"][j, grp] += m
                    out["n_images_fire"][j, grp] += 1
                    out["sum_m2"][j, grp] += m * m
    out["overlap"] = (cmap.astype(np.int64) ** 2).sum(axis=2)
    return out


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)
