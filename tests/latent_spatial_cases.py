"""Small named inputs of LATENT SPATIAL (include/saev_amd.h), each with the property it plants.  A case is a dict:
indptr (n_images * gh * gw + 1) int64, indices int32, data float32, n_images, gh, gw, s, groups (n_images) int32, g, thr.  The
host tests check that each case holds what it is said to hold; the GPU tests run every case against the restatement."""

import numpy as np

CHUNK = 64  # events a wave of the walk takes per trip


def build(events, *, n_images, gh, gw, s, groups, g, thr=0.0):
    """events: rows of (image, r, c, latent, value); at most one per (image, r, c, latent)."""
    T = gh * gw
    ev = np.asarray(events, dtype=np.float64).reshape(-1, 5)
    row = (ev[:, 0] * T + ev[:, 1] * gw + ev[:, 2]).astype(np.int64)
    lat = ev[:, 3].astype(np.int64)
    order = np.lexsort((lat, row))
    assert len(np.unique(row * (s + 2) + lat + 1)) == len(row), "one entry per (row, latent)"
    indptr = np.zeros(n_images * T + 1, dtype=np.int64)
    np.cumsum(np.bincount(row, minlength=n_images * T), out=indptr[1:])
    return dict(indptr=indptr, indices=lat[order].astype(np.int32), data=ev[:, 4].astype(np.float32)[order],
                n_images=n_images, gh=gh, gw=gw, s=s, groups=np.asarray(groups, dtype=np.int32), g=g, thr=float(thr))


def random_case(seed, *, n_images, gh, gw, s, g, density, free=0.2, thr=0.0):
    """Every (image, position, latent) fires with probability ``density``; a fifth of the images belong to no group."""
    rng = np.random.default_rng(seed)
    fire = rng.random((n_images, gh, gw, s)) < density
    i, r, c, j = np.nonzero(fire)
    v = rng.random(len(i)).astype(np.float32) * 4 + np.float32(0.01)
    groups = rng.integers(0, g, n_images).astype(np.int32)
    groups[rng.random(n_images) < free] = -1
    return build(np.stack([i, r, c, j, v], axis=1), n_images=n_images, gh=gh, gw=gw, s=s, groups=groups, g=g, thr=thr)


def grid(gh, gw):
    n = 12 if gh * gw < 100 else 3
    return random_case(gh * 100 + gw, n_images=n, gh=gh, gw=gw, s=5, g=3, density=0.45 if gh * gw < 100 else 0.3)


def row_end():
    """(r, gw - 1) and (r + 1, 0) are consecutive rows and no neighbours: no pair at all."""
    ev = [(0, 0, 4, 0, 1.0), (0, 1, 0, 0, 2.0), (1, 1, 4, 0, 1.5), (1, 2, 0, 0, 0.5)]
    return build(ev, n_images=2, gh=3, gw=5, s=1, groups=[0, 0], g=1)


def image_border():
    """(gh - 1, c) of image i and (0, c) of image i + 1 are gw rows apart and no neighbours: no pair at all."""
    ev = [(i, 2, c, 0, 1.0 + c) for i in range(3) for c in (1, 3)] + [(i, 0, c, 0, 2.0 + c) for i in range(3) for c in (1, 3)]
    return build(ev, n_images=3, gh=3, gw=5, s=1, groups=[0, 1, 0], g=2)


def full_image():
    """One image with all T positions firing: every grid edge is a pair."""
    ev = [(1, r, c, 2, 1.0 + r + 0.25 * c) for r in range(3) for c in range(5)]
    return build(ev, n_images=3, gh=3, gw=5, s=4, groups=[0, 0, 1], g=2)


def silent():
    """Latent 0 has no entry, latent 1 only entries that do not fire, latent 2 fires once."""
    ev = [(0, 0, 0, 1, 0.0), (1, 1, 1, 1, -3.0), (1, 0, 1, 2, 1.0)]
    return build(ev, n_images=2, gh=2, gw=2, s=3, groups=[0, 1], g=2)


def every_row():
    """Latent 1 fires on every row of 300 images of a 16 x 16 grid: 76 800 events, 1 200 trips of one wave."""
    n, gh, gw = 300, 16, 16
    i, r, c = np.meshgrid(np.arange(n), np.arange(gh), np.arange(gw), indexing="ij")
    rng = np.random.default_rng(5)
    v = rng.random(i.size).astype(np.float32) + np.float32(0.5)
    ev = np.stack([i.reshape(-1), r.reshape(-1), c.reshape(-1), np.ones(i.size), v], axis=1)
    sparse = np.array([(k, 3, 5, 0, 1.0) for k in range(0, n, 7)] + [(k, 15, 15, 2, 2.0) for k in range(0, n, 11)])
    groups = np.arange(n) % 3
    return build(np.concatenate([ev, sparse]), n_images=n, gh=gh, gw=gw, s=3, groups=groups, g=3)


LIST_LENGTHS = (CHUNK - 1, CHUNK, CHUNK + 1)


def lists():
    """Latent k has exactly LIST_LENGTHS[k] events: a list one short of a trip, a whole trip, and one more."""
    ev = []
    for k, n in enumerate(LIST_LENGTHS):
        ev += [(q // 9, (q % 9) // 3, q % 3, k, 1.0 + 0.5 * (q % 5)) for q in range(n)]
    return build(ev, n_images=8, gh=3, gw=3, s=3, groups=[0, 1, 0, 1, 0, 1, 0, 1], g=2)


STRADDLE_FIRST = 10


def straddle():
    """A 4 x 4 grid; latent 0 fires at the last 10 positions of image 0 and at all 16 of images 1 .. 9, so its events 58 .. 73 are
    image 4 and 122 .. 137 image 8: an image, its pairs and its m lie across each border of a trip (64, 128)."""
    ev = [(0, p // 4, p % 4, 0, 1.0 + p) for p in range(16 - STRADDLE_FIRST, 16)]
    ev += [(i, p // 4, p % 4, 0, 0.5 + i + 0.125 * p) for i in range(1, 10) for p in range(16)]
    return build(ev, n_images=10, gh=4, gw=4, s=2, groups=[0, 1] * 5, g=2)


def same_cell():
    """One event per image at the same position over 200 images: every event of a trip updates the same map cell."""
    ev = [(i, 1, 2, 0, 1.0 + (i % 13) * 0.37) for i in range(200)] + [(i, 0, i % 3, 1, 2.0) for i in range(200)]
    return build(ev, n_images=200, gh=2, gw=3, s=2, groups=np.arange(200) % 2, g=2)


def groups_free():
    """Group -1 holds firing images, group 1 of 3 is empty."""
    c = random_case(11, n_images=10, gh=3, gw=4, s=4, g=3, density=0.5, free=0.0)
    c["groups"] = np.array([0, -1, 2, 2, -1, 0, 0, 2, -1, 0], dtype=np.int32)
    return c


def one_group():
    return random_case(12, n_images=9, gh=3, gw=4, s=4, g=1, density=0.5)


def groups_64():
    c = random_case(13, n_images=130, gh=2, gw=3, s=3, g=64, density=0.5, free=0.0)
    c["groups"] = (np.arange(130) % 64).astype(np.int32)
    return c


KINDS_THR = 0.5


def value_kinds(thr):
    """Every kind of stored value; with thr = 0.5 some are equal to it, below it and above it."""
    vals = [0.0, -0.0, -1.0, np.nan, np.inf, -np.inf, 1e-45, 1e-39, 0.5, np.nextafter(np.float32(0.5), np.float32(1)), 0.25, 3.0]
    ev = []
    for k, v in enumerate(vals):
        ev.append((k % 2, (k // 2) % 2, (k // 4) % 3, k % 3, v))
    ev += [(2, r, c, 1, np.inf if (r, c) == (1, 1) else 1.0) for r in range(2) for c in range(3)]  # +Inf away from r = 0 and c = 0
    return build(ev, n_images=3, gh=2, gw=3, s=3, groups=[0, 1, 0], g=2, thr=thr)


def wide():
    """S = 70 001: the last latent fires, and so does one in the middle."""
    ev = [(0, 0, 0, 70_000, 1.0), (0, 0, 1, 70_000, 2.0), (1, 1, 1, 70_000, 1.0), (1, 1, 0, 35_000, 4.0), (0, 1, 0, 0, 1.0)]
    return build(ev, n_images=2, gh=2, gw=2, s=70_001, groups=[0, 0], g=1)


SMALL = {
    "grid_1x1": lambda: grid(1, 1), "grid_1x5": lambda: grid(1, 5), "grid_5x1": lambda: grid(5, 1), "grid_2x2": lambda: grid(2, 2),
    "grid_3x5": lambda: grid(3, 5), "grid_37x37": lambda: grid(37, 37), "row_end": row_end, "image_border": image_border,
    "full_image": full_image, "silent": silent, "lists": lists, "straddle": straddle, "same_cell": same_cell, "groups_free": groups_free,
    "one_group": one_group, "groups_64": groups_64, "values_thr_0": lambda: value_kinds(0.0), "values_thr_half": lambda: value_kinds(KINDS_THR),
    "wide": wide,
}
ALL = {**SMALL, "every_row": every_row}


def broken(kind):
    """(case, the error word it must raise)."""
    c = grid(3, 5)
    c["indices"], c["groups"] = c["indices"].copy(), c["groups"].copy()
    if kind == "latent_s":
        c["indices"][7] = c["s"]
        return c, 2
    if kind == "latent_negative":
        c["indices"][3] = -1
        return c, 2
    if kind == "group_g":
        c["groups"][2] = c["g"]
        return c, 1
    if kind == "group_g_of_an_image_without_entries":
        T = c["gh"] * c["gw"]
        keep = np.ones(len(c["indices"]), dtype=bool)
        keep[c["indptr"][2 * T]:c["indptr"][3 * T]] = False
        counts = np.diff(c["indptr"])
        counts[2 * T:3 * T] = 0
        c["indptr"] = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        c["indices"], c["data"] = c["indices"][keep], c["data"][keep]
        c["groups"][2] = c["g"] + 5
        return c, 1
    if kind == "both":
        c["indices"][7], c["groups"][2] = c["s"], -2
        return c, 2
    raise KeyError(kind)


BROKEN = ("latent_s", "latent_negative", "group_g", "group_g_of_an_image_without_entries", "both")


def _row_of_entries(c):
    return np.repeat(np.arange(len(c["indptr"]) - 1), np.diff(c["indptr"]))


def one_latent(c, j):
    """The case with latent j alone (as latent 0 of S = 1)."""
    keep = c["indices"] == j
    counts = np.bincount(_row_of_entries(c)[keep], minlength=len(c["indptr"]) - 1)
    return dict(c, indptr=np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), indices=np.zeros(int(keep.sum()), dtype=np.int32),
                data=c["data"][keep], s=1)


def permute_images(c, perm):
    """Image k of the result is image perm[k] of the case."""
    T = c["gh"] * c["gw"]
    perm = np.asarray(perm)
    rows = (perm[:, None] * T + np.arange(T)[None, :]).reshape(-1)  # new row -> old row
    new_of_old = np.empty_like(rows)
    new_of_old[rows] = np.arange(len(rows))
    order = np.argsort(new_of_old[_row_of_entries(c)], kind="stable")
    counts = np.diff(c["indptr"])[rows]
    return dict(c, indptr=np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), indices=c["indices"][order], data=c["data"][order],
                groups=c["groups"][perm])
