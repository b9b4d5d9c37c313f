"""Small named inputs of LATENT EXEMPLARS (include/saev_amd.h), each with the property it plants.  A case is a dict:
indptr (n_images * t + 1) int64, indices int32, data float32, n_images, t, s, groups (n_images) int32, g, k, thr.  The host tests
check that each case holds what it is said to hold; the GPU tests run every case against the restatement."""

import numpy as np

CHUNK = 64  # events a wave of the walk takes per trip


def build(events, *, n_images, t, s, groups, g, k, thr=0.0, shuffle_rows=None):
    """events: rows of (image, patch, latent, value); at most one per (image, patch, latent).  ``shuffle_rows`` (a seed) leaves the
    entries of every row in a random order of columns; otherwise they ascend."""
    ev = np.asarray(events, dtype=np.float64).reshape(-1, 4)
    row = (ev[:, 0] * t + ev[:, 1]).astype(np.int64)
    lat = ev[:, 2].astype(np.int64)
    minor = lat if shuffle_rows is None else np.random.default_rng(shuffle_rows).permutation(len(lat))
    order = np.lexsort((minor, row))
    assert len(np.unique(row * (s + 2) + lat + 1)) == len(row), "one entry per (row, latent)"
    indptr = np.zeros(n_images * t + 1, dtype=np.int64)
    np.cumsum(np.bincount(row, minlength=n_images * t), out=indptr[1:])
    return dict(indptr=indptr, indices=lat[order].astype(np.int32), data=ev[:, 3].astype(np.float32)[order],
                n_images=n_images, t=t, s=s, groups=np.asarray(groups, dtype=np.int32), g=g, k=k, thr=float(thr))


def random_case(seed, *, n_images, t, s, g, k, density, free=0.2, thr=0.0, shuffle_rows=None):
    """Every (image, patch, latent) fires with probability ``density`` at a value of its own (no two values of the case are equal);
    a fifth of the images belong to no group."""
    rng = np.random.default_rng(seed)
    i, p, j = np.nonzero(rng.random((n_images, t, s)) < density)
    v = (rng.permutation(len(i)) + 1).astype(np.float32) / np.float32(64)  # distinct and exact in fp32
    groups = rng.integers(0, g, n_images).astype(np.int32)
    groups[rng.random(n_images) < free] = -1
    return build(np.stack([i, p, j, v], axis=1), n_images=n_images, t=t, s=s, groups=groups, g=g, k=k, thr=thr, shuffle_rows=shuffle_rows)


def tokens(t):
    return random_case(100 + t, n_images=40 if t < 100 else 9, t=t, s=6, g=3, k=4, density=0.3 if t < 100 else 0.05, shuffle_rows=t)


def one_image():
    return build([(0, 3, 0, 1.0), (0, 1, 0, 2.0), (0, 4, 2, 0.5)], n_images=1, t=5, s=3, groups=[0], g=1, k=8)


def single_latent():
    return random_case(7, n_images=30, t=4, s=1, g=2, k=8, density=0.4)


def wide():
    """S = 70 001: the last latent fires, and so does one in the middle."""
    ev = [(0, 0, 70_000, 1.0), (0, 1, 70_000, 2.0), (1, 3, 70_000, 1.0), (1, 2, 35_000, 4.0), (0, 2, 0, 1.0)]
    return build(ev, n_images=2, t=4, s=70_001, groups=[0, 0], g=1, k=2)


def empty():
    """No stored entry: every list is empty and the silent lists are the first k members of each group."""
    return build([], n_images=12, t=3, s=4, groups=[0, 2, -1, 0, 0, 2, 0, -1, 0, 0, 0, 0], g=3, k=4)


LENGTH_KS = (1, 8, 32)


def lengths(k):
    """Latent q fires in exactly (0, k - 1, k, k + 1, 2 k + 1)[q] images of group 0 (the even images); all five fire in 3 odd ones."""
    n = 2 * (2 * k + 1) + 6
    rng = np.random.default_rng(k)
    ev = []
    for q, m in enumerate(lengths_of(k)):
        chosen = np.sort(rng.choice(n // 2, m, replace=False)) * 2
        ev += [(i, int(rng.integers(0, 3)), q, 1.0 + 0.25 * int(rng.integers(0, 4 * n))) for i in chosen]
        ev += [(i, 1, q, 3.0 + i) for i in (1, 5, 9)]
    return build(ev, n_images=n, t=3, s=5, groups=np.arange(n) % 2, g=2, k=k)


def lengths_of(k):
    return (0, k - 1, k, k + 1, 2 * k + 1)


LIST_LENGTHS = (CHUNK - 1, CHUNK, CHUNK + 1)


def lists():
    """Latent q has exactly LIST_LENGTHS[q] events: a list one short of a trip, a whole trip, and one more; 9 patches an image."""
    ev = []
    for q, n in enumerate(LIST_LENGTHS):
        ev += [(e // 9, e % 9, q, 1.0 + 0.5 * ((e * 7) % 11)) for e in range(n)]
    return build(ev, n_images=8, t=9, s=3, groups=[0, 1, 0, 1, 0, 1, 0, 1], g=2, k=3)


STRADDLE_FIRST = 10
STRADDLE_PEAKS = ((2,), (9,), (3, 11))  # the patches of the maximum in images 4 and 8, per latent


def straddle():
    """T = 16; every latent fires at the last 10 patches of image 0 and at all 16 of images 1 .. 9, so its events 58 .. 73 are image
    4 and 122 .. 137 image 8: both runs lie across a border of a trip (64, 128), patches 0 .. 5 before it and 6 .. 15 behind.  Latent
    0 has their maximum before the border, latent 1 behind it, latent 2 the same value on both sides (the carry must keep patch 3)."""
    ev = []
    for q, peaks in enumerate(STRADDLE_PEAKS):
        for i in range(10):
            for p in range(16 - STRADDLE_FIRST if i == 0 else 0, 16):
                v = 9.0 + i if i in (4, 8) and p in peaks else 0.5 + 0.25 * ((p * 5 + i) % 16)
                ev.append((i, p, q, v))
    return build(ev, n_images=10, t=16, s=3, groups=[0, 1] * 5, g=2, k=4)


LONG_T = 200


def long_run():
    """T = 200 and every patch of every image fires: a run is longer than three trips.  Image 0 has its maximum at patch 199, image
    1 at patch 0, image 2 the same maximum at patches 10 and 150 (two trips apart), image 3 one value everywhere."""
    ev = []
    for i in range(4):
        for p in range(LONG_T):
            v = 1.0 + (p % 7) * 0.125
            if (i, p) in ((0, 199), (1, 0), (2, 10), (2, 150)):
                v = 5.0 + i
            if i == 3:
                v = 2.5
            ev.append((i, p, 0, v))
    return build(ev, n_images=4, t=LONG_T, s=1, groups=[0, 0, 0, 0], g=1, k=8)


def ties():
    """Group 0 (the even images of 24): latent 0 has M = 2 in six images, 1 in four and 3 in two, so both ends cut through a block
    of equal M (k = 4); latent 1 has every image at one value; latent 2 has equal values inside every image (patches 1 and 3)."""
    ev = []
    for r, i in enumerate(range(0, 24, 2)):
        ev.append((i, r % 4, 0, (2.0, 1.0, 2.0, 3.0, 2.0, 1.0)[r % 6]))
        ev.append((i, (r * 3) % 4, 1, 1.5))
        ev += [(i, 3, 2, 1.0 + (r % 3)), (i, 1, 2, 1.0 + (r % 3)), (i, 2, 2, 0.5)]
    for i in range(1, 24, 2):
        ev.append((i, 0, 1, 1.5))
    return build(ev, n_images=24, t=4, s=3, groups=np.arange(24) % 2, g=2, k=4, shuffle_rows=3)


def inf_two():
    """+Inf in two images of the group (and twice inside one of them): they lead the top list in image order."""
    ev = [(5, 2, 0, np.inf), (2, 1, 0, np.inf), (2, 3, 0, np.inf), (1, 0, 0, 3.0), (3, 0, 0, 7.0), (4, 1, 0, 1e30), (0, 0, 0, 2.0)]
    return build(ev, n_images=6, t=4, s=1, groups=[0] * 6, g=1, k=3)


def one_group():
    return random_case(12, n_images=50, t=4, s=5, g=1, k=8, density=0.2, free=0.0)


def groups_64():
    c = random_case(13, n_images=200, t=3, s=4, g=64, k=2, density=0.3, free=0.0)
    c["groups"] = (np.arange(200) % 64).astype(np.int32)
    return c


def at_the_limits(g):
    """k = 32 with G = 64 -- the lists of one wave fill 48 KiB of LDS, a workgroup is one wave -- or G = 32: two waves a workgroup;
    S = 5 is a multiple of neither.  300 images, so a group holds 4 or 5 (G = 64: fewer than k) or 9 or 10."""
    c = random_case(14 + g, n_images=300, t=2, s=5, g=g, k=32, density=0.35, free=0.0)
    c["groups"] = ((np.arange(300) * 7) % g).astype(np.int32)
    return c


MIXED_K = 4
MIXED_GROUPS = np.array([0, 1, 4, 0, -1, 1, 0, 4, -1, 0, 1, 0, -1, 0, 3, 1, 0, 4, 3, -1, 0, 1, 0, 0, 4, 1, 0, 0, 0, 0], dtype=np.int32)


def groups_mixed():
    """30 images, 5 groups, k = 4: group 0 is large, group 1 fires in ALL its members (latent 0), group 2 is EMPTY, group 3 has 2 < k
    members, group 4 never fires; a fifth of the images are at -1 and they fire too."""
    ev = []
    for i, q in enumerate(MIXED_GROUPS):
        if q in (1, -1, 3) or (q == 0 and i % 3 == 0):
            ev.append((i, i % 3, 0, 1.0 + ((i * 7) % 10) * 0.5 + 0.01 * i))
        if q in (0, -1) and i % 2 == 0:
            ev.append((i, (i + 1) % 3, 1, 4.0 - 0.1 * i))
    return build(ev, n_images=30, t=3, s=2, groups=MIXED_GROUPS, g=5, k=MIXED_K)


GAP_RANKS = ((0, 39), (0, 7, 8, 20, 39), (39,), (5, 6))  # the ranks inside the group that fire, per latent


def gaps():
    """One group of 40 (with strangers of group -1 between its members), k = 3: the firing members stand at rank 0, at the last rank
    and behind gaps longer than k, so the silent cursor stops inside a gap and the tail flush has something, or nothing, left."""
    groups = np.zeros(60, dtype=np.int32)
    groups[1::3] = -1
    mem = np.flatnonzero(groups == 0)
    ev = [(int(mem[r]), r % 2, q, 1.0 + r) for q, ranks in enumerate(GAP_RANKS) for r in ranks]
    ev += [(i, 0, 0, 9.0) for i in (1, 4, 58)]
    return build(ev, n_images=60, t=2, s=4, groups=groups, g=1, k=3)


KINDS_THR = 0.5
KIND_VALUES = (0.0, -0.0, -1.0, np.nan, np.inf, -np.inf, 1e-45, 1e-39, 0.5, float(np.nextafter(np.float32(0.5), np.float32(1))), 0.25, 3.0)


def value_kinds(thr):
    """Every kind of stored value, one image each for latent 0 and patch q of image 12 for latent 1; with thr = 0.5 some are equal to
    it, below it and above it.  Image 13 holds nothing but non-events of latent 2 (it is silent), image 14 an event among them."""
    ev = [(q, q % 3, 0, v) for q, v in enumerate(KIND_VALUES)]
    ev += [(12, q, 1, v) for q, v in enumerate(KIND_VALUES[:3] + KIND_VALUES[5:])]
    ev += [(13, 0, 2, 0.0), (13, 1, 2, -2.0), (13, 2, 2, np.nan), (14, 0, 2, -0.0), (14, 1, 2, 0.75), (14, 2, 2, np.nan)]
    return build(ev, n_images=15, t=12, s=3, groups=[0, 1, 0] * 5, g=2, k=8, thr=thr)


def every_row():
    """Latent 1 fires on every row of 300 images x 256 patches: 76 800 events, 1 200 trips of one wave."""
    n, t = 300, 256
    i, p = np.meshgrid(np.arange(n), np.arange(t), indexing="ij")
    rng = np.random.default_rng(5)
    v = (rng.permutation(i.size) + 1).astype(np.float32) / np.float32(8)
    ev = np.stack([i.reshape(-1), p.reshape(-1), np.ones(i.size), v], axis=1)
    sparse = np.array([(q, 35, 0, 1.0 + q) for q in range(0, n, 7)] + [(q, 255, 2, 2.0) for q in range(0, n, 11)])
    return build(np.concatenate([ev, sparse]), n_images=n, t=t, s=3, groups=np.arange(n) % 3, g=3, k=8)


SMALL = {
    "one_image": one_image, "single_latent": single_latent, "wide": wide, "empty": empty,
    "tokens_1": lambda: tokens(1), "tokens_5": lambda: tokens(5), "tokens_16": lambda: tokens(16), "tokens_257": lambda: tokens(257),
    **{f"lengths_k{k}": (lambda k=k: lengths(k)) for k in LENGTH_KS},
    "lists": lists, "straddle": straddle, "long_run": long_run, "ties": ties, "inf_two": inf_two, "one_group": one_group, "groups_64": groups_64,
    "limits_g64_k32": lambda: at_the_limits(64), "limits_g32_k32": lambda: at_the_limits(32), "groups_mixed": groups_mixed, "gaps": gaps, "values_thr_0": lambda: value_kinds(0.0), "values_thr_half": lambda: value_kinds(KINDS_THR),
}
ALL = {**SMALL, "every_row": every_row}
UNTIED = ("tokens_5", "tokens_16", "one_group")  # no two values of the case are equal


def broken(kind):
    """(case, the error word it must raise): the bad value stands in the LAST entry / the last image."""
    c = tokens(5)
    c["indices"], c["groups"] = c["indices"].copy(), c["groups"].copy()
    if kind == "latent_s":
        c["indices"][-1] = c["s"]
        return c, 2
    if kind == "group_g":
        c["groups"][-1] = c["g"]
        return c, 1
    if kind == "both":
        c["indices"][-1], c["groups"][-1] = c["s"], c["g"]
        return c, 2
    raise KeyError(kind)


BROKEN = ("latent_s", "group_g", "both")


def row_of_entries(c):
    return np.repeat(np.arange(len(c["indptr"]) - 1), np.diff(c["indptr"]))


def one_latent(c, j):
    """The case with latent j alone (as latent 0 of S = 1)."""
    keep = c["indices"] == j
    counts = np.bincount(row_of_entries(c)[keep], minlength=len(c["indptr"]) - 1)
    return dict(c, indptr=np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), indices=np.zeros(int(keep.sum()), dtype=np.int32),
                data=c["data"][keep], s=1)


def one_group_of(c, g):
    """The case with group g alone: the other groups' images at -1, and G cut down to g + 1."""
    return dict(c, groups=np.where(c["groups"] == g, c["groups"], -1).astype(np.int32), g=g + 1)


def scipy_csr(c):
    import scipy.sparse

    return scipy.sparse.csr_matrix((c["data"], c["indices"], c["indptr"]), shape=(c["n_images"] * c["t"], c["s"]))
