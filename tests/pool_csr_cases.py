"""Small designs for POOL CSR (include/saev_amd.h), each a dict(indptr, indices, data, n_images, t, s, thr) of numpy
arrays, and each planted with one property the kernels can get wrong -- named in the builder's docstring and checked on the host by
tests/test_pool_csr_host_cpu.py.  ``RANGE`` is the implementation's latent range (a workgroup's bit set), read from kernels.h."""

import pathlib
import re

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
RANGE = int(re.search(r"constexpr int POOL_CSR_RANGE = (\d+);", (ROOT / "saev_amd" / "csrc" / "kernels.h").read_text()).group(1))
FLT_MAX = np.finfo(np.float32).max
DENSIFY_MAX = 1 << 22  # n_images * s up to which a test forms the dense matrix


def build(events, n_images, t, s, thr=0.0):
    """events: (image, patch, latent, value) in the order they are to be stored inside their row."""
    rows = [[] for _ in range(n_images * t)]
    for i, p, l, v in events:
        rows[i * t + p].append((l, v))
    indptr = np.zeros(n_images * t + 1, dtype=np.int64)
    indptr[1:] = np.cumsum([len(r) for r in rows])
    flat = [e for r in rows for e in r]
    return dict(indptr=indptr, indices=np.asarray([l for l, _ in flat], dtype=np.int32).reshape(-1),
                data=np.asarray([v for _, v in flat], dtype=np.float32).reshape(-1), n_images=n_images, t=t, s=s,
                thr=thr if np.ndim(thr) == 0 else np.asarray(thr, dtype=np.float32))


def random_design(seed, n_images, t, s, per_row, thr=0.0):
    """Rows of up to ``per_row`` distinct columns in SHUFFLED order, signed values on a grid of quarters (ties inside an image are
    common, about a third are negative, some are 0)."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, min(per_row, s) + 1, n_images * t)
    indptr = np.zeros(n_images * t + 1, dtype=np.int64)
    indptr[1:] = np.cumsum(lens)
    indices = np.concatenate([rng.permutation(s)[:k] for k in lens] + [np.zeros(0, dtype=np.int64)]).astype(np.int32)
    data = (rng.integers(-4, 9, len(indices)) / 4).astype(np.float32)
    return dict(indptr=indptr, indices=indices, data=data, n_images=n_images, t=t, s=s, thr=thr)


def one_image():
    """n_images = 1: the scan has one element and the grid one workgroup."""
    return random_design(1, 1, 5, 64, 9)


def tokens(t):
    return lambda: random_design(10 + t, 7, t, 65, 6)


def latents(s):
    """A random design of s latents whose LAST row holds, in descending order, the last latent and the latents on both sides of every
    range border below it: the edges of the bit set and of the walk over ranges fire."""
    def make():
        c = random_design(100 + s % 97, 5, 5, s, 40)
        cut = int(c["indptr"][-2])
        edge = sorted({s - 1, *(q for r in range(RANGE, s, RANGE) for q in (r - 1, r))}, reverse=True)
        indptr = c["indptr"].copy()
        indptr[-1] = cut + len(edge)
        return dict(c, indptr=indptr, indices=np.concatenate([c["indices"][:cut], np.asarray(edge, dtype=np.int32)]),
                    data=np.concatenate([c["data"][:cut], np.full(len(edge), 2.0, dtype=np.float32)]))
    return make


def spans():
    """Image spans of 0, 1, 63, 64, 65 entries (one trip of 64 lanes and its edges), an image whose rows are all empty between two that
    are not, and the last image empty."""
    ev = []
    for i, n in ((1, 1), (2, 63), (3, 64), (5, 65)):  # images 0, 4 and 6 store nothing
        ev += [(i, q % 5, q, 1.0 + q) for q in range(n)]
    return build(ev, 7, 5, 70)


SPAN_LENGTHS = (0, 1, 63, 64, 0, 65, 0)
LONG_SPAN = 70_000


def long_span():
    """One image of T = 257 patches that stores 70 000 entries -- past anything a workgroup might stage -- beside a short one."""
    rng = np.random.default_rng(5)
    t, s = 257, 1000
    lens = np.full(t, LONG_SPAN // t)
    lens[: LONG_SPAN - lens.sum()] += 1
    lens = np.concatenate([lens, np.zeros(t, dtype=np.int64)])
    lens[t + 3] = 2
    indptr = np.zeros(2 * t + 1, dtype=np.int64)
    indptr[1:] = np.cumsum(lens)
    indices = np.concatenate([rng.permutation(s)[:k] for k in lens]).astype(np.int32)
    data = (rng.integers(-8, 33, len(indices)) / 8).astype(np.float32)
    return dict(indptr=indptr, indices=indices, data=data, n_images=2, t=t, s=s, thr=0.0)


def no_entries():
    """nnz = 0: every row empty, out_indptr all zeros, nothing to fill."""
    return build([], 3, 4, 10)


FULL_S = 8193


def full_row():
    """Every one of 8 193 latents fires in image 0 (the output row is as long as S and spans more than one range), in shuffled
    storage order over two patches; image 1 stores as much and nothing passes."""
    order = np.random.default_rng(3).permutation(FULL_S)
    ev = [(0, int(q % 2), int(l), 0.5 + (int(l) % 7)) for q, l in enumerate(order)] + [(1, int(q % 2), int(l), -1.0 if l % 2 else 0.0) for q, l in enumerate(order)]
    return build(ev, 2, 2, FULL_S)


MANY = 70_000


def many_images():
    """70 000 images of one token with two codes each: more units than one grid holds, and more than one chunk of the scan."""
    rng = np.random.default_rng(7)
    s = 48
    first = rng.integers(0, s, MANY)
    indices = np.stack([first, (first + rng.integers(1, s, MANY)) % s], axis=1).astype(np.int32).reshape(-1)
    data = (rng.integers(-2, 7, 2 * MANY) / 2).astype(np.float32)
    return dict(indptr=np.arange(0, 2 * MANY + 1, 2, dtype=np.int64), indices=indices, data=data, n_images=MANY, t=1, s=s, thr=0.0)


def huge(n_images=200_000, s=70_001):
    """The run the dense detour could not hold: n_images x s float32 is 56 GB; two codes an image."""
    rng = np.random.default_rng(11)
    first = rng.integers(0, s, n_images)
    indices = np.stack([first, (first + rng.integers(1, s, n_images)) % s], axis=1).astype(np.int32).reshape(-1)
    data = (rng.integers(-2, 7, 2 * n_images) / 2).astype(np.float32)
    return dict(indptr=np.arange(0, 2 * n_images + 1, 2, dtype=np.int64), indices=indices, data=data, n_images=n_images, t=1, s=s, thr=0.0)


KINDS_THR = 0.5


def value_kinds(thr):
    """Latent 0 at thr, 1 one ulp above, 2 one ulp below; 3 +0.0, 4 -0.0, 5 negative, 6 and 7 denormals of both signs, 8 FLT_MAX,
    9 -FLT_MAX; latent 10 stored in EVERY patch with negative values only (the dense pooling gives its negative maximum, the clamp 0:
    no entry); image 1 repeats the values in another patch order."""
    th = np.float32(thr)
    up, down = np.nextafter(th, np.float32(np.inf)), np.nextafter(th, np.float32(-np.inf))
    vals = [th, up, down, 0.0, -0.0, -1.5, 1e-45, -1e-45, FLT_MAX, -FLT_MAX]
    ev = [(0, l % 3, l, v) for l, v in enumerate(vals)] + [(1, 2 - l % 3, l, v) for l, v in enumerate(vals)]
    ev += [(i, p, 10, -1.0 - p) for i in range(2) for p in range(3)]
    return build(ev, 2, 3, 11, thr)


def patches():
    """T = 6.  Latent 0: the maximum in the first patch; 1: in the last; 2: in patches 2 and 4 (the lower wins); 3: one equal value in
    every patch (patch 0, count 6); 4: ascending values (last patch), 5: descending (first)."""
    ev = [(0, 0, 0, 9.0), (0, 3, 0, 2.0), (0, 5, 0, 8.5), (0, 0, 1, 1.0), (0, 2, 1, 3.0), (0, 5, 1, 7.0), (0, 1, 2, 1.0), (0, 2, 2, 4.0), (0, 3, 2, 2.0), (0, 4, 2, 4.0)]
    ev += [(0, p, 3, 2.5) for p in range(6)] + [(0, p, 4, 1.0 + p) for p in range(6)] + [(0, p, 5, 9.0 - p) for p in range(6)]
    return build(ev, 1, 6, 6)


def columns():
    """Rows with descending columns, and column 3 TWICE in row (0, 1): the maximum ignores the repeat (2.0 then 5.0 -> 5.0 at patch 1), the
    count takes both; in image 1 the repeat holds the same value twice."""
    ev = [(0, 0, 7, 1.0), (0, 0, 3, 1.0), (0, 0, 1, 2.0), (0, 1, 3, 2.0), (0, 1, 6, 1.0), (0, 1, 3, 5.0), (1, 0, 3, 4.0), (1, 0, 3, 4.0), (1, 1, 2, 1.0), (1, 1, 0, 1.0)]
    return build(ev, 2, 2, 8)


def vector_thresholds():
    """Per-latent thresholds: 0, 0.5, 2, +Inf (silenced), NaN (passes nothing), FLT_MAX, 0 again, 1.0 -- latents 1 and 7 hold values
    exactly at theirs in one image and above it in another."""
    thr = np.asarray([0.0, 0.5, 2.0, np.inf, np.nan, FLT_MAX, 0.0, 1.0], dtype=np.float32)
    ev = []
    for i in range(3):
        for p in range(4):
            ev += [(i, p, l, v) for l, v in ((0, 0.25 * p), (1, 0.5 + 0.25 * i * p), (2, 1.0 + i), (3, FLT_MAX), (4, 3.0), (5, FLT_MAX), (6, -1.0 + p), (7, 1.0 + (i == 2) * p))]
    return build(ev, 3, 4, 8, thr)


def vector_random():
    """A random design past one range under random thresholds (a tenth +Inf, a tenth NaN, a fifth 0)."""
    rng = np.random.default_rng(13)
    s = RANGE + 37
    thr = (rng.integers(0, 6, s) / 4).astype(np.float32)
    kind = rng.integers(0, 10, s)
    thr[kind == 0], thr[kind == 1], thr[(kind == 2) | (kind == 3)] = np.inf, np.nan, 0.0
    return dict(random_design(14, 6, 5, s, 300), thr=thr)


SMALL = {
    "one_image": one_image, "tokens_1": tokens(1), "tokens_5": tokens(5), "tokens_16": tokens(16), "tokens_257": tokens(257),
    "s_1": latents(1), "s_64": latents(64), "s_65": latents(65), "s_range_minus_1": latents(RANGE - 1), "s_range": latents(RANGE),
    "s_range_plus_1": latents(RANGE + 1), "s_70001": latents(70_001), "spans": spans, "long_span": long_span, "no_entries": no_entries,
    "full_row": full_row, "many_images": many_images, "values_thr_0": lambda: value_kinds(0.0), "values_thr_half": lambda: value_kinds(KINDS_THR),
    "patches": patches, "columns": columns, "vector_thresholds": vector_thresholds, "vector_random": vector_random,
}


def densifiable(c):
    return c["n_images"] * c["s"] <= DENSIFY_MAX


BROKEN = ("column_negative", "column_s", "value_nan", "value_inf", "indptr_decreasing", "indptr_past_nnz", "threshold_negative")


def broken(kind):
    """(case, error code): a good design with ONE fault.  The faulty column is once negative and once = s; the bad indptr once steps
    back inside an image and once runs past nnz."""
    c = random_design(21, 4, 3, 40, 8)
    c = dict(c, indptr=c["indptr"].copy(), indices=c["indices"].copy(), data=c["data"].copy())
    mid = len(c["data"]) // 2
    if kind == "column_negative":
        c["indices"][mid] = -1
        return c, 1
    if kind == "column_s":
        c["indices"][mid] = c["s"]
        return c, 1
    if kind == "value_nan":
        c["data"][mid] = np.nan
        return c, 2
    if kind == "value_inf":
        c["data"][mid] = np.inf
        return c, 2
    if kind == "indptr_decreasing":
        at = int(np.flatnonzero(np.diff(c["indptr"]) > 1)[1])
        assert c["indptr"][at] > 0
        c["indptr"][at + 1] = c["indptr"][at] - 1  # still a position into indices: only the order is wrong
        return c, 3
    if kind == "indptr_past_nnz":
        c["indptr"][-1] += 5
        return c, 3
    assert kind == "threshold_negative"
    thr = np.zeros(c["s"], dtype=np.float32)
    thr[17] = -0.25
    return dict(c, thr=thr), 4


def one_image_of(c, i):
    """Image i of a case, alone."""
    t = c["t"]
    lo, hi = c["indptr"][i * t], c["indptr"][(i + 1) * t]
    return dict(c, indptr=c["indptr"][i * t : (i + 1) * t + 1] - lo, indices=c["indices"][lo:hi], data=c["data"][lo:hi], n_images=1)


def permuted(c, perm):
    """The images of a case in the order ``perm``."""
    t = c["t"]
    parts = [one_image_of(c, int(i)) for i in perm]
    lens = np.concatenate([np.diff(p["indptr"]) for p in parts] + [np.zeros(0, dtype=np.int64)])
    indptr = np.zeros(len(perm) * t + 1, dtype=np.int64)
    indptr[1:] = np.cumsum(lens)
    return dict(c, indptr=indptr, indices=np.concatenate([p["indices"] for p in parts]), data=np.concatenate([p["data"] for p in parts]), n_images=len(perm))
