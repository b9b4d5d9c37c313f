"""The latent-major regroup that latent_spatial and latent_exemplars open with (saev_amd/csrc/latent_major.h), restated in
numpy, the offsets at which both entries keep its product in their workspace, and the inputs of tests/test_gpu_latent_major.py, each
the smallest that reaches its branch.  tests/test_latent_major_host_cpu.py checks on the CPU that every case does what it is named for.

A case is a dict: indptr (n_images * T + 1) int64, indices int32, data float32, n_images, gh, gw (T = gh * gw rows an image), s,
groups (n_images) int32 in [-1, g), g, thr."""

import numpy as np

LM_PARTS = 1024           # entry_util.h
LM_CNT_ENTRIES = 1 << 26  # entry_util.h, lm_parts: parts x S counters at the most
TRIP = 64                 # entries a wave of the place pass takes per trip
GH = GW = 2
T = GH * GW
SHIFT = 777               # of the case whose indptr holds absolute positions


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------

def parts_of(s, nnz):
    """(parts laid out, part_len) of the counting sort, restated from entry_util.h (lm_parts, lm_part_len)."""
    parts = max(1, min(LM_PARTS, -(-nnz // 64), max(1, LM_CNT_ENTRIES // max(s, 1))))
    return parts, max(64, -(-(-(-nnz // parts)) // 64) * 64)


def is_event(c):
    """Per stored entry: a latent in [0, s), the image's group in [0, g), the value > thr (NaN and == thr are no events)."""
    rows = np.repeat(np.arange(c["indptr"].size - 1), np.diff(c["indptr"]))
    grp = c["groups"][rows // T]
    with np.errstate(invalid="ignore"):
        return (c["indices"] >= 0) & (c["indices"] < c["s"]) & (grp >= 0) & (grp < c["g"]) & (c["data"] > np.float32(c["thr"])), rows


def restate(c):
    """(starts (s + 1) int64 with the total at starts[s], row int32, val float32): the events by latent, rows ascending inside one."""
    ev, rows = is_event(c)
    lat = c["indices"][ev]
    order = np.argsort(lat, kind="stable")  # the entries are in row order: a stable sort keeps it inside a latent
    starts = np.concatenate([[0], np.cumsum(np.bincount(lat, minlength=c["s"]))]).astype(np.int64)
    return starts, rows[ev][order].astype(np.int32), c["data"][ev][order]


def _r256(b):
    return -(-max(b, 1) // 256) * 256


def offsets(s, nnz):
    """Byte offsets of starts, row and val in either entry's workspace, and where the regroup's arrays end: the error word's 256
    bytes, then starts, tot, cnt, fire_row, row, val (as test_latent_spatial_host_cpu.py and test_latent_exemplars_host_cpu.py
    restate the sizes)."""
    parts, _ = parts_of(s, nnz)
    starts = 256
    row = starts + _r256(8 * (s + 1)) + _r256(4 * s) + _r256(4 * parts * s) + _r256(4 * nnz)
    val = row + _r256(4 * nnz)
    return dict(starts=starts, row=row, val=val, end=val + _r256(4 * nnz))


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------

def _case(indptr, indices, data, s, groups, g, thr=0.0):
    n_images = (indptr.size - 1) // T
    assert n_images * T == indptr.size - 1 and groups.size == n_images
    return dict(indptr=indptr.astype(np.int64), indices=indices.astype(np.int32), data=data.astype(np.float32), n_images=n_images, gh=GH, gw=GW,
                s=s, groups=groups.astype(np.int32), g=g, thr=float(thr))


def _from_mask(mask, rng):
    rows, cols = np.nonzero(mask)  # row-major: the CSR order
    indptr = np.concatenate([[0], np.cumsum(mask.sum(axis=1))])
    return indptr, cols, rng.random(rows.size).astype(np.float32) * 4 + np.float32(0.01)


def three_trips():
    """About 150 000 entries over 300 latents on 5 000 rows: 1 024 parts of 192 entries (three trips a part) laid out, fewer used, the
    last one ragged.  Every image has a group and every value fires."""
    rng = np.random.default_rng(1201)
    n, s, g = 5000, 300, 3
    indptr, cols, vals = _from_mask(rng.random((n, s)) < 0.1, rng)
    return _case(indptr, cols, vals, s, rng.integers(0, g, n // T), g)


def cap():
    """33 or 34 latents a row on 3 000 rows, drawn from 30 000 of 131 072: about 100 000 entries, and the parts x S counters cap the
    parts at 512.  Most latents and the last one are empty; the scan over the latents carries 128 times."""
    rng = np.random.default_rng(1202)
    n, s, g = 3000, 131072, 2
    pool = np.sort(rng.choice(s - 1, size=30000, replace=False))
    draw = np.sort(rng.integers(0, pool.size, size=(n, 34)), axis=1)
    keep = np.concatenate([np.ones((n, 1), dtype=bool), np.diff(draw, axis=1) != 0], axis=1)  # (a repeated draw is dropped)
    indptr = np.concatenate([[0], np.cumsum(keep.sum(axis=1))])
    vals = rng.random(int(indptr[-1])).astype(np.float32) * 4 + np.float32(0.01)
    return _case(indptr, pool[draw[keep]], vals, s, rng.integers(0, g, n // T), g)


def one_and_distinct():
    """256 rows that store latent 0 alone, then 60 rows that store latent 0 and 127 others: parts of one trip each; the first four
    trips hold latent 0 64 times, every later one 64 distinct latents.  Every entry is an event."""
    rng = np.random.default_rng(1203)
    s, g = 200, 2
    mask = np.zeros((316, s), dtype=bool)
    mask[:, 0] = True
    for r in range(256, 316):
        mask[r, 1 + rng.choice(s - 1, size=127, replace=False)] = True
    indptr, cols, vals = _from_mask(mask, rng)
    return _case(indptr, cols, vals, s, rng.integers(0, g, 316 // T), g)


def no_events():
    """thr = 0.5 on 400 rows of 50 latents: a third of the images in no group, a fifth of the values exactly thr, a fifth below it,
    one NaN; latents 0 .. 4 store nothing, 5 .. 9 only values that do not fire, latent 10 only in images of no group."""
    rng = np.random.default_rng(1204)
    n, s, g, thr = 400, 50, 3, 0.5
    groups = rng.integers(0, g, n // T)
    groups[rng.random(n // T) < 0.33] = -1
    mask = rng.random((n, s)) < 0.2
    mask[:, :5] = False
    mask[:, 10] &= np.repeat(groups, T) < 0
    indptr, cols, vals = _from_mask(mask, rng)
    vals += np.float32(thr)
    kind = rng.random(vals.size)
    vals[kind < 0.2] = thr
    vals[(kind >= 0.2) & (kind < 0.4)] = rng.random(int(((kind >= 0.2) & (kind < 0.4)).sum())).astype(np.float32) * np.float32(0.499)
    low = (cols >= 5) & (cols < 10)
    vals[low] = np.where(rng.random(int(low.sum())) < 0.5, np.float32(thr), np.float32(0.25))
    free = np.flatnonzero(~low & (cols != 10) & (np.repeat(groups, T)[np.repeat(np.arange(n), np.diff(indptr))] >= 0))
    vals[free[free.size // 2]] = np.nan
    return _case(indptr, cols, vals, s, groups, g, thr)


def empty():
    """No stored entry at all: the count and place passes are skipped, starts is zeros."""
    return _case(np.zeros(8 * T + 1), np.zeros(0), np.zeros(0), 70, np.array([0, 1, -1, 0, 1, 1, 0, -1]), 2)


def under_a_trip():
    """37 entries: one part, one ragged trip."""
    rng = np.random.default_rng(1206)
    mask = np.zeros((8 * T, 70), dtype=bool)
    mask.reshape(-1)[rng.choice(mask.size, size=37, replace=False)] = True
    indptr, cols, vals = _from_mask(mask, rng)
    return _case(indptr, cols, vals, 70, np.array([0, 1, -1, 0, 1, 1, 0, -1]), 2)


def shifted(c=None):
    """no_events with SHIFT entries in front that no row owns -- an index out of range, a NaN value -- and an indptr of absolute
    positions: (case, nnz).  The regroup's product is that of no_events."""
    c = dict(no_events() if c is None else c)
    nnz = c["indices"].size
    c["indptr"] = c["indptr"] + SHIFT
    c["indices"] = np.concatenate([np.full(SHIFT, c["s"], dtype=np.int32), c["indices"]])
    c["data"] = np.concatenate([np.full(SHIFT, np.nan, dtype=np.float32), c["data"]])
    return c, nnz


ALL = dict(three_trips=three_trips, cap=cap, one_and_distinct=one_and_distinct, no_events=no_events, empty=empty, under_a_trip=under_a_trip)
