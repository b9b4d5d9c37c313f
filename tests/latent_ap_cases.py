"""The designs the latent AP tests run (include/saev_amd.h: LATENT AP): shapes, value images, tie groups and zero groups, each at the
smallest size where that piece of the kernels can go wrong.  Every builder returns a dict with the CSR (indptr int64, indices int32,
data float32), the shape n, s, c and ``cls`` (n int32, -1 = no class); everything is seeded.

DIRECT_MAX mirrors saev_latent_ap_layout.direct_max (tests/test_latent_ap_host_cpu.py compares the two)."""

import numpy as np
import scipy.sparse

DIRECT_MAX = 8
GROUP_SIZES = (1, 2, DIRECT_MAX - 1, DIRECT_MAX, DIRECT_MAX + 1, 63, 64, 65, 1000)   # and n, in `whole_group`
GROUP_T = (0, 1, 31, 63, 64, 65, 1000, "last")                                       # "last": t = n - size


def _pack(dense, stored, cls, n_classes, shift=0):
    rows, cols = np.nonzero(stored)
    csr = scipy.sparse.csr_matrix((dense[rows, cols].astype(np.float32), (rows, cols)), shape=dense.shape)
    csr.sort_indices()
    assert csr.nnz == int(stored.sum())
    indptr = csr.indptr.astype(np.int64) + shift
    pad = np.zeros(shift, dtype=np.int32)
    return dict(indptr=indptr, indices=np.concatenate([pad, csr.indices.astype(np.int32)]),
                data=np.concatenate([pad.astype(np.float32), csr.data.astype(np.float32)]), n=dense.shape[0], s=dense.shape[1], c=n_classes,
                cls=np.asarray(cls, dtype=np.int32))


def _labels(rng, n, c, present=None, none=0.1):
    present = np.arange(c) if present is None else np.asarray(present)
    cls = rng.choice(present, size=n).astype(np.int32)
    cls[:min(len(present), n)] = present[:n]
    cls[rng.random(n) < none] = -1
    return cls


def single():
    """(N, S, C) = (1, 1, 1): one row, one event, its class the only one."""
    return _pack(np.array([[2.0]], dtype=np.float32), np.array([[True]]), [0], 1)


def kinds(n=257, s=48, c=11, seed=1):
    """The fixture's latent kinds at (257, 48, 11): no events, one event, every row distinct, every row one value, 0/1, quantised,
    signed, signed and quantised, stored +0.0 / -0.0; column c - 1 never occurs."""
    rng = np.random.default_rng(seed)
    cls = _labels(rng, n, c, present=np.arange(c - 1))
    dense = np.zeros((n, s), dtype=np.float32)
    stored = np.zeros((n, s), dtype=bool)
    for j in range(s):
        on = rng.random(n) < rng.uniform(0.02, 0.5)
        v = rng.gamma(2.0, 0.6, size=n).astype(np.float32) + np.float32(0.01)
        v = v + np.where(cls == j % (c - 1), rng.uniform(0.3, 1.5), 0.0).astype(np.float32)
        if j % 4 == 2:
            v = v * np.where(rng.random(n) < 0.4, -1.0, 1.0).astype(np.float32)
        if j % 3 == 1:
            v = np.sign(v) * np.ceil(np.abs(v) * (2 if j % 2 else 4)) / (2 if j % 2 else 4)
        dense[:, j], stored[:, j] = np.where(on, v, 0), on
    stored[:, 0] = False
    stored[:, 5] = False
    stored[200, 5], dense[200, 5] = True, -0.75
    stored[:, 7] = True
    dense[:, 7] = rng.permutation(n).astype(np.float32) - np.float32(100.5)  # every row, distinct, both signs
    stored[:, 9], dense[:, 9] = True, 1.5
    stored[:, 11], dense[:, 11] = True, -2.0
    dense[:, 13] = np.where(stored[:, 13], 1.0, 0.0)
    dense = np.where(stored, dense, 0).astype(np.float32)
    r = np.flatnonzero(stored[:, 15])[:2]
    dense[r[0], 15], dense[r[1], 15] = 0.0, -0.0
    return _pack(dense, stored, cls, c)


def wide(n, s, c, seed):
    """(257, 1, 65) and (300, 2, 4096): class columns past one 64-lane group and at the limit, most columns empty."""
    rng = np.random.default_rng(seed)
    present = np.unique(np.concatenate([[0, 63, 64 % c, c - 1], rng.integers(0, c, size=12)]))
    cls = _labels(rng, n, c, present=present)
    dense = np.zeros((n, s), dtype=np.float32)
    stored = rng.random((n, s)) < 0.4
    dense[stored] = np.ceil(rng.gamma(2.0, 1.0, size=int(stored.sum())) * 4) / 4 * rng.choice([1.0, 1.0, -1.0], size=int(stored.sum()))
    stored &= dense != 0
    return _pack(dense, stored, cls, c)


def ragged(n=5000, s=1031, c=64, seed=3):
    """(5000, 1031, 64): a latent with 5000 events next to a thousand with 0-3; row_ptr shifted by a constant."""
    rng = np.random.default_rng(seed)
    cls = _labels(rng, n, c)
    dense = np.zeros((n, s), dtype=np.float32)
    stored = np.zeros((n, s), dtype=bool)
    for j in range(s):
        k = int(rng.integers(0, 4))
        rows = rng.choice(n, size=k, replace=False)
        stored[rows, j] = True
        dense[rows, j] = rng.choice([0.5, 1.0, -1.0, 2.25], size=k)
    stored[:, 517] = True
    dense[:, 517] = np.ceil(rng.gamma(2.0, 2.0, size=n) * 8) / 8 + 0.125
    return _pack(dense, stored, cls, c, shift=37)


def deep(n=70_000, s=3, c=5, seed=4):
    """(70 000, 3, 5): ranks past 2^16 -- a latent with 60 events, a dense latent of 64 999 positive events (its zero group of 5001
    rows behind them) with a few hundred tie groups, and a signed one."""
    rng = np.random.default_rng(seed)
    cls = _labels(rng, n, c)
    dense = np.zeros((n, s), dtype=np.float32)
    stored = np.zeros((n, s), dtype=bool)
    rows = rng.choice(n, size=60, replace=False)
    stored[rows, 0], dense[rows, 0] = True, rng.gamma(2.0, 1.0, size=60) + 0.1
    rows = rng.choice(n, size=64_999, replace=False)
    stored[rows, 1] = True
    dense[rows, 1] = np.ceil(rng.gamma(2.0, 8.0, size=64_999) * 4) / 4 + 0.25
    rows = rng.choice(n, size=3000, replace=False)
    stored[rows, 2] = True
    dense[rows, 2] = (np.ceil(rng.gamma(2.0, 2.0, size=3000) * 2) / 2 + 0.5) * rng.choice([1.0, -1.0], size=3000)
    return _pack(dense, stored, cls, c)


def value_images(n=300, s=3, c=4, seed=5):
    """Values whose key differs in every byte: random bit patterns (no NaN, no zero), denormals and +-Inf, so that every radix digit
    of the sort matters.  Duplicated values make ties that only the row order breaks."""
    rng = np.random.default_rng(seed)
    cls = _labels(rng, n, c)
    bits = rng.integers(0, 1 << 32, size=(n, s), dtype=np.uint64).astype(np.uint32)
    dense = bits.view(np.float32).copy()
    dense[np.isnan(dense)] = 1.0
    dense[:20, 0] = (rng.integers(1, 1 << 20, size=20).astype(np.uint32)).view(np.float32)             # positive denormals
    dense[20:40, 0] = (rng.integers(1, 1 << 20, size=20).astype(np.uint32) | np.uint32(1 << 31)).view(np.float32)  # negative ones
    dense[40:43, 1], dense[43:46, 1] = np.inf, -np.inf
    dense[100:140, 2] = dense[60:100, 2]  # ties across rows
    stored = rng.random((n, s)) < 0.8
    stored &= dense != 0
    return _pack(dense, stored, cls, c)


# the five latents of one (size, t, sign): what lies before the group and what the group holds, as (class, count) lists in terms of
# n = size; class 3 stands for "no class".  Together: r in {0, 1, n/2, n} and R in {0, t} for classes 0 and 1.
def _variants(size, t):
    half = size // 2
    return [
        ([(0, t)], [(0, size)]),                                   # class 0: R = t, r = n;  class 1: r = 0
        ([(0, t)], [(1, min(1, size - half)), (0, half), (2, size - half - min(1, size - half))]),  # 0: R = t, r = n/2;  1: R = 0, r = 1
        ([(3, t)], [(0, half), (1, min(1, size - half)), (3, size - half - min(1, size - half))]),  # 0: R = 0, r = n/2
        ([(1, t)], [(0, size)]),                                   # 0: R = 0, r = n;  1: R = t, r = 0
        ([(0, t)], [(0, 1), (3, size - 1)]),                       # 0: R = t, r = 1
    ]


def tie_groups(size, seed=6):
    """One tie group of ``size`` rows at every t of GROUP_T, with positive and with negative values, in the five variants above.
    Positive: t distinct larger values, the group, then the zero group.  Negative: t // 2 distinct positive values and a zero group
    of t - t // 2 rows before the group, distinct smaller values on every other row behind it."""
    rng = np.random.default_rng(seed + size)
    pool = {0: 1000 + size, 1: 1000, 2: size, 3: 1000 + size}   # rows of each class (3: none)
    cls = np.concatenate([np.full(k, c if c < 3 else -1, dtype=np.int32) for c, k in pool.items()])
    n = len(cls)
    perm = rng.permutation(n)
    cls = cls[perm]
    rows_of = {c: np.flatnonzero(cls == (c if c < 3 else -1)) for c in pool}
    cols = []
    for t_name in GROUP_T:
        t = n - size if t_name == "last" else t_name
        for sign in (1.0, -1.0):
            for before, group in _variants(size, t):
                if t_name == "last" and sign > 0:
                    before = [(None, t)]  # any rows: more than one class has
                v = np.zeros(n, dtype=np.float32)
                free = {c: list(rng.permutation(r)) for c, r in rows_of.items()}
                take = lambda c, k: [free[c].pop() for _ in range(k)]  # noqa: E731
                g_rows = np.asarray([r for c, k in group for r in take(c, k)], dtype=np.int64)
                if before[0][0] is None or t_name == "last":
                    rest = np.asarray([r for c in free for r in free[c]], dtype=np.int64)
                    b_rows = rng.permutation(rest)[:t]
                else:
                    b_rows = np.asarray([r for c, k in before for r in take(c, k)], dtype=np.int64)
                assert len(b_rows) == t and len(g_rows) == size
                if sign > 0:
                    v[b_rows] = 2.0 + 0.25 * np.arange(t, dtype=np.float32)
                    v[g_rows] = 0.5
                else:
                    n_pos = t // 2
                    v[b_rows[:n_pos]] = 2.0 + 0.25 * np.arange(n_pos, dtype=np.float32)
                    others = np.setdiff1d(np.arange(n), np.concatenate([b_rows, g_rows]))
                    v[g_rows] = -0.5
                    v[others] = -1.0 - 0.25 * rng.permutation(len(others)).astype(np.float32)
                cols.append(v)
    dense = np.stack(cols, axis=1)
    return _pack(dense, dense != 0, cls, 3)


def whole_group(n=257, seed=7):
    """A tie group of all N rows (positive, and negative), Z = 0."""
    rng = np.random.default_rng(seed)
    cls = _labels(rng, n, 3)
    dense = np.stack([np.full(n, 0.5, dtype=np.float32), np.full(n, -3.0, dtype=np.float32)], axis=1)
    return _pack(dense, dense != 0, cls, 3)


def zero_groups(n=200, seed=8):
    """Zero groups of Z = 0, 1, DIRECT_MAX - 1, DIRECT_MAX + 1 and N - 1 rows behind distinct positive values, and the same Z with
    negative values behind them; class 2 has one row, class 3's rows never fire (all of them lie in every zero group but Z = 0's)."""
    rng = np.random.default_rng(seed)
    cls = rng.integers(0, 2, size=n).astype(np.int32)
    cls[5] = 2
    quiet = np.arange(n - 4, n)
    cls[quiet] = 3
    cls[rng.choice(n - 4, size=15, replace=False) + 0] = -1
    cls[5] = 2
    cols = []
    for z in (0, 1, DIRECT_MAX - 1, DIRECT_MAX + 1, n - 1):
        for neg in (False, True):
            v = np.zeros(n, dtype=np.float32)
            order = np.concatenate([rng.permutation(n - 4), quiet])  # the quiet rows are the last to fire
            fire = order[:n - z]
            v[fire] = 1.0 + 0.5 * rng.permutation(len(fire)).astype(np.float32)
            if neg:
                v[fire[::2]] *= -1.0
            cols.append(v)
    dense = np.stack(cols, axis=1)
    return _pack(dense, dense != 0, cls, 4)


# name -> builder of the designs whose exact evaluation takes seconds on the CPU as well (the host test runs these too)
SMALL = {"single": single, "kinds": kinds, "wide_65": lambda: wide(257, 1, 65, 21), "whole_group": whole_group, "zero_groups": zero_groups,
         "value_images": value_images, "tie_2": lambda: tie_groups(2), "tie_dm+1": lambda: tie_groups(DIRECT_MAX + 1)}
LARGE = {"wide_4096": lambda: wide(300, 2, 4096, 22), "ragged": ragged, "deep": deep,
         **{f"tie_{k}": (lambda k=k: tie_groups(k)) for k in GROUP_SIZES if k not in (2, DIRECT_MAX + 1)}}
