"""Small inputs of the per-latent histogram and quantile tests (tests/test_latent_hist_host_cpu.py, tests/test_gpu_latent_hist.py).
Every builder returns a dict: ``indptr, indices, data`` (CSR, int64 / int32 / float32), ``S``, ``q``, ``over`` (the mode the case
is about; the tests run both), optionally ``splits`` (row boundaries of the batches it is fed in) and ``hist_only``; and ``holds``,
a predicate on the case itself that the CPU suite asserts, so that a case cannot silently stop exercising what it names.

Where the kernels of saev_amd/csrc/latenthist.hip change behaviour, and the case on each side:
  GRID_ENTRIES   one grid of the update kernel covers LH_GRID_CAP * 256 = 262 144 entries in one step per workgroup; past it a
                 workgroup takes several steps and its LDS table lives across them                 (past_grid, flush0 | the rest)
  FLUSH_KEYS     a workgroup flushes its table mid-stream when a step could push it past LH_FILL = 3 584 keys: at level 0 after 13
                 steps of distinct counters (flush0), at levels 1 and 2 with 16 targets before every later step (past_grid)
  S              no kernel changes with S (one workgroup per latent locates; the update indexes S x 4096 counters in 32 bits, which
                 the entry refuses from S = 1 048 575 on); S = 1, 3 .. 8, 257, 400, 4 097 and 70 001 are here
"""

import numpy as np

GRID_ENTRIES = 1024 * 256
FLUSH_KEYS = 3584
F32 = np.float32


def _bits(*u):
    return np.array(u, dtype=np.uint32).view(np.float32)


def _csr(rows, S, q, over="rows", **more):
    """rows: one (latents, values) pair per row."""
    indptr = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum([len(r[0]) for r in rows], out=indptr[1:])
    cat = lambda k, dt: np.concatenate([np.asarray(r[k], dtype=dt) for r in rows]) if rows else np.zeros(0, dt)
    return dict(indptr=indptr, indices=cat(0, np.int32), data=cat(1, np.float32), S=S, q=tuple(q), over=over, **more)


def _columns(cols, n, S, q, over="rows", **more):
    """cols: {latent: values of rows 0 .. len - 1} (at most n each)."""
    rows = [([], []) for _ in range(n)]
    for j, vals in sorted(cols.items()):
        for r, v in enumerate(np.asarray(vals, dtype=np.float32)):
            rows[r][0].append(j)
            rows[r][1].append(v)
    return _csr(rows, S, q, over, **more)


def _per_latent(c):
    return np.bincount(c["indices"][(c["data"] != 0) & (c["indices"] >= 0) & (c["indices"] < c["S"])], minlength=c["S"])


def n1():
    c = _csr([([0, 2, 4], [1.5, -2.0, 0.25])], 5, (0.0, 0.5, 1.0))
    return dict(c, holds=lambda c: c["indptr"].size == 2)


def empty_batch_between():
    rng = np.random.default_rng(1)
    rows = [(rng.choice(9, 3, replace=False), rng.standard_normal(3)) for _ in range(12)]
    c = _csr(rows, 9, (0.5, 0.9), splits=(0, 5, 5, 12))
    return dict(c, holds=lambda c: 5 in c["splits"] and c["splits"].count(5) == 2)


def ragged_0_300():
    rng = np.random.default_rng(2)
    rows = [(np.sort(rng.choice(400, i, replace=False)), rng.standard_normal(i) * np.exp2(rng.integers(-8, 8, i))) for i in range(301)]
    c = _csr(rows, 400, (0.5, 0.9, 0.95, 0.99))
    return dict(c, holds=lambda c: sorted(np.diff(c["indptr"]).tolist()) == list(range(301)) and (c["data"] < 0).any())


def silent_and_dense():
    rng = np.random.default_rng(3)
    n = 40
    cols = {0: rng.standard_normal(17), 1: np.abs(rng.standard_normal(5)), 3: rng.standard_normal(n) + 3, 5: -np.abs(rng.standard_normal(n))}
    c = _columns(cols, n, 6, (0.0, 0.5, 1.0))
    return dict(c, holds=lambda c: _per_latent(c)[2] == 0 and _per_latent(c)[3] == 40 and _per_latent(c)[5] == 40)


def third_pass_decides():
    c = _columns({0: _bits(0x3F800001, 0x3F800000), 1: _bits(0xBF800000, 0xBF800001)}, 2, 2, (0.0, 1.0), over="entries")
    return dict(c, holds=lambda c: len(set((c["data"].view(np.uint32) >> 10).tolist())) == 2 and len(set(c["data"].view(np.uint32).tolist())) == 4)


def bin_borders():
    """Ranks 1 and 3 of latent 0 are the first and the last element of level-0 bin [1, 1.125); ranks 1 .. 4 of latent 1 are the last
    element of level-1 bin 0, the first and the last of bin 1 and the first of bin 2, all inside one level-0 bin."""
    lat0 = _bits(0x3F900000, 0x3F7FFFFF, 0x3F8FFFFF, 0x3F800000, 0x3F880000)   # 1.125, <1, <1.125, 1, 1.0625
    lat1 = _bits(0x3F800800, 0x3F8003FF, 0x3F8007FF, 0x3F800000, 0x3F800400)
    c = _columns({0: lat0, 1: lat1}, 5, 2, (0.0, 0.25, 0.5, 0.75, 1.0), over="entries")
    return dict(c, holds=lambda c: (np.sort(c["data"][c["indices"] == 0]).view(np.uint32) >> 20).tolist() == [0x3F7, 0x3F8, 0x3F8, 0x3F8, 0x3F9])


def q_one():
    rng = np.random.default_rng(4)
    c = _columns({j: rng.standard_normal(rng.integers(1, 30)) for j in range(7)}, 30, 8, (0.95,))
    return dict(c, holds=lambda c: len(c["q"]) == 1)


def q_eight():
    rng = np.random.default_rng(5)
    c = _columns({j: rng.standard_normal(rng.integers(1, 60)) * 100 for j in range(63)}, 60, 63, (0.0, 0.01, 0.25, 0.5, 0.75, 0.9, 0.999, 1.0))
    return dict(c, holds=lambda c: len(c["q"]) == 8)


def zero_block():
    """N = 10, h = 9 q.  Latent 0 (2 negatives, 5 zeros, 3 positives): ranks 1 | 2 .. 6 | 7 lie before, on the first and last element
    of, and after the block; q = 0.5 falls entirely inside; q = 0.15 straddles its start.  Latent 1 has no negatives, latent 2 no
    silent row, latent 3 only negatives.  q = 1/9, 2/9, 6/9, 7/9 make h integral: lower == higher."""
    cols = {0: [-1.5, 2.0, -0.5, 4.0, 3.0], 1: [1.0, 2.0, 3.0, 4.0], 2: [-3, 5, -1, 2, 7, -8, 9, 1.5, -2.5, 6], 3: [-1.0, -2.0, -3.0]}
    c = _columns(cols, 10, 4, (0.0, 1 / 9, 2 / 9, 0.5, 6 / 9, 7 / 9, 1.0, 0.15))
    return dict(c, holds=lambda c: _per_latent(c).tolist() == [5, 4, 10, 3] and all(float(np.float64(9) * np.float64(k / 9)) == k for k in (1, 2, 6, 7)))


def value_classes():
    big = np.finfo(np.float32).max
    cols = {0: _bits(0x00000001, 0x807FFFFF, 0x00400000), 1: [big, -big, 1.0], 2: [np.inf, -np.inf, 2.0, -2.0], 3: [-0.0, 0.0, 5.0],
            -1: [1.0, 2.0], 8: [3.0], 13: [4.0]}
    c = _columns(cols, 6, 8, (0.0, 0.5, 1.0))
    return dict(c, holds=lambda c: np.isinf(c["data"]).sum() == 2 and (c["data"] == 0).sum() == 2 and np.signbit(c["data"][c["data"] == 0]).any()
                and (c["indices"] < 0).any() and (c["indices"] >= 8).sum() == 2 and (np.abs(c["data"][c["data"] != 0]) < np.finfo(np.float32).tiny).sum() == 3)


def crowded_bin():
    n = 70_000
    rng = np.random.default_rng(6)
    sparse = np.zeros(n, dtype=np.float32)
    sparse[rng.choice(n, 50, replace=False)] = rng.standard_normal(50).astype(np.float32)
    rows = [([0, 1], [2.5, sparse[r]]) if sparse[r] != 0 else ([0], [2.5]) for r in range(n)]
    c = _csr(rows, 3, (0.5,))
    return dict(c, holds=lambda c: _per_latent(c)[0] == 70_000 and np.unique(c["data"][c["indices"] == 0]).size == 1)


def crowded_pair():
    n = 70_000
    c = dict(indptr=np.arange(0, 2 * n + 1, 2, dtype=np.int64), indices=np.tile(np.array([0, 1], np.int32), n),
             data=np.tile(np.array([2.5, -1.25], np.float32), n), S=2, q=(0.25, 0.5), over="rows")
    return dict(c, holds=lambda c: _per_latent(c).tolist() == [70_000, 70_000] and np.unique(c["data"]).size == 2)


def past_grid():
    """More entries than one grid covers, all in one level-0 bin, 16 targets: every workgroup takes a second step at every level, and at
    levels 1 and 2 flushes before it."""
    rng = np.random.default_rng(7)
    n, cap, S = 9000, 32, 257
    idx = np.stack([np.sort(rng.choice(S, cap, replace=False)) for _ in range(n)]).astype(np.int32)
    val = (1 + rng.integers(0, 1 << 20, (n, cap)) * 2.0**-23).astype(np.float32)  # [1, 1.125)
    c = dict(indptr=np.arange(0, n * cap + 1, cap, dtype=np.int64), indices=idx.reshape(-1), data=val.reshape(-1), S=S,
             q=(0.0, 0.1, 0.25, 0.5, 0.75, 0.9, 0.99, 1.0), over="rows")
    return dict(c, holds=lambda c: c["data"].size > GRID_ENTRIES and set((c["data"].view(np.uint32) >> 20).tolist()) == {0x3F8} and 2 * len(c["q"]) * 256 > FLUSH_KEYS)


def flush0():
    """A level-0 update whose workgroups each meet more than FLUSH_KEYS distinct counters: flushed mid-stream, then again at the end."""
    rng = np.random.default_rng(8)
    S, nnz, n = 4097, 17 * GRID_ENTRIES + 77, 4001
    cuts = np.sort(rng.integers(0, nnz + 1, n - 1))
    c = dict(indptr=np.concatenate([[0], cuts, [nnz]]).astype(np.int64), indices=rng.integers(0, S, nnz).astype(np.int32),
             data=(rng.standard_normal(nnz) * np.exp2(rng.integers(-20, 20, nnz))).astype(np.float32), S=S, q=(0.5,), over="entries", hist_only=True)
    first = (np.arange(17)[:, None] * GRID_ENTRIES + np.arange(256)).ravel()  # the entries of workgroup 0
    return dict(c, first=first, holds=lambda c: np.unique(c["indices"][c["first"]].astype(np.int64) * 4096 + (c["data"][c["first"]].view(np.uint32) >> 20)).size
                > FLUSH_KEYS + 256 and (c["data"] != 0).all())


def s_70001():
    rng = np.random.default_rng(9)
    S = 70_001
    rows = [(np.sort(rng.choice(S, 9, replace=False)), rng.standard_normal(9)) for _ in range(50)]
    rows[7] = ([0, S - 1], [1.0, -1.0])
    c = _csr(rows, S, (0.5,), hist_only=True)
    return dict(c, holds=lambda c: c["S"] == 70_001 and c["data"].size < 1000 and (c["indices"] == 70_000).any())


CASES = {f.__name__: f for f in (n1, empty_batch_between, ragged_0_300, silent_and_dense, third_pass_decides, bin_borders, q_one, q_eight,
                                 zero_block, value_classes, crowded_bin, crowded_pair, past_grid, flush0, s_70001)}
SMALL = [name for name in CASES if name not in ("crowded_bin", "crowded_pair", "past_grid", "flush0", "s_70001")]

_built = {}


def get(name):
    """The case, built once and shared (treat it as read-only)."""
    if name not in _built:
        _built[name] = CASES[name]()
    return _built[name]
