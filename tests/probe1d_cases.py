"""The inputs of the probe1d tests, as functions of nothing but their arguments (numpy arrays from seeded generators), so that the host
tests (test_probe1d_host_cpu.py) can check on the CPU, with the fp64 restatement (probe1d_restatement.py), the conditions the GPU
tests (test_gpu_probe1d.py, test_gpu_probe1d_geometry.py) rely on for the very same arrays: how many groups of 64 a part of the
counting sort holds, which slabs of a fit stop when and how far from tol, how far every probability lies from a threshold."""

import dataclasses

import numpy as np

import probe1d_restatement as R

CHUNK = 512
P1_PARTS = 1024          # entry_util.h: LM_PARTS
P1_CNT_ENTRIES = 1 << 26  # entry_util.h, lm_parts: parts x S counters at the most


def parts_of(s, nnz):
    """(parts, part_len) of prepare's counting sort, restated from entry_util.h (lm_parts, lm_part_len)."""
    parts = max(1, min(P1_PARTS, -(-nnz // 64), max(1, P1_CNT_ENTRIES // max(s, 1))))
    return parts, max(64, -(-(-(-nnz // parts)) // 64) * 64)


@dataclasses.dataclass
class Design:
    n: int
    s: int
    c: int
    indptr: np.ndarray   # (n + 1) int64
    indices: np.ndarray  # (nnz) int32
    data: np.ndarray     # (nnz) float32
    ymat: np.ndarray     # (n, c) bool
    ids: np.ndarray | None = None  # (n) class ids where the labels are one-hot
    kinds: tuple = ()    # fit designs: the kind of every class

    @property
    def nnz(self):
        return int(self.data.size)

    @property
    def csr(self):
        return self.indptr, self.indices, self.data


# ---- the designs of test_gpu_probe1d.py (moved here: the host tests check their threshold gaps) ---------------------------------------------

def make_design(n, s, seed, *, full=False, specials=True):
    """A CSR matrix with signed values, one stored 0.0, and -- where they fit -- latents with 0, 1, CHUNK - 1, CHUNK, CHUNK + 1 and (full)
    n entries; without `full` some rows hold no entry at all."""
    rng = np.random.default_rng(seed)
    counts = rng.integers(0, min(n, 40) + 1, size=s)
    wanted = [0, 1, CHUNK - 1, CHUNK, CHUNK + 1] + ([n] if full else [])
    if specials:
        for j, k in enumerate(k for k in wanted if k <= n):
            if j < s:
                counts[j] = k
    if full and s < 6:
        counts[s - 1] = n
    free_rows = np.arange(n) if full or n < 8 else np.setdiff1d(np.arange(n), np.arange(3, n, 17))  # rows 3, 20, ... stay empty
    rows, cols = [], []
    for j in range(s):
        k = min(int(counts[j]), free_rows.size) if counts[j] < n else n
        r = np.arange(n) if k == n else rng.choice(free_rows, size=k, replace=False)
        rows.append(r)
        cols.append(np.full(k, j))
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    vals = rng.standard_normal(rows.size).astype(np.float32) * 1.5
    if vals.size:
        vals[rng.integers(vals.size)] = 0.0
    order = np.lexsort((cols, rows))
    rows, cols, vals = rows[order], cols[order], vals[order]
    indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int64)
    return indptr, cols.astype(np.int32), vals


def make_labels(n, c, seed):
    rng = np.random.default_rng(seed + 1000)
    ids = rng.integers(0, c, size=n)
    if c > 2 and n > c:
        ids[ids == c - 2] = 0  # a class that never occurs
    return ids.astype(np.uint8 if c <= 256 else np.int32)


# every C of the contract's dispatch (1, <= 8, <= 16, <= 32, one group, several groups, a ragged last word) on the three sizes
CASES = [(1, 1, 1, False), (257, 48, 11, False), (257, 1, 32, True), (257, 48, 33, False), (5000, 1031, 64, True), (5000, 48, 65, False),
         (5000, 1031, 151, True), (5000, 1031, 256, False), (1, 48, 11, True)]
CASE_IDS = [f"n{n}_s{s}_c{c}" for n, s, c, _ in CASES]


def case_design(i):
    n, s, c, full = CASES[i]
    seed = 50 + i
    ids = make_labels(n, c, seed)
    return Design(n, s, c, *make_design(n, s, seed, full=full), R.labels_matrix(ids, c), ids)


def coefficients(s, c, seed):
    """(b, w) with ordinary pairs, logits beyond +-40 and products w v beyond +-800."""
    rng = np.random.default_rng(seed)
    b, w = rng.normal(0, 2, size=(s, c)), rng.normal(0, 1, size=(s, c))
    far = rng.random((s, c))
    b = np.where(far < 0.05, 45.0, np.where(far < 0.10, -45.0, b))
    w = np.where((far > 0.10) & (far < 0.15), 900.0, np.where((far > 0.15) & (far < 0.20), -900.0, w))
    return b, w


# ---- A: placement across groups and parts ---------------------------------------------------------------------------------------------------

def _from_mask(mask, rng):
    rows, cols = np.nonzero(mask)  # row-major: the CSR order
    vals = (rng.standard_normal(rows.size) * 1.5).astype(np.float32)
    indptr = np.concatenate([[0], np.cumsum(mask.sum(axis=1))]).astype(np.int64)
    return indptr, cols.astype(np.int32), vals


def _ids(rng, n, c, absent):
    ids = rng.integers(0, c, size=n)
    ids[ids == absent] = 0
    ids[:2] = (c - 1, 0)
    return ids.astype(np.uint8)


def two_groups():
    """31 or 32 distinct latents of 300 on each of 2 100 rows: parts of 128 entries, two groups of 64 each."""
    rng = np.random.default_rng(701)
    n, s, c = 2100, 300, 11
    r = rng.random((n, s))
    kth = np.sort(r, axis=1)[np.arange(n), rng.integers(31, 33, size=n) - 1]
    ids = _ids(rng, n, c, 9)
    return Design(n, s, c, *_from_mask(r <= kth[:, None], rng), R.labels_matrix(ids, c), ids)


def four_groups(seed=702):
    """About 40 latents on each of 5 000 rows: parts of 256 entries.  Latent 0 on every row that stores anything (ten chunks), latent 1
    on every second row, latent 2 nowhere; rows 3, 20, 37, ..., the first and the last row store nothing."""
    rng = np.random.default_rng(seed)
    n, s, c = 5000, 1031, 33
    mask = rng.random((n, s)) < (rng.integers(38, 47, size=n) / (s - 3))[:, None]
    mask[:, 0] = True
    mask[:, 1] = np.arange(n) % 2 == 0
    mask[:, 2] = False
    mask[np.arange(3, n, 17)] = False
    mask[[0, n - 1]] = False
    ids = _ids(rng, n, c, 31)
    return Design(n, s, c, *_from_mask(mask, rng), R.labels_matrix(ids, c), ids)


def four_groups_other():
    """Another design with four_groups' four sizes (N, S, C, nnz): its rows and latents in reverse order, other values, other labels."""
    d = four_groups()
    rng = np.random.default_rng(703)
    per = np.diff(d.indptr)[::-1]
    indptr = np.concatenate([[0], np.cumsum(per)]).astype(np.int64)
    indices = (d.s - 1 - d.indices[::-1]).astype(np.int32)
    data = (rng.standard_normal(d.nnz) * 0.7).astype(np.float32)
    ids = _ids(rng, d.n, d.c, 5)
    return Design(d.n, d.s, d.c, indptr, indices, data, R.labels_matrix(ids, d.c), ids)


def many_latents():
    """33 or 34 latents a row, drawn from 30 000 of the 131 072: the (parts x S) counters cap the parts at 512, most latents and the last
    one are empty, and the scan over the latents carries 128 times."""
    rng = np.random.default_rng(704)
    n, s = 3000, 131072
    pool = np.sort(rng.choice(s - 1, size=30000, replace=False))
    draw = np.sort(rng.integers(0, pool.size, size=(n, 34)), axis=1)
    keep = np.concatenate([np.ones((n, 1), dtype=bool), np.diff(draw, axis=1) != 0], axis=1)  # (a repeated draw is dropped)
    indptr = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int64)
    indices = pool[draw[keep]].astype(np.int32)
    data = (rng.standard_normal(indices.size) * 1.5).astype(np.float32)
    return Design(n, s, 1, indptr, indices, data, rng.random((n, 1)) < 0.4)


def one_latent_rows():
    """Every one of 70 000 rows stores latent 3 of 5 and nothing else: every group of 64 holds one latent (same = 64, rank = lane)."""
    rng = np.random.default_rng(705)
    n, s = 70000, 5
    data = (rng.standard_normal(n) * 1.5).astype(np.float32)
    return Design(n, s, 1, np.arange(n + 1, dtype=np.int64), np.full(n, 3, dtype=np.int32), data, rng.random((n, 1)) < 0.4)


def long_rows():
    """Every one of 40 rows stores all 2 048 latents: a row spans 32 groups of 64 and crosses parts; a group holds one row id 64 times."""
    rng = np.random.default_rng(706)
    n, s, c = 40, 2048, 3
    data = (rng.standard_normal(n * s) * 1.5).astype(np.float32)
    ids = _ids(rng, n, c, 1)
    return Design(n, s, c, np.arange(n + 1, dtype=np.int64) * s, np.tile(np.arange(s, dtype=np.int32), n), data, R.labels_matrix(ids, c), ids)


# name -> (design, groups of 64 per part, parts, whether the last used part is ragged)
PLACEMENT = {"two_groups": (two_groups, 2, 1024, True), "four_groups": (four_groups, 4, 1024, True), "many_latents": (many_latents, 4, 512, None),
             "one_latent_rows": (one_latent_rows, 2, 1024, None), "long_rows": (long_rows, 2, 1024, None)}
ROW_PTR_SHIFT = 777


# ---- B: labels ------------------------------------------------------------------------------------------------------------------------------

LABEL_CLASSES = (257, 1000, 4096)
LABEL_COUNTS = (0, 1, CHUNK - 1, CHUNK, CHUNK + 1, 300, 200, 64)  # entries per latent: a small nnz keeps the numpy side of C = 4 096 small
ALONE_CLASSES = (0, 63, 64, 255, 256, 4095)


def label_design(c):
    """5 000 rows, 8 latents, class ids in [0, c): classes 0 and c - 1 occur, class c - 3 does not, and the classes at the edges of the
    64-lane groups and of the 256 a uint8 can name (ALONE_CLASSES) have a few dozen rows each."""
    rng = np.random.default_rng(800 + c)
    n, s = 5000, len(LABEL_COUNTS)
    mask = np.zeros((n, s), dtype=bool)
    for j, k in enumerate(LABEL_COUNTS):
        mask[rng.choice(n, size=k, replace=False), j] = True
    ids = rng.integers(0, c, size=n)
    edge = np.array([k for k in ALONE_CLASSES if k < c] + [c - 1])
    ids[:240] = np.tile(edge, 240 // edge.size + 1)[:240]
    ids[ids == c - 3] = 0
    ids = rng.permutation(ids)
    return Design(n, s, c, *_from_mask(mask, rng), R.labels_matrix(ids, c), ids.astype(np.int64))


# ---- C: the fit, slab by slab ---------------------------------------------------------------------------------------------------------------

# (C, slab) -> seed.  Every layout of the events kernel (C <= 8, 16, 32, one group, several) and slabs that end inside a
# 32-bit label word or a 64-class group ((16, 5), (70, 24), (130, 64)'s last) or on them
FIT_PAIRS = {(5, 2): 900, (8, 8): 901, (16, 5): 902, (32, 32): 903, (33, 8): 904, (70, 32): 905, (151, 8): 906, (130, 64): 907, (70, 24): 908}
# ridge 1 outweighs every pair's own curvature (at most 0.25), and the damping starts at 2 000 and falls tenfold per accepted step: every
# pair's gradient shrinks by nearly the same factor lam / (1 + h + lam) per iteration -- almost nothing at first, then 1.5, 2.5 and 3.5
# decades -- so the slabs' largest gradients keep their distances and pass tol in big steps, 10 x clear of it on both sides.  tol
# stays 10 x above 1e-8, the gradient of a class without rows (its probability is clamped there)
FIT_ROWS, FIT_MEAN = 120, 0.8
FIT_HYPER = dict(ridge=1.0, tol=2e-7, lam_init=2e3, max_iter=8)
FIT_N, FIT_S = 600, 24
POLLED = ((33, 8), (151, 8))


def slabs_of(c, slab):
    return [(c0, min(c0 + slab, c)) for c0 in range(0, c, slab)]


def fit_kinds(c, slab):
    """The kind of every class.  absent: no row has it (its slab stops at iteration 1); weak: exactly one row has it (a small first
    gradient); strong: x_1 > 0 where latent 1 fires on every row (the largest first gradient a class can have, 4 decades above
    a weak one's).  Under FIT_HYPER a slab of weak classes passes tol at iteration 8 and one that holds a strong class would at 9.  Slab 1 is absent, in C = 151 also slabs 8 .. 15 (the whole second 64-class group); the last slab holds a
    strong class; a single slab is all weak (C = 32: it stops) or holds a strong class (C = 8: it does not)."""
    slabs = slabs_of(c, slab)
    kinds = ["weak"] * c
    if len(slabs) == 1:
        if c == 8:
            kinds[3] = "strong"
        return tuple(kinds)
    absent = [1] + (list(range(8, 16)) if (c, slab) == (151, 8) else [])
    for i in absent:
        for k in range(*slabs[i]):
            kinds[k] = "absent"
    kinds[slabs[-1][0]] = "strong"
    return tuple(kinds)


def _moments(z, mean, std):
    """z shifted and scaled to the given mean and standard deviation (float32)."""
    return ((z - z.mean()) / z.std() * std + mean).astype(np.float32)


def fit_design(c, slab):
    """600 rows x 24 latents with signed values: latent 0 without entries, latent 1 on every row (two chunks), the others on 120 rows
    each; the labels are an N x C 0/1 matrix after fit_kinds.  Made so that all pairs of the weak classes start from the same scaled
    gradient pi sum(v) / (n qx): the row of a weak class is stored by latent 1 alone, as an explicit 0.0, and every latent's values
    have the same sum and the same qx.  With FIT_HYPER their gradients then fall
    together, and no pair is left behind just under tol when the others pass it."""
    rng = np.random.default_rng(FIT_PAIRS[c, slab])
    n, s = FIT_N, FIT_S
    kinds = fit_kinds(c, slab)
    perm = rng.permutation(n)
    ones, free = perm[:c], perm[c:]  # class k, if weak, has row ones[k]
    dense = np.zeros((n, s))
    mask = np.zeros((n, s), dtype=bool)
    for j in range(2, s):
        rows = rng.choice(free, size=FIT_ROWS, replace=False)
        mask[rows, j] = True
        dense[rows, j] = _moments(rng.standard_normal(FIT_ROWS), FIT_MEAN, 1.5)
    mask[:, 1] = True
    # latent 1 (n rows, m of them non-zero): the same sum(v) and the same qx^2 = sum(v^2) / n as the others have with sum(v^2) / FIT_ROWS
    m, qx_sq = free.size, 1.5 ** 2 + FIT_MEAN ** 2
    mu = FIT_ROWS * FIT_MEAN / m
    dense[free, 1] = _moments(rng.standard_normal(m), mu, np.sqrt(qx_sq * n / m - mu ** 2))
    indptr = np.concatenate([[0], np.cumsum(mask.sum(axis=1))]).astype(np.int64)
    rows, cols = np.nonzero(mask)
    data = dense[rows, cols].astype(np.float32)
    ymat = np.zeros((n, c), dtype=bool)
    for k, kind in enumerate(kinds):
        if kind == "weak":
            ymat[ones[k], k] = True
        elif kind == "strong":
            ymat[:, k] = dense[:, 1] > 0
    return Design(n, s, c, indptr, cols.astype(np.int32), data, ymat, None, kinds)


def fit_hyper(c, slab, cls=R.Hyper):
    return cls(class_slab_size=slab, **FIT_HYPER)


def fit_trace(d, hp):
    """R.fit, keeping what it decides on: (b, w, n_iter per class, gmax (max_iter, slabs): every running slab's largest scaled
    gradient at each iteration, NaN once it has stopped; done per slab)."""
    starts, rows, vals, qx = R.prepare(*d.csr, d.s)
    n, pos, counts = d.n, d.ymat.sum(axis=0), np.diff(starts)
    state = R.init_state(d.s, pos, n, hp)
    slabs = slabs_of(d.c, hp.class_slab_size)
    running = np.ones(len(slabs), dtype=bool)
    n_iter = np.zeros(d.c, dtype=np.int32)
    gmax = np.full((hp.max_iter, len(slabs)), np.nan)
    for it in range(hp.max_iter):
        if not running.any():
            break
        sums, _ = R.event_sums(starts, rows, vals, d.ymat, state["b"], state["w"])
        new, info = R.update(sums, state, counts, qx, pos, n, hp)
        for i, (c0, c1) in enumerate(slabs):
            if not running[i]:
                continue
            for k in state:
                state[k][:, c0:c1] = new[k][:, c0:c1]
            n_iter[c0:c1] += 1
            gmax[it, i] = info["grad"][:, c0:c1].max()
            running[i] = not gmax[it, i] <= hp.tol
    return state["b"], state["w"], n_iter, gmax, ~running


# ---- D: evaluate ----------------------------------------------------------------------------------------------------------------------------

THRESHOLDS = (0.2, 0.5, 0.9)
EVAL_SEED = 300  # coefficients(s, c, EVAL_SEED + i) for CASES[i], EVAL_SEED - 1 for four_groups


def threshold_gap(d, b, w, thresholds=THRESHOLDS):
    """The smallest |mu - threshold| over all events, zero rows, pairs and thresholds at (b, w)."""
    starts, _, vals, _ = R.prepare(*d.csr, d.s)
    with np.errstate(over="ignore", under="ignore"):
        z, _ = R._event_logits(starts, vals, b, w)
        mu, mu0 = R._sigma(z), R._sigma(b)
    return min(min(float(np.abs(m - t).min()) for m in (mu, mu0) if m.size) for t in thresholds)
