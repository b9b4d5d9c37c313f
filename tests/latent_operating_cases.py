"""The designs the latent operating-point tests run (include/saev_amd.h: LATENT OPERATING POINTS), each at the smallest shape where
that piece of the kernel can go wrong.  The dict of a design is that of tests/latent_auroc_cases.py (CSR, n, s, c, ``cls``, ``roles``),
and its small designs are run as they are: latents without events, with positive events only, negative only and both, +-Inf, stored
+-0.0, rows of class -1, void tasks, tie groups of 1, 2, 63, 64, 65 and 130 events on and across the 64-event chunks (the last of
them closing on the latent's last event), T in {1, 64, 65, 130} and C on both sides of the LDS / L2 choice of the role table.  What
is added here is what only this entry can get wrong; tests/test_latent_operating_host_cpu.py asserts what each design plants."""

import numpy as np

import latent_auroc_cases as AK

F32 = np.float32


def from_columns(n, columns, cls, c, roles):
    """A design from one {row: value} dict per latent (every entry stored, in ascending column order within a row)."""
    rows, cols, vals = [], [], []
    for j, col in enumerate(columns):
        for r, v in col.items():
            rows.append(r), cols.append(j), vals.append(v)
    order = np.lexsort((cols, rows))
    rows, cols, vals = np.asarray(rows, dtype=np.int64)[order], np.asarray(cols, dtype=np.int32)[order], np.asarray(vals, dtype=F32)[order]
    indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int64)
    return dict(indptr=indptr, indices=cols, data=vals, n=n, s=len(columns), c=c, cls=np.asarray(cls, dtype=np.int32),
                roles=np.ascontiguousarray(roles, dtype=np.uint8))


def single():
    """N = 1, three latents (an event above 0, an event below 0, none), tasks with the row as positive, as negative and left out."""
    return from_columns(1, [{0: 2.0}, {0: -2.0}, {}], [0], 1, [[2], [1], [0]])


# rows 0, 1 positive and 2, 3 negative in task 0 (n_pos = n_neg = 2); row 4 has no class and row 5 a class that task 0 leaves out:
# both sit INSIDE the tie groups.  Task 1 swaps the sides and takes class 2 in as a positive; task 2 is task 0 again
PLANTED = {
    # F1 ties decided by cross-multiplication: (TP 1, FP 0) -> 2 / 3 against (TP 2, FP 2) -> 4 / 6; the higher threshold wins
    "f1_down": ({0: 3.0, 1: 2.0, 2: 2.0, 3: 2.0, 4: 2.0, 5: 2.0}, "f1", (1, 0, 3.0)),
    "f1_up": ({0: -1.0, 1: -2.0, 2: -2.0, 3: -2.0, 4: -2.0, 5: -1.0}, "f1", (1, 0, -1.0)),
    "f1_across": ({0: 1.0, 1: -1.0, 2: -1.0, 3: -1.0, 4: 1.0, 5: -1.0}, "f1", (1, 0, 1.0)),
    "f1_event_against_zero_block": ({0: 1.0, 5: 1.0}, "f1", (1, 0, 1.0)),
    "f1_zero_block_against_event": ({1: -1.0, 2: -1.0, 3: -1.0, 4: -1.0}, "f1", (1, 0, 0.0)),
    # J2 ties with n_pos = n_neg: (TP 1, FP 0) -> 2 against (TP 2, FP 1) -> 2
    "j_down": ({0: 3.0, 1: 2.0, 2: 2.0, 3: 1.0, 4: 2.0, 5: 3.0}, "j", (1, 0, 3.0)),
    "j_up": ({0: -1.0, 1: -2.0, 2: -2.0, 3: -3.0, 4: -2.0, 5: -3.0}, "j", (1, 0, -1.0)),
    "j_across": ({0: 1.0, 1: -1.0, 2: -1.0, 3: -2.0, 4: -1.0}, "j", (1, 0, 1.0)),
    "j_event_against_zero_block": ({0: 1.0, 3: -1.0, 5: -1.0}, "j", (1, 0, 1.0)),
    "j_zero_block_against_event": ({1: -1.0, 2: -1.0, 3: -2.0}, "j", (1, 0, 0.0)),
    # the lower candidate is strictly better: it must win (TP 2, FP 0 after TP 1, FP 0)
    "lower_wins": ({0: 3.0, 1: 2.0, 2: 1.0, 3: 1.0}, "both", (2, 0, 2.0)),
}


def planted():
    cls = [0, 0, 1, 1, -1, 2]
    roles = [[2, 1, 0], [1, 2, 2], [2, 1, 0]]
    return from_columns(6, [col for col, _, _ in PLANTED.values()], cls, 3, roles)


def marks_negatives():
    """Latent 0 fires on class 1 only (12 rows of 20, at three values, a stored 0.0 among them is no event); latent 1 has negative
    values on class 0 only -- which ranks class 1 above it.  Task 0 has class 0 as its positives, task 1 the roles swapped."""
    cls = [0] * 10 + [1] * 10
    col0 = {10 + i: (3.0, 2.0, 1.0)[i % 3] for i in range(9)}
    col0[19] = 0.0
    col1 = {i: -1.0 - (i % 2) for i in range(8)}
    return from_columns(20, [col0, col1], cls, 2, [[2, 1], [1, 2]])


def zero_block_lanes():
    """Four classes of 3 rows.  Latent 0 stores a signed value in every row of classes 0 and 1 and in none of classes 2 and 3: the zero
    block is empty for task 0 (classes 0 against 1), holds every row of task 1 (2 against 3) and the negatives only of task 2 (0
    against 2).  Latent 1 is the same with positive values only."""
    cls = np.repeat(np.arange(4), 3)
    col0 = {0: 2.0, 1: 1.0, 2: -1.0, 3: 1.0, 4: -1.0, 5: -2.0}
    col1 = {r: abs(v) for r, v in col0.items()}
    return from_columns(12, [col0, col1], cls, 4, [[2, 1, 0, 0], [0, 0, 2, 1], [2, 0, 1, 0]])


TINY, ONE = F32(1e-45), F32(1.0)
ABOVE_ONE = np.nextafter(ONE, F32(2.0))


def specials():
    """+Inf as an event value that wins; -Inf as the lowest group, where theta = -Inf predicts every row; denormals; values one ulp
    apart.  Classes: rows 0-3 class 0, rows 4-7 class 1.  Task 0: class 0 positive against class 1; task 1: class 0 alone (no
    negatives: the best F1 predicts everything)."""
    cls = [0] * 4 + [1] * 4
    inf = np.inf
    cols = [
        {0: inf, 1: inf, 4: 1.0},                                       # +Inf wins: (TP 2, FP 0)
        {0: 1.0, 1: 2.0, 2: 3.0, 3: -inf, 4: -inf, 5: -inf, 6: -inf, 7: -inf},  # every row an event, -Inf the lowest group
        {0: 2 * TINY, 1: TINY, 4: TINY, 5: -TINY, 2: -2 * TINY},        # denormals of both signs round the zero block
        {0: ABOVE_ONE, 1: ABOVE_ONE, 2: ONE, 4: ONE, 5: ONE, 6: ONE},   # one ulp apart: two groups
        {0: -inf, 4: inf},
    ]
    return from_columns(8, cols, cls, 2, [[2, 1], [2, 0]])


def many_latents(s=70_001, seed=5):
    """S = 70 001 (past one grid row of 65 535 blocks of four latents is not reached; past 2^16 latents is), 240 events on 60 rows:
    the first and the last latent have some."""
    rng = np.random.default_rng(seed)
    n = 60
    cols = [dict() for _ in range(s)]
    for j in np.concatenate([[0, s - 1, s - 1, 0, 65_536, 65_535], rng.integers(0, s, size=234)]):
        cols[int(j)][int(rng.integers(0, n))] = float(rng.integers(-2, 6)) / 2 or 0.5
    cls = AK.K._labels(rng, n, 4)
    return from_columns(n, cols, cls, 4, [[2, 1, 0, 0], [1, 1, 2, 0], [0, 2, 1, 1]])


def wide_products(n=150_000, seed=13):
    """Cross products past 2^32 and the serial walk over thousands of trips: 150 000 rows in two classes of 75 000, latent 0 firing
    on EVERY row at distinct values (k / 8: exact in fp32), latent 1 the same values signed (a third negative, so the count pass runs
    at this length too).  Class 1 lies three standard deviations above class 0, so the winners sit in the middle of the walk: TP and TP + FP + n_pos there
    multiply to over 2^32, and so does J2."""
    rng = np.random.default_rng(seed)
    cls = (np.arange(n) % 2).astype(np.int32)
    score = rng.normal(size=n) + 3.0 * cls
    rank = np.argsort(np.argsort(score))
    v0 = ((rank + 1) / 8).astype(F32)
    v1 = ((rank - n // 3 + (rank >= n // 3)) / 8).astype(F32)  # no zero among them
    indptr = (2 * np.arange(n + 1)).astype(np.int64)
    indices = np.tile(np.array([0, 1], dtype=np.int32), n)
    data = np.stack([v0, v1], axis=1).reshape(-1)
    return dict(indptr=indptr, indices=indices, data=data, n=n, s=2, c=2, cls=cls, roles=np.array([[1, 2], [2, 1]], dtype=np.uint8))


def big_group(n=70_050, seed=14):
    """Many rows on one value: 70 000 events in ONE tie group (more than 2^16, and over a thousand 64-event chunks without a close),
    20 single events above and 10 below it, 20 silent rows."""
    rng = np.random.default_rng(seed)
    cls = rng.integers(0, 3, size=n).astype(np.int32)
    rows = rng.permutation(n)
    col = {int(r): 1.0 for r in rows[:70_000]}
    col.update({int(r): 2.0 + i for i, r in enumerate(rows[70_000:70_020])})
    col.update({int(r): -1.0 - i for i, r in enumerate(rows[70_020:70_030])})
    return from_columns(n, [col], cls, 3, [[2, 1, 0], [1, 0, 2]])


OWN = {"single": single, "planted": planted, "marks_negatives": marks_negatives, "zero_block_lanes": zero_block_lanes, "specials": specials}
SMALL = {**AK.SMALL, **OWN}
LARGE = {"many_latents": many_latents, "wide_products": wide_products, "big_group": big_group}
