"""The designs the probe AP tests run (include/saev_amd.h: PROBE AP): the CSR and classes of tests/latent_ap_cases.py or small ones made
here, plus ``w`` and ``b`` (S x C float64 holding float32-representable numbers, so that one design serves both score dtypes), each
at the smallest size where that piece of the kernel can go wrong.  Every builder returns the dict of latent_ap_cases with w and b
added; everything is seeded."""

import numpy as np

import latent_ap_cases as K

DIRECT_MAX = K.DIRECT_MAX


def _f32(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def _mixed(rng, s, c):
    """Weights of both signs inside every 64-lane group, biases of both signs."""
    w = _f32(rng.uniform(0.25, 3.0, size=(s, c)) * rng.choice([1.0, -1.0], size=(s, c)))
    b = _f32(rng.uniform(-2.0, 1.0, size=(s, c)))
    return w, b


def kinds(seed=31):
    """latent_ap_cases.kinds (257, 48, 11: a latent without events, latents with an event in every row, signed ones, stored zeros;
    class 10 never occurs, a tenth of the rows has no class) with one kind of weight per column:
    0: w > 0   1: w < 0   2: +0.0   3: -0.0   4: 1e-30 with b = 1 (every score collapses to b)   5: 3e38 (events above 1.14 tie at
    +Inf, those below -1.14 at -Inf)   6: w = 1e-3, b = 1e6 (fp32: spacing 1/16, everything collapses; fp64: nothing does)
    7: b = 0, w of either sign   8: w = -0.05, b = 1e6 (fp32: scores in steps of 1/16 -- ties among events, and |a| < 0.625 merges
    with the zero block)   9: mixed   10: mixed, pos_c = 0."""
    d = K.kinds()
    rng = np.random.default_rng(seed)
    w, b = _mixed(rng, d["s"], d["c"])
    w[:, 0], w[:, 1] = np.abs(w[:, 0]), -np.abs(w[:, 1])
    w[:, 2], w[:, 3] = 0.0, -0.0
    w[:, 4], b[:, 4] = _f32(1e-30), 1.0
    w[:, 5] = _f32(3e38)
    w[:, 6], b[:, 6] = _f32(1e-3), 1e6
    b[:, 7] = 0.0
    w[:, 8], b[:, 8] = _f32(-0.05), 1e6
    return dict(d, w=w, b=b)


def middle(n=40):
    """Negative stored values under both signs of w: the zero block sits in the middle of the walk.  b = 1 and |w| = 2^-10; values
    of +-2^-60 have |w a| = 2^-70 below half an ulp of b in both dtypes, values of 1 and 2 do not.  Latent 0: tiny values of both
    signs (the block merges on both sides), 1: tiny positive and large negative (one side), 2: tiny negative and large positive
    (the other side), 3: large values only (neither).  Columns: w > 0, w < 0, and the same with b = 0 (nothing merges)."""
    rng = np.random.default_rng(32)
    tiny = 2.0 ** -60
    cls = rng.integers(0, 2, size=n).astype(np.int32)
    cls[rng.random(n) < 0.15] = -1
    dense = np.zeros((n, 4), dtype=np.float32)
    pools = [[tiny, 2 * tiny, -tiny, -3 * tiny, 1.0, -2.0], [tiny, 2 * tiny, -1.0, -2.0, 1.5], [-tiny, -2 * tiny, 1.0, 2.0, -1.5], [1.0, 2.0, -1.0, -2.0]]
    for j, pool in enumerate(pools):
        rows = rng.choice(n, size=24, replace=False)
        dense[rows, j] = rng.choice(pool, size=24)
    w = np.tile(np.array([2.0 ** -10, -(2.0 ** -10), 2.0 ** -10, -(2.0 ** -10)]), (4, 1))
    b = np.tile(np.array([1.0, 1.0, 0.0, 0.0]), (4, 1))
    cls4 = np.where(cls >= 0, cls * 2 + rng.integers(0, 2, size=n), -1).astype(np.int32)  # four classes: every column has rows
    return dict(K._pack(dense, dense != 0, cls4, 4), w=w, b=b)


def wide70(seed=33):
    """(257, 3, 70): two class blocks, both signs of w inside one wave."""
    d = K.wide(257, 3, 70, 23)
    w, b = _mixed(np.random.default_rng(seed), d["s"], d["c"])
    return dict(d, w=w, b=b)


def chunks(n=200, seed=34):
    """Latents of 63, 64, 65 and 129 events, walked ascending (columns 0 and 2, w < 0) and descending (column 1): the chunk borders
    of the reverse walk, a last chunk that is not full.  Values distinct, a third of them negative; column 2 has b = 0."""
    rng = np.random.default_rng(seed)
    cls = K._labels(rng, n, 3)
    dense = np.zeros((n, 4), dtype=np.float32)
    for j, m in enumerate((63, 64, 65, 129)):
        rows = rng.choice(n, size=m, replace=False)
        dense[rows, j] = (0.5 + 0.25 * rng.permutation(m)) * rng.choice([1.0, 1.0, -1.0], size=m)
    w = np.tile(np.array([-1.5, 0.75, -0.5]), (4, 1))
    b = np.tile(np.array([0.25, -1.0, 0.0]), (4, 1))
    return dict(K._pack(dense, dense != 0, cls, 3), w=w, b=b)


def created(n=120, seed=35):
    """Tie groups that exist in the score only: groups of DIRECT_MAX - 1, DIRECT_MAX and DIRECT_MAX + 1 events whose values are
    consecutive float32 numbers above an integer in [32, 64) (spacing 2^-18), first at ranks 0..23, then, behind 20 single events,
    at ranks 44..67.  Column 0: w = 1, b = 1024 (fp32 scores have spacing 2^-13: each group collapses; fp64 keeps them apart);
    column 1: w = 1, b = 2^40 (fp64 spacing 2^-12: each group collapses; fp32 collapses everything); columns 2 and 3: the same with
    w = -1, the groups met in the opposite order behind the zero block."""
    rng = np.random.default_rng(seed)
    cls = K._labels(rng, n, 4, none=0.05)
    sizes = (DIRECT_MAX - 1, DIRECT_MAX, DIRECT_MAX + 1)
    vals, k = [], 63
    for part in range(2):
        for size in sizes:
            v = np.float32(k)
            for _ in range(size):
                vals.append(v)
                v = np.nextafter(v, np.float32(np.inf))
            k -= 1
        if part == 0:
            vals += [np.float32(k - i) for i in range(20)]
            k -= 20
    vals = np.asarray(vals, dtype=np.float32)
    assert len(np.unique(vals)) == len(vals) == 68 and vals.min() >= 32
    dense = np.zeros((n, 2), dtype=np.float32)
    dense[rng.choice(n, size=len(vals), replace=False), 0] = vals
    dense[rng.choice(n, size=len(vals), replace=False), 1] = -vals  # negative events: the zero block comes first for w > 0
    w = np.tile(np.array([1.0, 1.0, -1.0, -1.0]), (2, 1))
    b = np.tile(np.array([1024.0, 2.0 ** 40, 1024.0, 2.0 ** 40]), (2, 1))
    return dict(K._pack(dense, dense != 0, cls, 4), w=w, b=b)


def silent(n=64, seed=36):
    """Latents that are silent on rows of the class they are scored for: the zero block holds positive rows, so the AP depends on
    how its ties are counted."""
    rng = np.random.default_rng(seed)
    cls = K._labels(rng, n, 3, none=0.0)
    dense = np.zeros((n, 3), dtype=np.float32)
    for j in range(3):
        rows = np.flatnonzero((cls == j) & (rng.random(n) < 0.5))
        dense[rows, j] = 0.5 + 0.125 * rng.permutation(len(rows))
    w, b = _mixed(rng, 3, 3)
    return dict(K._pack(dense, dense != 0, cls, 3), w=w, b=b)


def deep(seed=37):
    """latent_ap_cases.deep (70 000, 3, 5): ranks past 2^16, under weights of both signs."""
    d = K.deep()
    w, b = _mixed(np.random.default_rng(seed), d["s"], d["c"])
    return dict(d, w=w, b=b)


def tiny(seed):
    """At most 7 rows, 2 latents, 2 classes, quantised values and weights: small enough to enumerate every order of the tied rows."""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(2, 8))
    cls = rng.integers(-1, 2, size=n).astype(np.int32)
    dense = (rng.integers(-2, 4, size=(n, 2)) * (rng.random((n, 2)) < 0.7)).astype(np.float32)
    w = rng.choice([1.0, -1.0, 0.0, 0.5, -2.0 ** -30], size=(2, 2))
    b = rng.choice([0.0, 1.0, -1.0, 2.0 ** 24], size=(2, 2))
    return dict(K._pack(dense, dense != 0, cls, 2), w=w, b=b)


SMALL = {"kinds": kinds, "middle": middle, "wide70": wide70, "chunks": chunks, "created": created, "silent": silent}
LARGE = {"deep": deep}


def g28_run(tmp_path, g, *, leave_out=()):
    """The run directory of fixture G28 (tools/gen_golden_probe_metrics.py) rebuilt under ``tmp_path``: (run_dir, train_shards,
    test_shards).  ``leave_out`` names files not to write: "train_acts", "test_acts", "probe", "labels"."""
    import scipy.sparse

    from saev_amd import disk
    from saev_amd.data import write_shards

    rng = np.random.default_rng(1)
    n_ex, tokens, s, c = int(g["n_examples"]), int(g["tokens_per_example"]), int(g["n_latents"]), int(g["n_classes"])
    test_shards = write_shards(tmp_path, rng.standard_normal((n_ex, 1, tokens, 4)).astype(np.float32), labels=g["labels"].reshape(n_ex, tokens))
    train_ex = int(g["train_examples"])
    train_shards = write_shards(tmp_path, rng.standard_normal((train_ex, 1, tokens, 4)).astype(np.float32),
                                labels=rng.integers(0, c, size=(train_ex, tokens)).astype(np.uint8))
    run = disk.Run.new("g28probe", train_shards_dir=train_shards, val_shards_dir=test_shards, runs_root=tmp_path / "saev" / "runs")
    csr = scipy.sparse.csr_matrix((g["data"], g["indices"], g["indptr"]), shape=(n_ex * tokens, s))
    train = scipy.sparse.random(train_ex * tokens, s, density=0.2, format="csr", dtype=np.float32, random_state=2)
    for shards, acts, name in ((train_shards, train, "train_acts"), (test_shards, csr, "test_acts")):
        (run.inference / shards.name).mkdir()
        if name not in leave_out:
            scipy.sparse.save_npz(run.inference / shards.name / "token_acts.npz", acts)
    if "probe" not in leave_out:
        np.savez(run.inference / train_shards.name / "probe1d_metrics.npz", loss=g["loss"], weights=g["weights"], biases=g["biases"])
    if "labels" in leave_out:
        (test_shards / "labels.bin").unlink()
    return run.run_dir, train_shards, test_shards
