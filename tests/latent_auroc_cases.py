"""The designs the latent AUROC tests run (include/saev_amd.h: LATENT AUROC), each at the smallest shape where that piece of the
kernels can go wrong.  Every builder returns a dict with the CSR (indptr int64, indices int32, data float32), the shape n, s, c,
``cls`` (n int32, -1 = no class) and ``roles`` (T x C uint8); everything is seeded."""

import numpy as np
import scipy.sparse

import latent_ap_cases as K

CHUNK_GROUPS = (63, 1, 64, 2, 65, 130, 1, 62, 2)  # tie groups of latent 0 of `chunks`: they end on, straddle and span the 64-event chunks


def _roles(rng, t, c, p_out=0.3):
    roles = rng.choice(np.array([0, 1, 2], dtype=np.uint8), size=(t, c), p=[p_out, (1 - p_out) / 2, (1 - p_out) / 2])
    return np.ascontiguousarray(roles)


def kinds():
    """latent_ap_cases.kinds (257 x 48 x 11: latents with no events, one event, positive only, negative only in every row, both
    signs, every row distinct, every row one value, stored +-0.0, rows of class -1, a class that never occurs) with +-Inf added, and
    seven tasks: plain pairs, a class left out of one task and positive in another, overlapping tasks, a task without positives
    (its only positive class never occurs), one without negatives, one-vs-rest, and an empty one."""
    d = K.kinds()
    data = d["data"].copy()
    at = np.flatnonzero(d["indices"] == 6)
    data[at[0]], data[at[1]], data[at[2]] = np.inf, np.inf, -np.inf  # a tie at +Inf; the sums become NaN where both signs meet
    at = np.flatnonzero(d["indices"] == 10)
    data[at[0]] = -np.inf
    c = d["c"]
    roles = np.zeros((7, c), dtype=np.uint8)
    roles[0, 0], roles[0, 1] = 2, 1
    roles[1, 1], roles[1, 2] = 2, 1                # class 0 is left out here and positive in task 0; class 1 changes sides
    roles[2, :5], roles[2, 5:] = 2, 1              # overlaps both
    roles[3, c - 1], roles[3, :3] = 2, 1           # no positives: class c - 1 never occurs
    roles[4, 3] = 2                                # no negatives
    roles[5, :], roles[5, 4] = 1, 2                # one-vs-rest
    return dict(d, data=data, roles=roles)


def chunks(seed=11):
    """S = 5, C = 3, T = 3.  Latent 0: tie groups of CHUNK_GROUPS events, positive then negative values; latent 1: one group of 130
    events and silent rows; latent 2: every row one value (one group covers the latent, no silent rows); latent 3: nothing; latent 4: a
    group of 130 negative events, then single ones."""
    rng = np.random.default_rng(seed)
    n = sum(CHUNK_GROUPS) + 37
    dense = np.zeros((n, 5), dtype=np.float32)
    stored = np.zeros((n, 5), dtype=bool)
    order = rng.permutation(n)
    at, level = 0, 3.0
    for g, size in enumerate(CHUNK_GROUPS):
        rows = order[at:at + size]
        dense[rows, 0], stored[rows, 0] = (level if g < 5 else -level), True
        at, level = at + size, (level - 0.25 if g < 5 else level + 0.25)
    rows = rng.permutation(n)[:130]
    dense[rows, 1], stored[rows, 1] = 0.75, True
    dense[:, 2], stored[:, 2] = 1.25, True
    rows = rng.permutation(n)[:140]
    dense[rows[:130], 4], dense[rows[130:], 4], stored[rows, 4] = -0.5, -np.arange(1, 11, dtype=np.float32), True
    cls = K._labels(rng, n, 3)
    roles = np.array([[2, 1, 0], [1, 2, 2], [0, 1, 2]], dtype=np.uint8)
    return dict(K._pack(dense, stored, cls, 3), roles=roles)


def grid(n, s, c, t, seed):
    """A random design of the given shape: values in quarters (ties abound), every other latent signed, one latent of the five stored
    in every row, stored +-0.0, rows of class -1, random roles."""
    rng = np.random.default_rng(seed)
    dense = (rng.integers(1, 9, size=(n, s)) / 4).astype(np.float32)
    dense[:, 1::2] *= rng.choice(np.array([-1.0, 1.0], dtype=np.float32), size=dense[:, 1::2].shape)
    stored = rng.random((n, s)) < 0.4
    if s > 2:
        stored[:, 2] = True
    zero = stored & (rng.random((n, s)) < 0.05)
    dense[zero] = rng.choice(np.array([0.0, -0.0], dtype=np.float32), size=int(zero.sum()))
    dense = np.where(stored, dense, 0).astype(np.float32)
    cls = K._labels(rng, n, c, present=np.arange(c) if c <= n // 2 else rng.choice(c, size=n // 2, replace=False))
    return dict(K._pack(dense, stored, cls, c), roles=_roles(rng, t, c))


# (n, s, c, t): T in {1, 64, 65, 130}, C in {1, 300, 4096} and both sides of the LDS / L2 choice of the role table, S in {1, 5}
GRID = {"1x1x1": (40, 1, 1, 1), "5x300x64": (300, 5, 300, 64), "5x300x65": (300, 5, 300, 65), "1x4096x130": (600, 1, 4096, 130),
        "5x4096x1": (600, 5, 4096, 1), "5x255x65": (300, 5, 255, 65), "5x256x64": (300, 5, 256, 64), "5x11x130": (200, 5, 11, 130)}

SMALL = {"kinds": kinds, "chunks": chunks, **{f"grid_{k}": (lambda k=k, i=i: grid(*GRID[k], seed=100 + i)) for i, k in enumerate(GRID)}}


def wide_counts(n=140_000, seed=12):
    """u2 past 2^32 at the least cost: 140 000 rows in two classes of 70 000 (n_pos n_neg = 4.9e9), two tasks with the roles swapped,
    latent 0 with 500 signed events in quarters, latent 1 with none (u2 = n_pos n_neg, the closed form alone)."""
    rng = np.random.default_rng(seed)
    cls = (np.arange(n) % 2).astype(np.int32)
    rows = np.sort(rng.choice(n, size=500, replace=False))
    vals = (rng.integers(1, 9, size=500) / 4 * rng.choice([-1.0, 1.0], size=500)).astype(np.float32)
    indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int64)
    return dict(indptr=indptr, indices=np.zeros(500, dtype=np.int32), data=vals, n=n, s=2, c=2, cls=cls, roles=np.array([[1, 2], [2, 1]], dtype=np.uint8))


def as_bytes(d):
    """The design with its classes as uint8 labels and a remap with -1 entries: byte = 2 * class + 3, byte 1 for the rows of class -1
    (remap[1] = -1, like every byte no class uses).  Classes up to 126."""
    assert d["c"] <= 126
    remap = np.full(256, -1, dtype=np.int32)
    remap[2 * np.arange(d["c"]) + 3] = np.arange(d["c"], dtype=np.int32)
    labels = np.where(d["cls"] >= 0, 2 * d["cls"] + 3, 1).astype(np.uint8)
    return labels, remap


def one_latent(d, j):
    """The design cut down to latent j (S = 1)."""
    assert d["indptr"][0] == 0
    keep = d["indices"] == j
    rows = np.repeat(np.arange(d["n"]), np.diff(d["indptr"]))[keep]
    indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=d["n"]))]).astype(np.int64)
    return dict(d, indptr=indptr, indices=np.zeros(int(keep.sum()), dtype=np.int32), data=d["data"][keep], s=1)


PAST_CAP_ROLES = np.array([[2, 1, 1, 1, 1], [1, 2, 0, 2, 0], [0, 0, 1, 1, 2]], dtype=np.uint8)  # over the 5 classes of analysis_scale_cases.past_cap


# ---------------------------------------------------------------- fixture G29 -------------------------------------------------------------

def g29_designs(g):
    """The designs of tests/golden/g29_latent_auroc.npz as dicts."""
    out = []
    for i in range(int(g["n_designs"])):
        d = {k[len(f"d{i}_"):]: g[k] for k in g if k.startswith(f"d{i}_")}
        d["sv"] = d["labels"].tolist()
        d["pair_specs"] = [tuple(p) for p in d["pair_specs"].tolist()]
        d["views"] = d["views"].tolist()
        n_images, tpi, s, min_samples, feature_chunk = (int(x) for x in d["shape"])
        d.update(n_images=n_images, tpi=tpi, s=s, min_samples=min_samples, feature_chunk=feature_chunk)
        out.append(d)
    return out


def g29_run(tmp_path, d, run_id="mimic001"):
    """(run_root, shards directory) of a small run written from a design of G29: shards with ``image_labels.csv`` and
    ``<run_root>/<run_id>/inference/<shards>/token_acts.npz``."""
    from saev_amd.data import write_shards

    shards = write_shards(tmp_path / "shards", np.zeros((d["n_images"], 1, d["tpi"], 4), dtype=np.float32))
    with open(shards / "image_labels.csv", "w") as fd:
        fd.write("stem,subspecies_view\n" + "".join(f"img{i},{lbl}\n" for i, lbl in enumerate(d["sv"])))
    inference = tmp_path / "runs" / run_id / "inference" / shards.name
    inference.mkdir(parents=True)
    csr = scipy.sparse.csr_matrix((d["data"], d["indices"], d["indptr"]), shape=(d["n_images"] * d["tpi"], d["s"]))
    scipy.sparse.save_npz(inference / "token_acts.npz", csr)
    return tmp_path / "runs", shards
