"""CSR blocks at the edges of the pieces the analysis entries share: the row search (empty rows at the start, at the end and in a run
of three in the middle, cut out of a longer CSR so that indptr[0] != 0) and the rounds of the single-workgroup scan.  Expected
values come from numpy alone."""

import numpy as np


def empty_rows_block(shift: int, n: int = 203, s: int = 50, seed: int = 5) -> dict:
    """A block of n rows over s latents whose rows 0-1, 57, 100-102 and n-2, n-1 are empty, one to eight distinct latents in every other
    row, positive values.  ``indptr`` holds absolute positions: the block starts at ``shift`` in ``indices`` / ``data``, and the
    entries in front of it (a latent out of range, a NaN) must never be looked at.  ``rows`` / ``cols`` / ``vals`` are the block's
    entries in storage order, ``rows`` being np.repeat of the row ids."""
    rng = np.random.default_rng(seed)
    counts = rng.integers(1, 9, n)
    counts[[0, 1, 57, 100, 101, 102, n - 2, n - 1]] = 0
    cols = np.concatenate([np.sort(rng.choice(s, c, replace=False)) for c in counts]).astype(np.int32)
    vals = (0.5 + rng.random(cols.size)).astype(np.float32)
    vals[::7] = 1.0  # ties inside a latent: the row decides
    rows = np.repeat(np.arange(n), counts)
    indptr = (shift + np.concatenate([[0], np.cumsum(counts)])).astype(np.int64)
    assert indptr[0] == indptr[2] and indptr[100] == indptr[103] and indptr[n - 2] == indptr[n] and (np.bincount(cols, minlength=s) >= 2).all()
    return dict(n=n, s=s, nnz=int(cols.size), indptr=indptr, rows=rows, cols=cols, vals=vals,
                indices=np.concatenate([np.full(shift, s, dtype=np.int32), cols]),
                data=np.concatenate([np.full(shift, np.nan, dtype=np.float32), vals]))


def by_latent(d: dict, by_value: bool) -> np.ndarray:
    """The block's entries ordered by (latent, value descending, row ascending), or by (latent, row ascending): positions into
    ``rows`` / ``cols`` / ``vals``."""
    return np.lexsort((d["rows"], -d["vals"], d["cols"])) if by_value else np.lexsort((d["rows"], d["cols"]))


def scan_rounds_block(s: int, n: int = 600, seed: int = 9) -> dict:
    """n rows over s latents, five random latents in each plus the LAST latent in every row: more than one chunk of 512 for it, so
    both halves of the packed scan carry something into the last round."""
    rng = np.random.default_rng(seed + s)
    cols = np.stack([np.sort(np.append(rng.choice(s - 1, 5, replace=False), s - 1)) for _ in range(n)]).astype(np.int32).ravel()
    return dict(n=n, s=s, nnz=int(cols.size), indptr=(6 * np.arange(n + 1)).astype(np.int64), indices=cols,
                data=(0.5 + rng.random(cols.size)).astype(np.float32))
