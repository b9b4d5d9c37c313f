"""The designs of the analysis entries' scale tests (tests/test_gpu_analysis_scale.py, tests/test_analysis_scale_host_cpu.py): inputs
past the grid caps of the grid-stride kernels, latent counts at the byte borders of the radix sort's latent key, and solver shapes
whose row chunks are longer than 64.  Every builder is a function of nothing but its arguments (seeded generators), so the host tests
check on the CPU, from the library's own layout functions, that the very arrays the GPU tests run reach what they are meant to reach.

The caps are not exported; they are restated here once:
  GRID_CAP_ENTRIES     8192 workgroups of 256: la_sort (la_init_kernel) and saev_probe_ap (pa_values_kernel, pa_top_rows_kernel) in
                       latentap.hip, saev_latent_topk_update (lt_count_kernel, lt_place_kernel) in latenttopk.hip,
                       saev_probe1d_prepare (p1_count_kernel) in probe1d.hip, saev_l1_logistic_init (sl_check_kernel) in sparselinear.hip
  SL_OUT_CAP_ENTRIES   4096 workgroups of 256: saev_l1_logistic_result (sl_out_kernel) in sparselinear.hip
An index at or above a cap is visited in a kernel's second trip round its loop."""

import numpy as np
import scipy.sparse

import latent_ap_cases as K
import probe1d_cases as P1
import probe_ap_cases as PK
import sparse_linear_cases as SK

GRID_CAP_ENTRIES = 8192 * 256
SL_OUT_CAP_ENTRIES = 4096 * 256
LA_MAX_PARTS = 2048  # latentap.hip

# ---- past_cap: one CSR for latent AP, probe AP, latent top-k and the probes' prepare --------------------------------------------------------

PAST_CAP = dict(n=70_000, s=48, c=5, per_row=32)
PAST_CAP_ZEROS = 12  # stored +0.0 / -0.0 entries in rows of the second trip


def past_cap(seed=41):
    """(70 000, 48, 5): every row stores 32 distinct latents, so nnz = 2 240 000 and the entries from GRID_CAP_ENTRIES on are those of
    rows >= 65 536.  Values k / 4, k = 1 .. 32 (a few dozen tie groups per latent); every third latent is signed, about 40 % of its
    values negative; PAST_CAP_ZEROS stored values in rows >= 65 536 are +0.0 or -0.0 (no events: they get the sort's sentinel)."""
    n, s, c, per_row = (PAST_CAP[k] for k in ("n", "s", "c", "per_row"))
    rng = np.random.default_rng(seed)
    cls = K._labels(rng, n, c)
    r = rng.random((n, s))
    stored = r <= np.partition(r, per_row - 1, axis=1)[:, per_row - 1:per_row]
    dense = (rng.integers(1, 33, size=(n, s)) / 4.0).astype(np.float32)
    signed = np.arange(s) % 3 == 0
    dense = np.where(signed[None, :] & (rng.random((n, s)) < 0.4), -dense, dense)
    first_row = GRID_CAP_ENTRIES // per_row
    rows = rng.choice(np.arange(first_row, n), size=PAST_CAP_ZEROS, replace=False)
    rows[-1] = n - 1
    for i, row in enumerate(rows):
        col = rng.choice(np.flatnonzero(stored[row]))
        dense[row, col] = 0.0 if i % 2 else -0.0
    return K._pack(dense, stored, cls, c)


def past_cap_tail_doubled(d):
    """``past_cap`` with the values of the second trip's entries doubled (exactly): among the tied k / 4 the lowest rows win, so the
    top-k lists of ``past_cap`` hold first-trip entries only; here they hold second-trip entries only."""
    data = d["data"].copy()
    data[GRID_CAP_ENTRIES:] *= np.float32(2)
    return dict(d, data=data)


def past_cap_weights(d, seed=42):
    """(w, b) of probe_ap_cases._mixed: both signs inside every wave."""
    return PK._mixed(np.random.default_rng(seed), d["s"], d["c"])


def past_cap_padded(d, seed=43):
    """The entries of ``past_cap`` as padded code rows: (idx, val (N, 32), row_nnz in 0 .. 34 -- a count above 32 reads as 32 --, keep)."""
    n, per_row = d["n"], PAST_CAP["per_row"]
    rng = np.random.default_rng(seed)
    idx, val = d["indices"].reshape(n, per_row).copy(), d["data"].reshape(n, per_row).copy()
    return idx, val, rng.integers(0, per_row + 3, size=n).astype(np.int32), rng.random(n) < 0.8


def past_cap_probe1d(d):
    """``past_cap`` as a probe1d design: the labels as an N x C 0/1 matrix (a row without a class is a row of zeros)."""
    ymat = np.zeros((d["n"], d["c"]), dtype=bool)
    has = d["cls"] >= 0
    ymat[np.flatnonzero(has), d["cls"][has]] = True
    return P1.Design(d["n"], d["s"], d["c"], d["indptr"], d["indices"], d["data"], ymat)


# ---- pa_top_rows_kernel past its cap ----------------------------------------------------------------------------------------------------------

TOP_ROWS = dict(n=300, s=8200, c=3, top_k=256)
TOP_ROWS_LONG = (5, 8191, 8195)  # latents with more than top_k events, on both sides of output index GRID_CAP_ENTRIES


def top_rows_design(seed=44):
    """(300, 8200, 3) for top_k = 256: S * top_k = 2 099 200 outputs, those of latents >= 8192 written in the second trip.  Most latents
    have 0 .. 3 events, the three of TOP_ROWS_LONG have 270, 280 and 300; values quantised and signed."""
    n, s, c = (TOP_ROWS[k] for k in ("n", "s", "c"))
    rng = np.random.default_rng(seed)
    cls = K._labels(rng, n, c)
    dense = np.zeros((n, s), dtype=np.float32)
    for j in range(s):
        k = int(rng.integers(0, 4))
        dense[rng.choice(n, size=k, replace=False), j] = rng.choice([0.5, 1.0, -1.0, 2.25], size=k)
    for j, m in zip(TOP_ROWS_LONG, (270, 280, 300)):
        dense[:, j] = 0
        dense[rng.choice(n, size=m, replace=False), j] = (np.ceil(rng.gamma(2.0, 2.0, size=m) * 4) / 4) * rng.choice([1.0, 1.0, -1.0], size=m)
    d = K._pack(dense, dense != 0, cls, c)
    w, b = PK._mixed(rng, s, c)
    return dict(d, w=w, b=b)


# ---- the radix byte edges of the latent key -------------------------------------------------------------------------------------------------

RADIX_S = (255, 256, 65_535, 65_536, 1 << 24)
RADIX_PASSES = dict(zip(RADIX_S, (5, 6, 6, 7, 8)))  # four value bytes and as many latent bytes as hold the sentinel S
RADIX_N = 300
RADIX_ZEROS = 3  # stored +0.0 and as many -0.0 entries per used latent


def radix_latents(s):
    """The latents that get events: 0, 1, S - 1 and, where they exist, the neighbours across a byte border of the key."""
    pool = (0, 1, s - 1, 255, 256, 257, 65_535, 65_536, 65_537, (1 << 24) - 1)
    return np.array(sorted({j for j in pool if 0 <= j < s}), dtype=np.int64)


def _from_triples(rows, cols, vals, n, s, cls, c):
    m = scipy.sparse.csr_matrix((vals.astype(np.float32), (rows, cols)), shape=(n, s))
    m.sort_indices()
    assert m.nnz == len(vals)
    return dict(indptr=m.indptr.astype(np.int64), indices=m.indices.astype(np.int32), data=m.data.astype(np.float32), n=n, s=s, c=c,
                cls=np.asarray(cls, dtype=np.int32))


def radix_edges(s, seed=45):
    """(wide, compact, used): ``wide`` has S latents with events in ``used`` = radix_latents(S) only -- quantised, signed, and
    RADIX_ZEROS stored +0.0 and -0.0 entries per used latent --, ``compact`` the same columns renumbered 0 .. len(used) - 1 with one
    more latent, without entries, behind them.  C = 3, or 1 at S = 2^24 (whose outputs and workspace take half a gigabyte)."""
    n, c = RADIX_N, (1 if s == 1 << 24 else 3)
    used = radix_latents(s)
    rng = np.random.default_rng([seed, s])
    cls = K._labels(rng, n, c)
    rows, ranks, vals = [], [], []
    for i in range(len(used)):
        r = rng.choice(n, size=int(rng.integers(90, 150)), replace=False)
        v = np.ceil(rng.gamma(2.0, 1.0, size=len(r)) * 4) / 4 * rng.choice([1.0, 1.0, -1.0], size=len(r))
        v[:RADIX_ZEROS], v[RADIX_ZEROS:2 * RADIX_ZEROS] = 0.0, -0.0
        rows.append(r)
        ranks.append(np.full(len(r), i))
        vals.append(v)
    rows, ranks, vals = np.concatenate(rows), np.concatenate(ranks), np.concatenate(vals)
    return _from_triples(rows, used[ranks], vals, n, s, cls, c), _from_triples(rows, ranks, vals, n, len(used) + 1, cls, c), used


# ---- sparse linear --------------------------------------------------------------------------------------------------------------------------

# (n, S, K) -> (chunk_rows, n_chunks): n > 2048 makes a chunk longer than 64 rows; each has a ragged last chunk (one row at n = 2049)
LONG_CHUNKS = {(2049, 33, 3): (128, 17), (4097, 31, 2): (192, 22), (6145, 257, 7): (256, 25)}


def long_chunk_design(shape):
    """(X, y, C) as test_gpu_sparse_linear.test_ragged_shapes builds its designs."""
    n, s, k = shape
    x, y = SK.make_design(n, s, k, 7 * n + s + k)
    return x, y, SK.c_keeping_features(x, y)


OUT_SHAPE = (64, 20_000, 64)  # 1 280 000 coefficients; rows k >= OUT_FIRST_ROW of coef_ lie wholly past SL_OUT_CAP_ENTRIES
OUT_FIRST_ROW = 53
OUT_MAX_ITER = 12  # (tests/test_analysis_scale_host_cpu.py: not converged by then, and coef[OUT_FIRST_ROW:] holds non-zero entries)


def out_design():
    n, s, k = OUT_SHAPE
    x, y = SK.make_design(n, s, k, 77)
    return x, y, SK.c_keeping_features(x, y)


CHECK_SHAPE = (1025, 4097, 7)
CHECK_FLAT = (GRID_CAP_ENTRIES + 1, 1025 * 4097 - 1)  # where the inf, then the nan, goes: both in sl_check_kernel's second trip


def check_design():
    n, s, k = CHECK_SHAPE
    x, y = SK.make_design(n, s, k, 7 * n + s + k)
    return x, y, SK.c_keeping_features(x, y)


def stats_coefficients(d, seed=46):
    return P1.coefficients(d.s, d.c, seed)

