"""Builders of the inputs of the coactivation tests (tests/test_coactivation_host_cpu.py, tests/test_gpu_coactivation.py): every case
is a pair of scipy CSR matrices with the call's settings and a ``holds(expected)`` check of the property the case was built for,
where ``expected`` is what tests/coactivation_restatement.py:match makes of it.  The CPU test runs every ``holds``; the GPU test
demands that the device equals ``expected``.  The kernel's constants come in as arguments (the library's accessors give them)."""

from __future__ import annotations

import dataclasses
from typing import Callable

import numpy as np
import scipy.sparse

CHUNK_ROWS, WINDOW, SLOTS = 8192, 32768, 512  # the library's values, asserted by the CPU test
SMALL_WINDOW, MID_WINDOW = 8192, 16384  # Sb up to these runs the walk with a smaller window and workgroup (coactivation.hip)


@dataclasses.dataclass
class Case:
    name: str
    A: scipy.sparse.csr_matrix
    B: scipy.sparse.csr_matrix | None
    holds: Callable[[dict], None]
    thr_a: float = 0.0
    thr_b: float = 0.0
    measure: str = "jaccard"
    top_m: int = 1

    @property
    def settings(self) -> dict:
        return dict(thr_a=self.thr_a, thr_b=self.thr_b, measure=self.measure, top_m=self.top_m)


def from_sets(sets: dict[int, np.ndarray | list | range], n_rows: int, n_latents: int, value: float = 1.0) -> scipy.sparse.csr_matrix:
    """The CSR matrix in which latent l is stored (with ``value``) in exactly the rows ``sets[l]``."""
    rows = np.concatenate([np.asarray(list(r) if not isinstance(r, np.ndarray) else r, dtype=np.int64) for r in sets.values()] or [np.zeros(0, np.int64)])
    cols = np.concatenate([np.full(len(r), l, dtype=np.int64) for l, r in sets.items()] or [np.zeros(0, np.int64)])
    m = scipy.sparse.csr_matrix((np.full(rows.size, value, dtype=np.float32), (rows, cols)), shape=(n_rows, n_latents))
    m.sort_indices()
    return m


def random_csr(rng, n_rows: int, n_latents: int, per_row, values=None) -> scipy.sparse.csr_matrix:
    """``per_row`` distinct random columns in every row (an int, or one int per row); values uniform in (0.1, 1) or drawn from ``values``."""
    lens = np.broadcast_to(np.asarray(per_row, dtype=np.int64), (n_rows,))
    cols = [rng.choice(n_latents, size=int(k), replace=False) for k in lens]
    indices = np.concatenate(cols) if cols else np.zeros(0, np.int64)
    data = rng.uniform(0.1, 1.0, indices.size) if values is None else rng.choice(np.asarray(values), indices.size)
    indptr = np.concatenate([[0], np.cumsum(lens)])
    return scipy.sparse.csr_matrix((data.astype(np.float32), indices.astype(np.int32), indptr.astype(np.int64)), shape=(n_rows, n_latents))


def _nothing(_):
    pass


def shape_edges() -> list[Case]:
    rng = np.random.default_rng(11)
    out = [Case("n_rows_1", from_sets({0: [0], 2: [0]}, 1, 3), from_sets({1: [0]}, 1, 2),
                lambda e: _eq(e["index"][:, 0], [1, -1, 1]))]
    # rows of 0, 1, 63, 64, 65 and 300 entries (twice over, in a mixed order), Sa = 400 so that some latents have no event
    lens = np.array([0, 300, 1, 63, 0, 64, 65, 300, 1, 0, 65, 64, 63], dtype=np.int64)
    A, B = random_csr(rng, len(lens), 400, lens), random_csr(rng, len(lens), 400, lens[::-1].copy())

    def some_latent_is_empty(e):
        assert (e["support_a"] == 0).any() and (e["index"][e["support_a"] == 0] == -1).all()
    out.append(Case("row_lengths", A, B, some_latent_is_empty, top_m=3))
    out.append(Case("row_lengths_self", A, None, some_latent_is_empty, top_m=3))
    out.append(Case("sa_1", from_sets({0: [0, 1, 2]}, 4, 1), from_sets({0: [0], 3: [1, 2, 3]}, 4, 5),
                    lambda e: _eq(e["index"], [[3, 0]]), top_m=2))
    out.append(Case("sb_1", from_sets({0: [0, 1], 2: [3]}, 4, 3), from_sets({0: [1, 2]}, 4, 1),
                    lambda e: _eq(e["index"], [[0, -1], [-1, -1], [-1, -1]]), top_m=2))
    out.append(Case("sa_1_self", from_sets({0: [0, 1]}, 2, 1), None, lambda e: _eq(e["index"], [[-1]])))
    return out


def window_edges(window: int, tag: str) -> list[Case]:
    """Sb one below, at and one past ``window`` with five latents of A; ``hi`` is B's last latent.  At Sb = window + 1 it is alone in the
    second window: there sits the best partner of latent 0, and latent 1 has two equal partners, hi - 1 and hi, either side of the
    border (the lower index ranks first) after a better one in the first window."""
    out = []
    n = 60
    A = from_sets({0: range(0, 10), 1: range(10, 20), 2: range(20, 32), 4: [39]}, n, 5)
    for Sb in (window - 1, window, window + 1):
        hi = Sb - 1
        sets = {3: range(0, 4), hi: list(range(0, 9)) + list(range(15, 20)),        # latent 0: hi (9 of 14) beats 3 (4 of 4)
                hi - 1: list(range(10, 15)) + list(range(40, 49)), 7: range(10, 18),  # latent 1: 7, then hi - 1 and hi at 5 of 14 each
                1: range(20, 24), hi - 2: range(20, 28), 9: range(20, 30), 0: [39]}

        def holds(e, hi=hi):
            _eq(e["index"][0, :2], [hi, 3])
            _eq(e["index"][1], [7, hi - 1, hi])
            _eq(e["intersection"][1], [8, 5, 5])
            _eq(e["index"][2], [9, hi - 2, 1])
            _eq(e["index"][3], [-1, -1, -1])
            _eq(e["index"][4], [0, -1, -1])
        out.append(Case(f"{tag}_sb_{Sb}", A, from_sets(sets, n, Sb), holds, top_m=3))
    return out


def heavy_lists(chunk: int) -> list[Case]:
    rng = np.random.default_rng(5)
    lens = [chunk - 1, chunk, chunk + 1, 3 * chunk + 5, 40]
    n = 3 * chunk + 5
    A = from_sets({l: np.sort(rng.choice(n, size=k, replace=False)) for l, k in enumerate(lens)}, n, 6)
    B = random_csr(rng, n, 50, 3)

    def holds(e):
        _eq(e["support_a"], lens + [0])
        assert (e["index"][:5] >= 0).all()
    out = [Case("heavy_lists", A, B, holds, top_m=8), Case("heavy_lists_containment", A, B, holds, measure="containment", top_m=3),
           Case("heavy_lists_self", A, None, holds, top_m=3)]
    # every row: a latent of A and one of B that fire everywhere, and a pair that co-fires on more rows than 16 bits count
    n = 70000
    A = from_sets({0: range(n), 1: range(0, 66000), 2: rng.choice(n, size=300, replace=False)}, n, 3)
    B = from_sets({0: range(n), 1: range(100, n), 3: rng.choice(n, size=5000, replace=False)}, n, 4)

    def wide(e):
        assert e["index"][0, 0] == 0 and e["intersection"][0, 0] == n > 65536
        assert e["intersection"][1, 0] > 65536
    out.append(Case("every_row", A, B, wide, top_m=3))
    return out


def many_heavy(chunk: int, slots: int) -> Case:
    """More heavy latents than counter rows: the heavy route runs a second round."""
    rng = np.random.default_rng(6)
    n, Sa = chunk + 1, slots + 8
    A = scipy.sparse.csr_matrix(np.ones((n, Sa), dtype=np.float32))
    B = random_csr(rng, n, 6, 2)

    def holds(e):
        assert (e["support_a"] == n).all() and len(e["support_a"]) > slots
        assert (e["index"] == e["index"][0]).all()  # every latent of A is the same set
    return Case("many_heavy", A, B, holds, top_m=2)


def ranking() -> list[Case]:
    out = []
    # partners: latent 0 has 2, latent 1 has 3, latent 2 has 10, latent 3 none
    A = from_sets({0: range(0, 10), 1: range(10, 20), 2: range(20, 40)}, 40, 4)
    sets = {0: range(0, 5), 1: range(3, 10), 2: range(10, 12), 3: range(12, 16), 4: range(15, 20)}
    sets.update({5 + j: range(20 + j, 22 + 2 * j) for j in range(10)})
    B = from_sets(sets, 40, 16)
    for top_m in (1, 3, 8):
        def holds(e, top_m=top_m):
            found = (e["index"] >= 0).sum(axis=1)
            _eq(found, [min(2, top_m), min(3, top_m), min(10, top_m), 0])
            assert ((e["intersection"] == 0) == (e["index"] == -1)).all()
        out.append(Case(f"top_m_{top_m}", A, B, holds, top_m=top_m))
        out.append(Case(f"top_m_{top_m}_containment", A, B, holds, top_m=top_m, measure="containment"))
    # Jaccard 1/2 against 2/4: equal cross-products with different I and U, the lower index first
    A = from_sets({0: [0, 1], 1: [10, 11]}, 20, 2)
    B = from_sets({3: [0, 1, 5, 6], 7: [0], 2: [10], 9: [10, 11, 15, 16]}, 20, 10)

    def jaccard_tie(e):
        _eq(e["index"], [[3, 7], [2, 9]])
        _eq(e["intersection"], [[2, 1], [1, 2]])
        _eq(e["jaccard"], [[0.5, 0.5], [0.5, 0.5]])
    out.append(Case("jaccard_tie", A, B, jaccard_tie, top_m=2))
    # containment: equal I, the smaller n_b first, then the lower index
    A = from_sets({0: range(0, 4)}, 12, 1)
    B = from_sets({1: [0, 1, 6, 7, 8], 4: [2, 3, 9], 6: [0, 3, 10], 2: [1]}, 12, 8)

    def containment_tie(e):
        _eq(e["index"], [[4, 6, 1, 2]])
        _eq(e["intersection"], [[2, 2, 2, 1]])
    out.append(Case("containment_tie", A, B, containment_tie, measure="containment", top_m=4))
    # the measures disagree: latent 0 of B covers a entirely but is huge, latent 1 is a's near copy
    A = from_sets({0: range(0, 10)}, 100, 1)
    B = from_sets({0: range(0, 100), 1: range(0, 8)}, 100, 2)
    out.append(Case("measures_jaccard", A, B, lambda e: _eq(e["index"], [[1, 0]]), top_m=2))
    out.append(Case("measures_containment", A, B, lambda e: _eq(e["index"], [[0, 1]]), measure="containment", top_m=2))
    # products near 2^31 x 2^32 cannot be built from real rows; the CPU test holds the order against Python ints there
    return out


def thresholds() -> list[Case]:
    rng = np.random.default_rng(9)
    vals = [-2.0, -1.0, -0.5, 0.0, 0.5, 1.0, 2.0]
    A, B = random_csr(rng, 300, 40, 6, vals), random_csr(rng, 300, 50, 5, vals)

    def holds(thr_a, thr_b):
        def check(e):
            _eq(e["support_a"], np.bincount(A.indices[A.data > thr_a], minlength=40))
            _eq(e["support_b"], np.bincount(B.indices[B.data > thr_b], minlength=50))
            assert (A.data == np.float32(thr_a)).any()  # value == thr is met and must not fire
        return check
    return [Case("thr_equal_does_not_fire", A, B, holds(0.5, 0.5), thr_a=0.5, thr_b=0.5, top_m=3),
            Case("thr_negative", A, B, holds(-1.0, -1.0), thr_a=-1.0, thr_b=-1.0, top_m=3),
            Case("thr_differ", A, B, holds(-1.0, 0.5), thr_a=-1.0, thr_b=0.5, top_m=3, measure="containment"),
            Case("thr_self", A, None, lambda e: _eq(e["support_b"], e["support_a"]), thr_a=0.5, thr_b=123.0, top_m=3)]


def self_mode() -> list[Case]:
    rng = np.random.default_rng(3)
    A = random_csr(rng, 500, 30, 4).tolil()
    A[:, 9] = A[:, 5]   # latents 5 and 9, and 20 and 21, are duplicates
    A[:, 21] = A[:, 20]
    A = scipy.sparse.csr_matrix(A, dtype=np.float32)

    def holds(e):
        assert (e["index"] != np.arange(30)[:, None]).all()  # the self pair is no partner
        assert e["index"][5, 0] == 9 and e["index"][9, 0] == 5 and e["jaccard"][5, 0] == 1.0 and e["jaccard"][9, 0] == 1.0
        assert e["index"][20, 0] == 21 and e["mutual"][[5, 9, 20, 21]].all()
    return [Case("self_duplicates", A, None, holds, top_m=4)]


def random_mid() -> list[Case]:
    rng = np.random.default_rng(21)
    A, B = random_csr(rng, 3000, 200, 8), random_csr(rng, 3000, 300, 6)
    wide = random_csr(rng, 200, 9000, 120)  # long rows and Sb past the small window: 64 lanes a row, the 128 KB walk
    return [Case("random_jaccard", A, B, _nothing, top_m=8), Case("random_containment", A, B, _nothing, top_m=8, measure="containment"),
            Case("random_self", A, None, _nothing, top_m=8),
            Case("random_long_rows", random_csr(rng, 200, 40, 4), wide, _nothing, top_m=5),
            Case("random_long_rows_swapped", wide, random_csr(rng, 200, 40, 4), _nothing, top_m=2)]


def all_cases(chunk: int = CHUNK_ROWS, window: int = WINDOW, slots: int = SLOTS) -> list[Case]:
    return (shape_edges() + window_edges(window, "window") + window_edges(SMALL_WINDOW, "small_window") + window_edges(MID_WINDOW, "mid_window") + heavy_lists(chunk) + [many_heavy(chunk, slots)]
            + ranking() + thresholds() + self_mode() + random_mid())


def _eq(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and (got == want).all(), (got, want)
