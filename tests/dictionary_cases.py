"""The inputs of test_gpu_dictionary_geometry.py, as functions of nothing but their arguments (CPU tensors from seeded generators),
so that test_dictionary_cases_host_cpu.py can check on the CPU, with the restated candidate rule, what the GPU tests rely on for
the very same bits: that the fp16 images alone misorder the pairs, that fp64 still decides every asserted index, and on which side
of the list capacity the candidate count falls.

Why small D.  The image error of a cosine falls like 1 / sqrt(D) (about 4e-4 at D = 16, 1e-5 at D = 256) while the tolerance of the
refined value, (2 D + 6) 2^-24, grows with D (2e-6 at D = 16, 3e-5 at D = 256): at D = 16 pairs 4e-5 apart are 17 tolerances apart
for fp64 and the fp32 refinement, and in arbitrary order for the images.  Only a filter whose bound E really covers the image error
keeps the true maximiser among its candidates there.

Every seed below is a constant chosen once, as the first of a short list for which the preconditions of the host tests hold."""

import dataclasses

import torch

CORR = 0.9          # the cosine of decoy 0 / planted pair 0
STEP = 4e-5         # the cosine step between decoys / planted pairs
SA = 300            # 2 x 128 + 44 rows of A
DECOY_SEEDS = {"decoys": 101, "decoys_absolute": 102, "decoys_overflow": 103, "decoys_d64": 104}
OFFSET_SEED = 201
# The image's global argmax must lose by more than 8 tol(D): one step at D = 16 (17.7 tol), two at D = 64 (5.0 tol each).  D = 16: the
# second of 301, 302, ... (about one seed in three qualifies); D = 64: the first that did of 311 .. 331 (about one seed in eight).
PLANTED_SEEDS = {16: 302, 64: 331}
PLANTED_PAIRS = 300


def _unit(x):
    return x / x.norm(dim=1, keepdim=True)


def _at_cosine(a, r, g):
    """Unit rows at cosine r (a scalar or one per row) to the unit rows a, in a random direction orthogonal to them."""
    o = torch.randn(a.shape, generator=g, dtype=torch.float64)
    o = _unit(o - (o * a).sum(dim=1, keepdim=True) * a)
    r = torch.as_tensor(r, dtype=torch.float64).reshape(-1, 1)
    return r * a + (1 - r * r).sqrt() * o


@dataclasses.dataclass
class MatchCase:
    A: torch.Tensor            # (Sa, D) fp32
    B: torch.Tensor | None     # (Sb, D) fp32; None: self mode
    absolute: bool
    planted: torch.Tensor | None  # (n,) the index of the best match of rows 0 .. n - 1; None: no planted answer
    D: int

    @property
    def self_mode(self):
        return self.B is None

    @property
    def shape(self):
        return self.A.shape[0], (self.A if self.B is None else self.B).shape[0]


def _decoys(seed, D, nd, step, negate_odd):
    g = torch.Generator().manual_seed(seed)
    a = _unit(torch.randn(SA, D, generator=g, dtype=torch.float64))
    A = a * (0.5 + 2.0 * torch.rand(SA, 1, generator=g, dtype=torch.float64))
    B = torch.empty(nd * SA, D, dtype=torch.float64)
    for j in range(nd):  # decoy j of row i at index j SA + i: a row's decoys lie in different 128-row tiles of B
        b = _at_cosine(a, CORR + step * j, g) * (0.5 + 2.0 * torch.rand(SA, 1, generator=g, dtype=torch.float64))
        B[j * SA:(j + 1) * SA] = -b if negate_odd and j % 2 else b
    return A.float(), B.float(), (nd - 1) * SA + torch.arange(SA)


def decoys():
    """300 rows at D = 16, each with 8 decoys in B at cosines 0.9 + 4e-5 j and row scales in [0.5, 2.5]: Sb = 2 400, ragged last
    tiles on both sides (300 = 2 x 128 + 44, 2 400 = 18 x 128 + 96).  The answer of row i is 7 x 300 + i."""
    A, B, planted = _decoys(DECOY_SEEDS["decoys"], 16, 8, STEP, False)
    return MatchCase(A, B, False, planted, 16)


def decoys_absolute():
    """decoys with the odd decoys negated: the best one is antiparallel, and only |c| finds it."""
    A, B, planted = _decoys(DECOY_SEEDS["decoys_absolute"], 16, 8, STEP, True)
    return MatchCase(A, B, True, planted, 16)


def decoys_self():
    """W = cat(A, B) of decoys in self mode: rows 0 .. 299 keep their answer (moved by 300), the decoy rows have none planted."""
    c = decoys()
    return MatchCase(torch.cat([c.A, c.B]), None, False, c.planted + SA, 16)


def decoys_overflow():
    """16 decoys per row at cosines 0.9 + 2e-5 j: Sb = 4 800, and every row's 16 decoys are candidates -- 4 800 against a list of
    4 096.  The answer of row i is 15 x 300 + i."""
    A, B, planted = _decoys(DECOY_SEEDS["decoys_overflow"], 16, 16, STEP / 2, False)
    return MatchCase(A, B, False, planted, 16)


def decoys_d64():
    """decoys at D = 64, one full k stage of the filter: the step is 5.0 tol(64), just above the 4 tol of the index rule."""
    A, B, planted = _decoys(DECOY_SEEDS["decoys_d64"], 64, 8, STEP, False)
    return MatchCase(A, B, False, planted, 64)


def common_offset(eps):
    """Rows that share a unit offset, off + eps randn / sqrt(D): 150 against 200 at D = 64, every cosine near 1 / (1 + eps^2).  At
    eps = 0.1 a few candidates per row; at eps = 0.03 nearly all 30 000 pairs, from data that is realistic rather than built equal."""
    Sa, Sb, D = 150, 200, 64
    g = torch.Generator().manual_seed(OFFSET_SEED)
    off = _unit(torch.randn(1, D, generator=g, dtype=torch.float64))
    A = off + eps * torch.randn(Sa, D, generator=g, dtype=torch.float64) / D ** 0.5
    B = off + eps * torch.randn(Sb, D, generator=g, dtype=torch.float64) / D ** 0.5
    return MatchCase(A.float(), B.float(), False, None, D)


MATCH_FILTER_CASES = {"decoys": decoys, "decoys_absolute": decoys_absolute, "decoys_self": decoys_self, "decoys_d64": decoys_d64,
                      "common_offset_0.1": lambda: common_offset(0.1)}
MATCH_OVERFLOW_CASES = {"decoys_overflow": decoys_overflow, "common_offset_0.03": lambda: common_offset(0.03)}
MATCH_CASES = {**MATCH_FILTER_CASES, **MATCH_OVERFLOW_CASES}


def planted_pairs(D):
    """(W, (i, j)): 300 pairs of rows, pair p at cosine 0.9 + 4e-5 p with row scales in [0.5, 2.5], laid out pair by pair in a
    seeded random order of the pairs: S = 600, and the best pair (p = 299) sits wherever the permutation put it."""
    g = torch.Generator().manual_seed(PLANTED_SEEDS[D])
    P = PLANTED_PAIRS
    a = _unit(torch.randn(P, D, generator=g, dtype=torch.float64))
    b = _at_cosine(a, CORR + STEP * torch.arange(P, dtype=torch.float64), g)
    a = a * (0.5 + 2.0 * torch.rand(P, 1, generator=g, dtype=torch.float64))
    b = b * (0.5 + 2.0 * torch.rand(P, 1, generator=g, dtype=torch.float64))
    order = torch.randperm(P, generator=g)
    W = torch.empty(2 * P, D, dtype=torch.float64)
    W[0::2], W[1::2] = a[order], b[order]
    k = int((order == P - 1).nonzero())
    return W.float(), (2 * k, 2 * k + 1)


COHERENCE_DS = (16, 64)


# ---- families that only the host tests use: the bound |c~ - c| <= E away from the planted cases ----------------------------------

def scaled_rows(D, seed=401):
    """Gaussian rows, every row multiplied by 10^U(-3, 3)."""
    g = torch.Generator().manual_seed(seed + D)
    A = torch.randn(120, D, generator=g) * 10.0 ** (6 * torch.rand(120, 1, generator=g) - 3)
    B = torch.randn(150, D, generator=g) * 10.0 ** (6 * torch.rand(150, 1, generator=g) - 3)
    return A, B


def flushed_rows(D, seed=411):
    """Rows with a few elements of order 1 and the rest spread over 2^-30 .. 2^-22 of them: 2^13 u of the small ones straddles the
    smallest normal fp16 number 2^-14, below which the image is flushed to zero."""
    g = torch.Generator().manual_seed(seed + D)

    def rows(S):
        X = torch.randn(S, D, generator=g) * 2.0 ** (-30 + 8 * torch.rand(S, D, generator=g))
        big = torch.rand(S, D, generator=g) < 3.0 / D
        big[:, 0] = True
        return torch.where(big, torch.randn(S, D, generator=g) + 2.0 * torch.randn(S, D, generator=g).sign(), X)

    return rows(120), rows(150)


def midpoint_rows(D, seed=421):
    """Unit rows whose elements but the largest have 2^13 u halfway between two fp16 numbers (the largest element makes the norm 1
    in fp64, so that the fp32 division moves the others by a few 2^-24 only): the largest ||d|| a row can have."""
    g = torch.Generator().manual_seed(seed + D)

    def rows(S):
        s = _unit(torch.randn(S, D, generator=g, dtype=torch.float64)) * 8192.0
        h = s.half().double()
        ulp = 2.0 ** (torch.floor(torch.log2(h.abs().clamp_min(2.0 ** -14))) - 10)
        t = h.sign() * (h.abs() + 0.5 * ulp) / 8192.0  # (away from zero: the midpoint above |h| lies in h's own binade)
        big = s.abs().argmax(dim=1, keepdim=True)
        sign = s.gather(1, big).sign()
        t.scatter_(1, big, 0.0)
        rest = 1.0 - (t ** 2).sum(dim=1, keepdim=True)
        assert (rest > 0).all()
        t.scatter_(1, big, sign * rest.sqrt())
        return t.float()

    return rows(120), rows(150)


BOUND_DS = (4, 16, 68, 132, 256)
BOUND_FAMILIES = {"scaled": scaled_rows, "flushed": flushed_rows, "midpoints": midpoint_rows}
