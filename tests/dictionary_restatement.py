"""Torch restatement of the CANDIDATE RULE of the two dictionary filters (DESIGN.md 3.11 "Why the maximiser is always kept", 3.16
"Why each row's maximiser is always kept"), in fp64 and fp32, so that it runs on the CPU in the host tests and on the device in the
GPU tests.  It is the cosine-level half of kmeans_restatement's second part: the same prepare pass (filter_rows with mu = 0: W - 0
is exact), the same accumulation term, and coh_pair_bound itself instead of km_pair.

Everything the rule is made of is a function of the inputs alone except the fp32 MFMA sum of the image dot product, which the
device forms in an order of its own.  The restatement forms that dot product in fp64 and carries the accumulation term the bound
already states, coh_gamma(Dp) (rn.x + rn.y)_i (rn.x + rn.y)_j, as the half-width delta_ij of an interval around the device's c~_ij:
derived, not measured.  (The term counts 2^-22 per addition of Dp terms, once for the filter's sum and once for the refinement's:
the whole of it is taken, so the filter's half leaves the other half, at least 1.6e-5 at Dp = 64, to the fp32 roundings of
c~ + E and c~ - E, 2^-24 each on numbers below 2.)

With L_i = max_j (s~ - E) the device's L_i lies in [max (s~ - E - delta), max (s~ - E + delta)], so a correct filter reports
    sure <= candidates <= maybe,    sure = #{s~ + E - delta >= max (s~ - E + delta)},    maybe = #{s~ + E + delta >= max (s~ - E - delta)},
and revisits in pass 2 a number of 128 x 128 tiles inside the bracket the same two inequalities give for the tile maxima."""

import torch

from kmeans_restatement import coh_gamma, filter_rows, padded

TILE = 128
MATCH_CAND_PER_ROW, MATCH_CAND_MIN = 8, 4096
COHERENCE_MAX_CANDIDATES = 2 ** 20
NEG_INF = float("-inf")


def tol(D: int) -> float:
    """The GPU tests' tolerance of a refined fp32 cosine (test_gpu_coherence.py, test_gpu_dictionary_match.py)."""
    return (2 * D + 6) * 2.0 ** -24


def match_capacity(Sa: int, Sb: int, self_mode: bool = False) -> int:
    pairs = Sa * (Sa - 1) if self_mode else Sa * Sb
    return max(1, min(pairs, max(MATCH_CAND_MIN, MATCH_CAND_PER_ROW * Sa)))


def coherence_capacity(S: int) -> int:
    return max(1, min(COHERENCE_MAX_CANDIDATES, S * (S - 1) // 2))


def cos64(A: torch.Tensor, B: torch.Tensor) -> torch.Tensor:
    """(Sa, Sb) fp64 cosines of the fp32 rows."""
    A64, B64 = A.double(), B.double()
    return (A64 / A64.norm(dim=1, keepdim=True)) @ (B64 / B64.norm(dim=1, keepdim=True)).T


def pair_values(A: torch.Tensor, B: torch.Tensor | None = None):
    """(c~, E, delta), each (Sa, Sb) fp64 (B absent: A against itself, from one preparation as on the device).  c~ is the exact
    image dot product times 2^-26; E is coh_pair_bound(rn_i, rn_j, gamma) in fp32, in its own order of operations, the row of A as
    its first argument; delta is the bound's accumulation term in fp64."""
    D = A.shape[1]
    zero = torch.zeros(D, dtype=torch.float32, device=A.device)
    x = filter_rows(A, zero)
    c = x if B is None else filter_rows(B, zero)
    assert bool(x.has_image.all()) and bool(c.has_image.all()), "a row without a unit image: the filter answers NaN"
    ct = (x.img @ c.img.T) * 2.0 ** -26
    ax, ay = x.rnx[:, None], x.rny[:, None]
    bx, by = c.rnx[None, :], c.rny[None, :]
    gam = float(coh_gamma(padded(D)))
    gam_t = torch.tensor(gam, dtype=torch.float32, device=A.device)
    # (fp32 tensors throughout: the Python constants are taken as fp32, every operation rounds once, nothing is contracted)
    E = 1.02 * ((ay * bx + ax * by + ay * by) + gam_t * (ax + ay) * (bx + by)) + 1e-30
    assert E.dtype == torch.float32
    delta = gam * (ax.double() + ay.double()) * (bx.double() + by.double())
    return ct, E.double(), delta


def _scores(A, B, absolute, self_mode, e_scale=1.0):
    """(s~, E, delta, admissible) of a match call."""
    assert not (self_mode and B is not None)
    ct, E, delta = pair_values(A, None if self_mode else B)
    ok = torch.ones_like(ct, dtype=torch.bool)
    if self_mode:
        ok.fill_diagonal_(False)
    return (ct.abs() if absolute else ct), E * e_scale, delta, ok


def _masked(v, ok):
    return torch.where(ok, v, torch.full_like(v, NEG_INF))


def match_candidates(A, B=None, *, absolute=False, self_mode=False, e_scale=1.0) -> torch.Tensor:
    """(Sa, Sb) bool: the pairs with s~ + E >= L_i = max_j (s~ - E) at delta = 0 -- the rule itself.  ``e_scale`` multiplies E: what
    a bound too tight by that factor would keep."""
    s, E, _, ok = _scores(A, B, absolute, self_mode, e_scale)
    L = _masked(s - E, ok).max(dim=1, keepdim=True).values
    return ok & (s + E >= L)


def coherence_candidates(W, *, e_scale=1.0) -> torch.Tensor:
    """(S, S) bool, upper triangle: the pairs i < j with |c~| + E >= L = max_{i<j} (|c~| - E) at delta = 0."""
    s, E, _, _ = _scores(W, None, True, True, e_scale)
    ok = torch.ones_like(s, dtype=torch.bool).triu(1)
    return ok & (s + E >= _masked(s - E, ok).max())


def _tile_max(v: torch.Tensor) -> torch.Tensor:
    """(Sa, ceil(Sb / 128)): per row the maximum over each 128-wide block of columns (-inf entries: not admissible)."""
    Sa, Sb = v.shape
    nT = -(-Sb // TILE)
    pad = torch.full((Sa, nT * TILE), NEG_INF, dtype=v.dtype, device=v.device)
    pad[:, :Sb] = v
    return pad.view(Sa, nT, TILE).max(dim=2).values


def _row_tiles(hit: torch.Tensor) -> int:
    """hit: (Sa, nTB) bool per (row, tile of B).  The number of (I, J) tiles in which some row of I hits."""
    Sa, nTB = hit.shape
    nTA = -(-Sa // TILE)
    pad = torch.zeros(nTA * TILE, nTB, dtype=torch.bool, device=hit.device)
    pad[:Sa] = hit
    return int(pad.view(nTA, TILE, nTB).any(dim=1).sum())


def _match_brackets(A, B, absolute, self_mode):
    s, E, delta, ok = _scores(A, B, absolute, self_mode)
    L_hi = _masked(s - E + delta, ok).max(dim=1, keepdim=True).values
    L_lo = _masked(s - E - delta, ok).max(dim=1, keepdim=True).values
    up_lo, up_hi = _masked(s + E - delta, ok), _masked(s + E + delta, ok)
    pairs = int((up_lo >= L_hi).sum()), int((up_hi >= L_lo).sum())
    tiles = _row_tiles(_tile_max(up_lo) >= L_hi), _row_tiles(_tile_max(up_hi) >= L_lo)
    return pairs, tiles


def match_bracket(A, B=None, *, absolute=False, self_mode=False):
    """(sure, maybe) of MatchResult.candidates."""
    return _match_brackets(A, B, absolute, self_mode)[0]


def match_tile_bracket(A, B=None, *, absolute=False, self_mode=False):
    """(sure, maybe) of MatchResult.tiles_refiltered: tile (I, J) is revisited when some row of I has max over J of (s~ + E) >= L_i."""
    return _match_brackets(A, B, absolute, self_mode)[1]


def _coherence_brackets(W):
    s, E, delta, _ = _scores(W, None, True, True)
    ok = torch.ones_like(s, dtype=torch.bool).triu(1)
    L_hi, L_lo = _masked(s - E + delta, ok).max(), _masked(s - E - delta, ok).max()
    up_lo, up_hi = _masked(s + E - delta, ok), _masked(s + E + delta, ok)
    pairs = int((up_lo >= L_hi).sum()), int((up_hi >= L_lo).sum())
    # (the masked lower triangle holds -inf, so tiles with I > J never hit; the order t = J (J + 1) / 2 + I does not show in a count)
    tiles = _row_tiles(_tile_max(up_lo) >= L_hi), _row_tiles(_tile_max(up_hi) >= L_lo)
    return pairs, tiles


def coherence_bracket(W):
    """(sure, maybe) of CoherenceResult.candidates: one global L over i < j, s = |c|."""
    return _coherence_brackets(W)[0]


def coherence_tile_bracket(W):
    """(sure, maybe) of CoherenceResult.tiles_refiltered: an upper-triangle tile is revisited when its max of (|c~| + E) >= L."""
    return _coherence_brackets(W)[1]
