"""CPU-only tests of the inputs of test_gpu_dictionary_geometry.py (dictionary_cases.py) under the restated candidate rule of the
two dictionary filters (dictionary_restatement.py).  They prove on the very tensors the GPU tests use what those tests rely on:

* the bound: |c~ - c64| <= E for every admissible pair, c64 the fp64 cosine of the fp32 rows -- also on families the GPU tests
  do not run (row scales 1e-3 .. 1e3, elements under the image's flush threshold, elements at fp16 rounding midpoints, D from 4
  to 256);
* the preconditions: every asserted index is decided in fp64 by more than 4 tol(D), and the argmax of the images alone is wrong by
  more than 8 tol(D) for at least a quarter of the asserted rows (D = 64: at least 10 rows), so only a filter whose bound holds
  returns the planted index;
* the side of the list capacity the candidate bracket falls on, which decides the route the GPU tests assert;
* that the tests bite: with the true E every planted best is a candidate of the restated rule, with E = 0 at least a quarter
  are dropped.

tol(D), 4 tol(D) and the capacities are those of the GPU tests and of kernels.h; the shares are conditions on the inputs."""

import functools

import pytest
import torch

import dictionary_cases as K
import dictionary_restatement as R

MATCH = sorted(K.MATCH_CASES)
PLANTED = ["decoys", "decoys_absolute", "decoys_d64", "decoys_overflow", "decoys_self"]


@functools.lru_cache(maxsize=None)
def match_case(name):
    """The case, (c~, E, delta), the fp64 scores with inadmissible pairs at -inf, and per row (best, second, argmax) of them."""
    c = K.MATCH_CASES[name]()
    vals = R.pair_values(c.A, c.B)
    g = R.cos64(c.A, c.A if c.self_mode else c.B)
    c64 = g.clone()
    if c.absolute:
        g = g.abs()
    if c.self_mode:
        g.fill_diagonal_(R.NEG_INF)
    top = g.topk(2, dim=1)
    return c, vals, c64, g, (top.values[:, 0], top.values[:, 1], top.indices[:, 0])


@functools.lru_cache(maxsize=None)
def coherence_case(D):
    W, pair = K.planted_pairs(D)
    return W, pair, R.pair_values(W), R.cos64(W, W)


def image_scores(name):
    c, (ct, _, _), _, _, _ = match_case(name)
    s = ct.abs() if c.absolute else ct.clone()
    if c.self_mode:
        s.fill_diagonal_(R.NEG_INF)
    return s


def test_the_planted_cases_are_the_ones_with_a_planted_answer():
    assert PLANTED == sorted(n for n in MATCH if K.MATCH_CASES[n]().planted is not None)


def test_the_inputs_are_small_fp32_matrices():
    """At most 4 800 rows (decoys_overflow, D = 16) and 2 400 x 64 floats (decoys_d64)."""
    for name in MATCH:
        c = K.MATCH_CASES[name]()
        for t in (c.A,) if c.B is None else (c.A, c.B):
            assert t.dtype == torch.float32 and t.shape[1] == c.D and t.shape[0] <= 4800 and t.numel() <= 2400 * 64, (name, t.shape)


# ---- the bound ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", MATCH)
def test_the_bound_holds_on_every_pair_of_a_match_case(name):
    c, (ct, E, _), c64, _, _ = match_case(name)
    slack = E - (ct - c64).abs()
    if c.self_mode:
        slack.fill_diagonal_(float("inf"))
    print(f"{name}: max |c~ - c| {(ct - c64).abs().max():.3g}, E in [{E.min():.3g}, {E.max():.3g}], least slack {slack.min():.3g}")
    assert slack.min() >= 0


@pytest.mark.parametrize("D", K.COHERENCE_DS)
def test_the_bound_holds_on_every_pair_of_a_coherence_case(D):
    W, _, (ct, E, _), c64 = coherence_case(D)
    slack = (E - (ct - c64).abs())[torch.ones_like(ct, dtype=torch.bool).triu(1)]
    assert slack.min() >= 0, slack.min()


@pytest.mark.parametrize("D", K.BOUND_DS)
@pytest.mark.parametrize("family", sorted(K.BOUND_FAMILIES))
def test_the_bound_holds_on_further_families(family, D):
    A, B = K.BOUND_FAMILIES[family](D)
    ct, E, _ = R.pair_values(A, B)
    err = (ct - R.cos64(A, B)).abs()
    print(f"{family} D={D}: max |c~ - c| {err.max():.3g}, least slack {(E - err).min():.3g}")
    assert (E - err).min() >= 0


def test_the_further_families_are_what_they_say():
    from kmeans_restatement import F16_MIN_NORMAL, IMG_SCALE, filter_rows

    A, _ = K.scaled_rows(16)
    assert A.norm(dim=1).min() < 1e-2 and A.norm(dim=1).max() > 1e2
    for D in K.BOUND_DS:
        A, _ = K.flushed_rows(D)
        s = (A / A.norm(dim=1, keepdim=True)).abs() * IMG_SCALE
        small = (s > 0) & (s < 4 * F16_MIN_NORMAL)
        assert (small & (s < F16_MIN_NORMAL)).any() and (small & (s >= F16_MIN_NORMAL)).any()  # both sides of the threshold
        A, _ = K.midpoint_rows(D)
        rows = filter_rows(A, torch.zeros(D))
        s = (A.double() / A.double().norm(dim=1, keepdim=True)) * IMG_SCALE
        ulp = 2.0 ** (torch.floor(torch.log2(s.abs().clamp_min(2.0 ** -14))) - 10)
        d = (s - rows.img).abs() / ulp
        # every element but one per row is rounded by half an fp16 ulp (to within the fp32 division's 2^-24, 2^-13 of that ulp)
        assert ((d - 0.5).abs() < 1e-3).sum(dim=1).min() >= D - 1


# ---- preconditions --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", PLANTED)
def test_fp64_decides_every_planted_row_and_the_images_alone_do_not(name):
    c, _, _, g, (best, second, arg) = match_case(name)
    n, D = c.planted.numel(), c.D
    assert n == K.SA and torch.equal(arg[:n], c.planted)
    gap = (best - second)[:n]
    assert gap.min() > 4 * R.tol(D), (gap.min().item() / R.tol(D))
    pick = image_scores(name).argmax(dim=1)[:n]
    loss = best[:n] - g[torch.arange(n), pick]
    wrong = int((loss > 8 * R.tol(D)).sum())
    print(f"{name}: least fp64 gap {gap.min() / R.tol(D):.1f} tol, image argmax loses by more than 8 tol on {wrong} of {n} rows")
    assert wrong >= (10 if name == "decoys_d64" else n // 4)


@pytest.mark.parametrize("D", K.COHERENCE_DS)
def test_fp64_decides_the_planted_pair_and_the_images_alone_do_not(D):
    W, (i, j), (ct, _, _), c64 = coherence_case(D)
    S = W.shape[0]
    assert S == 2 * K.PLANTED_PAIRS and 0 <= i < j < S
    g = c64.abs().triu(1)
    top = g.flatten().topk(2)
    assert divmod(int(top.indices[0]), S) == (i, j)
    assert top.values[0] - top.values[1] > 4 * R.tol(D)
    pi, pj = divmod(int(ct.abs().triu(1).argmax()), S)
    loss = (top.values[0] - g[pi, pj]).item()
    print(f"planted pairs D={D}: the image's argmax {(pi, pj)} loses by {loss / R.tol(D):.1f} tol to {(i, j)}")
    assert loss > 8 * R.tol(D)
    # the best pair is not in the last tile
    assert j // R.TILE < (S - 1) // R.TILE


def test_fp64_decides_the_coherence_pair_of_decoys_self():
    """What the consistency test between the two entries relies on: one pair of cat(A, B) is the largest |c| by far more than
    4 tol, both entries answer on the filter route, and each end of the pair has the other as its clear nearest neighbour."""
    c, _, c64, _, _ = match_case("decoys_self")
    S = c.A.shape[0]
    g = c64.abs()
    g.fill_diagonal_(R.NEG_INF)
    top = g.triu(1).flatten().topk(2)
    assert top.values[0] - top.values[1] > 4 * R.tol(c.D)
    i, j = divmod(int(top.indices[0]), S)
    for a, b in ((i, j), (j, i)):
        row = g[a].topk(2)
        assert int(row.indices[0]) == b and row.values[0] - row.values[1] > 4 * R.tol(c.D)
    assert R.match_bracket(c.A, None, absolute=True, self_mode=True)[1] <= R.match_capacity(S, S, True)
    assert R.coherence_bracket(c.A)[1] <= R.coherence_capacity(S)


@pytest.mark.parametrize("name,least", [("common_offset_0.1", 75), ("common_offset_0.03", 50)])
def test_common_offset_has_clear_rows(name, least):
    c, _, _, _, (best, second, _) = match_case(name)
    clear = int((best - second > 4 * R.tol(c.D)).sum())
    print(f"{name}: {clear} of {c.A.shape[0]} rows clear")
    assert c.A.shape[0] == 150 and least <= clear < 150  # (and not all: the clear-row rule has both kinds to tell apart)


# ---- brackets against the capacity ------------------------------------------------------------------------------------------------

def brackets(name):
    c = K.MATCH_CASES[name]()
    kw = dict(absolute=c.absolute, self_mode=c.self_mode)
    return c, R.match_bracket(c.A, c.B, **kw), R.match_tile_bracket(c.A, c.B, **kw), R.match_capacity(*c.shape, c.self_mode)


@pytest.mark.parametrize("name", sorted(K.MATCH_FILTER_CASES))
def test_filter_route_cases_fit_the_list(name):
    c, (sure, maybe), (tsure, tmaybe), cap = brackets(name)
    Sa, Sb = c.shape
    ntiles = -(-Sa // R.TILE) * -(-Sb // R.TILE)
    print(f"{name}: candidates in [{sure}, {maybe}] of {cap}, tiles in [{tsure}, {tmaybe}] of {ntiles}")
    assert Sa <= sure <= maybe <= cap
    assert -(-Sa // R.TILE) <= tsure <= tmaybe <= ntiles
    if name in ("decoys", "decoys_absolute", "decoys_d64"):
        assert sure == maybe == 8 * K.SA and cap == 4096  # a row's 8 decoys and nothing else
        assert tsure == tmaybe < ntiles
    if name == "common_offset_0.1":
        assert sure < maybe  # a bracket that is not degenerate


@pytest.mark.parametrize("name", sorted(K.MATCH_OVERFLOW_CASES))
def test_overflow_cases_do_not_fit_the_list(name):
    c, (sure, maybe), _, cap = brackets(name)
    print(f"{name}: candidates in [{sure}, {maybe}] of {cap}")
    assert cap == 4096 < sure <= maybe <= c.shape[0] * c.shape[1]
    if name == "decoys_overflow":
        assert sure == maybe == 16 * K.SA


@pytest.mark.parametrize("D", K.COHERENCE_DS)
def test_planted_pairs_fit_the_list(D):
    W = coherence_case(D)[0]
    (sure, maybe), (tsure, tmaybe), cap = R.coherence_bracket(W), R.coherence_tile_bracket(W), R.coherence_capacity(W.shape[0])
    print(f"planted pairs D={D}: candidates in [{sure}, {maybe}] of {cap}, tiles in [{tsure}, {tmaybe}]")
    assert 2 <= sure <= maybe <= 40 and cap == 600 * 599 // 2  # about 2 E / step pairs: a list, not a single survivor
    assert 1 <= tsure <= tmaybe <= 15


def test_capacities_are_the_librarys():
    assert R.match_capacity(300, 2400) == 4096 and R.match_capacity(2700, 2700, True) == 21600 and R.match_capacity(65, 65) == 4096
    assert R.match_capacity(3, 5) == 15 and R.match_capacity(64, 64, True) == 64 * 63
    assert R.coherence_capacity(600) == 179700 and R.coherence_capacity(4097) == 2 ** 20 and R.coherence_capacity(2) == 1


def test_tile_brackets_count_tiles():
    """Two rows of A against 300 of B, one copy of each planted far apart: every row's only candidate is its copy."""
    g = torch.Generator().manual_seed(5)
    B = torch.randn(300, 64, generator=g)
    A = torch.stack([B[3] * 2, B[290] * 0.5])
    assert R.match_bracket(A, B) == (2, 2) and R.match_tile_bracket(A, B) == (2, 2)  # tiles (0, 0) and (0, 2)
    assert R.match_bracket(A[:1], B) == (1, 1) and R.match_tile_bracket(A[:1], B) == (1, 1)
    W = torch.randn(300, 64, generator=g)
    W[299] = -W[5]
    assert R.coherence_bracket(W) == (1, 1) and R.coherence_tile_bracket(W) == (1, 1)
    m = R.coherence_candidates(W)
    assert m.sum() == 1 and m[5, 299]


# ---- the tests bite -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", PLANTED)
def test_a_bound_of_zero_drops_planted_maximisers(name):
    c = K.MATCH_CASES[name]()
    n = c.planted.numel()
    rows = torch.arange(n)
    kw = dict(absolute=c.absolute, self_mode=c.self_mode)
    kept = R.match_candidates(c.A, c.B, **kw)[rows, c.planted]
    assert kept.all()
    kept0 = R.match_candidates(c.A, c.B, e_scale=0.0, **kw)[rows, c.planted]
    print(f"{name}: E = 0 drops the planted best of {n - int(kept0.sum())} of {n} rows")
    assert n - int(kept0.sum()) >= (10 if name == "decoys_d64" else n // 4)


@pytest.mark.parametrize("D", K.COHERENCE_DS)
def test_a_bound_of_zero_drops_the_planted_pair(D):
    W, (i, j), _, _ = coherence_case(D)
    assert R.coherence_candidates(W)[i, j]
    m = R.coherence_candidates(W, e_scale=0.0)
    assert m.sum() == 1 and not m[i, j]
