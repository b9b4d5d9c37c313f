"""Dictionary match on the MI355X (needs -m gpu): saev_dictionary_match (fp16 filter with per-row bounds, exact fp32 refinement,
exact fp32 route) against an fp64 computation of max_j <a_i, b_j> / (||a_i|| ||b_j||) per row in the test itself, in row blocks.

Tolerance: test_gpu_coherence's tol(D) = (2 D + 6) 2^-24 -- (D + 2) 2^-24 for an fp32 dot product of unit rows plus
2 (D / 2 + 2) 2^-24 for the fp32 normalisation of the two rows.  Every value must be within it of the fp64 row maximum, and the
fp64 score of the pair returned within twice it (the pair's own error and the maximiser's).  Index EQUALITY with the fp64 argmax
is asserted only for rows whose fp64 gap between best and second best exceeds 4 tol(D): below that the fp32 order may
legitimately differ.  A test that asserts equality for every row first asserts that gap for its inputs.

The filter's tile is 128 rows of A x 128 rows of B with 64-wide k stages; the shapes are the smallest that reach each class.

On these inputs the fp16 images err by less than tol(D), or the planted ties are equal in fp64: the index a row returns never
depends on the filter's bound here.  The inputs on which it does -- small D, decoys a few tol apart that the images misorder --
and the bracket of the candidate count live in test_gpu_dictionary_geometry.py."""

import json
import pathlib
import subprocess
import sys

import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.encoder_modes("f32")]

DEV = "cuda:0"
ROOT = pathlib.Path(__file__).resolve().parents[1]
MODES = [pytest.param(False, id="signed"), pytest.param(True, id="absolute")]


def tol(D: int) -> float:
    return (2 * D + 6) * 2.0**-24


def match(A, B=None, **kw):
    from saev_amd.engine import dictionary_match

    return dictionary_match(A, B, **kw)


def randn(S, D, seed):
    return torch.randn(S, D, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))


def unit64(X: torch.Tensor) -> torch.Tensor:
    X64 = X.double()
    return X64 / X64.norm(dim=1, keepdim=True)


def fp64_rows(A: torch.Tensor, B: torch.Tensor | None, absolute: bool):
    """Per row of A in fp64: the best score, the second best (-inf if there is none) and the smallest j attaining the best."""
    An, Bn = unit64(A), unit64(A if B is None else B)
    Sa, Sb = An.shape[0], Bn.shape[0]
    best = torch.empty(Sa, dtype=torch.float64, device=A.device)
    second = torch.full((Sa,), float("-inf"), dtype=torch.float64, device=A.device)
    arg = torch.empty(Sa, dtype=torch.long, device=A.device)
    for lo in range(0, Sa, 2048):
        g = An[lo : lo + 2048] @ Bn.T
        if absolute:
            g = g.abs()
        rows = torch.arange(lo, lo + g.shape[0], device=A.device)
        if B is None:
            g[rows - lo, rows] = float("-inf")
        top = g.topk(min(2, Sb), dim=1)
        best[rows] = top.values[:, 0]
        if Sb >= 2:
            second[rows] = top.values[:, 1]
        arg[rows] = (g == top.values[:, :1]).int().argmax(dim=1)  # the first j among equals
    return best, second, arg


def fp64_scores(A, B, idx, absolute):
    An, Bn = unit64(A), unit64(A if B is None else B)
    s = (An * Bn[idx]).sum(dim=1)
    return s.abs() if absolute else s


def check(A, B, r, absolute, *, every_index=False, ref=None):
    """Every row's value and pair against fp64; index equality where the fp64 gap decides it (`every_index`: the inputs must make
    that every row)."""
    Sa, D = A.shape
    Sb = Sa if B is None else B.shape[0]
    best, second, arg = fp64_rows(A, B, absolute) if ref is None else ref
    assert r.values.shape == (Sa,) and r.values.dtype == torch.float32 and r.values.device == A.device
    assert r.indices.shape == (Sa,) and r.indices.dtype == torch.int32 and r.indices.device == A.device
    idx = r.indices.long()
    assert ((idx >= 0) & (idx < Sb)).all(), (int(idx.min()), int(idx.max()))
    if B is None:
        assert (idx != torch.arange(Sa, device=A.device)).all()
    err = (r.values.double() - best).abs().max().item()
    assert err <= tol(D), (err, tol(D))
    perr = (fp64_scores(A, B, idx, absolute) - best).abs().max().item()
    assert perr <= 2 * tol(D), (perr, 2 * tol(D))
    clear = best - second > 4 * tol(D)
    if every_index:
        assert clear.all(), int((~clear).sum())
    assert (idx[clear] == arg[clear]).all(), int((idx[clear] != arg[clear]).sum())
    return best, second, arg


def same_bits(r1, r2) -> bool:
    return torch.equal(r1.values.view(torch.int32), r2.values.view(torch.int32)) and torch.equal(r1.indices, r2.indices)


@pytest.mark.parametrize("absolute", MODES)
@pytest.mark.parametrize("shape", [(1, 1, 4), (1, 300, 16), (300, 1, 16), (37, 129, 64), (129, 37, 68), (257, 1000, 128),
                                   (1000, 4097, 256), (300, 200, 4096), (3000, 20000, 1280)])
def test_random_dictionaries(shape, absolute):
    Sa, Sb, D = shape
    A, B = randn(Sa, D, seed=Sa), randn(Sb, D, seed=Sb + 1)
    r = match(A, B, absolute=absolute)
    assert r.route == "filter" and not r.overflow and Sa <= r.candidates <= r.capacity, r
    check(A, B, r, absolute)
    assert abs(r.mmcs - r.values.double().mean().item()) == 0.0


def test_configs1_against_a_second_dictionary():
    A, B = randn(32768, 1024, seed=21), randn(32768, 1024, seed=22)
    r = match(A, B)
    assert r.route == "filter" and not r.overflow and 32768 <= r.candidates <= r.capacity, r
    assert r.tiles_refiltered <= 256 * 256
    check(A, B, r, False)


@pytest.mark.parametrize("absolute", MODES)
def test_self_mode_small(absolute):
    r = match(randn(1, 64, seed=30), absolute=absolute)
    assert r.values.tolist() == [0.0] and r.indices.tolist() == [-1] and r.candidates == 0, r
    W = randn(2, 16, seed=31)
    r = match(W, absolute=absolute)
    assert r.indices.tolist() == [1, 0], r
    check(W, None, r, absolute, every_index=True)


@pytest.mark.parametrize("absolute", MODES)
@pytest.mark.parametrize("shape", [(129, 64), (4097, 256)])
def test_self_mode_excludes_the_diagonal(shape, absolute):
    """(129, 64): the excluded diagonal crosses a tile edge (row 128 sits alone in tile (1, 1) with nothing admissible there)."""
    W = randn(*shape, seed=shape[0])
    r = match(W, absolute=absolute)
    assert r.route == "filter" and not r.overflow, r
    check(W, None, r, absolute)


def test_absolute_self_mode_contains_the_coherence():
    from saev_amd.engine import dictionary_coherence

    W = randn(4097, 256, seed=33)
    r, c = match(W, absolute=True), dictionary_coherence(W)
    top = r.values.max().item()
    assert abs(top - c.value) <= tol(256), (top, c)
    i = int(r.values.argmax())
    assert i in (c.i, c.j) and int(r.indices[i]) in (c.i, c.j) and int(r.indices[i]) != i, (i, int(r.indices[i]), c)
    check(W, None, r, True)


@pytest.mark.parametrize("absolute", MODES)
def test_planted_near_duplicate_is_the_match(absolute):
    A, B = randn(2000, 512, seed=40), randn(3000, 512, seed=41)
    B[2100] = 2.5 * A[1234] + 0.035 * randn(1, 512, seed=42)[0]
    r = match(A, B, absolute=absolute)
    assert int(r.indices[1234]) == 2100 and 0.9998 < r.values[1234].item() < 0.99999, (r.indices[1234], r.values[1234])
    check(A, B, r, absolute)


def test_planted_antiparallel_copy_matches_in_absolute_mode_only():
    A, B = randn(2000, 512, seed=43), randn(3000, 512, seed=44)
    B[2900] = -3.0 * A[17]
    r = match(A, B, absolute=True)
    assert int(r.indices[17]) == 2900 and abs(r.values[17].item() - 1.0) <= tol(512), (r.indices[17], r.values[17])
    check(A, B, r, True)
    r = match(A, B, absolute=False)
    assert int(r.indices[17]) != 2900 and r.values[17].item() < 0.5, (r.indices[17], r.values[17])
    check(A, B, r, False)


@pytest.mark.parametrize("absolute", MODES)
def test_rows_of_very_different_norms(absolute):
    A, B = randn(1000, 256, seed=45), randn(3000, 256, seed=46)
    g = torch.Generator(device=DEV).manual_seed(47)
    A = A * 10.0 ** (6 * torch.rand(1000, 1, device=DEV, generator=g) - 3)
    B = B * 10.0 ** (6 * torch.rand(3000, 1, device=DEV, generator=g) - 3)
    r = match(A, B, absolute=absolute)
    assert r.route == "filter", r
    check(A, B, r, absolute)


@pytest.mark.parametrize("absolute", MODES)
def test_a_row_permutation_gives_the_inverse_permutation(absolute):
    A = randn(3000, 256, seed=48)
    perm = torch.randperm(3000, device=DEV, generator=torch.Generator(device=DEV).manual_seed(49))
    B = A[perm].contiguous()
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(3000, device=DEV)
    r = match(A, B, absolute=absolute)
    check(A, B, r, absolute, every_index=True)
    assert torch.equal(r.indices.long(), inv)
    assert (r.values.double() - 1.0).abs().max().item() <= tol(256)


@pytest.mark.parametrize("absolute", MODES)
def test_near_ties_take_the_candidate_path_and_are_reproducible(absolute):
    """For 500 rows of A two rows of B at cosine 0.97 each (equal in fp64; in fp32 they differ by roundings, about 1e-7): both are
    candidates, the refinement decides, and two calls give bit-identical values and indices."""
    Sa, Sb, D, rho = 1000, 4097, 256, 0.97
    g = torch.Generator(device=DEV).manual_seed(50)
    A = unit64(torch.randn(Sa, D, device=DEV, generator=g, dtype=torch.float64))
    B = torch.randn(Sb, D, device=DEV, generator=g, dtype=torch.float64)
    a = A[:500]
    for k in range(2):
        o = torch.randn(500, D, device=DEV, generator=g, dtype=torch.float64)
        o = o - (o * a).sum(dim=1, keepdim=True) * a
        B[k:1000:2] = rho * a + (1 - rho * rho) ** 0.5 * o / o.norm(dim=1, keepdim=True)
    A, B = A.float(), B.float()
    r1, r2 = match(A, B, absolute=absolute), match(A, B, absolute=absolute)
    assert r1.route == "filter" and not r1.overflow and r1.candidates >= Sa + 500, r1
    assert same_bits(r1, r2) and r1.candidates == r2.candidates
    planted = torch.arange(500, device=DEV)
    assert (r1.indices[:500].long() // 2 == planted).all()
    assert (r1.values[:500].double() - rho).abs().max().item() <= tol(D)
    check(A, B, r1, absolute)


@pytest.mark.parametrize("self_mode", [False, True], ids=["pair", "self"])
def test_all_equal_cosines_overflow_to_the_exact_route(self_mode):
    """w_i = sqrt(rho) u + sqrt(1 - rho) e_i with orthonormal u, e_i: every pair has cosine rho and every pair qualifies.  The list
    holds min(Sa Sb, max(4096, 8 Sa)) pairs, so 65 rows against 65 (4 225 pairs; self mode: 4 160) are the smallest that overflow:
    the call answers on the exact route, says so, and returns what route="exact" returns, bit for bit -- the smallest admissible j
    that attains the maximum of that route's own values."""
    S, D, rho = 65, 132, 0.3
    q, _ = torch.linalg.qr(torch.randn(D, 2 * S + 1, generator=torch.Generator().manual_seed(7), dtype=torch.float64))
    W = (rho**0.5 * q[:, :1].T + (1 - rho) ** 0.5 * q[:, 1:].T).float().to(DEV)
    A, B = (W[:S].contiguous(), None) if self_mode else (W[:S].contiguous(), W[S:].contiguous())
    r = match(A, B)
    assert r.route == "exact" and r.overflow and r.candidates > r.capacity == 4096, r
    assert (r.values.double() - rho).abs().max().item() <= tol(D)
    check(A, B, r, False)
    e = match(A, B, route="exact")
    assert e.route == "exact" and not e.overflow and e.candidates == 0, e
    assert same_bits(r, e)
    # one row below the threshold nothing overflows
    A1, B1 = (A[:64].contiguous(), None) if self_mode else (A[:64].contiguous(), B[:64].contiguous())
    r = match(A1, B1)
    assert r.route == "filter" and not r.overflow and r.candidates == (64 * 63 if self_mode else 64 * 64), r
    check(A1, B1, r, False)


@pytest.mark.parametrize("absolute", MODES)
def test_exact_route_agrees_with_auto(absolute):
    A, B = randn(1000, 256, seed=60), randn(4097, 256, seed=61)
    auto, exact = match(A, B, absolute=absolute), match(A, B, absolute=absolute, route="exact")
    assert auto.route == "filter" and exact.route == "exact" and not exact.overflow
    assert (auto.values.double() - exact.values.double()).abs().max().item() <= 2 * tol(256)
    ref = check(A, B, auto, absolute)
    check(A, B, exact, absolute, ref=ref)
    clear = ref[0] - ref[1] > 4 * tol(256)
    assert clear.sum() > 900 and torch.equal(auto.indices[clear], exact.indices[clear])
    assert same_bits(exact, match(A, B, absolute=absolute, route="exact"))


@pytest.mark.parametrize("route", ["auto", "exact"])
def test_self_mode_exact_route(route):
    W = randn(300, 68, seed=62)
    check(W, None, match(W, route=route), False)


def nan_check(A, B, r, nan_rows, nan_index, absolute=False):
    """Rows in `nan_rows` are NaN with index `nan_index` (per row); the others are checked against fp64 as usual."""
    Sa = A.shape[0]
    isn = torch.zeros(Sa, dtype=torch.bool, device=DEV)
    isn[nan_rows] = True
    assert torch.equal(torch.isnan(r.values), isn), r.values
    assert r.indices[isn].tolist() == nan_index
    best, second, arg = fp64_rows(A, B, absolute)
    assert torch.equal(torch.isnan(best), isn)  # as torch's max propagates it
    ok = ~isn
    if ok.any():
        D = A.shape[1]
        assert (r.values.double()[ok] - best[ok]).abs().max().item() <= tol(D)
        idx = r.indices.long()
        s = fp64_scores(A, B, idx.clamp_min(0), absolute)
        assert (s[ok] - best[ok]).abs().max().item() <= 2 * tol(D)


@pytest.mark.parametrize("route", ["auto", "exact"])
@pytest.mark.parametrize("bad", [0.0, float("inf"), float("nan")], ids=["zero_row", "inf_entry", "nan_entry"])
def test_nan_rules(bad, route):
    def spoil(X, row):
        if bad == 0.0:
            X[row] = 0.0
        else:
            X[row, 3] = bad

    # a bad row in A: that row alone is NaN, with the smallest admissible j
    A, B = randn(100, 64, seed=70), randn(200, 64, seed=71)
    spoil(A, 37)
    nan_check(A, B, match(A, B, route=route), [37], [0])
    # a bad row in B at j0 (and a later one): every row is NaN with index j0
    A, B = randn(100, 64, seed=72), randn(200, 64, seed=73)
    spoil(B, 150)
    spoil(B, 180)
    nan_check(A, B, match(A, B, route=route, absolute=True), list(range(100)), [150] * 100, absolute=True)
    # self mode: row 0 is bad -- its smallest admissible j is 1, every other row meets it at j = 0
    W = randn(130, 64, seed=74)
    spoil(W, 0)
    nan_check(W, None, match(W, route=route), list(range(130)), [1] + [0] * 129)
    # self mode: row 129 is bad -- it takes j = 0, the others j = 129
    W = randn(130, 64, seed=75)
    spoil(W, 129)
    nan_check(W, None, match(W, route=route), list(range(130)), [129] * 129 + [0])


def test_match_saes_tool(tmp_path):
    from saev_amd import nn

    paths = []
    for k, d_sae in enumerate((256, 512)):
        torch.manual_seed(80 + k)
        sae = nn.SparseAutoencoder(nn.SparseAutoencoderConfig(d_model=32, d_sae=d_sae))
        with torch.no_grad():
            sae.W_dec.copy_(torch.randn(d_sae, 32))
            sae.W_enc.copy_(torch.randn(32, d_sae))
        paths.append(tmp_path / f"sae{k}.pt")
        nn.dump(paths[-1], sae)

    def run(*args):
        p = subprocess.run([sys.executable, str(ROOT / "tools" / "match_saes.py"), *map(str, args)], capture_output=True, text=True,
                           timeout=300)
        assert p.returncode == 0, p.stderr[-2000:]
        return json.loads(p.stdout.strip().splitlines()[-1])

    out = run(paths[0], paths[1], "--which", "W_enc", "--out", tmp_path / "m.pt")
    assert out["mode"] == "pair" and out["a"]["shape"] == [256, 32] and out["b"]["shape"] == [512, 32]
    assert 0 < out["mmcs_a_to_b"] < 1 and 0 < out["mmcs_b_to_a"] < 1 and 0 <= out["mutual_fraction"] <= 1
    assert len(out["closest"]) == 10 and len(out["farthest"]) == 10 and out["closest"][0][2] >= out["farthest"][0][2]
    saved = torch.load(tmp_path / "m.pt", weights_only=True)
    assert saved["values_a_to_b"].shape == (256,) and saved["indices_b_to_a"].shape == (512,)
    A = nn.load(paths[0]).W_enc.detach().T.contiguous().to(DEV)
    B = nn.load(paths[1]).W_enc.detach().T.contiguous().to(DEV)
    best, _, _ = fp64_rows(A, B, False)
    assert abs(out["mmcs_a_to_b"] - best.mean().item()) <= tol(32)
    out = run(paths[0], "--absolute")
    assert out["mode"] == "self" and out["absolute"] and 0 < out["mmcs"] < 1 and len(out["closest"]) == 10
