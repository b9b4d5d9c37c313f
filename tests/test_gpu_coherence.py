"""Dictionary coherence on the MI355X (needs -m gpu): saev_dictionary_coherence (fp16 filter, exact fp32 refinement, exact
fp32 route) against an fp64 computation of max_{i<j} |<w_i, w_j>| / (||w_i|| ||w_j||) in the test itself.

Tolerance: (D + 2) 2^-24 for an fp32 dot product of unit rows, plus 2 (D / 2 + 2) 2^-24 for the fp32 normalisation of the two
rows (the norm's fp32 sum and the division).  The value must be within it of the fp64 max; the fp64 coherence of the pair
returned within twice it (the pair's own error and the maximiser's).

On these inputs the fp16 images err by less than that tolerance, or the planted ties are equal in fp64: the pair returned never
depends on the filter's bound here.  The inputs on which it does -- small D, planted pairs a few tol apart that the images
misorder -- and the bracket of the candidate count live in test_gpu_dictionary_geometry.py."""

import struct
import types

import pytest
import torch

from conftest import load_golden

pytestmark = [pytest.mark.gpu, pytest.mark.encoder_modes("f32")]

DEV = "cuda:0"


def tol(D: int) -> float:
    return (2 * D + 6) * 2.0**-24


def fp64_max(W: torch.Tensor) -> float:
    W64 = W.double()
    Wn = W64 / W64.norm(dim=1, keepdim=True)
    S = Wn.shape[0]
    best = torch.zeros((), dtype=torch.float64, device=W.device)
    cols = torch.arange(S, device=W.device)[None, :]
    for lo in range(0, S, 2048):
        g = (Wn[lo : lo + 2048] @ Wn.T).abs()
        rows = torch.arange(lo, lo + g.shape[0], device=W.device)[:, None]
        best = torch.maximum(best, torch.where(cols > rows, g, torch.zeros((), dtype=g.dtype, device=g.device)).max())
    return best.item()


def fp64_pair(W: torch.Tensor, i: int, j: int) -> float:
    a, b = W[i].double(), W[j].double()
    return (a @ b / (a.norm() * b.norm())).abs().item()


def check(W: torch.Tensor, r, want: float | None = None):
    S, D = W.shape
    want = fp64_max(W) if want is None else want
    assert 0 <= r.i < r.j < S, r
    assert abs(r.value - want) <= tol(D), (r, want)
    assert abs(fp64_pair(W, r.i, r.j) - want) <= 2 * tol(D), (r, want, fp64_pair(W, r.i, r.j))


def coherence(W, **kw):
    from saev_amd.engine import dictionary_coherence

    return dictionary_coherence(W, **kw)


def randn(S, D, seed):
    return torch.randn(S, D, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))


@pytest.mark.parametrize("shape", [(2, 16), (37, 64), (1000, 128), (4097, 256), (20000, 1280), (3000, 4096), (32768, 1024)])
def test_random_dictionaries(shape):
    W = randn(*shape, seed=shape[0])
    r = coherence(W)
    assert r.route == "filter" and not r.overflow and 1 <= r.candidates <= r.capacity, r
    check(W, r)


def test_rows_of_very_different_norms():
    W = randn(3000, 256, seed=1)
    scale = 10.0 ** (6 * torch.rand(3000, 1, device=DEV, generator=torch.Generator(device=DEV).manual_seed(2)) - 3)
    W = W * scale
    r = coherence(W)
    assert r.route == "filter"
    check(W, r)


def test_planted_near_duplicate_is_found():
    W = randn(5000, 512, seed=3)
    W[3100] = 2.5 * W[1234] + 0.035 * randn(1, 512, seed=4)[0]
    want = fp64_pair(W, 1234, 3100)
    assert 0.9998 < want < 0.99999
    r = coherence(W)
    assert (r.i, r.j) == (1234, 3100), r
    check(W, r)


def test_planted_antiparallel_pair_is_found():
    W = randn(5000, 512, seed=5)
    W[4000] = -3.0 * W[17]
    r = coherence(W)
    assert (r.i, r.j) == (17, 4000), r
    check(W, r, want=1.0)


def test_near_ties_take_the_candidate_path_and_are_reproducible():
    """1 000 pairs planted at coherence 0.97 (equal in fp64; in fp32 they differ by roundings, about 1e-7): all of them are
    candidates, the refinement decides, and two calls give bit-identical value and pair."""
    S, D, rho = 4097, 256, 0.97
    g = torch.Generator(device=DEV).manual_seed(6)
    W = torch.randn(S, D, device=DEV, generator=g, dtype=torch.float64)
    a = W[0:2000:2] / W[0:2000:2].norm(dim=1, keepdim=True)
    o = torch.randn(1000, D, device=DEV, generator=g, dtype=torch.float64)
    o = o - (o * a).sum(dim=1, keepdim=True) * a
    o = o / o.norm(dim=1, keepdim=True)
    W[0:2000:2] = a
    W[1:2000:2] = rho * a + (1 - rho * rho) ** 0.5 * o
    W = W.float()
    r1, r2 = coherence(W), coherence(W)
    assert r1.route == "filter" and not r1.overflow and r1.candidates >= 1000, r1
    assert struct.pack("f", r1.value) == struct.pack("f", r2.value) and (r1.i, r1.j) == (r2.i, r2.j), (r1, r2)
    assert r1.i % 2 == 0 and r1.j == r1.i + 1 < 2000, r1
    check(W, r1)


def test_all_equal_coherences_overflow_to_the_exact_route():
    """w_i = sqrt(rho) u + sqrt(1 - rho) e_i with orthonormal u, e_i: every pair has coherence rho, 1 124 250 pairs qualify,
    more than the list holds -- the call answers on the exact route and says so."""
    S, D, rho = 1500, 2048, 0.3
    q, _ = torch.linalg.qr(torch.randn(D, S + 1, generator=torch.Generator().manual_seed(7), dtype=torch.float64))
    W = (rho**0.5 * q[:, :1].T + (1 - rho) ** 0.5 * q[:, 1:].T).float().to(DEV)
    r = coherence(W)
    assert r.route == "exact" and r.overflow and r.candidates > r.capacity, r
    check(W, r)
    assert abs(r.value - rho) <= tol(D)


def test_filter_route_ties_to_the_smallest_pair():
    """Four bit-identical rows among random ones: six pairs tie at the refined maximum, far below the list capacity, and the
    filter route returns the lexicographically smallest, with the value the refinement gives every one of them."""
    W = randn(3000, 256, seed=13)
    W[500] = W[900] = W[2100] = W[1700]
    r = coherence(W)
    assert r.route == "filter" and not r.overflow and 6 <= r.candidates < r.capacity, r
    assert (r.i, r.j) == (500, 900), r
    assert abs(r.value - 1.0) <= tol(256), r
    check(W, r)


def test_identical_rows_overflow_and_tie_to_the_first_pair():
    W = randn(1, 64, seed=8).expand(2048, 64).contiguous()
    r = coherence(W)
    assert r.route == "exact" and r.overflow, r
    assert (r.i, r.j) == (0, 1) and abs(r.value - 1.0) <= tol(64), r


@pytest.mark.parametrize("shape", [(5000, 384), (1000, 1024), (300, 4096)])
def test_exact_route_agrees_with_auto(shape):
    W = randn(*shape, seed=9)
    auto, exact = coherence(W), coherence(W, route="exact")
    assert auto.route == "filter" and exact.route == "exact" and not exact.overflow
    assert (auto.i, auto.j) == (exact.i, exact.j), (auto, exact)
    assert abs(auto.value - exact.value) <= 2 * tol(shape[1])
    check(W, exact)


def test_single_row_zero_row_and_nan():
    r = coherence(randn(1, 64, seed=10))
    assert r.value == 0.0 and (r.i, r.j) == (-1, -1)
    W = randn(100, 64, seed=11)
    W[37] = 0.0
    for route in ("auto", "exact"):
        r = coherence(W, route=route)
        assert r.value != r.value and (r.i, r.j) == (0, 37), r
    W = randn(100, 64, seed=12)
    W[5, 3] = float("nan")
    r = coherence(W)
    assert r.value != r.value and (r.i, r.j) == (0, 5), r
    ref = W / W.norm(dim=1, keepdim=True)
    assert torch.isnan((ref @ ref.T).abs().triu(1).max())


def test_decoder_metrics_match_the_torch_expression():
    from saev_amd.framework import train as T

    W = load_golden("g9_train_a")["init_W_dec"].to(DEV)
    got = T._decoder_metrics(types.SimpleNamespace(W_dec=W), types.SimpleNamespace(log_coherence=True))
    Wn = W / W.norm(dim=1, keepdim=True)
    want = (Wn @ Wn.T).abs().triu(1).max().item()
    assert abs(got["metrics/dictionary_coherence"] - want) <= tol(W.shape[1]), (got, want)
