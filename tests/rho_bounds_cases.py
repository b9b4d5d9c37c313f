"""Inputs of tests/test_gpu_rho_bounds.py that a CPU test can look at too (tests/test_rho_bounds_host_cpu.py): parameters and
batches come from CPU generators, so the fp64 reference of the failing batch is the same object on both sides."""

import math

import torch

D, S, K, N = 256, 4096, 32, 512
FAIL_SEEDS = (27, 31)  # (no near-ties at the cut of the fp64 reference: tests/test_rho_bounds_host_cpu.py)
BIG, TINY = 1000.0, 1e-3
N_BIG = 4  # rows at 1 000 x the batch scale -- in EVERY batch of the failing case, so that the x scale of the streamed step fits them


def params(d, s, seed):
    g = torch.Generator().manual_seed(seed)
    W = (torch.rand(s, d, generator=g) * 2 - 1) * math.sqrt(6.0 / d)
    W /= W.norm(dim=1, keepdim=True)
    return {"W_dec": W, "W_enc": (W.t() + 0.01 * torch.randn(d, s, generator=g)).contiguous(),
            "b_enc": 0.05 * torch.randn(s, generator=g), "b_dec": 0.05 * torch.randn(d, generator=g)}


def mean_batches(d, n, count, seed):
    """x = z + mu, the benchmark's headline data."""
    g = torch.Generator().manual_seed(seed)
    mu = torch.randn(d, generator=g)
    return [torch.randn(n, d, generator=g) + mu for _ in range(count)]


def lowrank_batches(d, n, count, seed):
    """x = A s + 0.1 eps, A (4 d x d) with unit rows, s 16-sparse with exp(1) magnitudes (bench.py: synthetic_pool "lowrank")."""
    g = torch.Generator().manual_seed(seed)
    A = torch.randn(4 * d, d, generator=g)
    A /= A.norm(dim=1, keepdim=True)
    out = []
    for _ in range(count):
        idx = torch.randint(0, 4 * d, (n, 16), generator=g)
        mag = -torch.log(torch.rand(n, 16, generator=g).clamp_min(1e-12))
        out.append(torch.einsum("nk,nkd->nd", mag, A[idx]) + 0.1 * torch.randn(n, d, generator=g))
    return out


def failing_case(seed):
    """(params, warm-up batches, failing batch, the batch after).  Every batch is x = z + mu with its first N_BIG rows at 1 000 x
    that scale.  The failing batch also holds four rows that are exact multiples of decoder directions, four rows at 1e-3 x the
    batch scale and one all-zero row: their k-th largest pre-activation is (nearly) that of the biases alone, far below
    rho_lo * ||x_b - mu|| -- the prediction must fail for them."""
    p = params(D, S, seed)
    g = torch.Generator().manual_seed(1000 + seed)
    mu = torch.randn(D, generator=g)

    def batch():
        x = torch.randn(N, D, generator=g) + mu
        x[:N_BIG] *= BIG
        return x

    warm = [batch() for _ in range(4)]
    bad = batch()
    for j in range(4):
        bad[8 + j] = (2.0 + j) * p["W_dec"][37 * (j + 1)]
        bad[16 + j] *= TINY
    bad[24] = 0.0
    return p, warm, bad, batch()


def fp64_reference(p, x, k):
    """Sorted pre-activations' top k + 1 in fp64: values (n, k + 1) and indices."""
    h = x.double() @ p["W_enc"].double() + p["b_enc"].double()
    return torch.topk(h, k + 1, dim=1)
