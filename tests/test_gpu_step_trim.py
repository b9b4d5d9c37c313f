"""saev_train_step against the four phase entry points, bit for bit.

The fused step leaves out work only it can do without: its plain decode writes no row-major dL/dx_hat (the column sums of db_dec
read the slice-major copy), and its predicated dense fallback is launched as a short grid that walks the rows.  The phases keep
the row-major g and the full grids.  Both run the same arithmetic in the same order, so from identical state they must leave
identical parameters, Adam moments, codes, statistics and db_dec.

The phased tail is the trusted one (it takes the decoder rows' projection from the statistics the backward left, as the fused Adam
does), and max_norm is far above the gradient norm: the clip coefficient is exactly 1 on both sides, so that the two clip norms --
sums of the same squares grouped differently -- cannot enter the parameters."""

import math

import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.encoder_modes("f16r")]  # the slice routes and the streamed step belong to the f16r encoder

LR, NO_CLIP = 1e-3, 1e6
# (every field of the step's statistics but cand_max, the longest candidate list: the fused encoder's row bounds tighten with whatever
# the row's other latent ranges have published so far -- a race by design, any outcome a valid bound -- so the lists' lengths differ
# between two runs of the same entry point already; the codes selected from them do not)
STATS = ("mse", "l0", "l1", "aux", "grad_norm", "n_dead", "dense_route", "n_overflow_rows", "sse", "sum_sq", "upper")


def _engine(d, s, k, b, seed, **kw):
    from saev_amd.engine import EngineConfig, SaeEngine

    eng = SaeEngine(EngineConfig(d_model=d, d_sae=s, top_k=k, max_batch=b, k_aux=0, **kw))
    g = torch.Generator(device="cuda").manual_seed(seed)
    W = (torch.rand(s, d, device="cuda", generator=g) * 2 - 1) * math.sqrt(6.0 / d)
    W /= W.norm(dim=1, keepdim=True)
    eng.view("W_dec").copy_(W)
    eng.view("W_enc").copy_(W.t() + 0.01 * torch.randn(d, s, device="cuda", generator=g))
    eng.view("b_enc").copy_(0.05 * torch.randn(s, device="cuda", generator=g))
    eng.view("b_dec").copy_(0.05 * torch.randn(d, device="cuda", generator=g))
    return eng


def _batches(d, n, count, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    mu = torch.randn(d, device="cuda", generator=g)
    return mu, [torch.randn(n, d, device="cuda", generator=g) + mu for _ in range(count)]


def _fused(eng, x):
    eng.train_step(x, LR, NO_CLIP)
    return eng.view("b_dec", eng.grads).clone()


def _phases(eng, x):
    n = x.shape[0]
    eng.step_forward(x, training=True)
    eng.step_dead(n)
    eng.step_backward()
    db_dec = eng.view("b_dec", eng.grads).clone()
    eng.step_tail(LR, NO_CLIP, trusted=True)
    return db_dec


def _assert_same_step(fused, phased, xs, what):
    """The same batches through saev_train_step and through the phases, compared after every step (the first step prepares its
    operands in full on both sides; from the second on the fused side streams them)."""
    for i, x in enumerate(xs):
        n = x.shape[0]
        db_f, db_p = _fused(fused, x), _phases(phased, x)
        sf, sp = fused.read_stats(), phased.read_stats()
        print(f"{what} step {i}: grad_norm {sf.grad_norm!r} / {sp.grad_norm!r}  mse {sf.mse!r} / {sp.mse!r}  "
              f"db_dec differs in {(db_f != db_p).sum().item()} of {db_f.numel()}")
        assert torch.equal(db_f, db_p), f"{what} step {i}: db_dec differs in {(db_f != db_p).sum().item()} of {db_f.numel()} columns"
        (if_, vf, xf), (ip, vp, xp) = fused.last_codes(n), phased.last_codes(n)
        assert torch.equal(if_, ip) and torch.equal(vf, vp), f"{what} step {i}: codes differ"
        assert torch.equal(xf, xp), f"{what} step {i}: x_hat differs"
        for name in STATS:
            a, b = getattr(sf, name), getattr(sp, name)
            assert a == b, f"{what} step {i}: read_stats().{name} {a!r} != {b!r}"
        assert sf.grad_norm < NO_CLIP and sf.dense_route == 0
        for name in ("params", "adam_m", "adam_v"):
            a, b = getattr(fused, name), getattr(phased, name)
            assert torch.equal(a, b), f"{what} step {i}: {name} differ in {(a != b).sum().item()} elements"
        assert torch.equal(fused.toks_since_active, phased.toks_since_active)


@pytest.mark.parametrize("d", [256, 1024])
@pytest.mark.parametrize("n", [1, 257])
def test_db_dec_from_the_slice_major_gradient(d, n):
    """The column sums of dL/dx_hat with one partial (1 row) and with a ragged last block of 64 rows (257 rows), at one and at
    four float4 columns per thread of the partial sums."""
    s, k = 2048, 32
    engs = [_engine(d, s, k, n, seed=11) for _ in range(2)]
    _, xs = _batches(d, n, 3, seed=12)
    _assert_same_step(*engs, xs, f"d_model {d}, {n} rows")
    for e in engs:
        e.close()


@pytest.mark.parametrize("prefixes", [None, (512, 1024, 2048)], ids=["plain", "matryoshka3"])
def test_a_latent_that_fires_on_every_row(prefixes):
    """300 rows, d_sae 2 048, k = 32: 9 600 pairs in runs of the slice kernels, and latent 0 -- its W_enc column points along the
    batch mean -- in every row's codes, so that its pair list is cut by run boundaries and has head and tail partials."""
    d, s, k, n = 256, 2048, 32, 300
    engs = [_engine(d, s, k, n, seed=21) for _ in range(2)]
    mu, xs = _batches(d, n, 3, seed=22)
    for e in engs:
        e.view("W_enc")[:, 0] = 4.0 * mu / mu.norm()
        if prefixes is not None:
            e.set_prefixes(prefixes)
    _assert_same_step(*engs, xs, f"prefixes {prefixes}")
    idx, _, _ = engs[0].last_codes(n)
    assert (idx == 0).any(dim=1).all(), "latent 0 is meant to be in every row's codes"
    for e in engs:
        e.close()


@pytest.mark.parametrize("n", [64, 1100])
def test_the_armed_fallback_walks_every_row(n):
    """64 rows (one workgroup per row still) and 1 100 rows (the first 76 workgroups of the 1 024 take a second row) at d_sae 512,
    k = 32.  The third batch is 1e4 times the second: the streamed images, scaled with the previous batch's
    maximum, leave fp16's range and the step takes the exact dense route IN THAT STEP -- through the short walking grid.  Its codes
    must be those of saev_encode_dense + saev_topk_dense on the same rows with the parameters the step started from; the step
    after it (a batch of the same size as the large one) is back on the fused route."""
    d, s, k = 256, 512, 32
    eng = _engine(d, s, k, n, seed=31)
    twin = _engine(d, s, k, n, seed=32)
    _, xs = _batches(d, n, 4, seed=33)
    xs[2] = xs[2] * 1e4
    xs[3] = xs[3] * 1e4
    routes = []
    for i, x in enumerate(xs):
        if i == 2:
            twin.load_params({name: eng.view(name).clone() for name in ("W_dec", "b_dec", "W_enc", "b_enc")})
            idx_ref, val_ref = twin.topk_dense(twin.encode_dense(x), k)
        eng.train_step(x, 1e-4, 1.0)
        routes.append(eng.read_stats().dense_route)
        if i == 2:
            idx, val, _ = eng.last_codes(n)
            order = idx_ref.argsort(dim=1)  # (both emit ascending latents; sorted anyway, so that the comparison does not rest on it)
            idx_ref, val_ref = idx_ref.gather(1, order), val_ref.gather(1, order)
            assert torch.equal(idx, idx_ref.to(idx.dtype)), f"{(idx != idx_ref).sum().item()} codes name another latent"
            assert torch.equal(val, val_ref), f"{(val != val_ref).sum().item()} code values differ"
    print("dense_route per step:", routes)
    assert routes[2] == 1, routes
    assert routes[3] == 0, routes
    eng.close()
    twin.close()
