"""Muon at ragged shapes, in every split-K class and under every hyper-parameter (needs -m gpu).  test_gpu_muon.py runs the
Newton-Schulz kernels at four shapes of 200 rows and more and the tail on whole 64 x 64 tiles with the defaults; here, at the
rows of tests/muon_restatement.py: CASES (one per class of gemm_splits / muon_layout, pinned by test_muon_restatement_host_cpu.py):

  1. the normalisation alone (ns_steps = 0), every element bit-equal to the fp64 emulation, on inputs whose bf16 norm the
     reference alone decides, and through the eps clamp;
  2. one iteration, with and without the normalisation, by the procedure and bounds of
     test_gpu_muon.py::test_one_iteration_every_element_within_one_ulp; reproducibility, a tall input, a 1 x 1 known answer;
  3. the tail at ragged (d_model, d_sae) as the composition of its pieces: torch's device lerp on the engine's own projected
     gradients, the standalone newton_schulz entry, and p * decay - adj_lr * O in fp64;
  4. every hyper-parameter setting of muon_restatement.CONFIGS against torch.optim.Muon on the device (G9 fixture);
  5. the refusal of d_model > d_sae.

Worst cases printed on the MI355X:

  1. normalisation: no element differs, at any case, heavy tile, scale or eps.
  2. one iteration, max |d| / bf16 ulp and unequal elements (cap = ceil(1e-4 numel)):
       case        normalize=False              normalize=True
       4x8         0      0 of 32       (1)     0      0 of 32       (1)
       36x260      0      0 of 9360     (1)     0      0 of 9360     (1)
       128x128     0      0 of 16384    (2)     0      0 of 16384    (2)
       132x132     0      0 of 17424    (2)     0      0 of 17424    (2)
       100x1250    1.000  2 of 125000   (13)    0      0 of 125000   (13)
       300x516     1.000  1 of 154800   (16)    1.000  1 of 154800   (16)
       200x5201    1.000  10 of 1040200 (105)   1.000  2 of 1040200  (105)
     (equal share 0.99998 or more everywhere: the project's figure of about 1e-5 unequal holds at these shapes too.)
  3. tail, worst |d| / fp32 ulp of the result (bound 1; the derivation gives a half, the final rounding): 0.500 for W_dec and
     W_enc at (36, 260) (the clipped step included), (132, 516) and (200, 1000) and with adjust_lr_fn "none"; ns_steps 0: 0.500,
     0.498; ns_steps 4: 0.500, 0.499.  The momentum is bit-equal to torch's lerp_ in every step.
  4. update rel err per setting, the larger of W_dec / W_enc over the two steps (bound NS_REL_TOL = 1e-2; in brackets torch's own
     device step against its CPU step on the same inputs): defaults 5.9e-3 (4.3e-3), momentum 0.3 5.2e-3 (5.3e-3), momentum 0
     5.2e-3 (6.3e-3), nesterov=False 6.6e-3 (7.1e-3), weight_decay 0.5 5.4e-3 (4.0e-3), weight_decay 0 5.8e-3 (5.2e-3),
     match_rms_adamw 6.0e-3 (5.0e-3), ns_steps 3 1.0e-3 (4.6e-4), ns_steps 0 exactly 0 (bound 1e-3).  No setting needed the
     fall-back to twice torch's own discrepancy.
"""

import math

import pytest
import torch

from muon_restatement import CASES, CONFIGS, adjusted_lr, layout, margin_input, muon_step_fp64, ulp_of
from test_gpu_muon import COEF, NS_REL_TOL, _engine, _segments, rel
from test_gpu_parity import make_engine, rand_params
from test_muon_host_cpu import bf16, ns_emulate

pytestmark = pytest.mark.gpu

CASE_IDS = [c.id for c in CASES]


def _ns(x, normalize=True, **kw):
    from saev_amd.engine import MuonConfig, newton_schulz

    return newton_schulz(x, MuonConfig(**kw), normalize=normalize)


# ------------------------------------------------------------------------------------------------
# 1. the normalisation alone
# ------------------------------------------------------------------------------------------------


def _assert_normalised(x, eps=1e-7, what=""):
    got = _ns(x.cuda(), ns_steps=0, eps=eps).cpu()
    want = ns_emulate(x, steps=0, eps=eps)
    assert got.dtype == torch.bfloat16 and got.shape == x.shape
    bad = got.double() != want
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.numel()} elements differ from the emulation, first at {bad.nonzero()[0].tolist()}"
    return got


@pytest.mark.encoder_modes("f32")
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_normalisation_is_bit_equal_to_the_emulation(case, encoder_mode):
    """X / clamp(bf16(||X||), eps), every element.  The kernel's norm -- doubles summed in a fixed order, an fp32 square root -- is
    within about 2^-23 of the fp64 one; margin_input puts the fp64 norm at least 2^-20 from a bf16 rounding boundary, so both
    round to the same bf16 norm and the fp32 division (correctly rounded) and its rounding to bf16 are the emulation's.  A
    partial sum dropped or read stale moves the norm by far more than an ulp of bf16 in at least one of the scales below."""
    x, seed = margin_input(case.shape, 1000 + case.rows)
    got = _assert_normalised(x, what=f"{case.id} seed {seed}")
    assert abs(got.double().norm().item() - 1.0) < 0.02  # (it did normalise)
    # one 64 x 64 tile of the element-wise pass 64 times heavier than the rest, so that its partial sum carries the norm: the
    # last (corner) tile, the middle one and, where there are more than 256, number 256 -- the strided loop's second round
    L = layout(*case.shape)
    gx = -(-case.cols // 64)
    for tile in sorted({L.nb - 1, L.nb // 2, min(256, L.nb - 1)}):
        def heavy(y, tile=tile):
            r0, c0 = tile // gx * 64, tile % gx * 64
            y[r0:r0 + 64, c0:c0 + 64] *= 64.0
            assert y[r0:r0 + 64, c0:c0 + 64].numel() > 0
            return y
        y, seed = margin_input(case.shape, 1100 + tile, edit=heavy)
        _assert_normalised(y, what=f"{case.id} heavy tile {tile} seed {seed}")


@pytest.mark.encoder_modes("f32")
@pytest.mark.parametrize("case", [CASES[1], CASES[6]], ids=[CASE_IDS[1], CASE_IDS[6]])
def test_normalisation_through_the_clamp_and_at_extreme_scales(case, encoder_mode):
    zero = _ns(torch.zeros(case.shape).cuda(), ns_steps=0).cpu()
    assert torch.equal(zero, torch.zeros(case.shape, dtype=torch.bfloat16)), "0 / eps is not 0"
    tiny, _ = margin_input(case.shape, 2000 + case.rows, scale=1e-12)
    assert tiny.bfloat16().double().norm().item() < 1e-7  # the clamp decides
    got = _assert_normalised(tiny, what=f"{case.id} 1e-12")
    assert got.double().abs().max().item() > 1e-6  # (divided by eps, not by the norm -- and not flushed)
    huge, _ = margin_input(case.shape, 3000 + case.rows, scale=1e12)
    _assert_normalised(huge, what=f"{case.id} 1e12")
    plain, _ = margin_input(case.shape, 4000 + case.rows, scale=5e-3 / math.sqrt(case.rows * case.cols))
    n = plain.bfloat16().double().norm().item()
    assert 1e-3 < n < 1e-2  # an ordinary gradient's norm, below eps = 1e-2: the clamp engages
    got = _assert_normalised(plain, eps=1e-2, what=f"{case.id} eps 1e-2")
    assert got.double().norm().item() < 0.99


# ------------------------------------------------------------------------------------------------
# 2. one iteration
# ------------------------------------------------------------------------------------------------


def _one_iteration(case, normalize):
    """test_one_iteration_every_element_within_one_ulp's procedure: the ulp is that of bf16 at the larger of the element and
    the magnitude of the terms that form it, |a X| + |U| |X|; the cap on unequal elements is ceil(1e-4 numel)."""
    a, b, c = COEF
    x, seed = margin_input(case.shape, 5000 + case.rows)
    X = x if normalize else (x / x.norm()).bfloat16()
    out = _ns(X.cuda(), normalize=normalize, ns_steps=1)
    got = out.cpu().double()
    Xd = ns_emulate(X.cuda().double(), steps=0, normalize=normalize)  # (the iteration's input: bf16(X), normalised or not)
    emu = ns_emulate(X.cuda().double(), steps=1, normalize=normalize).cpu()
    G = bf16(Xd @ Xd.T)
    U = bf16(c * (G @ G) + b * G)
    terms = ((a * Xd).abs() + U.abs() @ Xd.abs()).cpu()
    mag = torch.maximum(torch.maximum(got.abs(), emu.abs()), terms).clamp_min(1e-38)
    ulp = ulp_of(mag, 7)
    d = (got - emu).abs()
    unequal, cap = int((d != 0).sum()), math.ceil(1e-4 * d.numel())
    print(f"{case.id} normalize={normalize}: max |d| / ulp {(d / ulp).max().item():.3f}, equal {(d == 0).double().mean().item():.6f} "
          f"({unequal} unequal of {d.numel()}, cap {cap})")
    assert unequal <= cap, f"{unequal} elements differ from the emulation (cap {cap})"
    assert (d <= ulp).all(), f"{int((d > ulp).sum())} elements more than one bf16 ulp from the emulation"
    assert emu.abs().max().item() > 0
    return X, out


@pytest.mark.encoder_modes("f32")
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_one_iteration_without_normalisation(case, encoder_mode):
    _one_iteration(case, normalize=False)


@pytest.mark.encoder_modes("f32")
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_one_iteration_with_normalisation_and_twice_the_same(case, encoder_mode):
    X, out = _one_iteration(case, normalize=True)
    again = _ns(X.cuda(), normalize=True, ns_steps=1)
    assert torch.equal(out, again), "two calls on the same input differ"


@pytest.mark.encoder_modes("f32")
def test_tall_input_is_the_transpose_and_a_scalar_follows_the_polynomial(encoder_mode):
    x, _ = margin_input((100, 1250), 6000)
    wide = _ns(x.cuda())
    tall = _ns(x.t().contiguous().cuda())
    assert tall.shape == (1250, 100) and torch.equal(tall, wide.t())
    assert torch.equal(_ns(x.t().cuda()), wide.t())  # (a transposed view, not contiguous)
    # 1 x 1: 3 / bf16(3) = 1, then five times x <- bf16(a x + bf16(c g g + b g) x) with g = bf16(x x): no sum has two terms
    one = torch.tensor([[3.0]])
    want = ns_emulate(one)
    x_, (a, b, c) = 1.0, COEF
    r = lambda v: bf16(torch.tensor(v, dtype=torch.float64)).item()
    for _ in range(5):
        g = r(x_ * x_)
        u = r(c * (g * g) + b * g)
        x_ = r(a * x_ + u * x_)
    assert want.item() == x_ and 0.5 < x_ < 1.5
    got = _ns(one.cuda()).cpu().double()
    assert got.item() == want.item(), (got.item(), want.item())


# ------------------------------------------------------------------------------------------------
# 3. the tail is the composition of its pieces
# ------------------------------------------------------------------------------------------------

W_KEYS = ("W_dec", "W_enc")


def _tail_is_its_pieces(d, s, cfg_kw, schedule):
    """Steps of forward, dead, backward, muon_tail at (d_model, d_sae) = (d, s); schedule: (lr, max_norm) per step.  After each:
    the momentum segments of adam_m are torch's device lerp_ on the engine's own projected gradient (times the clip coefficient,
    formed from the tail's own sum of squares as the kernel forms it: the fp64 square root rounded to fp32), the adam_v segments
    of the matrices are untouched, and each matrix is fl32(before * decay) - adj_lr * O in fp64 (muon_step_fp64: before * decay
    rounded where torch's mul_ and the apply kernel round it) with O = newton_schulz(u), the standalone entry, on torch's device
    lerp u.  The tail and the entry run the same kernels on the same X with the same partial sums, so O is the tail's own: the
    tail may differ from the reference by the final fp32 rounding of its fused multiply-add only -- half an ulp; the bound is one
    fp32 ulp of the result."""
    from saev_amd.engine import MuonConfig, newton_schulz

    cfg = MuonConfig(**cfg_kw)
    n, k = 65, 4
    eng = make_engine(d, s, k, k_aux=0, max_batch=n, remove_parallel_grads=True)
    eng.load_params(rand_params(d, s, seed=d + s))
    gen = torch.Generator().manual_seed(d)
    for key in W_KEYS:  # (not zeros, so that "untouched" says something)
        eng.view(key, eng.adam_v).copy_(torch.rand(eng.shapes[key], generator=gen))
    worst = {key: 0.0 for key in W_KEYS}
    for step, (lr, max_norm) in enumerate(schedule):
        x = torch.randn(n, d, generator=gen).cuda()
        eng.step_forward(x, training=True, n_rows_global=n)
        eng.step_dead(n)
        eng.step_backward()
        before, m0, v0 = _segments(eng, eng.params), _segments(eng, eng.adam_m), _segments(eng, eng.adam_v)
        eng.muon_tail(lr, max_norm, muon=cfg)
        torch.cuda.synchronize()
        grads, mom, v1, after = _segments(eng, eng.grads), _segments(eng, eng.adam_m), _segments(eng, eng.adam_v), _segments(eng, eng.params)
        norm = torch.tensor(eng.sumsq.item(), dtype=torch.float64).sqrt().float()
        coef = torch.clamp(torch.tensor(max_norm, dtype=torch.float32) / (norm + 1e-6), max=1.0)
        assert (coef.item() == 1.0) == (max_norm >= 1.0), f"step {step}: clip coefficient {coef.item()} at max_norm {max_norm}"
        for key in W_KEYS:
            what = f"({d}, {s}) {cfg_kw} step {step} {key}"
            g = grads[key] * coef.cuda()
            m = m0[key].clone()
            want, u, O = muon_step_fp64(before[key], g, m, lr, cfg, ns=lambda u_: newton_schulz(u_, cfg))
            assert torch.equal(mom[key], m), f"{what}: momentum differs from torch's lerp_ in {int((mom[key] != m).sum())} elements"
            assert torch.equal(v1[key], v0[key]), f"{what}: adam_v written"
            assert O.shape == before[key].shape and O.dtype == torch.bfloat16
            ulp = ulp_of(want.abs(), 23)
            dd = (after[key].double() - want).abs()
            worst[key] = max(worst[key], (dd / ulp).max().item())
            moved = (after[key] - before[key]).abs().max().item()
            assert (dd <= ulp).all(), (f"{what}: {int((dd > ulp).sum())} elements more than one fp32 ulp from fl32(before * decay) - adj_lr * O, "
                                       f"worst {(dd / ulp).max().item():.3g} ulp at {(dd / ulp).argmax().item()}")
            assert moved > 0.1 * adjusted_lr(lr, cfg.adjust_lr_fn, before[key].shape) * O.float().abs().max().item() > 0
    print(f"tail ({d}, {s}) {cfg_kw}: worst |d| / fp32 ulp of the result " + ", ".join(f"{key} {v:.3f}" for key, v in worst.items()))
    eng.close()


@pytest.mark.encoder_modes("f32")
@pytest.mark.parametrize("d,s", [(36, 260), (132, 516), (200, 1000)])
def test_tail_is_the_composition_of_its_pieces(d, s, encoder_mode):
    schedule = [(1e-3, 1e9), (2e-3, 1e9), (3e-3, 1e9)]
    if (d, s) == (36, 260):
        schedule.append((2e-3, 1e-4))  # the clip active
    _tail_is_its_pieces(d, s, {}, schedule)


@pytest.mark.encoder_modes("f32")
@pytest.mark.parametrize("cfg_kw", [{"ns_steps": 0}, {"ns_steps": 4}, {"adjust_lr_fn": "none"}], ids=["ns_steps0", "ns_steps4", "adjust_none"])
def test_tail_with_no_iteration_an_even_count_and_the_plain_lr(cfg_kw, encoder_mode):
    """ns_steps 0: the result stays in workspace buffer 0, the normalised X itself; 4: the ping-pong ends in buffer 0;
    adjust_lr_fn "none": the third ratio, lr as it is -- a name torch.optim.Muon's constructor rejects (its _adjust_lr takes that
    branch for any other name), so it runs here, against the restatement, and not against torch.optim.Muon."""
    _tail_is_its_pieces(36, 260, cfg_kw, [(1e-3, 1e9), (2e-3, 1e9), (3e-3, 1e9)])


# ------------------------------------------------------------------------------------------------
# 4. every hyper-parameter against torch.optim.Muon on the device
# ------------------------------------------------------------------------------------------------


@pytest.mark.encoder_modes("f32")
@pytest.mark.parametrize("name", list(CONFIGS))
def test_every_hyper_parameter_matches_torch_muon(name, encoder_mode):
    """test_tail_step_matches_torch_muon_and_adam's procedure, two steps, under each setting: the momentum buffer bit-equal to
    torch's (both branches of lerp in both of its uses), the W updates to NS_REL_TOL -- or, should a setting exceed it, to twice
    what torch's own device step differs from torch's CPU step on the same inputs; ns_steps = 0 has no GEMM and is held to 1e-3.
    A wrong ratio, decay, step count or coefficient errs by 10 % or more."""
    from saev_amd.engine import MuonConfig

    kw = CONFIGS[name]
    cfg = MuonConfig(**kw)
    eng, batches, g = _engine()
    max_norm = 0.05
    W = {k: torch.nn.Parameter(eng.view(k).clone()) for k in W_KEYS}
    Wc = {k: torch.nn.Parameter(eng.view(k).cpu().clone()) for k in W_KEYS}
    muon = torch.optim.Muon([W[k] for k in W_KEYS], lr=0.0, **kw)
    muon_cpu = torch.optim.Muon([Wc[k] for k in W_KEYS], lr=0.0, **kw)
    for step, lr in enumerate((1e-3, 2e-3)):
        x = batches[step].cuda()
        eng.step_forward(x, training=True, n_rows_global=x.shape[0])
        eng.step_dead(x.shape[0])
        eng.step_backward()
        before = _segments(eng, eng.params)
        eng.muon_tail(lr, max_norm, muon=cfg)
        torch.cuda.synchronize()
        grads = _segments(eng, eng.grads)
        norm = torch.tensor(eng.sumsq.item(), dtype=torch.float64).sqrt().float()  # (as the kernel rounds it)
        coef = torch.clamp(torch.tensor(max_norm, dtype=torch.float32) / (norm + 1e-6), max=1.0)
        for opt, P, dev in ((muon, W, "cuda"), (muon_cpu, Wc, "cpu")):
            for k in W_KEYS:
                P[k].data.copy_(before[k])
                P[k].grad = (grads[k] * coef.cuda()).to(dev)
            opt.param_groups[0]["lr"] = lr
            opt.step()
        after, mom = _segments(eng, eng.params), _segments(eng, eng.adam_m)
        for k in W_KEYS:
            assert torch.equal(mom[k], muon.state[W[k]]["momentum_buffer"]), f"{name} step {step}: {k} momentum differs from torch's lerp_"
            upd_ours, upd_torch, upd_cpu = after[k] - before[k], W[k].data - before[k], Wc[k].data - before[k].cpu()
            e, disc = rel(upd_ours, upd_torch), rel(upd_torch.cpu(), upd_cpu)
            print(f"{name} step {step} {k}: update rel err {e:.3e} (torch device vs torch CPU {disc:.3e})")
            if cfg.ns_steps == 0:
                assert e <= 1e-3, (name, k, e)
            else:
                assert e <= NS_REL_TOL or e <= 2 * disc, (name, k, e, disc)
    eng.close()


# ------------------------------------------------------------------------------------------------
# 5. refusal
# ------------------------------------------------------------------------------------------------


@pytest.mark.encoder_modes("f32")
def test_muon_tail_refuses_d_model_above_d_sae_and_leaves_the_engine_usable(encoder_mode):
    from saev_amd._lib import SaevError

    d, s, n, k = 260, 132, 65, 4
    p = rand_params(d, s, seed=7)
    x = torch.randn(n, d, generator=torch.Generator().manual_seed(7)).cuda()
    engines = [make_engine(d, s, k, k_aux=0, max_batch=n, remove_parallel_grads=True) for _ in range(2)]
    for eng in engines:
        eng.load_params(p)
        eng.step_forward(x, training=True, n_rows_global=n)
        eng.step_dead(n)
        eng.step_backward()
    eng, twin = engines
    before, grads, m0 = eng.params.clone(), eng.grads.clone(), eng.adam_m.clone()
    assert torch.equal(twin.params, before) and torch.equal(twin.grads, grads)  # (two engines, the same bits: the tail is deterministic)
    with pytest.raises(SaevError, match="d_model > d_sae"):
        eng.muon_tail(1e-3, 1.0)
    torch.cuda.synchronize()
    assert torch.equal(eng.params, before) and torch.equal(eng.grads, grads) and torch.equal(eng.adam_m, m0)
    assert eng.scratch_bytes(3) == 0 and eng.adam_steps == 0  # (no workspace, and not counted as an optimizer step)
    # the Adam tail that follows is the one an engine that never asked for Muon takes
    eng.step_tail(1e-3, 1.0)
    twin.step_tail(1e-3, 1.0)
    torch.cuda.synchronize()
    assert not torch.equal(eng.params, before) and torch.isfinite(eng.params).all()
    for name in ("params", "adam_m", "adam_v"):  # the refused call returned before it touched anything: the same state, the same tail
        assert torch.equal(getattr(eng, name), getattr(twin, name)), f"{name} differs from the engine that never asked for Muon"
    for e_ in engines:
        e_.close()
