"""The dense ReLU train step away from unit scale, on the MI355X (needs -m gpu): the power-of-two scales that relu_pow2_kernel and
pow2_scale_kernel form on the device from the maxima of f, g, dH and x, at inputs where they are not the ones every other test
produces (cases and their input conditions in tests/relu_cases.py, measured on the CPU in tests/test_relu_cases_host_cpu.py):

  scale           x, b_enc and b_dec times 2^18 and 2^-20: the fp64 mask and its distance from zero, in bounds, are the base row's
  massive         one channel of x 300 times the rest (its W_enc row divided by 300): W_enc's gradient is held ROW BY ROW
  silent          no latent fires: f and dH are all zero and their scales fall back to 1; then a normal step on the same context
  zero_residual   and x = b_dec: g is zero too; nothing may become non-finite, not even in the tail

Tolerance: each case's ``bound`` (BOUND = 2e-5 of tests/step_restatement.py; the fp32 torch restatement of every case stays under a
quarter of it) through _step_and_check of tests/test_gpu_relu_train.py, against the fp64 restatement teacher-forced on the step's
own mask.  What must be zero is compared with zero.  Each test prints its worst ratios.

Observed on an MI355X, worst over the three encoder modes, |difference| / max|fp64|: scale 4.4e-7 per tensor and 9.1e-7 row by
row of W_enc's gradient (257x512x516 times 2^18); massive channel 4.5e-7 and 9.4e-7; the silent batch's b_dec gradient 9.7e-8, every
other gradient and both zero-residual steps exactly zero.  Without the `m > 0` fallback of relu_pow2_kernel the silent and the
zero-residual tests fail in every mode (tried).  What these tests found: the f16x3 encoder's images of x carried no scale, so at
65x36x260 times 2^18 x overflowed fp16 and the step's mask differed from fp64; a ReLU training context now scales them by the
power of two of max |x| (csrc/ctx_forward.hip: prepare_dense_scaled)."""

import math

import pytest
import torch

from relu_cases import SCALE_CASES, assert_rows_close, scale_case_inputs
from relu_step_restatement import relu_row_inputs
from test_gpu_relu_train import _step_and_check, rt_engine

pytestmark = pytest.mark.gpu


def _cases(*kinds):
    return pytest.mark.parametrize("case", [c for c in SCALE_CASES if c.kind in kinds], ids=lambda c: c.id)


def _engine(case, p):
    eng = rt_engine(case.base.d, case.base.s, case.base.n, l1=case.l1_coeff)
    eng.load_params(p)
    return eng


def _finite(eng, what):
    grads = {k: v.cpu() for k, v in eng.grad_views().items()}
    for k, v in grads.items():
        assert torch.isfinite(v).all(), f"{what}: {k}.grad holds a non-finite element"
    st = eng.read_stats()
    for k in ("mse", "aux", "l0", "l1", "grad_norm"):
        assert math.isfinite(getattr(st, k)), f"{what}: {k} = {getattr(st, k)}"
    return grads, st


@_cases("scale")
def test_any_activation_scale(case, encoder_mode):
    p, x = scale_case_inputs(case)
    eng = _engine(case, p)
    mask, ref = _step_and_check(eng, case.id, x.cuda(), case.bound, strict_mask=True)
    grads, _ = _finite(eng, case.id)
    by_row = assert_rows_close(grads["W_enc"], ref["W_enc"], case.bound, what=f"{case.id}: W_enc.grad ")
    print(f"{case.id} {encoder_mode}: W_enc.grad row by row, worst |difference| / the row's max|fp64| {by_row:.2e}")
    # the mask is the base row's: a power of two changes no comparison with zero
    p0, x0 = relu_row_inputs(case.base)
    assert torch.equal(mask, (x0.double() @ p0["W_enc"].double() + p0["b_enc"].double()) > 0)
    eng.step_tail(1e-3, 1.0)
    assert torch.isfinite(eng.params).all() and math.isfinite(eng.read_stats().grad_norm)


@_cases("massive")
def test_a_channel_far_larger_than_the_rest(case, encoder_mode):
    p, x = scale_case_inputs(case)
    eng = _engine(case, p)
    mask, ref = _step_and_check(eng, case.id, x.cuda(), case.bound, strict_mask=False)
    grads, _ = _finite(eng, case.id)
    by_row = assert_rows_close(grads["W_enc"], ref["W_enc"], case.bound, what=f"{case.id}: W_enc.grad ")
    print(f"{case.id} {encoder_mode}: W_enc.grad row by row, worst |difference| / the row's max|fp64| {by_row:.2e}")


@_cases("silent")
def test_a_batch_in_which_no_latent_fires(case, encoder_mode):
    p, x = scale_case_inputs(case)
    eng = _engine(case, p)
    mask, ref = _step_and_check(eng, case.id, x.cuda(), case.bound, strict_mask=True)
    grads, st = _finite(eng, case.id)
    assert not mask.any() and st.l0 == 0 and st.l1 == 0 and st.mse > 0
    _, _, x_hat, _ = eng.last_codes(case.base.n, row_nnz=True)
    assert torch.equal(x_hat.cpu(), p["b_dec"][None, :].expand(case.base.n, -1)), "x_hat of a row without a code is not b_dec"
    assert not grads["W_dec"].any() and not grads["W_enc"].any() and not grads["b_enc"].any()
    assert grads["b_dec"].abs().max() > 0  # (held to the restatement at the bound by _step_and_check)
    # the tail, then a normal step on the same context: the base row's biases back in place
    eng.step_tail(1e-3, 1.0)
    assert torch.isfinite(eng.params).all()
    p0, x0 = relu_row_inputs(case.base)
    eng.load_params(p0)
    mask, _ = _step_and_check(eng, f"{case.id}, then the base row", x0.cuda(), case.bound, strict_mask=True)
    assert mask.any()
    _finite(eng, f"{case.id}, then the base row")


@_cases("zero_residual")
def test_a_residual_that_is_exactly_zero(case, encoder_mode):
    """g = dL/dx_hat is zero in every element (seen through mse = 0 and a b_dec gradient, its column sums, of exact zeros), as are f
    and dH: all three device-side scales fall back to 1."""
    p, x = scale_case_inputs(case)
    eng = _engine(case, p)
    mask, ref = _step_and_check(eng, case.id, x.cuda(), case.bound, strict_mask=True)
    grads, st = _finite(eng, case.id)
    assert not mask.any() and st.l0 == 0 and st.l1 == 0 and st.mse == 0
    _, _, x_hat, _ = eng.last_codes(case.base.n, row_nnz=True)
    assert torch.equal(x_hat.cpu(), x)
    for k, v in grads.items():
        assert not v.any(), f"{k}.grad is not exactly zero"
    before = eng.params.clone()
    eng.step_tail(1e-3, 1.0)
    assert eng.read_stats().grad_norm == 0
    assert torch.isfinite(eng.params).all()
    moved = (eng.params - before).abs().max().item()
    print(f"{case.id} {encoder_mode}: the tail on zero gradients moved the parameters by at most {moved:.2e}")
