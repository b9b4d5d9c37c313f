"""What the bf16 GPU tests (tests/test_gpu_bf16_geometry.py) rely on, fixed without a GPU.  On every row of
tests/step_restatement.py: SHAPES, with the mask being the fp64 top-k of the bf16 product:

  - the bf16 restatement (restated_gradients(bf16_codes=True)) evaluated in fp32 passes the GPU test's own check against its fp64
    evaluation at a quarter of the row's bound -- the margin tests/test_step_restatement_host_cpu.py holds the plain one to;
  - the tests discriminate: the plain restatement on the exact top-k -- a step that quietly ran another arithmetic -- lies more than
    four bounds away on every tensor, and on every batch row some selected bf16 pre-activation is more than 2 tol_b off the exact one;
  - the inputs keep their conditions under the rounding: no dead latent selected, the dead gap, gradient on the edges;
  - the checker rejects the exact-codes gradients at the row's bound, and a single doubled element of b_enc.grad."""

import functools

import pytest
import torch

import sae_ref as R
from bf16_cases import EXTRA_CODE_SHAPES, bf16r, extra_inputs, overflow_inputs, pre_activations, tol_b
from step_restatement import DEAD_THR, SHAPES, assert_grads_close, input_conditions, restated_gradients, row_inputs
from test_step_restatement_host_cpu import ALPHA, REJECTION_ROWS
from test_step_restatement_host_cpu import _reference as _plain_reference  # (the plain fp64 reference on the exact top-k, computed once per row)


@functools.lru_cache(maxsize=None)
def _reference(row):
    """(params, x, bf16 mask, dead mask, h unrounded, h of the rounded operands, fp64 (mse, aux, gradients)) of a row, once."""
    p, x, toks = row_inputs(row)
    h = pre_activations(x, p["W_enc"], p["b_enc"])
    h_bf = pre_activations(bf16r(x), bf16r(p["W_enc"]), p["b_enc"])
    k = min(row.k, row.s)
    mask = torch.zeros(row.n, row.s, dtype=torch.bool).scatter_(1, h_bf.topk(k, dim=1).indices, True)
    dead = toks >= DEAD_THR
    return p, x, mask, dead, h, h_bf, restated_gradients(p, x, mask, dead, row.prefixes, row.k_aux, ALPHA, bf16_codes=True)


def test_rounding_helper_is_round_to_nearest_even():
    one = torch.tensor([1.0, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, 1.0 + 3 * 2.0 ** -8, -(1.0 + 3 * 2.0 ** -8), 3e38, 1e-40])
    want = torch.tensor([1.0, 1.0, 1.0 + 2.0 ** -7, 1.0 + 2.0 ** -6, -(1.0 + 2.0 ** -6), 3e38, 1e-40])
    got = bf16r(one)
    assert got.dtype == one.dtype
    assert torch.equal(got[:5], want[:5])                     # ties to even, above a tie up, sign symmetric
    assert abs(got[5].item() - 3e38) <= 2.0 ** -8 * 3e38      # fp32's exponent range: no overflow where fp16 has long left
    assert abs(got[6].item() - 1e-40) <= 2.0 ** -133          # (a subnormal keeps 7 bits below 2^-126 -- or less)
    assert torch.equal(bf16r(one.double()), got.double())     # one rounding from fp64 too: fp32 -> fp64 is exact


def test_the_default_leaves_the_plain_restatement_alone():
    row = SHAPES[2]
    p, x, mask, dead, _, (mse, aux, ref) = _plain_reference(row)
    mse2, aux2, again = restated_gradients(p, x, mask, dead, row.prefixes, row.k_aux, ALPHA, bf16_codes=False)
    assert mse2 == mse and aux2 == aux and all(torch.equal(again[k], ref[k]) for k in R.PARAM_ORDER)


@pytest.mark.parametrize("row", SHAPES, ids=lambda r: r.id)
def test_fp32_bf16_restatement_passes_its_own_check(row):
    p, x, mask, dead, _, _, (mse, aux, ref) = _reference(row)
    mse32, aux32, got = restated_gradients(p, x, mask, dead, row.prefixes, row.k_aux, ALPHA, dtype=torch.float32, bf16_codes=True)
    ratios = assert_grads_close(got, ref, row.bound / 4, what=f"{row.id}: ")
    print(f"{row.id}: bf16 restatement, fp32 against fp64, worst |difference| / max|fp64|: " + "  ".join(f"{k} {v:.2e}" for k, v in ratios.items()))
    assert abs(mse32 - mse) <= 1e-5 * mse and abs(aux32 - aux) <= 1e-5 * aux + 1e-12


@pytest.mark.parametrize("row", SHAPES, ids=lambda r: r.id)
def test_the_bf16_reference_is_told_from_the_exact_one(row):
    p, x, mask, dead, h, h_bf, (mse, aux, ref) = _reference(row)
    exact = _plain_reference(row)
    exact_mask, plain = exact[2], exact[5][2]
    # gradients: a step on exact codes (another arithmetic, or the reference's plain formula) is far outside the bound, on every tensor
    apart = {}
    for name in R.PARAM_ORDER:
        apart[name] = ((plain[name] - ref[name]).abs().max() / ref[name].abs().max()).item()
        assert apart[name] > 4 * row.bound, f"{row.id}: {name}.grad on exact codes is only {apart[name]:.2e} of the largest element away"
    # codes: on every batch row some selected pre-activation moves by more than two tolerances under the rounding
    moved = ((h_bf - h).abs() * mask).amax(dim=1) / tol_b(x, p["W_enc"])
    assert (moved > 2.0).all(), f"{row.id}: batch row {int(moved.argmin())}: the selected bf16 pre-activations are within {moved.min().item():.2f} tol_b of the exact ones"
    flips = int((mask != exact_mask).sum()) // 2
    print(f"{row.id}: exact-codes gradients / max|bf16 fp64|: " + "  ".join(f"{k} {v:.2e}" for k, v in apart.items()) +
          f"; selected |h_bf - h| >= {moved.min().item():.0f} tol_b on every batch row; {flips} (row, latent) pairs differ from the exact top-k")


@pytest.mark.parametrize("row", SHAPES, ids=lambda r: r.id)
def test_inputs_keep_their_conditions_under_the_rounding(row):
    p, x, mask, dead, h, h_bf, (mse, aux, ref) = _reference(row)
    assert int(mask.sum()) == row.n * min(row.k, row.s)
    assert int(dead.sum()) == row.n_dead and not mask[:, dead].any(), f"{row.id}: a dead latent is among the bf16 top-k"
    # (the AuxK selection reads the unrounded h: its gap is the one input_conditions asserts)
    _, dead2, gaps = input_conditions(row, p["W_enc"], p["b_enc"], x, row_inputs(row)[2])
    assert torch.equal(dead, dead2) and (row.n_dead <= row.k_aux or gaps[1] > 2.0)
    assert (aux > 0) == (row.n_dead > 0) and mse > 0
    # the edges carry gradient: a kernel that dropped the last latent or the last column could not hide behind a zero
    assert ref["b_enc"][-1] != 0 and ref["W_dec"][-1].abs().max() > 0 and ref["W_enc"][:, -1].abs().max() > 0
    assert ref["W_dec"][:, -1].abs().max() > 0 and ref["b_dec"][-1] != 0
    # how close the bf16 selection itself comes to a tie (why the GPU test checks the cut, not set equality)
    k = min(row.k, row.s)
    if k < row.s:
        top = h_bf.topk(k + 1, dim=1).values
        gap = ((top[:, k - 1] - top[:, k]) / tol_b(bf16r(x), bf16r(p["W_enc"]))).min().item()
        print(f"{row.id}: smallest gap between the k-th and (k+1)-th bf16 pre-activation {gap:.2f} tol_b")


@pytest.mark.parametrize("kind", ["exact_codes", "b_enc_last_doubled"])
@pytest.mark.parametrize("row", REJECTION_ROWS, ids=lambda r: r.id)
def test_the_checker_rejects_another_arithmetic(row, kind):
    ref = _reference(row)[6][2]
    assert_grads_close(ref, ref, 0.0)  # (the reference itself passes, at any bound)
    if kind == "exact_codes":
        bad = _plain_reference(row)[5][2]
    else:
        bad = {k: v.clone() for k, v in ref.items()}
        bad["b_enc"][-1] *= 2
    n_off = sum(int(((bad[k] - ref[k]).abs() > row.bound * ref[k].abs().max()).sum()) for k in R.PARAM_ORDER)
    with pytest.raises(AssertionError, match=r"\.grad: flat index \d+ = \(row, column\)"):
        assert_grads_close(bad, ref, row.bound)
    print(f"{row.id} {kind}: {n_off} of {sum(v.numel() for v in ref.values())} elements off")
    if kind == "b_enc_last_doubled":
        assert n_off == 1


@pytest.mark.parametrize("shape", EXTRA_CODE_SHAPES + ("overflow",), ids=str)
def test_extra_shapes_are_told_from_the_exact_product(shape):
    """The GPU test's negative control asserts more than 2 tol_b between the kernel's values and the UNROUNDED product; the kernel's
    own error is at most 1, so the rounded and the unrounded product must lie more than 3 apart on some selected entry."""
    (p, x), k = (overflow_inputs(), 64) if shape == "overflow" else (extra_inputs(*shape), shape[3])
    h = pre_activations(x, p["W_enc"], p["b_enc"])
    h_bf = pre_activations(bf16r(x), bf16r(p["W_enc"]), p["b_enc"])
    sel = h_bf.topk(k, dim=1).indices
    worst = ((h_bf - h).gather(1, sel).abs().amax(dim=1) / tol_b(x, p["W_enc"])).max().item()
    print(f"{shape}: largest selected |h_bf - h| {worst:.0f} tol_b")
    assert worst > 3.0
