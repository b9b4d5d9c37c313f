"""What the bf16-encoder tests share (tests/test_gpu_bf16_geometry.py on the GPU, tests/test_bf16_cases_host_cpu.py without one): the
rounding of the operands, the exactness check of bf16 codes, and the shapes beyond tests/step_restatement.py: SHAPES.

The bf16 encoder contracts bf16-rounded x and W_enc (round to nearest even) with fp32 accumulation and adds the fp32 b_enc.  The
product of two bf16 numbers is exact in fp32, so against an fp64 product of the ROUNDED operands the kernel's only error is its
fp32 accumulation -- what tol_b of tests/topk_exactness.py bounds already.  No tolerance of its own."""

import torch

from topk_exactness import assert_topk_exact


def bf16r(t):
    """t rounded to bf16 (nearest even), in t's own dtype."""
    return t.to(torch.bfloat16).to(t.dtype)


def assert_bf16_codes_exact(x, idx, val, W_enc, b_enc, what=""):
    """assert_topk_exact on the rounded operands: values and cut of every row against the fp64 product of bf16r(x) and
    bf16r(W_enc), to tol_b.  Returns (worst value error, worst cut excess) / tol_b."""
    return assert_topk_exact(bf16r(x), idx, val, bf16r(W_enc), b_enc, what=what)


def assert_bf16_codes_exact_to_output_rounding(x, idx, val, W_enc, b_enc, what=""):
    """The same two properties where |b_enc| dwarfs the product (part D's second case: |x W_enc| ~ 1e-3 next to b_enc = 1).  tol_b
    bounds the error of the accumulated product and has no term for the rounding of (product + b_enc) to the fp32 it is stored
    as -- half an ulp, at most 2^-24 |h|, which there is twenty times tol_b: no fp32 output can meet tol_b alone.  Each value is
    held to tol_b + 2^-24 |h| of the fp64 pre-activation of the rounded operands at its latent, and nothing left out may exceed
    the smallest kept value by more than tol_b + 2^-24 |that value|.  Returns the two worst ratios to those bounds."""
    xr, Wr = bf16r(x), bf16r(W_enc)
    h = pre_activations(xr, Wr, b_enc)
    tol = tol_b(xr, Wr)
    got = h.gather(1, idx.long())
    err = (got - val.double()).abs() / (tol[:, None] + 2.0 ** -24 * got.abs())
    assert (err <= 1.0).all(), f"{what}value error {err.max().item():.2f} of tol_b + half an ulp"
    kth = val.min(dim=1).values.double()
    out = h.scatter(1, idx.long(), float("-inf")).amax(dim=1)
    over = (out - kth) / (tol + 2.0 ** -24 * out.abs())
    assert (over <= 1.0).all(), f"{what}a left-out pre-activation exceeds the smallest kept one by {over.max().item():.2f} of tol_b + half an ulp"
    return err.max().item(), over.max().item()


def tol_b(x, W_enc):
    """Per batch row, the tolerance of tests/topk_exactness.py: 8 * 2^-24 * ||x_b|| * max_s ||W_enc[:, s]||, in fp64."""
    return 8.0 * 2.0 ** -24 * x.double().norm(dim=1) * W_enc.double().norm(dim=0).max()


def pre_activations(x, W_enc, b_enc):
    """x W_enc + b_enc in fp64."""
    return x.double() @ W_enc.double() + b_enc.double()


def worst_value_error(x, idx, val, W_enc, b_enc):
    """The largest |val - h[idx]| / tol_b over all codes, h = the fp64 product of the operands AS GIVEN (nothing asserted): the
    negative control hands in the unrounded ones."""
    h = pre_activations(x, W_enc, b_enc)
    err = (h.gather(1, idx.long()) - val.double()).abs().amax(dim=1)
    return (err / tol_b(x, W_enc)).max().item()


# Part A beyond SHAPES: (n, d, s, k, factor on x).  What each reaches: tests/test_gpu_bf16_geometry.py.
EXTRA_CODE_SHAPES = (
    (2049, 64, 516, 8, 1.0),     # nine row blocks of 256: both branches of the encoder's XCD swizzle
    (257, 32, 260, 4, 1.0),      # nks = 1; a second row block that holds one row
    (65, 64, 260, 8, 1.0),       # nks = 2
    (65, 96, 260, 8, 1.0),       # nks = 3
    (300, 128, 1028, 16, 3e5),   # activation scales far from 1: bf16 has fp32's exponent range, the images carry no x scale
    (300, 128, 1028, 16, 1e-6),
)

# Part D with real weights: W_enc of rand_params scaled by this, b_enc = 1 except two strict maxima -- every pre-activation within
# ~1e-2 of 1; where the running bound is kept as a 16-bit key (top_k > 32) half of them pass it and the candidate lists overflow as
# they do for the exact ties.  (n, d, s, k of the tied case; the real-weights case picks its own k.)
OVERFLOW_SHAPE = (40, 32, 16384, 16)
OVERFLOW_W_SCALE = 1e-3

# Part E: (n, d, s, k) of the image hand-over.  The fused Adam leaves images where Dp == d_model and d_model % 32 == 0.
HANDOVER_SHAPES = (
    (65, 32, 36, 4),         # nks = 1, one partial latent tile
    (97, 256, 260, 33),      # the 64-group encoder (k > 32), nks = 8
    (130, 1280, 1028, 64),   # the benchmark's d_model at ragged d_sae, k = 64
    (130, 100, 1004, 8),     # d_model % 32 != 0: no hand-over; both engines split afresh on every step
)
LATE_CHECK_SHAPE = (256, 2048, 16, 512)  # (d, s, k, b) of tests/test_gpu_stream.py's staleness tests


def extra_inputs(n, d, s, k, x_scale):
    """(params, x) of an EXTRA_CODE_SHAPES row.  b_enc is scaled with x: the pre-activations then are those of the unscaled problem
    times the factor, and tol_b, which scales with ||x||, stays what a stored fp32 value can meet.  (Next to a b_enc of 0.05 an
    x of 1e-6 leaves h = b_enc to seven digits, and half an ulp of 0.1 is a thousand tol_b: tol_b has no term for the rounding
    of product + bias to fp32 and does not need one while |b_enc| <~ ||x|| ||w||.)"""
    from test_gpu_parity import rand_params  # (plain functions of a GPU test module: importing it needs no GPU)

    p = rand_params(d, s, seed=n + k)
    p["b_enc"] = p["b_enc"] * x_scale
    x = torch.randn(n, d, generator=torch.Generator().manual_seed(n + k + 1)) * x_scale
    return p, x


def overflow_inputs():
    """(params, x) of part D's second case."""
    from test_gpu_parity import rand_params

    n, d, s, k = OVERFLOW_SHAPE
    p = rand_params(d, s, seed=5)
    p["W_enc"] = p["W_enc"] * OVERFLOW_W_SCALE
    p["b_enc"] = torch.ones(s)
    p["b_enc"][7], p["b_enc"][9000] = 2.0, 3.0
    x = torch.randn(n, d, generator=torch.Generator().manual_seed(6))
    return p, x
