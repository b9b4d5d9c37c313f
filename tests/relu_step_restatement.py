"""What the ReLU train-step tests share (tests/test_gpu_relu_train.py on the GPU, tests/test_relu_train_host_cpu.py without one):
a dense autograd restatement of mse + coeff * L1 on a GIVEN mask, the table of shapes of the dense step and the inputs of a row.

The restatement is teacher-forced like tests/step_restatement.py's: f = h * mask with the mask a caller hands in (the step's own
f > 0), so a pre-activation closer to zero than fp32 can tell never decides a comparison.  ``relu_input_conditions`` asserts that
fp32 and fp64 cannot disagree on the mask for a row's inputs: no |h| of the fp64 pre-activations within 2 x the fp32 bound
8 * 2^-24 * max_b ||x_b|| * max_s ||W_enc[:, s]|| + 2^-23 * max |b_enc| (the bound of tests/test_gpu_relu.py) of zero."""

import dataclasses

import torch

import sae_ref as R
from step_restatement import BOUND

SILENT_BIAS = -6.0  # b_enc of a latent that must never fire (the other terms of h are ~N(0, 1): tests/test_relu_train_host_cpu.py asserts it)
LOUD_BIAS = 6.0     # ... and of one that fires on every row
L1_COEFF = 1e-2


def relu_restated_gradients(params, x, mask, l1_coeff, dtype=torch.float64):
    """loss = rescaled MSE (mean over n D) + l1_coeff * mean_b sum_s f, with f = h * mask (df/dh = the mask), in ``dtype``.
    Returns (mse, l1, {name: gradient})."""
    leaves = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in params.items()}
    x = x.to(dtype)
    h = x @ leaves["W_enc"] + leaves["b_enc"]
    f = h * mask.to(dtype)
    x_hat = R.decode(f, leaves["W_dec"], leaves["b_dec"], None)[:, 0, :]
    mse = R.mean_squared_err(x_hat, x).mean()
    l1 = f.abs().sum(dim=1).mean(dim=0)
    (mse + l1 * l1_coeff).backward()
    return mse.item(), l1.item(), {k: v.grad for k, v in leaves.items()}


def relu_bound(x, W_enc, b_enc) -> float:
    """Two fp32 evaluations of any pre-activation of the batch differ by at most 2 of it."""
    return float(8.0 * 2.0 ** -24 * x.double().norm(dim=1).max() * W_enc.double().norm(dim=0).max() + 2.0 ** -23 * b_enc.double().abs().max())


def relu_input_conditions(W_enc, b_enc, x):
    """(fp64 mask h > 0, min |h| / bound): asserts that no fp64 pre-activation lies within 2 bounds of zero."""
    h = x.double() @ W_enc.double() + b_enc.double()
    ratio = float(h.abs().min()) / relu_bound(x, W_enc, b_enc)
    assert ratio > 2.0, f"a pre-activation lies {ratio:.2f} fp32 bounds from zero"
    return h > 0, ratio


@dataclasses.dataclass(frozen=True)
class ReluRow:
    n: int
    d: int
    s: int
    seed: int = 0           # fixed by tests/test_relu_train_host_cpu.py: the input condition holds at this seed
    bound: float = BOUND    # 2e-5, or 4 x the row's measured fp32-restatement error where that exceeds a quarter of it (none does)
    quiet_row: bool = False  # batch row 0 is the zero vector and every b_enc is negative: the row has no code, contributes nothing
    extremes: bool = False   # latent 1 never fires (b_enc = SILENT_BIAS), latent 2 fires on every row (b_enc = LOUD_BIAS)

    @property
    def id(self) -> str:
        return f"{self.n}x{self.d}x{self.s}" + ("-quiet" if self.quiet_row else "") + ("-extremes" if self.extremes else "")


# The classes of the dense ReLU step: the row tiles (256) and latent tiles (256) of the split-fp16 contraction kernel, the 16 x n_split
# padding of the batch axis in the split-K weight gradients (ksplit_shape: R x C tiles x n_split >= 256 or n_split = 16), the 64-row
# blocks of relu_dact_kernel's column sums, its 1024-column workgroups, one wave per row in relu_act_kernel / relu_mse_kernel.
# Sizes are the smallest that reach the class.  n_split is 16 in every row (tiles <= 15 at these sizes; it is 1 from 256 tiles on:
# tests/test_gpu_relu_train.py::test_one_split_of_the_weight_gradients reaches that); Kp is PADDED wherever n % 256 != 0: all rows but
# the last two.  (A batch SMALLER than the context's max_batch, whose k-major images are laid out for Kp(max_batch):
# tests/test_gpu_relu_train.py::test_a_smaller_batch_after_a_full_one_on_the_same_context.)
RELU_SHAPES = (
    # one row, K = n = 1 in the split-K batches (Kp = 256: 255 rows of padding), a single partial tile of everything
    ReluRow(1, 20, 36, seed=0),
    # a 65th row (a second column-sum block that holds one row); one 256-latent tile + 4
    ReluRow(65, 36, 260, seed=0, extremes=True),
    # a second 256-row tile, ragged everywhere; S = 1004 < 1024: relu_dact_kernel's last lanes idle
    ReluRow(300, 100, 1004, seed=12, quiet_row=True),
    # S = 1024 + 4: a second 1024-column workgroup of relu_dact_kernel that holds one float4; d_model = one full 256 tile
    ReluRow(130, 256, 1028, seed=0),
    # 257 rows: a second row tile that holds one row; d_model = two tiles
    ReluRow(257, 512, 516, seed=3),
    # d_model = five tiles: more than one float4 trip per lane in relu_mse_kernel (320 float4 per row)
    ReluRow(70, 1280, 516, seed=3),
    # the largest ragged width (Dp = 4096)
    ReluRow(34, 4092, 260, seed=0),
    # Kp = n = 256: no padding of the batch axis, one whole row tile, four whole column-sum blocks
    ReluRow(256, 36, 260, seed=3),
    # two whole row tiles, Kp = n = 512; everything else a single partial tile
    ReluRow(512, 20, 36, seed=0),
)


def relu_row_inputs(row: ReluRow):
    """(params, x): rand_params of tests/test_gpu_parity.py and a standard normal batch at the row's seed, with the row's extras."""
    from test_gpu_parity import rand_params  # (plain functions of a GPU test module: importing it needs no GPU)

    p = rand_params(row.d, row.s, seed=row.seed)
    x = torch.randn(row.n, row.d, generator=torch.Generator().manual_seed(row.seed + 1))
    if row.quiet_row:
        p["b_enc"] = -(0.05 + p["b_enc"].abs())
        x[0] = 0.0
    if row.extremes:
        p["b_enc"][1] = SILENT_BIAS
        p["b_enc"][2] = LOUD_BIAS
    return p, x
