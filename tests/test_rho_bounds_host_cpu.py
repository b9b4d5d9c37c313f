"""The fp64 reference of tests/test_gpu_rho_bounds.py::test_failed_norm_prediction_is_repeated has no ties at the cut: for the
seeds in use, every row's k-th and (k + 1)-th largest pre-activation are further apart than fp32 arithmetic can move them, so the
GPU test may compare index sets without exclusions."""

import pytest
import torch

import rho_bounds_cases as C


@pytest.mark.parametrize("seed", C.FAIL_SEEDS)
def test_failing_batch_has_no_ties_at_the_cut(seed):
    p, warm, bad, after = C.failing_case(seed)
    wmax = p["W_enc"].norm(dim=0).max().item()
    bmax = p["b_enc"].abs().max().item()
    for name, x in (("failing batch", bad), ("batch after", after)):
        top = C.fp64_reference(p, x, C.K).values
        gap = top[:, C.K - 1] - top[:, C.K]
        # the rounding errors of an fp32 dot product of D terms add up like a random walk: sqrt(D) 2^-24 ||x|| ||w|| is its standard
        # size (the worst case, D 2^-24 ||x|| ||w||, is never met, and no seed keeps 1 024 rows of 4 096 latents that far apart:
        # the pre-activations near the cut are ~0.016 apart on average); twice that, plus the rounding of the bias add
        room = 2.0 * C.D**0.5 * 2.0**-24 * x.norm(dim=1) * wmax + 2.0**-23 * bmax
        worst = (gap / room.double()).min().item()
        print(f"seed {seed}, {name}: smallest gap / room = {worst:.3g}")
        assert (gap > room.double()).all(), f"{name}: a tie at the cut (gap / room {worst:.3g}); choose another seed"
