"""The step-geometry table without a GPU: every row's inputs meet the conditions under which fp32 and fp64 select alike (this is
where the seeds of tests/step_restatement.py: SHAPES are fixed), the fp32 restatement -- the CPU oracle's arithmetic -- passes the
GPU test's own check against fp64 at the row's bound with a factor 4 to spare (a different but equally valid fp32 summation
order and fma contraction; DESIGN.md, "Parity", keeps the printed ratios), and the checker rejects planted errors of the kind a
wrong last float4, an off-by-one tile bound or a dropped batch row would make."""

import functools

import pytest
import torch

import sae_ref as R
from step_restatement import BOUND, MAX_PREFIXES, SHAPES, assert_grads_close, input_conditions, restated_gradients, row_inputs

ALPHA = 1 / 32
REJECTION_ROWS = [r for r in SHAPES if (r.d, r.s) in ((36, 260), (1536, 1000)) or (r.d, r.s, r.prefixes is not None) == (96, 1000, True)]


@functools.lru_cache(maxsize=None)
def _reference(row):
    """(params, x, mask, dead, gap ratios, fp64 (mse, aux, gradients)) of a row, computed once."""
    p, x, toks = row_inputs(row)
    mask, dead, gaps = input_conditions(row, p["W_enc"], p["b_enc"], x, toks)
    return p, x, mask, dead, gaps, restated_gradients(p, x, mask, dead, row.prefixes, row.k_aux, ALPHA)


def test_the_table_is_well_formed():
    assert len({r.id for r in SHAPES}) == len(SHAPES)
    assert len(REJECTION_ROWS) == 3
    for r in SHAPES:
        assert r.d % 4 == 0 and r.s % 4 == 0 and r.d <= 4096 and r.bound >= BOUND
        assert (r.n_dead > 0) == (r.k_aux > 0) == (r.aux_route != 0)
        if r.prefixes:
            assert len(r.prefixes) <= MAX_PREFIXES and r.prefixes[-1] == r.s and list(r.prefixes) == sorted(set(r.prefixes))
    assert any(r.prefixes and len(r.prefixes) == MAX_PREFIXES and r.prefixes[0] == 1 for r in SHAPES)


@pytest.mark.parametrize("row", SHAPES, ids=lambda r: r.id)
def test_inputs_meet_the_selection_conditions(row):
    p, x, mask, dead, gaps, (mse, aux, ref) = _reference(row)
    print(f"{row.id}: smallest top-k gap {gaps[0]:.1f} tol_b, smallest dead gap {gaps[1]:.1f} tol_b")
    assert int(mask.sum()) == row.n * min(row.k, row.s)
    assert (aux > 0) == (row.n_dead > 0) and mse > 0
    # the edges carry gradient: a kernel that dropped the last latent or the last column could not hide behind a zero
    assert ref["b_enc"][-1] != 0 and ref["W_dec"][-1].abs().max() > 0 and ref["W_enc"][:, -1].abs().max() > 0
    assert ref["W_dec"][:, -1].abs().max() > 0 and ref["b_dec"][-1] != 0


@pytest.mark.parametrize("row", SHAPES, ids=lambda r: r.id)
def test_fp32_restatement_passes_its_own_check(row):
    p, x, mask, dead, _, (mse, aux, ref) = _reference(row)
    mse32, aux32, got = restated_gradients(p, x, mask, dead, row.prefixes, row.k_aux, ALPHA, dtype=torch.float32)
    ratios = assert_grads_close(got, ref, row.bound / 4, what=f"{row.id}: ")
    print(f"{row.id}: fp32 against fp64, worst |difference| / max|fp64|: " + "  ".join(f"{k} {v:.2e}" for k, v in ratios.items()))
    assert abs(mse32 - mse) <= 1e-5 * mse and abs(aux32 - aux) <= 1e-5 * aux + 1e-12


def _planted(row, kind):
    p, x, mask, dead, _, (_, _, ref) = _reference(row)
    bad = {k: v.clone() for k, v in ref.items()}
    if kind == "pair_removed":  # one (row, latent) pair of the last batch row missing from the mask
        m = mask.clone()
        m[-1, int(mask[-1].nonzero()[-1])] = False
        return restated_gradients(p, x, m, dead, row.prefixes, row.k_aux, ALPHA)[2]
    if kind == "w_dec_last_columns":
        bad["W_dec"][:, -4:] = 0
    elif kind == "w_enc_last_latents":
        bad["W_enc"][:, -4:] = 0
    elif kind == "b_enc_last_doubled":
        bad["b_enc"][-1] *= 2
    elif kind == "row_scaled":
        # The loss is a sum over batch rows given max |x|, n and the dead set, so the gradient without row r is the gradient of the
        # other rows' batch times (n - 1) / n, as long as max |x| stays where it was.  Row r's share, times 1e-3, is the planted error.
        r = row.n - 1
        keep = torch.arange(row.n) != r
        assert x[keep].abs().max() == x.abs().max()
        rest = restated_gradients(p, x[keep], mask[keep], dead, row.prefixes, row.k_aux, ALPHA)[2]
        for k in bad:
            bad[k] = ref[k] + 1e-3 * (ref[k] - rest[k] * (row.n - 1) / row.n)
    else:
        raise ValueError(kind)
    return bad


@pytest.mark.parametrize("kind", ["pair_removed", "w_dec_last_columns", "w_enc_last_latents", "b_enc_last_doubled", "row_scaled"])
@pytest.mark.parametrize("row", REJECTION_ROWS, ids=lambda r: r.id)
def test_the_checker_rejects_a_planted_error(row, kind):
    ref = _reference(row)[5][2]
    assert_grads_close(ref, ref, 0.0)  # (the reference itself passes, at any bound)
    bad = _planted(row, kind)
    n_off = sum(int(((bad[k] - ref[k]).abs() > row.bound * ref[k].abs().max()).sum()) for k in R.PARAM_ORDER)
    with pytest.raises(AssertionError, match=r"\.grad: flat index \d+ = \(row, column\)"):
        assert_grads_close(bad, ref, row.bound)
    total = sum(v.numel() for v in ref.values())
    print(f"{row.id} {kind}: {n_off} of {total} elements off")
    if kind == "b_enc_last_doubled":
        assert n_off == 1  # one element of tens of thousands: any allowance for outliers lets this one through
