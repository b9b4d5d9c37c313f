"""The BatchTopK step-geometry table without a GPU (tests/step_restatement.py: BTK_SHAPES, used by tests/test_gpu_batch_topk_geometry.py):
every row's inputs meet the conditions under which fp32 and fp64 make the same BATCH-WIDE selection (this is where the seeds are
fixed), the batch rows have the recorded lengths -- empty ones next to rows of several hundred codes --, the fp32 restatement passes
the GPU test's own check against fp64 at a quarter of the row's bound ("Parity", keeps the printed ratios), and the checker
rejects planted errors of the kind a kernel makes that mishandles a padded slot, a second 64-slot chunk of a row or a partial tile."""

import functools

import pytest
import torch

import sae_ref as R
from step_restatement import (BOUND, BTK_SHAPES, BTK_SPREAD, MAX_PREFIXES, assert_grads_close, btk_default_row_cap, btk_input_conditions,
                              btk_row_inputs, restated_gradients)

ALPHA = 1 / 32
REJECTION_ROWS = [r for r in BTK_SHAPES if (r.d, r.s) in ((100, 1004), (96, 1000), (1536, 1000))]


@functools.lru_cache(maxsize=None)
def _reference(row):
    """(params, x, mask, dead, gap ratios, fp64 (mse, aux, gradients)) of a row, computed once."""
    p, x, toks = btk_row_inputs(row)
    mask, dead, gaps = btk_input_conditions(row, p["W_enc"], p["b_enc"], x, toks)
    return p, x, mask, dead, gaps, restated_gradients(p, x, mask, dead, row.prefixes, row.k_aux, ALPHA)


def _lengths(row):
    return _reference(row)[2].sum(dim=1)


def test_the_table_is_well_formed():
    assert len({r.id for r in BTK_SHAPES}) == len(BTK_SHAPES)
    assert len(REJECTION_ROWS) == 3
    for r in BTK_SHAPES:
        assert r.d % 4 == 0 and r.s % 4 == 0 and r.d <= 4096 and r.bound >= BOUND and r.spread == BTK_SPREAD and r.lengths is not None
        assert (r.n_dead > 0) == (r.k_aux > 0) == (r.aux_route != 0)
        if r.prefixes:
            assert len(r.prefixes) <= MAX_PREFIXES and r.prefixes[-1] == r.s and list(r.prefixes) == sorted(set(r.prefixes))
    assert any(r.prefixes and len(r.prefixes) == MAX_PREFIXES and r.prefixes[0] == 1 for r in BTK_SHAPES)
    # NV = ceil(d_model / 256) of the row kernels: 1, 2, 6, 7 (of 8), 8, 10 (of 12), 16, and ragged widths among them
    assert {(r.d + 255) // 256 for r in BTK_SHAPES} >= {1, 2, 6, 7, 8, 10, 16}
    assert any(r.d % 32 for r in BTK_SHAPES) and any(r.s % 256 and r.s > 1024 for r in BTK_SHAPES) and any(r.k >= r.s for r in BTK_SHAPES)
    assert any(r.n == 1 for r in BTK_SHAPES)
    # variable rows of every kind somewhere in the table
    assert any(r.lengths[2] > 0 for r in BTK_SHAPES), "no row with an empty batch row"
    assert any(r.lengths[1] > 64 for r in BTK_SHAPES) and any(r.lengths[1] > 128 for r in BTK_SHAPES) and any(r.lengths[1] > 1024 for r in BTK_SHAPES)
    assert any(r.lengths[1] > btk_default_row_cap(r) for r in BTK_SHAPES) and any(0 < r.lengths[1] <= btk_default_row_cap(r) < r.s for r in BTK_SHAPES)


@pytest.mark.parametrize("row", BTK_SHAPES, ids=lambda r: r.id)
def test_inputs_meet_the_selection_conditions(row):
    p, x, mask, dead, gaps, (mse, aux, ref) = _reference(row)
    nnz = _lengths(row)
    print(f"{row.id}: cut gap {gaps[0]:.1f} tol_b, smallest dead gap {gaps[1]:.1f} tol_b; row lengths {int(nnz.min())}..{int(nnz.max())}, "
          f"{int((nnz == 0).sum())} empty; default row_cap {btk_default_row_cap(row)}")
    assert int(mask.sum()) == row.n * min(row.k, row.s)
    assert (int(nnz.min()), int(nnz.max()), int((nnz == 0).sum())) == row.lengths
    assert (aux > 0) == (row.n_dead > 0) and mse > 0
    # the edges of d_model carry gradient: a kernel that dropped the last column could not hide behind a zero
    assert ref["W_dec"][:, -1].abs().max() > 0 and ref["b_dec"][-1] != 0 and ref["W_enc"][-1].abs().max() > 0
    if row.prefixes == (1, 7, 130, 1000):
        low = mask[:, :7].any(dim=1)
        assert int((nnz == 0).sum()) > 0 and int(((nnz > 0) & ~low).sum()) > 0, "an empty row and a row with no code below the second cut"
        assert low.any() and mask[:, 0].any()  # (and the first two blocks are not empty altogether)


@pytest.mark.parametrize("row", BTK_SHAPES, ids=lambda r: r.id)
def test_fp32_restatement_passes_its_own_check(row):
    p, x, mask, dead, _, (mse, aux, ref) = _reference(row)
    mse32, aux32, got = restated_gradients(p, x, mask, dead, row.prefixes, row.k_aux, ALPHA, dtype=torch.float32)
    ratios = assert_grads_close(got, ref, row.bound / 4, what=f"{row.id}: ")
    print(f"{row.id}: fp32 against fp64, worst |difference| / max|fp64|: " + "  ".join(f"{k} {v:.2e}" for k, v in ratios.items()))
    assert abs(mse32 - mse) <= 1e-5 * mse and abs(aux32 - aux) <= 1e-5 * aux + 1e-12


def _planted(row, kind):
    p, x, mask, dead, _, (_, _, ref) = _reference(row)
    nnz = mask.sum(dim=1)
    bad = {k: v.clone() for k, v in ref.items()}
    m = mask.clone()
    if kind == "pair_of_the_longest_row_removed":
        b = int(nnz.argmax())
        m[b, int(mask[b].nonzero()[-1])] = False
    elif kind == "pair_added_to_an_empty_row":  # a padded slot read as latent 0, or as whatever it held before
        b = int((nnz == 0).nonzero()[0])
        m[b, 0] = True
    elif kind == "65th_code_of_a_row_dropped":  # the first slot of a row's second 64-slot chunk
        b = int((nnz > 64).nonzero()[0])
        m[b, int(mask[b].nonzero()[64])] = False
    elif kind == "w_dec_last_columns":
        bad["W_dec"][:, -4:] = 0
        return bad
    elif kind == "b_enc_last_fired_doubled":  # (the last latent that fires: the very last one may stay silent in a batch-wide select)
        bad["b_enc"][int(mask.any(dim=0).nonzero()[-1])] *= 2
        return bad
    else:
        raise ValueError(kind)
    assert int((m != mask).sum()) == 1
    return restated_gradients(p, x, m, dead, row.prefixes, row.k_aux, ALPHA)[2]


@pytest.mark.parametrize("kind", ["pair_of_the_longest_row_removed", "pair_added_to_an_empty_row", "65th_code_of_a_row_dropped",
                                  "w_dec_last_columns", "b_enc_last_fired_doubled"])
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
    if kind == "b_enc_last_fired_doubled":
        assert n_off == 1  # one element of tens of thousands: any allowance for outliers lets this one through
