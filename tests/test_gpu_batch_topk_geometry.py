"""The BatchTopK train step in the dispatch classes of its shape (needs -m gpu).  A BatchTopK context sizes by row_cap what a TopK context
sizes by top_k, and hands padded rows of variable length -- idx = -1, val = 0 past row_nnz -- to the generic downstream kernels
(decode_kernel / decode_matry_kernel, the CSC build, gather_rows_accum, dw_rows, AuxK).  Every other gradient, loss or trajectory
assertion of BatchTopK sits at fixture G20's one shape (d_model 64, d_sae 256: NV = 1, one tile, one scan block).  Here, at every row
of tests/step_restatement.py: BTK_SHAPES ("Parity": the BatchTopK class table), whose batch rows are scaled so that the
batch-wide select leaves empty rows next to rows of several hundred codes:

  A. one training step from the DEFAULT row_cap: the automatic regrow where the table says the longest row needs it, the form of the
     codes, the selection against the fp64 batch-wide top-(n k) as a SET (the input conditions of
     tests/test_batch_topk_restatement_host_cpu.py leave no freedom), values, tracker, AuxK route, threshold and losses, the four
     gradients against the fp64 restatement on that selection, EVERY element within row.bound of its tensor's largest, and then the
     eval-mode forward of the same batch against {h > threshold};
  B. on three rows the tail -- projection, active clip, Adam, renormalisation -- at the procedure and tolerances of
     tests/test_gpu_step_geometry.py::test_tail_at_every_row_kernel_width, and one more fused step whose selection is again the fp64
     one for the parameters it started from.

SAEV_AMD_DW is not varied: a BatchTopK context has no column slices, so both settings run the same code."""

import math

import pytest
import torch

import sae_ref as R
from step_restatement import (BTK_SHAPES, DEAD_THR, assert_grads_close, btk_default_row_cap, btk_input_conditions, btk_row_inputs, btk_tol,
                              restated_gradients)
from test_gpu_batch_topk import btk_engine, check_form, rows_to_dense

pytestmark = pytest.mark.gpu

ALPHA = 1 / 32
M = 0.1  # EngineConfig.batch_momentum

_REFERENCES = {}  # row.id -> (W_dec as the step normalised it, (mask, dead, h in fp64, (mse, aux, gradients))): computed once per row


def _reference(row, params, x, toks):
    """The fp64 batch-wide selection and the fp64 restatement on it with the step's own (renormalised) W_dec -- shared by the encoder
    modes of a row as long as they hand in the same parameters."""
    hit = _REFERENCES.get(row.id)
    if hit is not None and torch.equal(hit[0], params["W_dec"]):
        return hit[1]
    mask, dead, _ = btk_input_conditions(row, params["W_enc"], params["b_enc"], x, toks)
    h = x.double() @ params["W_enc"].double() + params["b_enc"].double()
    out = (mask, dead, h, restated_gradients(params, x, mask, dead, row.prefixes, row.k_aux, ALPHA))
    _REFERENCES[row.id] = (params["W_dec"], out)
    return out


def _codes(eng, n, s):
    """(idx, val, row_nnz, membership as a bool matrix on the CPU, dense f on the CPU) of the last forward, form checked."""
    idx, val, _, nnz = eng.last_codes(n, row_nnz=True)
    check_form(idx, val, nnz)
    f, m = rows_to_dense(idx, val, nnz, s)
    m = m.cpu()
    got = torch.zeros(n, s, dtype=torch.bool)
    rows = torch.arange(n)[:, None].expand_as(idx)
    got[rows[m], idx.cpu()[m].long()] = True
    assert int(got.sum()) == int(nnz.sum()), "a latent appears twice in a row's codes"
    return idx, val, nnz.cpu().long(), got, f.cpu()


def _engine(row, **kw):
    eng = btk_engine(row.d, row.s, row.k, row.n, k_aux=row.k_aux, alpha=ALPHA, thr=DEAD_THR, **kw)
    assert eng.row_cap == btk_default_row_cap(row) and eng.row_regrows == 0
    return eng


# ------------------------------------------------------------------------------------------------
# A. one step against fp64, then the eval-mode forward
# ------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("row", BTK_SHAPES, ids=lambda r: r.id)
def test_batch_topk_step_in_every_dispatch_class_matches_fp64(row, encoder_mode):
    p, x, toks = btk_row_inputs(row)
    n, s, k = row.n, row.s, min(row.k, row.s)
    eng = _engine(row, remove_parallel_grads=False)
    eng.load_params(p)
    eng.set_tracker(toks)
    if row.prefixes:
        eng.set_prefixes(list(row.prefixes))
    xg = x.cuda()
    eng.step_forward(xg, training=True)
    eng.step_dead(n)
    eng.step_backward()
    st = eng.read_stats()
    # the rows grew where the longest needs it, once, and hold it now
    longest = row.lengths[1]
    grows = longest > btk_default_row_cap(row)
    assert eng.row_regrows == int(grows), (eng.row_regrows, longest, btk_default_row_cap(row))
    assert eng.row_cap == (min(s, (longest + 63) // 64 * 64) if grows else btk_default_row_cap(row))
    idx, val, nnz, got, f = _codes(eng, n, s)
    assert int(nnz.sum()) == n * k and math.isclose(st.l0, float(k), rel_tol=1e-6)
    params = {key: v.cpu().clone() for key, v in eng.param_views().items()}  # (W_dec as the forward renormalised it)
    assert torch.equal(params["W_enc"], p["W_enc"]) and torch.equal(params["b_enc"], p["b_enc"]) and torch.equal(params["b_dec"], p["b_dec"])
    mask, dead, h64, (mse, aux, ref) = _reference(row, params, x, toks)
    tol_b = btk_tol(x, p["W_enc"])
    assert torch.equal(got, mask), f"{row.id}: the step's selection is not the fp64 batch-wide top-(n k) ({int((got != mask).sum())} entries differ)"
    worst_val = ((f.double() - h64).abs()[mask].max() / tol_b).item()
    assert worst_val <= 1.0, f"{row.id}: a kept value is {worst_val:.2f} tol_b from fp64"
    assert (int(nnz.min()), int(nnz.max()), int((nnz == 0).sum())) == row.lengths
    # tracker, AuxK route and dead set: a row cannot quietly take another route
    fired = mask.any(dim=0)
    assert torch.equal(eng.toks_since_active.cpu(), torch.where(fired, 0, toks + n))
    assert eng.aux_route() == row.aux_route, (eng.aux_route(), row.aux_route)
    assert st.n_dead == row.n_dead == int(dead.sum())
    # the threshold: the EMA from 0 of the smallest positive kept value
    vmin = h64[mask & (h64 > 0)].min().item()
    thr = float(eng.threshold)
    assert abs(thr - M * vmin) <= tol_b * M, (thr, M * vmin, tol_b)
    grads = {key: v.cpu() for key, v in eng.grad_views().items()}
    ratios = {}
    try:
        ratios = assert_grads_close(grads, ref, row.bound, what=f"{row.id} {encoder_mode}: ")
    finally:
        print(f"{row.id} {encoder_mode}: rows {int(nnz.min())}..{int(nnz.max())}, row_cap {eng.row_cap}; values {worst_val:.2f} tol_b; mse {st.mse:.9e} "
              f"(fp64 {mse:.9e}) aux {st.aux:.9e} (fp64 {aux:.9e}); worst |difference| / max|fp64|: " + "  ".join(f"{k_} {v:.2e}" for k_, v in ratios.items()))
    assert math.isclose(st.mse, mse, rel_tol=1e-4), (st.mse, mse)
    assert math.isclose(st.aux, aux, rel_tol=1e-4, abs_tol=1e-9), (st.aux, aux)
    assert (aux > 0) == (row.n_dead > 0)

    # eval mode on the same context and batch: exactly {h > threshold} outside tol_b of the threshold, values within tol_b.  The
    # threshold is a tenth of the cut, so these rows are far longer: the eval compaction and the dense encoder at every ragged shape.
    assert thr > 0
    eng.step_forward(xg, training=False)
    _, _, nnz_e, got_e, f_e = _codes(eng, n, s)
    assert float(eng.threshold) == thr, "eval mode moved the threshold"
    assert (got_e | ~(h64 > thr + tol_b)).all(), "an entry clearly above the threshold is missing"
    assert (~got_e | (h64 > thr - tol_b)).all(), "an entry clearly below the threshold was kept"
    assert ((f_e.double() - h64).abs()[got_e] <= tol_b).all()
    assert int(nnz_e.sum()) >= n * k or k == s  # (threshold <= the smallest positive kept value)
    assert eng.row_cap >= int(nnz_e.max())
    eng.close()


# ------------------------------------------------------------------------------------------------
# B. the tail, and the step after it, on variable rows
# ------------------------------------------------------------------------------------------------

TAIL_ROWS = [r for r in BTK_SHAPES if (r.d, r.s) in ((36, 260), (1536, 1000), (772, 5004))]  # NV = 1 ragged, NV = 6, ragged everything


@pytest.mark.encoder_modes("f32")  # one encoder mode is enough here
@pytest.mark.parametrize("row", TAIL_ROWS, ids=lambda r: r.id)
def test_tail_and_the_next_step_on_variable_rows(row, encoder_mode):
    """rpg, clip_grad_norm, Adam and the renormalisation of the next forward on the gradients of variable-length rows (AuxK's included
    where the row has dead latents): procedure and tolerances of test_tail_at_every_row_kernel_width, three steps so that the moments
    carry clipped history.  Then one fused step on the row's own batch: its selection is the fp64 batch-wide one for the parameters it
    started from, outside tol_b of the cut.  Where the first forward grew the rows, everything after it runs on the grown context."""
    assert len(TAIL_ROWS) == 3
    n, d, s, k = row.n, row.d, row.s, min(row.k, row.s)
    max_norm = 1e-4
    p, x0, toks = btk_row_inputs(row)
    eng = _engine(row, remove_parallel_grads=True)
    eng.load_params(p)
    eng.set_tracker(toks)
    state = R.TrainState.create({k_: v.clone() for k_, v in p.items()})
    g = torch.Generator().manual_seed(d)
    clipped = 0
    for i in range(3):
        lr = 1e-3 * (i + 1)
        x = x0 if i == 0 else torch.randn(n, d, generator=g) * torch.exp(row.spread * torch.randn(n, 1, generator=g))
        eng.step_forward(x.cuda(), training=True)
        eng.step_dead(n)
        eng.step_backward()
        _, _, nnz, _, _ = _codes(eng, n, s)
        assert int(nnz.sum()) == n * k and (n == 1 or int(nnz.min()) == 0)
        raw = {k_: v.cpu().clone() for k_, v in eng.grad_views().items()}       # un-projected, un-clipped
        params = {k_: v.cpu().clone() for k_, v in eng.param_views().items()}   # W_dec rows normalised by this forward
        norms = params["W_dec"].double().norm(dim=1)
        assert (norms - 1).abs().max().item() <= 1e-6, f"step {i}: W_dec row {int((norms - 1).abs().argmax())} has norm {norms[(norms - 1).abs().argmax()].item():.9f}"
        eng.step_tail(lr, max_norm)
        st = eng.read_stats()
        grads = dict(raw)
        grads["W_dec"] = R.remove_parallel_grads(raw["W_dec"], params["W_dec"])
        # sae_ref's clip evaluated in fp64, the tolerances unchanged: on these gradients (loud rows next to silent ones: elements of
        # very different size) torch's fp32 vector_norm on the CPU is itself 4e-5 (1536x1000) and 1.5e-4 (772x5004) off its own fp64
        # value on the same fp32 data, more than the 1e-5 the norm is held to; the engine sums the squares in fp64.
        scaled, total = R.clip_grad_norm([grads[k_].double() for k_ in R.PARAM_ORDER], max_norm)
        scaled = [g_.float() for g_ in scaled]
        clipped += total.item() > max_norm
        state.adam_steps += 1
        for k_, gk in zip(R.PARAM_ORDER, scaled):
            state.params[k_] = params[k_]
            R.adam_update(state.params[k_], gk, state.m[k_], state.v[k_], state.adam_steps, lr)
        assert math.isclose(st.grad_norm, total.item(), rel_tol=1e-5), (st.grad_norm, total.item())
        for k_ in R.PARAM_ORDER:
            torch.testing.assert_close(eng.view(k_).cpu(), state.params[k_], rtol=1e-5, atol=1e-7, msg=lambda m: f"step {i} {k_}: {m}")
            torch.testing.assert_close(eng.view(k_, eng.adam_m).cpu(), state.m[k_], rtol=1e-5, atol=1e-9, msg=lambda m: f"step {i} m {k_}: {m}")
            torch.testing.assert_close(eng.view(k_, eng.adam_v).cpu(), state.v[k_], rtol=1e-5, atol=1e-12, msg=lambda m: f"step {i} v {k_}: {m}")
    assert clipped == 3, "the clip must be active on every step"
    assert eng.row_regrows >= int(row.lengths[1] > btk_default_row_cap(row))
    moved = eng.view("W_dec").double().norm(dim=1)
    assert (moved - 1).abs().max().item() > 1e-6, "the last Adam step is meant to leave rows that need renormalising"
    # the step after the step: the fused entry on the (possibly grown) context, the row's own batch, the parameters Adam left
    W_enc, b_enc = eng.view("W_enc").cpu().clone(), eng.view("b_enc").cpu().clone()
    eng.train_step(x0.cuda(), 1e-3, max_norm)
    assert eng.adam_steps == 4
    _, _, nnz, got, f = _codes(eng, n, s)
    h64 = x0.double() @ W_enc.double() + b_enc.double()
    tol_b = btk_tol(x0, W_enc)
    cut = h64.flatten().sort(descending=True).values[n * k - 1]
    assert int(nnz.sum()) == n * k
    assert (got | ~(h64 > cut + tol_b)).all(), "an entry clearly above the cut is missing"
    assert (~got | (h64 > cut - tol_b)).all(), "an entry clearly below the cut was kept"
    assert ((f.double() - h64).abs()[got] <= tol_b).all()
    assert torch.isfinite(eng.params).all()
    eng.normalize_w_dec()
    norms = eng.view("W_dec").double().norm(dim=1)
    assert (norms - 1).abs().max().item() <= 1e-6, f"W_dec row {int((norms - 1).abs().argmax())} after the last step"
    eng.close()
