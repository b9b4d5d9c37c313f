"""The train step in every dispatch class of d_model, d_sae and top_k (needs -m gpu).  The step picks its kernels from the shape
("Parity": the class table with the predicate and file behind each class); almost every other backward, AuxK or tail test
sits at d_model in {48, 64, 128, 256, 512, 768, 1024, 1280}, d_sae a multiple of 64 and top_k <= 32.  Here:

  A. the four gradients of one step at every row of tests/step_restatement.py: SHAPES, teacher-forced on the step's own selection,
     against the fp64 restatement, EVERY element within 2e-5 of its tensor's largest (the bound tests/test_gpu_dw_slices.py holds the
     same gradients to at 16384-row sums; the fp32 CPU oracle itself is within 1.4e-6 of fp64 on these rows,
     tests/test_step_restatement_host_cpu.py, so 4 x its error stays below the bound on every row);
  B. the tail -- projection, clip, Adam, renormalisation -- at every NV class of the row kernels, on the engine's own gradients;
  C. the step after the step at ragged d_sae: operand images the fused Adam leaves for an edge tile surface as a wrong selection one
     step later."""

import math

import pytest
import torch

import sae_ref as R
from step_restatement import DEAD_THR, SHAPES, assert_grads_close, input_conditions, restated_gradients, row_inputs
from test_gpu_parity import make_engine, rand_params
from topk_exactness import assert_topk_exact

pytestmark = pytest.mark.gpu

ALPHA = 1 / 32

# ------------------------------------------------------------------------------------------------
# A. gradients against fp64
# ------------------------------------------------------------------------------------------------

_REFERENCES = {}  # row.id -> (mask, W_dec as the step normalised it, dead mask, (mse, aux, gradients)): computed once per row


def _reference(row, params, x, toks, mask):
    """The fp64 restatement on the step's own selection and its own (renormalised) W_dec -- shared by the routes and encoder modes of
    a row as long as they hand in the same mask and parameters, which they must: the input conditions leave no freedom."""
    hit = _REFERENCES.get(row.id)
    if hit is not None and torch.equal(hit[0], mask) and torch.equal(hit[1], params["W_dec"]):
        return hit[2], hit[3]
    want, dead, _ = input_conditions(row, params["W_enc"], params["b_enc"], x, toks)
    assert torch.equal(mask, want), f"{row.id}: the step's selection is not the fp64 top-k ({int((mask != want).sum())} entries differ)"
    out = restated_gradients(params, x, mask, dead, row.prefixes, row.k_aux, ALPHA)
    _REFERENCES[row.id] = (mask, params["W_dec"], dead, out)
    return dead, out


@pytest.mark.encoder_modes("f16r", "f32")  # (the two contexts allocate and prepare differently)
@pytest.mark.parametrize("dw", ["default", "rows"])  # (without slices -- d_model % 32 != 0, Matryoshka -- the two are the same code)
@pytest.mark.parametrize("row", SHAPES, ids=lambda r: r.id)
def test_gradients_in_every_dispatch_class_match_fp64(row, dw, encoder_mode, monkeypatch):
    if dw == "rows":
        monkeypatch.setenv("SAEV_AMD_DW", "rows")
    p, x, toks = row_inputs(row)
    k = min(row.k, row.s)
    eng = make_engine(row.d, row.s, row.k, k_aux=row.k_aux, alpha=ALPHA, thr=DEAD_THR, max_batch=row.n, remove_parallel_grads=False)
    eng.load_params(p)
    eng.set_tracker(toks)
    if row.prefixes:
        eng.set_prefixes(list(row.prefixes))
    xg = x.cuda()
    eng.step_forward(xg, training=True)
    eng.step_dead(row.n)
    eng.step_backward()
    st = eng.read_stats()
    idx, val, _ = eng.last_codes(row.n)
    worst = assert_topk_exact(xg, idx, val, eng.view("W_enc"), eng.view("b_enc"), what=f"{row.id}: ")
    mask = torch.zeros(row.n, row.s, dtype=torch.bool).scatter_(1, idx.cpu().long(), True)
    assert int(mask.sum()) == row.n * k, "a latent appears twice in a row's codes"
    params = {key: v.cpu().clone() for key, v in eng.param_views().items()}  # (W_dec as the forward renormalised it)
    assert torch.equal(params["W_enc"], p["W_enc"]) and torch.equal(params["b_enc"], p["b_enc"]) and torch.equal(params["b_dec"], p["b_dec"])
    dead, (mse, aux, ref) = _reference(row, params, x, toks, mask)
    # the AuxK route and the dead set: a row cannot quietly take another route
    assert eng.aux_route() == row.aux_route, (eng.aux_route(), row.aux_route)
    assert st.n_dead == row.n_dead == int(dead.sum())
    fired = mask.any(dim=0)
    assert torch.equal(eng.toks_since_active.cpu(), torch.where(fired, 0, toks + row.n))
    got = {key: v.cpu() for key, v in eng.grad_views().items()}
    ratios = {}
    try:
        ratios = assert_grads_close(got, ref, row.bound, what=f"{row.id} {dw} {encoder_mode}: ")
    finally:
        print(f"{row.id} {dw} {encoder_mode}: codes {worst[0]:.2f} / {worst[1]:.2f} tol_b; mse {st.mse:.9e} (fp64 {mse:.9e}) aux {st.aux:.9e} "
              f"(fp64 {aux:.9e}); worst |difference| / max|fp64|: " + "  ".join(f"{k_} {v:.2e}" for k_, v in ratios.items()))
    assert math.isclose(st.mse, mse, rel_tol=1e-4), (st.mse, mse)
    assert math.isclose(st.aux, aux, rel_tol=1e-4, abs_tol=1e-9), (st.aux, aux)
    assert (aux > 0) == (row.n_dead > 0)
    assert st.l0 == float(k)
    eng.close()


# ------------------------------------------------------------------------------------------------
# B. the tail at every NV class
# ------------------------------------------------------------------------------------------------


@pytest.mark.encoder_modes("f32")  # one encoder mode is enough here
@pytest.mark.parametrize("n,d,s,k", [(65, 36, 260, 4), (130, 1536, 516, 16), (70, 1664, 260, 8), (66, 2048, 260, 8), (66, 2560, 260, 8),
                                     (34, 3584, 260, 8), (34, 4092, 260, 8)])
def test_tail_at_every_row_kernel_width(n, d, s, k, encoder_mode):
    """rpg, clip_grad_norm, Adam and the renormalisation of the next forward at NV = ceil(d_model / 256) = 1 (ragged), 6, 7 of 8, 8,
    10 of 12, 14 of 16 and 16 with a ragged last float4: procedure and tolerances of
    tests/test_gpu_parity.py::test_tail_clip_and_grad_scale_branches, three steps so that the moments carry clipped history."""
    max_norm = 1e-4
    p = rand_params(d, s, seed=d + n)
    eng = make_engine(d, s, k, k_aux=0, max_batch=n, remove_parallel_grads=True)
    eng.load_params(p)
    state = R.TrainState.create({k_: v.clone() for k_, v in p.items()})
    g = torch.Generator().manual_seed(d)
    clipped = 0
    for i in range(3):
        lr = 1e-3 * (i + 1)
        x = torch.randn(n, d, generator=g)
        eng.step_forward(x.cuda(), training=True)
        eng.step_dead(n)
        eng.step_backward()
        raw = {k_: v.cpu().clone() for k_, v in eng.grad_views().items()}       # un-projected, un-clipped
        params = {k_: v.cpu().clone() for k_, v in eng.param_views().items()}   # W_dec rows normalised by this forward
        norms = params["W_dec"].double().norm(dim=1)
        assert (norms - 1).abs().max().item() <= 1e-6, f"step {i}: W_dec row {int((norms - 1).abs().argmax())} has norm {norms[(norms - 1).abs().argmax()].item():.9f}"
        eng.step_tail(lr, max_norm)
        st = eng.read_stats()
        grads = dict(raw)
        grads["W_dec"] = R.remove_parallel_grads(raw["W_dec"], params["W_dec"])
        scaled, total = R.clip_grad_norm([grads[k_] for k_ in R.PARAM_ORDER], max_norm)
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
    moved = eng.view("W_dec").double().norm(dim=1)
    assert (moved - 1).abs().max().item() > 1e-6, "the last Adam step is meant to leave rows that need renormalising"
    eng.normalize_w_dec()
    norms = eng.view("W_dec").double().norm(dim=1)
    assert (norms - 1).abs().max().item() <= 1e-6, f"W_dec row {int((norms - 1).abs().argmax())} after the last step"
    eng.close()


# ------------------------------------------------------------------------------------------------
# C. the step after the step, at ragged d_sae
# ------------------------------------------------------------------------------------------------


def _batches(n, d, seed):
    """Three fresh batches around a common mean, and the third once more."""
    g = torch.Generator().manual_seed(seed)
    mu = torch.randn(d, generator=g)
    xs = [(torch.randn(n, d, generator=g) + mu).cuda() for _ in range(3)]
    return xs + [xs[2]]


def _same(e0, e1):
    for name in ("params", "adam_m", "adam_v"):
        assert torch.equal(getattr(e0, name), getattr(e1, name)), f"{name} differ"
    assert torch.equal(e0.toks_since_active, e1.toks_since_active)


@pytest.mark.encoder_modes("f16r")  # the streamed preparation belongs to the f16r encoder
@pytest.mark.parametrize("n,d,s,k", [(130, 64, 1000, 8), (257, 96, 260, 16), (300, 256, 5004, 32), (65, 32, 36, 4)])
def test_streamed_steps_at_ragged_d_sae_equal_fully_prepared_steps(n, d, s, k, encoder_mode, monkeypatch):
    """d_model % 32 == 0: the context streams, and the fused Adam writes the next step's encoder images for a tile whose latents
    partly lie past d_sae.  The assertion of tests/test_gpu_stream.py::test_streamed_steps_equal_fully_prepared_steps_bit_for_bit
    (which has only multiples of 256), and the codes of the last step exact against the parameters that step started from."""
    p = rand_params(d, s, seed=s + n)
    engs = []
    for prep in ("0", "1"):
        with monkeypatch.context() as m:
            m.setenv("SAEV_AMD_PREP", prep)
            eng = make_engine(d, s, k, k_aux=32, thr=3 * n, max_batch=n)
        assert eng.cfg.prep_route == int(prep)
        eng.load_params(p)
        engs.append(eng)
    xs = _batches(n, d, seed=s)
    for i, x in enumerate(xs):
        if i == len(xs) - 1:
            W_enc, b_enc = engs[0].view("W_enc").clone(), engs[0].view("b_enc").clone()
        for eng in engs:
            eng.train_step(x, 1e-3, 0.05 if i % 2 else 1.0)
            assert eng.read_stats().n_overflow_rows == 0, i
        a, c = (e.read_stats() for e in engs)
        assert a.mse == c.mse and a.l1 == c.l1 and a.grad_norm == c.grad_norm and a.n_dead == c.n_dead, (i, a, c)
    torch.cuda.synchronize()
    _same(*engs)
    for eng in engs:
        idx, val, _ = eng.last_codes(n)
        worst = assert_topk_exact(xs[-1], idx, val, W_enc, b_enc, what=f"prep_route {eng.cfg.prep_route}: ")
        print(f"({n}, {d}, {s}, {k}) prep_route {eng.cfg.prep_route}: worst value error {worst[0]:.2f} tol_b, worst cut excess {worst[1]:.2f} tol_b")
    for eng in engs:
        eng.step_forward(xs[0], training=False)  # (a pending SAEV_STALE_PARAMS would raise here: none on an honest run)
        torch.cuda.synchronize()
        eng.close()


@pytest.mark.encoder_modes("f32")  # picks its own encoder mode; run once
@pytest.mark.parametrize("n,d,s,k", [(130, 64, 1000, 8), (257, 96, 260, 16)])
def test_bf16_images_left_by_adam_at_ragged_d_sae_equal_a_fresh_split(n, d, s, k, encoder_mode):
    """tests/test_gpu_stream.py::test_bf16_images_left_by_adam_equal_a_fresh_split where the last latent tile is partial."""
    p = rand_params(d, s, seed=s + n + 1)
    engs = [make_engine(d, s, k, k_aux=32, thr=3 * n, max_batch=n, encoder="bf16", prep_route=r) for r in (0, 1)]
    for eng in engs:
        eng.load_params(p)
    for i, x in enumerate(_batches(n, d, seed=s + 1)):
        for eng in engs:
            eng.train_step(x, 1e-3, 1.0)
            assert eng.read_stats().n_overflow_rows == 0, i
        a, c = (e.read_stats() for e in engs)
        assert a.mse == c.mse and a.dense_route == c.dense_route == 0, (i, a, c)
    torch.cuda.synchronize()
    _same(*engs)
    for eng in engs:
        eng.step_forward(x, training=False)  # (a pending SAEV_STALE_PARAMS would raise here)
        torch.cuda.synchronize()
        eng.close()
