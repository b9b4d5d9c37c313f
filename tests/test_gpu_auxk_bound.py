"""AuxK with the dead count left on the device (needs -m gpu).  From the fifth step after the tracker was last written saev_step_dead
sizes the auxiliary work by the n_near of the record DEAD_LAG = 4 steps back and the count stays in flags[4]; every step of a real
run but the first four takes that path.  The per-element AuxK tests elsewhere run one step after set_tracker -- a read-back step,
bound = count, no padding row or column anywhere.  Here the bound is ABOVE the count (tests/auxk_bound_cases.py: the scenario, the
rows; DESIGN.md, "Parity": the AuxK bound table; tests/test_auxk_bound_cases_host_cpu.py proves each row's bound, count, route and
kernel family without a GPU):

  A. all four gradients of the measured step, teacher-forced on the step's own selection, against the fp64 restatement of
     tests/step_restatement.py: EVERY element within 2e-5 of its tensor's largest; the route, the read-back count, n_dead and the
     tracker exactly;
  B. saev_train_step against the four phases with AuxK active (inside the fused entry the backward's ordered-sum launch also forms
     the auxiliary loss: aux_stats_pending);
  C. the gathered backward of a sparse-state exchange over one rank's rows: the auxiliary term's share of db_dec goes through db_aux
     (zeroed when the count may be zero), and the compact rows travel through saev_aux_compact_export / _import -- bound-many of
     them, of which only count-many may reach a gradient."""

import math

import pytest
import torch

import sae_ref as R
from auxk_bound_cases import DENSE_CASES, SMALL_CASES, STALE_CASES, replay, scenario
from step_restatement import BOUND, assert_grads_close, restated_gradients
from test_gpu_parity import make_engine

pytestmark = pytest.mark.gpu

ALPHA = 1 / 32

_REFERENCES = {}  # (case id, variant) -> (mask, W_dec as the step normalised it, (mse, aux, gradients)): computed once per scenario


def _reference(case, variant, params, x, mask, dead_mask):
    """The fp64 restatement on the step's own selection and its own (renormalised) W_dec, with the planted D latents as the dead
    set -- shared by the encoder modes and tests of a scenario as long as they hand in the same mask and parameters."""
    key = (case.id, variant)
    hit = _REFERENCES.get(key)
    if hit is not None and torch.equal(hit[0], mask) and torch.equal(hit[1], params["W_dec"]):
        return hit[2]
    out = restated_gradients(params, x, mask, dead_mask, None, case.k_aux, ALPHA)
    _REFERENCES[key] = (mask, params["W_dec"], out)
    return out


def _warmed_engine(case, variant, rpg=False):
    """An engine after the scenario's warm-up steps (learning rate 0), and what the measured step needs."""
    p, toks, xs, dead, sleepy = scenario(case, variant)
    eng = make_engine(case.d, case.s, case.k, k_aux=case.k_aux, alpha=ALPHA, thr=case.thr, max_batch=case.n, remove_parallel_grads=rpg)
    eng.load_params(p)
    eng.set_tracker(toks)
    steps = replay(case, variant)
    for i, x in enumerate(xs[:-1], 1):
        eng.train_step(x.cuda(), 0.0, 1.0)
        assert eng.read_stats().n_dead == int(steps[i - 1].dead.sum()), f"warm-up step {i}"
    return eng, p, xs[-1], dead, sleepy, steps


def _mask_of(eng, case):
    idx, _, _ = eng.last_codes(case.n)
    mask = torch.zeros(case.n, case.s, dtype=torch.bool).scatter_(1, idx.cpu().long(), True)
    assert int(mask.sum()) == case.n * min(case.k, case.s), "a latent appears twice in a row's codes"
    return mask


def _gathered_backward(eng, case, xg):
    """saev_amd/framework/ddp.py: _step_sparse with a world of one; the exported compact rows past the count come back as 1e30 (in a
    real exchange they are the sum of every rank's stale rows: anything)."""
    x_all, g_all, idx_all, val_all = eng.gather_buffers(1, case.n)
    x_all.copy_(xg)
    eng.copy_step_state(case.n, g_all, idx_all, val_all)
    eng.grad_w_enc_t()
    eng.backward_begin_gathered(x_all, g_all, idx_all, val_all)
    aux = eng.aux_compact_export()
    assert aux is not None, "the bound is above zero: the step has auxiliary work to exchange"
    rows = (aux.numel() - case.d) // (2 * case.d + 1)
    assert rows >= case.bound
    aux[:2 * rows * case.d].view(2, rows, case.d)[:, case.n_dead:] = 1e30
    aux[2 * rows * case.d:2 * rows * case.d + rows][case.n_dead:] = 1e30
    eng.aux_compact_import(aux)
    eng.backward_rows(0, case.s)
    eng.backward_end()


def _measured_step_matches_fp64(case, variant, encoder_mode, gathered=False):
    eng, p, x, dead, sleepy, steps = _warmed_engine(case, variant)
    claim = dict(case.claim)
    xg = x.cuda()
    eng.step_forward(xg, training=True)
    eng.step_dead(case.n)
    if gathered:
        _gathered_backward(eng, case, xg)
    else:
        eng.step_backward()
    st = eng.read_stats()
    route, readbacks = eng.aux_route(), eng.dead_readbacks()
    mask = _mask_of(eng, case)
    assert torch.equal(mask, steps[-1].mask), f"the step's selection is not the fp64 top-k ({int((mask != steps[-1].mask).sum())} entries differ)"
    params = {key: v.cpu().clone() for key, v in eng.param_views().items()}  # (W_dec as the forward renormalised it)
    assert torch.equal(params["W_enc"], p["W_enc"]) and torch.equal(params["b_enc"], p["b_enc"]) and torch.equal(params["b_dec"], p["b_dec"])
    dead_mask = torch.zeros(case.s, dtype=torch.bool)
    dead_mask[dead] = True
    mse, aux, ref = _reference(case, variant, params, x, mask, dead_mask)
    got = {key: v.cpu() for key, v in eng.grad_views().items()}
    ratios = {}
    try:
        ratios = assert_grads_close(got, ref, BOUND, what=f"{case.id} {variant} {encoder_mode}: ")
    finally:
        print(f"{case.id} {variant} {encoder_mode}: route {route} ({claim['family']}), bound {case.bound}, count {st.n_dead}; mse {st.mse:.9e} "
              f"(fp64 {mse:.9e}) aux {st.aux:.9e} (fp64 {aux:.9e}); worst |difference| / max|fp64|: "
              + "  ".join(f"{k_} {v:.2e}" for k_, v in ratios.items()))
    # the route and the count: the bound sized the step, nothing was read back for it
    assert route == claim["route"], (route, claim)
    assert readbacks == 4, readbacks  # steps 1-4 only
    assert st.n_dead == case.n_dead
    assert torch.equal(eng.toks_since_active.cpu(), steps[-1].toks)
    assert math.isclose(st.mse, mse, rel_tol=1e-4), (st.mse, mse)
    if case.n_dead == 0:
        assert st.aux == 0.0 and aux == 0.0, (st.aux, aux)
        if variant == "B":
            # the latents that were dead on step 4 left rows in the compact buffers: none of them may reach a gradient (the fp64
            # reference has no auxiliary term, and a silent latent's gradient is exactly zero)
            for name, g in (("W_dec", got["W_dec"][sleepy]), ("W_enc", got["W_enc"][:, sleepy]), ("b_enc", got["b_enc"][sleepy])):
                assert g.abs().max().item() <= BOUND * ref[name].abs().max().item(), f"{name}: a stale row reached the gradient of a latent that is not dead"
    else:
        assert aux > 0 and math.isclose(st.aux, aux, rel_tol=1e-4), (st.aux, aux)
    assert st.l0 == float(min(case.k, case.s))
    eng.close()


def _runs(cases):
    return [pytest.param(c, v, id=f"{c.id}-{v}") for c in cases for v in c.variants]


# ------------------------------------------------------------------------------------------------
# A. gradients against fp64
# ------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("case,variant", _runs(DENSE_CASES))  # all three encoder modes: f16x3 alone brings its own hi/lo x images
def test_dense_auxk_sized_by_a_bound_above_the_count_matches_fp64(case, variant, encoder_mode):
    _measured_step_matches_fp64(case, variant, encoder_mode)


@pytest.mark.encoder_modes("f16r", "f32")  # (the two contexts allocate and prepare differently)
@pytest.mark.parametrize("case,variant", _runs(SMALL_CASES))
def test_few_dead_latents_kernels_under_a_bound_above_the_count_match_fp64(case, variant, encoder_mode):
    _measured_step_matches_fp64(case, variant, encoder_mode)


# ------------------------------------------------------------------------------------------------
# B. the fused entry against the phases, AuxK active
# ------------------------------------------------------------------------------------------------


def _fused_entry_and_phases_agree(case, encoder_mode):
    variant = "A"
    a, p, x, dead, _, steps = _warmed_engine(case, variant, rpg=True)
    b = _warmed_engine(case, variant, rpg=True)[0]
    xg = x.cuda()
    a.train_step(xg, 1e-3, 0.05)
    b.step_forward(xg, training=True, n_rows_global=case.n)
    b.step_dead(case.n)
    b.step_backward()
    mask = _mask_of(b, case)
    params = {key: v.cpu().clone() for key, v in b.param_views().items()}  # (W_dec as the forward renormalised it, before the tail moves it)
    b.step_tail(1e-3, 0.05)
    sa, sb = a.read_stats(), b.read_stats()
    assert torch.equal(mask, steps[-1].mask)
    dead_mask = torch.zeros(case.s, dtype=torch.bool)
    dead_mask[dead] = True
    mse, aux, _ = _reference(case, variant, params, x, mask, dead_mask)
    print(f"{case.id} {encoder_mode}: route {a.aux_route()} / {b.aux_route()} ({dict(case.claim)['family']}); grad_norm {sa.grad_norm:.9e} / {sb.grad_norm:.9e}; "
          f"mse {sa.mse:.9e} / {sb.mse:.9e} (fp64 {mse:.9e}); aux {sa.aux:.9e} / {sb.aux:.9e} (fp64 {aux:.9e})")
    assert a.aux_route() == b.aux_route() == dict(case.claim)["route"]
    assert a.dead_readbacks() == b.dead_readbacks() == 4
    assert sa.grad_norm > 0.05, "the clip is meant to be active"
    assert math.isclose(sa.grad_norm, sb.grad_norm, rel_tol=2e-6), (sa.grad_norm, sb.grad_norm)
    assert math.isclose(sa.mse, sb.mse, rel_tol=1e-6), (sa.mse, sb.mse)
    assert sa.n_dead == sb.n_dead == case.n_dead
    for s_ in (sa, sb):
        if case.n_dead == 0:
            assert s_.aux == 0.0 and aux == 0.0
        else:
            assert math.isclose(s_.aux, aux, rel_tol=1e-4), (s_.aux, aux)
    for key in R.PARAM_ORDER:
        torch.testing.assert_close(a.view(key), b.view(key), rtol=1e-5, atol=1e-7, msg=lambda m: f"{key}: {m}")
    a.close()
    b.close()


@pytest.mark.parametrize("case", [c for c in STALE_CASES if c in DENSE_CASES], ids=lambda c: c.id)
def test_fused_train_step_and_phases_agree_with_dense_auxk_under_a_bound(case, encoder_mode):
    _fused_entry_and_phases_agree(case, encoder_mode)


@pytest.mark.encoder_modes("f16r", "f32")
@pytest.mark.parametrize("case", [c for c in STALE_CASES if c in SMALL_CASES], ids=lambda c: c.id)
def test_fused_train_step_and_phases_agree_with_few_dead_latents_under_a_bound(case, encoder_mode):
    _fused_entry_and_phases_agree(case, encoder_mode)


# ------------------------------------------------------------------------------------------------
# C. the gathered backward over one rank's rows
# ------------------------------------------------------------------------------------------------


@pytest.mark.encoder_modes("f16r", "f32")
@pytest.mark.parametrize("case", STALE_CASES, ids=lambda c: c.id)
def test_gathered_backward_under_a_bound_above_the_count_matches_fp64(case, encoder_mode):
    _measured_step_matches_fp64(case, "B", encoder_mode, gathered=True)
