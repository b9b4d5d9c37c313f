"""BatchTopK SAEs on the MI355X (needs -m gpu): the batch-wide select and the compaction against an fp64 sort, the forward, the
eval-mode threshold, the module API, gradients, optimizer trajectories and the inference pass against the reference's own outputs
(fixtures G20, tools/gen_golden_batch_topk.py), the automatic growth of the code rows, and train() / evaluate() end to end.

Tolerances.  Quantities that the TopK tests compare with the same reference quantities take those tests' tolerances:
tests/test_gpu_parity.py::test_g5_golden_objective_forward_backward (mse 1e-4, aux 1e-4 / 1e-9, l0 1e-6, l1 1e-5, f and x_hat
1e-5 / 1e-5, gradients 1e-3 / 1e-7), ::test_g9_golden_train_trajectory for the free-running trajectories (mse 1e-4, aux 1e-3 /
1e-8, l0 1e-6, l1 1e-4, gradient norm 2e-3, parameters 2e-3 / 5e-5 on all but 2e-3 of the elements -- without its allowance for
flipped selections, which the fixtures' gaps rule out) and tests/test_gpu_muon.py (NS_REL_TOL, biases 1e-4 / 1e-6).  What has no
counterpart there:
  * membership at a cut: tol = 8 * 2^-24 * max_b ||x_b|| * max_s ||W_enc[:, s]|| (+ 2^-23 max |b_enc|), the fp32 dot-product bound
    of tests/test_gpu_relu.py -- two fp32 evaluations of h differ by at most 2 tol, so entries farther than that from a cut or a
    threshold must agree, and the fixtures' gaps are >= 16 tol (stored; asserted here);
  * the threshold: threshold' = fl(fl(t (1 - m)) + fl(m v)) with v one of the kept pre-activations, itself within tol of the
    reference's: |dt'| <= (1 - m) |dt| + m tol + 3 ulp.  Over the four recorded steps that stays below tol + 12 ulp(0.5): the bound
    used is tol + 1e-6.
"""

import io
import json
import math

import numpy as np
import pytest
import scipy.sparse
import torch

import sae_ref as R
from conftest import load_golden
from step_restatement import BOUND, assert_grads_close, restated_gradients
from test_inference_host_cpu import write_cache

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------
# helpers
# ------------------------------------------------------------------------------------------------


def btk_engine(d, s, k, b, *, k_aux=0, alpha=1 / 32, thr=10_000_000, **kw):
    from saev_amd.engine import EngineConfig, SaeEngine

    return SaeEngine(EngineConfig(d_model=d, d_sae=s, top_k=k, k_aux=k_aux, alpha=alpha, dead_threshold_tokens=thr, max_batch=b,
                                  activation="batch_topk", **kw))


def ckpt_state(g) -> dict:
    raw = g["ckpt"].numpy().tobytes()
    return torch.load(io.BytesIO(raw[raw.index(b"\n") + 1:]), weights_only=True, map_location="cpu")


def expected_mask(h: torch.Tensor, t: int):
    """The selection the tie rule prescribes, from a sort in fp64: everything above the t-th largest value, and of the entries
    equal to it the first ones in flat (row-major) order.  Returns (mask, cut, n_above, quota, n_ties)."""
    flat = h.double().flatten()
    t = min(t, flat.numel())
    cut = flat.sort(descending=True).values[t - 1]
    above, ties = flat > cut, flat == cut
    quota = t - int(above.sum())
    keep = above.clone()
    keep[ties.nonzero().flatten()[:quota]] = True
    return keep.reshape(h.shape), float(cut), int(above.sum()), quota, int(ties.sum())


def check_form(idx, val, nnz):
    """Padded rows: row_nnz valid entries of ascending latents, then idx = -1 and val = 0."""
    n, cap = idx.shape
    slot = torch.arange(cap, device=idx.device)[None, :]
    m = slot < nnz[:, None]
    assert int(nnz.min()) >= 0 and int(nnz.max()) <= cap
    assert ((idx >= 0) == m).all(), "valid slots and the -1 padding do not follow row_nnz"
    assert (idx[~m] == -1).all() and (val[~m] == 0).all()
    asc = (idx[:, 1:] > idx[:, :-1]) | ~m[:, 1:]
    assert asc.all(), "latents of a row are not in ascending order"


def rows_to_dense(idx, val, nnz, s):
    f = torch.zeros(idx.shape[0], s, device=idx.device)
    m = torch.arange(idx.shape[1], device=idx.device)[None, :] < nnz[:, None]
    rows = torch.arange(idx.shape[0], device=idx.device)[:, None].expand_as(idx)
    f[rows[m], idx[m].long()] = val[m]
    return f, m


def dot_tol(x, W_enc, b_enc) -> float:
    return float(8.0 * 2.0 ** -24 * x.double().norm(dim=1).max() * W_enc.double().norm(dim=0).max() + 2.0 ** -23 * b_enc.abs().max())


# ------------------------------------------------------------------------------------------------
# select and compaction
# ------------------------------------------------------------------------------------------------


@pytest.mark.encoder_modes("f32")
@pytest.mark.parametrize("n,s,k,list_cap", [(300, 1024, 2, 0), (300, 1024, 2, 16), (257, 512, 8, 0), (64, 4096, 32, 64), (5, 24, 3, 0)])
def test_select_on_a_dense_matrix_is_exact(n, s, k, list_cap, encoder_mode):
    eng = btk_engine(16, s, k, 512, select_list_cap=list_cap)
    h = torch.randn(n, s, generator=torch.Generator().manual_seed(n + s + k)).cuda()
    idx, val, nnz = eng.batch_topk_dense(h, training=True)
    mask, cut, n_above, quota, n_ties = expected_mask(h.cpu(), n * k)
    check_form(idx, val, nnz)
    assert int(nnz.sum()) == n * k, "not exactly n * top_k codes"
    f, _ = rows_to_dense(idx, val, nnz, s)
    assert torch.equal(f.cpu(), torch.where(mask, h.cpu(), torch.zeros(())))  # tol = 0: h is given, the set must be exact
    assert torch.equal(nnz.cpu().long(), mask.sum(dim=1))
    if k * 4 < s and n >= 64 and k <= 2:
        assert int((nnz == 0).sum()) > 0, "this case is meant to have rows without codes"
    st = eng.batch_topk_state()
    assert (st["cut"], st["n_above"], st["tie_quota"], st["n_ties"]) == (float(np.float32(cut)), n_above, quota, n_ties)
    # the smallest positive kept value moved the threshold from 0: (1 - m) * 0 + m * min
    pos = h.cpu()[mask & (h.cpu() > 0)]
    want = torch.tensor(0.0).mul_(1 - 0.1).add_(0.1 * pos.min())
    assert float(eng.threshold) == float(want)


@pytest.mark.encoder_modes("f32")
@pytest.mark.parametrize("levels,s,list_cap", [(5, 256, 0), (5, 256, 8), (2, 1024, 0)])
def test_ties_at_the_cut_follow_the_flat_index_rule(levels, s, list_cap, encoder_mode):
    """A matrix of a few distinct values: thousands of entries equal the cut.  Lower flat index first, bit for bit.  With two
    levels every row holds ~512 entries >= the cut: the rows grow (the overflow count is taken before the tie rule) and the
    result is the same."""
    n, k = 64, 4
    eng = btk_engine(16, s, k, 64, select_list_cap=list_cap)
    h = torch.randint(0, levels, (n, s), generator=torch.Generator().manual_seed(levels)).float()
    h[h == 0] = -0.0  # (a signed zero is the same value as +0)
    idx, val, nnz = eng.batch_topk_dense(h.cuda(), training=True)
    mask, cut, n_above, quota, n_ties = expected_mask(h, n * k)
    assert n_ties > quota > 0, "the case must cut through a run of ties"
    check_form(idx, val, nnz)
    f, m = rows_to_dense(idx, val, nnz, s)
    got = torch.zeros(n, s, dtype=torch.bool)
    rows = torch.arange(n)[:, None].expand_as(idx)
    got[rows[m.cpu()], idx.cpu()[m.cpu()].long()] = True
    assert torch.equal(got, mask)
    assert torch.equal(f.cpu(), torch.where(mask, h, torch.zeros(())))
    assert int(nnz.sum()) == n * k
    # (the overflow count of a row is taken before the tie rule drops entries: all its entries >= the cut, against the default 64 slots)
    widest = int((h >= cut).sum(dim=1).max())
    assert eng.row_regrows == (1 if widest > 64 else 0) and (levels != 2 or widest > 64)
    assert eng.row_cap == (64 if widest <= 64 else min(s, (widest + 63) // 64 * 64))
    st = eng.batch_topk_state()
    assert (st["cut"], st["n_above"], st["tie_quota"], st["n_ties"]) == (cut, n_above, quota, n_ties)


@pytest.mark.encoder_modes("f32")
def test_all_negative_keeps_negative_values_and_leaves_the_threshold(encoder_mode):
    n, s, k = 48, 512, 4
    eng = btk_engine(16, s, k, 64)
    eng.threshold.fill_(0.375)
    h = -(torch.rand(n, s, generator=torch.Generator().manual_seed(3)) + 0.5)
    idx, val, nnz = eng.batch_topk_dense(h.cuda(), training=True)
    mask, *_ = expected_mask(h, n * k)
    check_form(idx, val, nnz)
    f, m = rows_to_dense(idx, val, nnz, s)
    assert int(nnz.sum()) == n * k and (val[m] < 0).all()
    assert torch.equal(f.cpu(), torch.where(mask, h, torch.zeros(())))
    assert float(eng.threshold) == 0.375  # nothing positive was kept (the reference would raise on the empty minimum)


@pytest.mark.encoder_modes("f32")
def test_a_budget_of_everything_keeps_everything(encoder_mode):
    n, s = 20, 64
    eng = btk_engine(16, s, 200, 32)  # top_k * n >= S * n
    assert eng.row_cap == s
    h = torch.randn(n, s, generator=torch.Generator().manual_seed(4))
    idx, val, nnz = eng.batch_topk_dense(h.cuda(), training=True)
    assert (nnz == s).all()
    assert torch.equal(idx.cpu(), torch.arange(s, dtype=torch.int32)[None, :].expand(n, s))
    assert torch.equal(val.cpu(), h)


@pytest.mark.encoder_modes("f32")
def test_eval_mode_is_an_elementwise_strict_threshold(encoder_mode):
    n, s = 70, 512
    eng = btk_engine(16, s, 4, 128)
    h = torch.randn(n, s, generator=torch.Generator().manual_seed(5))
    h[0, :5] = 0.75  # equal to the threshold: not kept
    for thr in (0.75, 0.0, -1.0):
        eng.threshold.fill_(thr)
        idx, val, nnz = eng.batch_topk_dense(h.cuda(), training=False)
        check_form(idx, val, nnz)
        f, _ = rows_to_dense(idx, val, nnz, s)
        assert torch.equal(f.cpu(), torch.where(h > max(thr, 0.0), h, torch.zeros(())))
        assert float(eng.threshold) == thr  # eval mode never moves it


def test_encode_keeps_everything_clear_of_the_cut(encoder_mode):
    """From x: exactly n * k codes, every entry above cut + tol kept, none below cut - tol (fp64 sort), values within tol."""
    d, s, k, n = 64, 2048, 8, 333
    eng = btk_engine(d, s, k, 512)
    eng.load_params(R.init_params(R.RefConfig(d_model=d, d_sae=s), torch.Generator().manual_seed(6)))
    x = torch.randn(n, d, generator=torch.Generator().manual_seed(7)).cuda()
    idx, val, nnz = eng.encode_batch_topk(x, training=True)
    check_form(idx, val, nnz)
    assert int(nnz.sum()) == n * k
    W, be = eng.view("W_enc").double(), eng.view("b_enc").double()
    h = x.double() @ W + be
    tol = dot_tol(x, eng.view("W_enc"), eng.view("b_enc"))
    cut = h.flatten().sort(descending=True).values[n * k - 1]
    f, m = rows_to_dense(idx, val, nnz, s)
    got = f != 0
    assert (got | ~(h > cut + tol)).all(), "an entry clearly above the cut is missing"
    assert (~got | (h > cut - tol)).all(), "an entry clearly below the cut was kept"
    assert ((f.double() - h).abs()[got] <= tol).all()


# ------------------------------------------------------------------------------------------------
# forward, eval mode and the module API against the reference
# ------------------------------------------------------------------------------------------------


def _load_module(tmp_path, g):
    from saev_amd import nn

    path = tmp_path / "sae.pt"
    path.write_bytes(g["ckpt"].numpy().tobytes())
    return nn.load(path, device="cuda")


@pytest.mark.parametrize("tag", ["p1", "p4"])
def test_objective_forward_matches_the_reference(tmp_path, monkeypatch, tag, encoder_mode):
    from saev_amd.nn import objectives as O

    g = load_golden("g20_batch_topk_forward")
    assert float(g["gap"]) >= 16 * float(g["bound"])
    sae = _load_module(tmp_path, g).train()
    n_pre = 1 if tag == "p1" else len(g["prefixes"])
    obj = O.get_objective(O.Matryoshka(n_prefixes=n_pre)).train()
    monkeypatch.setattr(O, "sample_prefixes", lambda d_sae, n, *a, **kw: g["prefixes"].clone() if n > 1 else torch.tensor([d_sae]))
    x = g["x"].cuda()
    assert float(sae.activation.threshold) == float(g["thr_before"])
    with torch.no_grad():
        loss, out = obj(sae, x)
    assert math.isclose(float(loss.mse), float(g[f"{tag}_mse"]), rel_tol=1e-4)
    assert float(loss.aux) == 0.0 == float(g[f"{tag}_aux"])
    assert math.isclose(float(loss.l0), float(g[f"{tag}_l0"]), rel_tol=1e-6)
    assert math.isclose(float(loss.l1), float(g[f"{tag}_l1"]), rel_tol=1e-5)
    check_form(out.idx, out.val, out.row_nnz)
    assert int(out.row_nnz.sum()) == x.shape[0] * int(g["k"]) and int((out.row_nnz == 0).sum()) > 0
    torch.testing.assert_close(out.f_x.cpu(), g["f_x"], rtol=1e-5, atol=1e-5)
    assert torch.equal(out.f_x.cpu() != 0, g["f_x"] != 0)
    torch.testing.assert_close(out.h_x.cpu(), g["h_x"], rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(out.x_hats.cpu(), g[f"{tag}_x_hats"], rtol=1e-5, atol=1e-5)
    thr_tol = float(g["bound"]) + 1e-6
    assert abs(float(sae.activation.threshold) - float(g[f"{tag}_thr_after"])) <= thr_tol
    assert float(sae.activation.threshold) == float(sae._eng().threshold)  # the buffer IS the device word


@pytest.mark.parametrize("tag", ["thr", "zero"])
def test_eval_mode_codes_match_the_reference(tmp_path, tag, encoder_mode):
    g = load_golden("g20_batch_topk_forward")
    sae = _load_module(tmp_path, g).eval()
    thr = float(g["thr_before"]) if tag == "thr" else 0.0
    sae.activation.threshold.fill_(thr)
    x = g["x"].cuda()
    out = sae(x)
    check_form(out.idx, out.val, out.row_nnz)
    # entries farther than 2 tol from the threshold are decided alike by any two fp32 evaluations of h
    sure = (g["h_x"].double() - thr).abs() > 2 * float(g["bound"])
    assert int((~sure).sum()) <= 4
    f = out.f_x.cpu()
    assert torch.equal((f != 0)[sure], (g[f"eval_{tag}_f_x"] != 0)[sure])
    torch.testing.assert_close(torch.where(sure, f, 0.0), torch.where(sure, g[f"eval_{tag}_f_x"], 0.0), rtol=1e-5, atol=1e-5)
    if bool(torch.equal(f != 0, g[f"eval_{tag}_f_x"] != 0)):
        torch.testing.assert_close(out.x_hats.cpu(), g[f"eval_{tag}_x_hats"], rtol=1e-5, atol=1e-5)
    assert float(sae.activation.threshold) == thr
    if tag == "zero":
        assert int(out.row_nnz.max()) > 64 and sae._eng().row_regrows >= 1  # eval right after init is dense: the rows grew


def test_module_api_matches_the_reference(tmp_path, encoder_mode):
    g = load_golden("g20_batch_topk_forward")
    sae = _load_module(tmp_path, g)
    assert sae.training
    x = g["x"].cuda()
    m, tol = float(g["momentum"]), float(g["bound"]) + 1e-6
    out = sae(x)  # training mode: the batch-wide select, and the threshold moves
    torch.testing.assert_close(out.f_x.cpu(), g["f_x"], rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(out.h_x.cpu(), g["h_x"], rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(out.x_hats.cpu(), g["p1_x_hats"], rtol=1e-5, atol=1e-5)
    t1 = float(sae.activation.threshold)
    assert abs(t1 - float(g["p1_thr_after"])) <= tol
    enc = sae.encode(x)  # ... on every training-mode encode, as in the reference
    torch.testing.assert_close(enc.f_x.cpu(), g["f_x"], rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(enc.h_x.cpu(), g["h_x"], rtol=1e-5, atol=1e-5)
    vmin = enc.f_x[enc.f_x > 0].min().cpu()
    want = torch.tensor(t1).mul_(1 - m).add_(m * vmin)
    assert float(sae.activation.threshold) == float(want)
    idx, val, nnz = sae.encode_sparse(x)
    check_form(idx, val, nnz)
    torch.testing.assert_close(sae._eng().scatter_rows(idx, val, nnz), enc.f_x, rtol=0, atol=0)
    torch.testing.assert_close(sae.decode(enc.f_x).cpu(), g["p1_x_hats"], rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(sae.decode(enc.f_x, prefixes=g["prefixes"]).cpu(), g["p4_x_hats"], rtol=1e-5, atol=1e-5)
    # the activation module alone on a dense matrix; eval mode afterwards leaves the threshold where it is
    t3 = float(sae.eval().activation.threshold)
    f_eval = sae.activation(enc.h_x)
    assert torch.equal(f_eval, torch.where(enc.h_x > t3, enc.h_x, torch.zeros((), device="cuda")))
    assert float(sae.activation.threshold) == t3
    # dump carries the moved threshold
    from saev_amd import nn

    nn.dump(tmp_path / "moved.pt", sae)
    assert float(nn.load(tmp_path / "moved.pt").activation.threshold) == t3


# ------------------------------------------------------------------------------------------------
# gradients: a dense fp64 autograd restatement, teacher-forced on the GPU's own selection
# ------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("case", ["plain", "prefixes", "dead"])
def test_gradients_match_a_dense_autograd_restatement(case, encoder_mode):
    g = load_golden("g20_batch_topk_train_p1")
    d, s, k, b, k_aux = int(g["d"]), int(g["s"]), int(g["k"]), int(g["bsz"]), int(g["k_aux"])
    thr = 2 * b if case == "dead" else 10_000_000
    eng = btk_engine(d, s, k, b, k_aux=k_aux, alpha=float(g["alpha"]), thr=thr, normalize_w_dec=False, remove_parallel_grads=False)
    params = {key: g["init_" + key].clone() for key in R.PARAM_ORDER}
    eng.load_params(params)
    prefixes = torch.tensor([5, 40, 120, s]) if case == "prefixes" else None
    eng.set_prefixes(prefixes)
    x = g["acts"][:b]
    toks = torch.zeros(s, dtype=torch.int64)
    if case == "dead":  # latents one batch short of dead: those the batch leaves silent die in this step
        toks[torch.randperm(s, generator=torch.Generator().manual_seed(8))[:120]] = b
    eng.set_tracker(toks)
    eng.step_forward(x.cuda(), training=True)
    eng.step_dead(b)
    eng.step_backward()
    st = eng.read_stats()
    idx, val, _, nnz = eng.last_codes(b, row_nnz=True)
    check_form(idx, val, nnz)
    f, _ = rows_to_dense(idx, val, nnz, s)
    # the band check first: the GPU's selection is the fp64 one outside +- tol of the cut, exactly n k codes
    h64 = x.double() @ params["W_enc"].double() + params["b_enc"].double()
    tol = dot_tol(x, params["W_enc"], params["b_enc"])
    cut = h64.flatten().sort(descending=True).values[b * k - 1]
    got = (f != 0).cpu()
    assert int(nnz.sum()) == b * k
    assert (got | ~(h64 > cut + tol)).all() and (~got | (h64 > cut - tol)).all()
    dead = R.update_dead_tracker(toks.clone(), f.cpu(), thr)
    assert torch.equal(eng.toks_since_active.cpu(), torch.where((f.cpu().abs() > 0).any(dim=0), 0, toks + b))
    assert st.n_dead == int(dead.sum()) and (case != "dead" or st.n_dead >= 1)
    mse, aux, grads = restated_gradients(params, x, got, dead, prefixes, k_aux, float(g["alpha"]))  # in fp64
    assert math.isclose(st.mse, mse, rel_tol=1e-4)
    assert math.isclose(st.aux, aux, rel_tol=1e-4, abs_tol=1e-9) and (case != "dead" or st.aux > 0)
    assert math.isclose(st.l0, float(k), rel_tol=1e-6)
    # every element within BOUND of its tensor's largest (tests/step_restatement.py; the fixture's shape is one more row of BTK_SHAPES)
    assert_grads_close({key: v.cpu() for key, v in eng.grad_views().items()}, grads, BOUND, what=f"{case}: ")


@pytest.mark.parametrize("tag", ["p1", "p4"])
@pytest.mark.parametrize("fused", [False, True])
def test_adam_trajectory_matches_the_reference(tag, fused, encoder_mode):
    """Four steps with renormalisation, rpg, an active clip and (from step 2) dead latents and a non-zero AuxK term."""
    g = load_golden(f"g20_batch_topk_train_{tag}")
    d, s, k, b = int(g["d"]), int(g["s"]), int(g["k"]), int(g["bsz"])
    assert (g["log_gap"] >= 16 * g["log_bound"]).all() and g["log_n_dead"].max() >= 1 and g["log_aux"].max() > 0
    eng = btk_engine(d, s, k, b, k_aux=int(g["k_aux"]), alpha=float(g["alpha"]), thr=int(g["thr_tokens"]),
                     batch_momentum=float(g["momentum"]))
    eng.load_params({key: g["init_" + key] for key in R.PARAM_ORDER})
    eng.threshold.copy_(g["init_activation_threshold"])
    eng.set_prefixes(g["prefixes"] if len(g["prefixes"]) > 1 else None)
    lr, clip = float(g["lr"]), float(g["grad_clip"])
    thr_tol = float(g["log_bound"].max()) + 1e-6
    for i in range(int(g["n_steps"])):
        x = g["acts"][i * b:(i + 1) * b].cuda()
        if fused:
            eng.train_step(x, lr, clip)
        else:
            eng.step_forward(x, training=True)
            eng.step_dead(b)
            eng.step_backward()
            idx, val, _, nnz = eng.last_codes(b, row_nnz=True)
            f, _ = rows_to_dense(idx, val, nnz, s)
            assert torch.equal((f != 0).cpu(), g["f_x"][i] != 0), f"step {i}: the selection differs (gap {float(g['log_gap'][i]):.2e})"
            torch.testing.assert_close(f.cpu(), g["f_x"][i], rtol=1e-5, atol=1e-5)
            eng.step_tail(lr, clip)
        st = eng.read_stats()
        # (the tolerances test_g9_golden_train_trajectory applies to the same quantities of a free-running trajectory -- without its
        # allowance for flipped selections: the fixture's gaps rule them out)
        assert math.isclose(st.mse, float(g["log_mse"][i]), rel_tol=1e-4), (i, st.mse)
        assert math.isclose(st.aux, float(g["log_aux"][i]), rel_tol=1e-3, abs_tol=1e-8), (i, st.aux)
        assert math.isclose(st.l0, float(g["log_l0"][i]), rel_tol=1e-6) and math.isclose(st.l1, float(g["log_l1"][i]), rel_tol=1e-4)
        assert st.n_dead == int(g["log_n_dead"][i])
        assert math.isclose(st.grad_norm, float(g["log_grad_norm"][i]), rel_tol=2e-3) and st.grad_norm > clip
        assert abs(float(eng.threshold) - float(g["log_thr"][i])) <= thr_tol, (i, float(eng.threshold), float(g["log_thr"][i]))
        for key in ("b_enc", "b_dec"):
            bad = ~torch.isclose(eng.view(key).cpu(), g[key + "_steps"][i], rtol=2e-3, atol=5e-5)
            assert bad.float().mean() < 2e-3, f"step {i} {key}: {bad.sum().item()} of {bad.numel()} elements off"
    assert torch.equal(eng.toks_since_active.cpu(), g["toks_final"])
    for key in R.PARAM_ORDER:
        bad = ~torch.isclose(eng.view(key).cpu(), g["final_" + key], rtol=2e-3, atol=5e-5)
        assert bad.float().mean() < 2e-3, f"{key}: {bad.sum().item()} of {bad.numel()} elements off"


@pytest.mark.encoder_modes("f32")
def test_muon_tail_after_the_phases_matches_torch(encoder_mode):
    """The phases + muon_tail against tests/test_gpu_muon.py's restatement: torch's Muon and fused Adam on the engine's own
    projected gradient times the clip coefficient formed from the tail's own sum of squares."""
    from test_gpu_muon import NS_REL_TOL, _segments, rel

    g = load_golden("g20_batch_topk_train_p1")
    d, s, k, b = int(g["d"]), int(g["s"]), int(g["k"]), int(g["bsz"])
    eng = btk_engine(d, s, k, b, k_aux=int(g["k_aux"]), alpha=float(g["alpha"]), thr=int(g["thr_tokens"]))
    eng.load_params({key: g["init_" + key] for key in R.PARAM_ORDER})
    max_norm = float(g["grad_clip"])
    W = {k_: torch.nn.Parameter(eng.view(k_).clone()) for k_ in R.PARAM_ORDER}
    muon = torch.optim.Muon([W["W_dec"], W["W_enc"]], lr=0.0)
    adam = torch.optim.Adam([W["b_dec"], W["b_enc"]], lr=0.0, fused=True)
    for step, lr in enumerate((1e-3, 2e-3, 1e-3)):
        x = g["acts"][step * b:(step + 1) * b].cuda()
        eng.step_forward(x, training=True, n_rows_global=b)
        eng.step_dead(b)
        eng.step_backward()
        before = _segments(eng, eng.params)
        eng.muon_tail(lr, max_norm)
        torch.cuda.synchronize()
        grads = _segments(eng, eng.grads)
        norm = torch.tensor(math.sqrt(eng.sumsq.item()), dtype=torch.float32)  # (the tail: the root in fp64, rounded once to fp32)
        coef = torch.clamp(torch.tensor(max_norm, dtype=torch.float32) / (norm + 1e-6), max=1.0)
        for k_ in R.PARAM_ORDER:
            W[k_].data.copy_(before[k_])
            W[k_].grad = grads[k_] * coef.cuda()
        for opt in (muon, adam):
            for pg in opt.param_groups:
                pg["lr"] = lr
            opt.step()
        after = _segments(eng, eng.params)
        mom = _segments(eng, eng.adam_m)
        for k_ in ("W_dec", "W_enc"):
            assert torch.equal(mom[k_], muon.state[W[k_]]["momentum_buffer"]), f"step {step}: {k_} momentum differs from torch's lerp_"
            e = rel(after[k_] - before[k_], W[k_].data - before[k_])
            assert e <= NS_REL_TOL, (step, k_, e)
        for k_ in ("b_dec", "b_enc"):
            torch.testing.assert_close(after[k_], W[k_].data, rtol=1e-4, atol=1e-6)
    assert eng.read_stats().n_dead >= 1  # (the third step has dead latents: the AuxK gradient went through the Muon tail too)
    eng.train_step_muon(g["acts"][3 * b:4 * b].cuda(), 1e-3, max_norm)  # the same phases and tail in one call
    assert eng.adam_steps == 4 and float(eng.threshold) > 0


# ------------------------------------------------------------------------------------------------
# overflow: the rows grow, nothing else changes
# ------------------------------------------------------------------------------------------------


def test_a_context_with_small_rows_grows_and_gives_identical_results(encoder_mode):
    """top_k = 64 on 256 latents: rows of 64 codes on average, so a context created with row_cap = 64 meets longer ones in its first
    forward.  After the automatic regrow: bit-identical codes, losses, gradients and threshold to a context created large enough."""
    g = load_golden("g20_batch_topk_train_p1")
    d, s, b = int(g["d"]), int(g["s"]), int(g["bsz"])
    x = g["acts"][:b].cuda()
    res, engs = [], []
    for row_cap in (64, 256):
        eng = btk_engine(d, s, 64, b, k_aux=int(g["k_aux"]), thr=int(g["thr_tokens"]), row_cap=row_cap)
        assert eng.row_cap == row_cap
        eng.load_params({key: g["init_" + key] for key in R.PARAM_ORDER})
        eng.threshold.fill_(0.25)
        eng.step_forward(x, training=True)
        eng.step_dead(b)
        eng.step_backward()
        st = eng.read_stats()
        idx, val, x_hat, nnz = eng.last_codes(b, row_nnz=True)
        check_form(idx, val, nnz)
        f, _ = rows_to_dense(idx, val, nnz, s)
        res.append((f, nnz, x_hat, (st.mse, st.aux, st.l0, st.l1, st.n_dead), eng.grads.clone(), float(eng.threshold)))
        engs.append(eng)
    small, large = engs
    assert int(res[1][1].max()) > 64, "the batch must hold a row longer than the small context's rows"
    assert small.row_regrows == 1 and large.row_regrows == 0 and small.row_cap >= int(res[1][1].max()) and small.row_cap % 64 == 0
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]) and torch.equal(res[0][2], res[1][2])
    assert res[0][3] == res[1][3]
    assert torch.equal(res[0][4], res[1][4]), "gradients differ after the regrow"
    # the EMA ran once: (1 - m) * 0.25 + m * the smallest positive kept value
    vmin = res[1][0][res[1][0] > 0].min().cpu()
    want = torch.tensor(0.25).mul_(1 - 0.1).add_(0.1 * vmin)
    assert res[0][5] == res[1][5] == float(want)
    # the grown rows stay: a tail and a whole step run on them without a second regrow
    small.step_tail(1e-3, 1.0)
    small.train_step(x, 1e-3, 1.0)
    assert small.row_regrows == 1 and small.adam_steps == 2
    # the same through the single ops: encode_batch_topk of a context with small rows
    again = btk_engine(d, s, 64, b, row_cap=64)
    again.load_params({key: g["init_" + key] for key in R.PARAM_ORDER})
    again.threshold.fill_(0.25)
    idx, val, nnz = again.encode_batch_topk(x, training=True)
    f2, _ = rows_to_dense(idx, val, nnz, s)
    assert again.row_regrows == 1 and torch.equal(f2, res[1][0]) and float(again.threshold) == float(want)


@pytest.mark.encoder_modes("f32")
def test_entries_a_batch_topk_context_refuses(encoder_mode):
    from saev_amd.engine import EngineConfig, SaeEngine

    eng = btk_engine(16, 64, 4, 32)
    topk = SaeEngine(EngineConfig(d_model=16, d_sae=64, top_k=4, k_aux=0, max_batch=32))
    x = torch.randn(8, 16).cuda()
    pool, rows = torch.randn(64, 16).cuda(), torch.arange(8).cuda()
    for call in (lambda: eng.encode_topk(x), lambda: eng.train_step_gather(pool, rows, 1e-3), lambda: eng.train_step_dp(x, 1e-3),
                 lambda: eng.share_x(topk), lambda: topk.share_x(eng), lambda: eng.backward_begin()):
        with pytest.raises(NotImplementedError):
            call()
    with pytest.raises(NotImplementedError):
        btk_engine(16, 64, 4, 32, encoder="bf16")
    eng.step_forward(x, training=True)
    eng.step_dead(8)
    with pytest.raises(Exception, match="all latents"):
        eng.backward_rows(0, 32)


# ------------------------------------------------------------------------------------------------
# end to end
# ------------------------------------------------------------------------------------------------


def _cfg(tmp_path, g, activation, **kw):
    from saev_amd import data
    from saev_amd.framework import train as T
    from saev_amd.nn import modeling as M
    from saev_amd.nn import objectives as O

    dc = data.ShuffledConfig(batch_size=int(g["bsz"]), seed=3)
    return T.Config(train_data=dc, val_data=dc, n_train=int(g["n_train"]), n_val=10**9,
                    sae=M.SparseAutoencoderConfig(d_model=int(g["d"]), d_sae=int(g["s"]), reinit_blend=0.0, activation=activation),
                    objective=O.Matryoshka(n_prefixes=1, dead_threshold_tokens=int(g["thr"])), lr=float(g["lr"]),
                    n_lr_warmup=int(g["n_warm"]), track=False, log_every=5, runs_root=tmp_path / "runs", **kw)


@pytest.mark.encoder_modes("f16r")
@pytest.mark.parametrize("optim", ["adam", "muon"])
def test_train_and_evaluate_alone_and_in_a_group_with_a_topk_sae(tmp_path, optim, encoder_mode):
    from saev_amd.framework import train as T
    from saev_amd.nn import modeling as M

    g = load_golden("g9_train_b")
    k, k_aux = int(g["k"]), int(g["k_aux"])
    btk = _cfg(tmp_path, g, M.BatchTopK(top_k=k, aux=M.AuxK(k_aux=k_aux)), optim=optim)
    topk = _cfg(tmp_path, g, M.TopK(top_k=k, aux=M.AuxK(k_aux=k_aux)), optim=optim)

    def run(cfgs):
        saes, objs, log, steps = T.train(cfgs, train_pool=g["acts"])
        ev = T.evaluate(cfgs, saes, objs, val_pool=g["val"])
        return [{k_: v.detach().cpu().clone() for k_, v in s_.state_dict().items()} for s_ in saes], log, ev, steps

    alone, log, ev, steps = run([btk])
    assert steps == int(g["n_steps"])
    recs = [m for _, m in log.records[0]]
    assert recs and all(math.isfinite(r["loss/mse"]) for r in recs) and recs[-1]["loss/mse"] < recs[0]["loss/mse"]
    assert all(math.isclose(r["loss/l0"], k, rel_tol=1e-6) for r in recs)  # training mode: exactly k codes per row on average
    assert float(alone[0]["activation.threshold"]) > 0
    # (24 steps, most of them warm-up: nothing is claimed about how good the SAE is by then, only that the pass is consistent)
    assert 0 < ev[0].l0 < int(g["s"]) and math.isfinite(ev[0].mse) and ev[0].mse > 0
    assert ev[0].normalized_mse == pytest.approx(ev[0].sse_sae / ev[0].sse_baseline, rel=1e-12)
    assert ev[0].freqs.shape == (int(g["s"]),)
    again, *_ = run([btk])
    for k_ in alone[0]:
        assert torch.equal(alone[0][k_], again[0][k_]), f"{k_} differs between identical runs"
    topk_alone, _, ev_t, _ = run([topk])
    # In a group every member is initialised from one RNG stream, so only the FIRST member starts where it starts alone: it must
    # end bit for bit where it ends alone, whoever else trains on its batches.  (A BatchTopK engine shares nothing with the
    # others; a TopK one that follows it neither borrows from it nor draws its batch inside its step.)
    for order, first_alone, ev_alone in (((topk, btk), topk_alone, ev_t), ((btk, topk), alone, ev)):
        both, _, ev_b, _ = run(list(order))
        for k_ in first_alone[0]:
            assert torch.equal(both[0][k_], first_alone[0][k_]), f"{type(order[0].sae.activation).__name__} first, {k_}: differs from training it alone"
        assert ev_b[0].mse == ev_alone[0].mse
        assert all(math.isfinite(e.mse) and e.mse > 0 and 0 < e.l0 < int(g["s"]) for e in ev_b)


@pytest.mark.parametrize("tag", ["plain", "labels"])
def test_inference_artifacts_match_the_reference(tmp_path, tag, encoder_mode):
    from saev_amd import disk
    from saev_amd.data import Metadata, OrderedConfig
    from saev_amd.framework import inference

    g = load_golden(f"g20_inference_batch_topk_{tag}")
    d = write_cache(tmp_path, g)
    md = Metadata.load(d)
    runs_root = tmp_path / "saev" / "runs"
    runs_root.mkdir(parents=True)
    run = disk.Run.new("gpu00020", train_shards_dir=d, val_shards_dir=d, runs_root=runs_root)
    run.ckpt.parent.mkdir(parents=True, exist_ok=True)
    run.ckpt.write_bytes(g["ckpt"].numpy().tobytes())  # the reference's own nn.dump, threshold included
    cfg = inference.Config(run=run.run_dir, data=OrderedConfig(shards=d, layer=11, batch_size=int(g["batch_size"])),
                           n_dists=int(g["n_dists"]), ignore_labels=g["ignore_labels"].tolist())
    inference.worker_fn(cfg)
    out = run.inference / md.hash
    csr = scipy.sparse.load_npz(out / "token_acts.npz")
    assert csr.shape == tuple(g["csr_shape"].tolist())
    assert csr.indices.dtype == np.int32 and csr.indptr.dtype == np.int32 and csr.data.dtype == np.float32
    np.testing.assert_array_equal(csr.indptr, g["csr_indptr"].numpy())
    np.testing.assert_array_equal(csr.indices, g["csr_indices"].numpy())  # no pre-activation within 2e-5 of the threshold here
    np.testing.assert_allclose(csr.data, g["csr_data"].numpy(), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(torch.load(out / "mean_values.pt"), g["mean_values"], rtol=1e-5, atol=1e-6, equal_nan=True)
    torch.testing.assert_close(torch.load(out / "sparsity.pt"), g["sparsity"], rtol=1e-6, atol=0)
    torch.testing.assert_close(torch.load(out / "distributions.pt"), g["distributions"], rtol=1e-5, atol=1e-6)
    got = json.loads((out / "metrics.json").read_text())
    want = dict(zip(g["metrics_keys"].tolist(), g["metrics_vals"].tolist()))
    assert list(got) == list(want)
    for k_, v in want.items():
        assert got[k_] == pytest.approx(v, rel=1e-5), k_
