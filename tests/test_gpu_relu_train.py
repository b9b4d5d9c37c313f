"""ReLU SAEs TRAIN on the MI355X (needs -m gpu): the dense step against the reference's own trajectories (fixtures G22,
tools/gen_golden_relu_train.py), every gradient element against an fp64 restatement in each class of the step's geometry
(tests/relu_step_restatement.py: RELU_SHAPES), determinism, the compaction of the dense codes (saev_copy_last_rows), train() /
evaluate() end to end, Muon, and the refusals.

Tolerances.  G22: the mask of every step EQUALS the fixture's (its pre-activations keep >= 16 fp32 bounds from zero: stored, asserted
in tests/test_relu_train_host_cpu.py); f_x at 1e-5 / 1e-5; mse, sparsity, l0, l1 and the gradient norm at rel 1e-5; the gradients of
step 1 element by element at BOUND = 2e-5 of each tensor's largest element (tests/step_restatement.py); parameters at 2e-3 / 5e-5 on
all but 2e-3 of the elements, as tests/test_gpu_batch_topk.py holds its free-running trajectory.  Geometry: BOUND against the fp64
restatement teacher-forced on the step's own mask, which must equal the fp64 mask (everywhere at the table's fixed seeds; outside the
band of 2 fp32 bounds around zero for the step that follows the tail, whose parameters the tail made)."""

import math

import pytest
import torch

import sae_ref as R
from conftest import load_golden
from relu_step_restatement import L1_COEFF, RELU_SHAPES, relu_bound, relu_input_conditions, relu_restated_gradients, relu_row_inputs
from step_restatement import BOUND, assert_grads_close

pytestmark = pytest.mark.gpu

TAGS = ("l1", "nosparsity")


def rt_engine(d, s, b, *, l1=0.0, thr=10_000_000, **kw):
    from saev_amd.engine import EngineConfig, SaeEngine

    return SaeEngine(EngineConfig(d_model=d, d_sae=s, k_aux=0, alpha=0.0, dead_threshold_tokens=thr, max_batch=b, activation="relu_train",
                                  l1_coeff=l1, **kw))


def rows_to_dense(idx, val, nnz, s):
    """Dense f of padded rows, after checking their form: ascending latents in the first nnz slots, idx = -1 / val = 0 behind them."""
    n, cap = idx.shape
    idx, val, nnz = idx.cpu(), val.cpu(), nnz.cpu()
    assert int(nnz.max()) <= cap
    slot = torch.arange(cap)[None, :]
    live = slot < nnz[:, None]
    assert (idx[~live] == -1).all() and (val[~live] == 0).all() and (val[live] > 0).all()
    asc = (idx[:, 1:] > idx[:, :-1]) | ~live[:, 1:]
    assert asc.all() and (idx[live] >= 0).all() and (idx[live] < s).all()
    f = torch.zeros(n, s)
    rows = torch.arange(n)[:, None].expand_as(idx)
    f[rows[live], idx[live].long()] = val[live]
    return f


def sparsity_of(l1: float, coeff: float) -> float:
    return float(torch.tensor(l1, dtype=torch.float32) * coeff)  # (as the reference forms it: an fp32 tensor times a Python float)


# ------------------------------------------------------------------------------------------------
# G22: the reference's own trajectories
# ------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("fused", [False, True])
def test_adam_trajectory_matches_the_reference(tag, fused, encoder_mode):
    """Four steps with renormalisation, rpg, an active clip and (from step 2) dead latents, through the phases and through train_step."""
    g = load_golden(f"g22_relu_train_{tag}")
    d, s, b, coeff = int(g["d"]), int(g["s"]), int(g["bsz"]), float(g["l1_coeff"])
    silent = g["silent"]
    eng = rt_engine(d, s, b, l1=coeff, thr=int(g["thr_tokens"]))
    eng.load_params({key: g["init_" + key] for key in R.PARAM_ORDER})
    lr, clip = float(g["lr"]), float(g["grad_clip"])
    for i in range(int(g["n_steps"])):
        x = g["acts"][i * b:(i + 1) * b].cuda()
        if fused:
            eng.train_step(x, lr, clip)
            idx, val, _, nnz = eng.last_codes(b, row_nnz=True)  # (the step's dense f is still in place after the tail)
            f = rows_to_dense(idx, val, nnz, s)
            assert torch.equal(f > 0, g["f_x"][i] > 0), f"step {i}: the mask differs (gap {float(g['log_gap'][i]):.2e})"
            torch.testing.assert_close(f, g["f_x"][i], rtol=1e-5, atol=1e-5)
        else:
            eng.step_forward(x, training=True)
            eng.step_dead(b)
            eng.step_backward()
            idx, val, _, nnz = eng.last_codes(b, row_nnz=True)
            f = rows_to_dense(idx, val, nnz, s)
            assert torch.equal(f > 0, g["f_x"][i] > 0), f"step {i}: the mask differs (gap {float(g['log_gap'][i]):.2e})"
            torch.testing.assert_close(f, g["f_x"][i], rtol=1e-5, atol=1e-5)
            grads = {k: v.cpu().clone() for k, v in eng.grad_views().items()}
            # latents that never fire: exactly zero rows in all three of their gradients
            assert not grads["W_dec"][silent].any() and not grads["W_enc"][:, silent].any() and not grads["b_enc"][silent].any()
            if i == 0:
                ratios = assert_grads_close(grads, {k: g["grad1_" + k] for k in R.PARAM_ORDER}, BOUND, what=f"G22 {tag} step 1: ")
                print(f"G22 {tag} {encoder_mode}: step-1 gradients, worst |difference| / max: " + "  ".join(f"{k} {v:.2e}" for k, v in ratios.items()))
            eng.step_tail(lr, clip)
        st = eng.read_stats()
        got = {"mse": st.mse, "sparsity": sparsity_of(st.l1, coeff), "l0": st.l0, "l1": st.l1, "grad_norm": st.grad_norm}
        print(f"G22 {tag} {encoder_mode} fused={fused} step {i}: " + "  ".join(f"{k} {v:.9g} (ref {float(g['log_' + k][i]):.9g})" for k, v in got.items()))
        for k, v in got.items():
            assert math.isclose(v, float(g["log_" + k][i]), rel_tol=1e-5, abs_tol=0.0 if float(g["log_" + k][i]) else 1e-30), (i, k, v)
        assert st.aux == 0.0 and eng.aux_route() == 0
        assert st.n_dead == int(g["log_n_dead"][i])
        assert st.grad_norm > clip
        for key in ("b_enc", "b_dec"):
            bad = ~torch.isclose(eng.view(key).cpu(), g[key + "_steps"][i], rtol=2e-3, atol=5e-5)
            assert bad.float().mean() < 2e-3, f"step {i} {key}: {bad.sum().item()} of {bad.numel()} elements off"
    assert torch.equal(eng.toks_since_active.cpu(), g["toks_final"])
    for key in R.PARAM_ORDER:
        bad = ~torch.isclose(eng.view(key).cpu(), g["final_" + key], rtol=2e-3, atol=5e-5)
        assert bad.float().mean() < 2e-3, f"{key}: {bad.sum().item()} of {bad.numel()} elements off"


@pytest.mark.parametrize("tag", TAGS)
def test_objective_returns_the_reference_loss_fields_and_gradients(tag, encoder_mode):
    """The module API: a Relu module builds the forward-only engine until an objective binds it, the training engine afterwards
    (parameters carried over); the objective's loss fields, Output and loss.backward() against the fixture's first step."""
    from saev_amd.nn import modeling as M
    from saev_amd.nn import objectives as O

    g = load_golden(f"g22_relu_train_{tag}")
    d, s, b, coeff = int(g["d"]), int(g["s"]), int(g["bsz"]), float(g["l1_coeff"])
    sparsity = M.L1Sparsity(coeff=coeff) if coeff else M.NoSparsity()
    sae = M.SparseAutoencoder(M.SparseAutoencoderConfig(d_model=d, d_sae=s, reinit_blend=0.0, activation=M.Relu(sparsity=sparsity)))
    sae.load_state_dict({key: g["init_" + key] for key in R.PARAM_ORDER})
    sae = sae.to("cuda")
    x = g["acts"][:b].cuda()
    sae.normalize_w_dec()
    assert sae._eng().cfg.activation == "relu"
    out0 = sae(x)
    obj = O.get_objective(O.Matryoshka(n_prefixes=1, dead_threshold_tokens=int(g["thr_tokens"])))
    loss, out = obj(sae, x)
    assert sae._eng().cfg.activation == "relu_train"
    torch.testing.assert_close(sae.W_enc.detach().cpu(), g["init_W_enc"], rtol=0, atol=0)  # the rebuild carried the parameters over
    assert math.isclose(loss.mse.item(), float(g["log_mse"][0]), rel_tol=1e-5) and math.isclose(loss.l1.item(), float(g["log_l1"][0]), rel_tol=1e-5)
    assert loss.l0.item() == float(g["log_l0"][0]) and loss.aux.item() == 0.0 and int(loss.n_dead) == 0
    assert math.isclose(loss.sparsity.item(), float(g["log_sparsity"][0]), rel_tol=1e-5, abs_tol=0.0 if coeff else 1e-30)
    assert math.isclose(loss.loss.item(), float(g["log_mse"][0]) + float(g["log_sparsity"][0]), rel_tol=1e-5)
    assert out.row_nnz is not None and torch.equal(out.f_x.cpu() > 0, g["f_x"][0] > 0)
    torch.testing.assert_close(out.f_x.cpu(), g["f_x"][0], rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(out.f_x, out0.f_x, rtol=1e-6, atol=1e-6)  # the forward-only engine saw the same codes
    loss.loss.backward()
    assert_grads_close({k: getattr(sae, k).grad for k in R.PARAM_ORDER}, {k: g["grad1_" + k] for k in R.PARAM_ORDER}, BOUND, what=f"G22 {tag}: ")


# ------------------------------------------------------------------------------------------------
# geometry: every gradient element in every class of the dense step
# ------------------------------------------------------------------------------------------------


def _step_and_check(eng, row_id, x, bound, strict_mask):
    """One training forward + backward; the step's mask against fp64, its gradients against the restatement on that mask."""
    n, s = x.shape[0], eng.cfg.d_sae
    eng.step_forward(x, training=True)
    eng.step_dead(n)
    eng.step_backward()
    p = {k: v.cpu().clone() for k, v in eng.param_views().items()}  # (W_dec as the forward renormalised it)
    idx, val, x_hat, nnz = eng.last_codes(n, row_nnz=True)
    mask = rows_to_dense(idx, val, nnz, s) > 0
    h = x.cpu().double() @ p["W_enc"].double() + p["b_enc"].double()
    band = h.abs() <= 2 * relu_bound(x.cpu(), p["W_enc"], p["b_enc"])
    if strict_mask:
        assert not band.any(), f"{row_id}: a pre-activation within two fp32 bounds of zero"
    assert torch.equal(mask | band, (h > 0) | band), f"{row_id}: the step's mask differs from fp64 outside the band"
    mse, l1, ref = relu_restated_gradients(p, x.cpu(), mask, L1_COEFF)
    st = eng.read_stats()
    assert math.isclose(st.mse, mse, rel_tol=1e-5) and math.isclose(st.l1, l1, rel_tol=1e-5), (row_id, st.mse, mse, st.l1, l1)
    assert st.l0 == pytest.approx(float(mask.sum(dim=1).float().mean()), rel=1e-6)
    x_hat64 = (h * mask) @ p["W_dec"].double() + p["b_dec"].double()
    assert (x_hat.cpu().double() - x_hat64).abs().max() <= BOUND * x_hat64.abs().max()
    ratios = assert_grads_close({k: v.cpu() for k, v in eng.grad_views().items()}, ref, bound, what=f"{row_id}: ")
    print(f"{row_id}: worst |difference| / max|fp64|: " + "  ".join(f"{k} {v:.2e}" for k, v in ratios.items()))
    return mask, ref


@pytest.mark.parametrize("row", RELU_SHAPES, ids=lambda r: r.id)
def test_gradients_match_the_fp64_restatement_in_every_class(row, encoder_mode):
    p, x = relu_row_inputs(row)
    mask64, _ = relu_input_conditions(p["W_enc"], p["b_enc"], x)
    eng = rt_engine(row.d, row.s, row.n, l1=L1_COEFF)
    eng.load_params(p)
    mask, ref = _step_and_check(eng, f"{row.id} step 1", x.cuda(), row.bound, strict_mask=True)
    assert torch.equal(mask, mask64)
    if row.quiet_row:
        assert not mask[0].any()
    if row.extremes:
        g = {k: v.cpu() for k, v in eng.grad_views().items()}
        assert not mask[:, 1].any() and mask[:, 2].all()
        assert not g["W_dec"][1].any() and not g["W_enc"][:, 1].any() and g["b_enc"][1] == 0
    # the tail, and the step after it (parameters the tail wrote; another batch)
    eng.step_tail(1e-3, 1.0)
    x2 = torch.randn(row.n, row.d, generator=torch.Generator().manual_seed(row.seed + 77))
    _step_and_check(eng, f"{row.id} step 2", x2.cuda(), row.bound, strict_mask=False)


@pytest.mark.encoder_modes("f32")
def test_one_split_of_the_weight_gradients(encoder_mode):
    """256 tiles of 256 x 256 in a weight gradient: ksplit_shape gives ONE split (the table's rows all have 16), the contraction
    writes straight into the gradient buffer, Kp = 32 for 20 rows.  (164 k pre-activations: some lie within the band, where the
    step's own mask decides.)"""
    d, s, n = 2048, 8192, 20
    from test_gpu_parity import rand_params

    eng = rt_engine(d, s, n, l1=L1_COEFF)
    eng.load_params(rand_params(d, s, seed=1))
    x = torch.randn(n, d, generator=torch.Generator().manual_seed(2))
    _step_and_check(eng, f"{n}x{d}x{s}", x.cuda(), BOUND, strict_mask=False)


def test_a_smaller_batch_after_a_full_one_on_the_same_context(encoder_mode):
    """The ragged last batch of train() / evaluate(): the context lays its k-major operand images out for Kp(max_batch) = 512 and
    a step of n rows uses Kp(n) = 256 of it (n = 65, n = 1), over whatever the full batch before left there; then a full batch
    again.  Every step against the restatement, a tail between them."""
    from test_gpu_parity import rand_params

    d, s, mb = 100, 1004, 300
    eng = rt_engine(d, s, mb, l1=L1_COEFF)
    eng.load_params(rand_params(d, s, seed=12))
    for i, n in enumerate((300, 65, 1, 300)):
        if i:
            eng.step_tail(1e-3, 1.0)
        x = torch.randn(n, d, generator=torch.Generator().manual_seed(40 + i))
        _step_and_check(eng, f"max_batch {mb}, step {i} of {n} rows", x.cuda(), BOUND, strict_mask=False)


def test_the_same_step_twice_gives_the_same_bits(encoder_mode):
    row = RELU_SHAPES[2]
    p, x = relu_row_inputs(row)
    x = x.cuda()
    out = []
    for _ in range(2):
        eng = rt_engine(row.d, row.s, row.n, l1=L1_COEFF)
        eng.load_params(p)
        per = []
        for _ in range(2):
            eng.step_forward(x, training=True)
            eng.step_dead(row.n)
            eng.step_backward()
            per.append(eng.grads.clone())
            eng.step_tail(1e-3, 0.5)
            per.append(eng.params.clone())
            per.append(torch.tensor(list(vars(eng.read_stats()).values()), dtype=torch.float64))
        eng.train_step(x, 1e-3, 0.5)
        per.append(eng.params.clone())
        out.append(per)
    for a, b in zip(*out):
        assert torch.equal(a.cpu(), b.cpu())


# ------------------------------------------------------------------------------------------------
# saev_copy_last_rows
# ------------------------------------------------------------------------------------------------


def test_copy_last_rows_is_the_nonzero_of_the_dense_codes(encoder_mode):
    import ctypes as C

    row = RELU_SHAPES[1]
    p, x = relu_row_inputs(row)
    x = x.cuda()
    eng = rt_engine(row.d, row.s, row.n)
    eng.load_params(p)
    eng.relu_row_cap = 8  # far too small: the first launch reports the longest row, the second holds every row
    eng.step_forward(x, training=False)
    f = torch.relu(eng.encode_dense(x))  # the step's h comes from the same exact encoder: the same bits
    idx, val, x_hat, nnz = eng.last_codes(row.n, row_nnz=True)
    longest = int((f > 0).sum(dim=1).max())
    assert eng.relu_second_launches == 1 and eng.relu_row_cap >= longest and idx.shape[1] == longest
    assert torch.equal(nnz.cpu(), (f > 0).sum(dim=1).int().cpu())
    nz = torch.nonzero(f)  # row-major: ascending latents within each row
    live = (torch.arange(idx.shape[1])[None, :] < nnz.cpu()[:, None])
    assert torch.equal(idx.cpu()[live].long(), nz[:, 1].cpu()) and torch.equal(val.cpu()[live], f[f > 0].cpu())
    assert torch.equal(rows_to_dense(idx, val, nnz, row.s), f.cpu())
    idx2, val2, _ = eng.last_codes(row.n, x_hat=False)
    assert eng.relu_second_launches == 1 and torch.equal(idx2[:, :longest], idx) and torch.equal(val2[:, :longest], val)
    # a capacity one short of the longest row: that row's count is reported, its first cap entries are stored, nothing else changes
    cap = longest - 1
    over = torch.full((1,), -5, device="cuda", dtype=torch.int32)
    n3 = torch.empty(row.n, device="cuda", dtype=torch.int32)
    i3 = torch.empty(row.n, cap, device="cuda", dtype=torch.int32)
    v3 = torch.empty(row.n, cap, device="cuda", dtype=torch.float32)
    s_ = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = eng.lib.saev_copy_last_rows(eng.ctx, row.n, cap, C.c_void_p(n3.data_ptr()), C.c_void_p(i3.data_ptr()), C.c_void_p(v3.data_ptr()),
                                     C.c_void_p(over.data_ptr()), s_)
    assert rc == 0 and int(over.item()) == longest and torch.equal(n3, nnz)
    assert torch.equal(i3, idx[:, :cap]) and torch.equal(v3, val[:, :cap])
    assert eng.lib.saev_copy_last_rows(eng.ctx, row.n + 1, cap, C.c_void_p(n3.data_ptr()), C.c_void_p(i3.data_ptr()), C.c_void_p(v3.data_ptr()),
                                       C.c_void_p(over.data_ptr()), s_) == -1  # not the batch of the last forward


# ------------------------------------------------------------------------------------------------
# Muon
# ------------------------------------------------------------------------------------------------


@pytest.mark.encoder_modes("f32")
def test_first_muon_step_matches_torch(encoder_mode):
    """The phases + muon_tail from G22's initial state against tests/test_gpu_muon.py's restatement: torch's Muon and fused Adam on
    the gradients the phases left, projected, times the clip coefficient formed from the tail's own sum of squares."""
    from test_gpu_muon import NS_REL_TOL, _segments, rel

    g = load_golden("g22_relu_train_l1")
    d, s, b = int(g["d"]), int(g["s"]), int(g["bsz"])
    eng = rt_engine(d, s, b, l1=float(g["l1_coeff"]), thr=int(g["thr_tokens"]))
    eng.load_params({key: g["init_" + key] for key in R.PARAM_ORDER})
    max_norm, lr = float(g["grad_clip"]), 1e-3
    W = {k_: torch.nn.Parameter(eng.view(k_).clone()) for k_ in R.PARAM_ORDER}
    muon = torch.optim.Muon([W["W_dec"], W["W_enc"]], lr=lr)
    adam = torch.optim.Adam([W["b_dec"], W["b_enc"]], lr=lr, fused=True)
    x = g["acts"][:b].cuda()
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
    muon.step()
    adam.step()
    after = _segments(eng, eng.params)
    mom = _segments(eng, eng.adam_m)
    for k_ in ("W_dec", "W_enc"):
        assert torch.equal(mom[k_], muon.state[W[k_]]["momentum_buffer"]), f"{k_} momentum differs from torch's lerp_"
        e = rel(after[k_] - before[k_], W[k_].data - before[k_])
        assert e <= NS_REL_TOL, (k_, e)
    for k_ in ("b_dec", "b_enc"):
        torch.testing.assert_close(after[k_], W[k_].data, rtol=1e-4, atol=1e-6)
    eng.train_step_muon(g["acts"][b:2 * b].cuda(), lr, max_norm)  # the same phases and tail in one call
    assert eng.adam_steps == 2


# ------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------


@pytest.mark.encoder_modes("f32")
def test_entries_a_relu_training_context_refuses(encoder_mode):
    from saev_amd.engine import EngineConfig, SaeEngine

    eng = rt_engine(16, 64, 32, l1=1e-2)
    topk = SaeEngine(EngineConfig(d_model=16, d_sae=64, top_k=4, k_aux=0, max_batch=32))
    x = torch.randn(8, 16).cuda()
    pool, rows = torch.randn(64, 16).cuda(), torch.arange(8).cuda()
    bufs = (torch.empty(8, 16).cuda(), torch.empty(8, 16).cuda(), torch.empty(8, 1, dtype=torch.int32).cuda(), torch.empty(8, 1).cuda())
    eng.step_forward(x, training=True)
    eng.step_dead(8)
    for call in (lambda: eng.encode_topk(x), lambda: eng.train_step_gather(pool, rows, 1e-3), lambda: eng.train_step_dp(x, 1e-3),
                 lambda: eng.share_x(topk), lambda: topk.share_x(eng), lambda: eng.backward_begin(), lambda: eng.backward_rows(0, 32),
                 lambda: eng.backward_rows(0, 64), lambda: eng.backward_end(), lambda: eng.backward_begin_gathered(*bufs),
                 lambda: eng.copy_step_state(8, *bufs[1:]), lambda: eng.set_prefixes([8, 64]), lambda: eng.tail_prepare(),
                 lambda: eng.step_forward(x, training=True, n_rows_global=16)):
        with pytest.raises(NotImplementedError):
            call()
    for kw in (dict(encoder="bf16"), dict(shard_world=2), dict(max_backward_rows=64)):
        with pytest.raises(NotImplementedError):
            rt_engine(16, 64, 32, **kw)
    with pytest.raises(ValueError):
        SaeEngine(EngineConfig(d_model=16, d_sae=64, k_aux=8, max_batch=32, activation="relu_train"))
    with pytest.raises(ValueError):
        SaeEngine(EngineConfig(d_model=16, d_sae=64, max_batch=32, activation="relu_trains"))
    # the library itself says the same to a caller that goes past the Python host
    import ctypes as C

    s_ = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    pre = (C.c_int64 * 2)(8, 64)
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    lib = eng.lib
    for rc in (lib.saev_set_prefixes(eng.ctx, pre, 2), lib.saev_backward_begin(eng.ctx, s_), lib.saev_backward_rows(eng.ctx, 0, 32, s_),
               lib.saev_backward_end(eng.ctx, s_), lib.saev_share_x(eng.ctx, topk.ctx), lib.saev_share_x(topk.ctx, eng.ctx),
               lib.saev_copy_step_state(eng.ctx, 8, P(bufs[1]), P(bufs[2]), P(bufs[3]), s_),
               lib.saev_backward_override(eng.ctx, P(bufs[0]), P(bufs[1]), P(bufs[2]), P(bufs[3]), 8),
               lib.saev_train_step_gather(eng.ctx, P(pool), P(rows), P(bufs[0]), 8, 1e-3, 1.0, 1, s_),
               lib.saev_train_step_dp(eng.ctx, P(x), 8, 1e-3, 1.0, 1, s_), lib.saev_step_forward(eng.ctx, P(x), 8, 16, 1, s_),
               lib.saev_copy_last_rows(topk.ctx, 8, 4, P(bufs[2]), P(bufs[2]), P(bufs[3]), P(bufs[2]), s_)):
        assert rc == -3, rc  # SAEV_UNSUPPORTED
    # ... and the step that was in flight still finishes; the forward entries of a ReLU context are served too
    eng.step_forward(x, training=True)
    eng.step_dead(8)
    eng.step_backward()
    with pytest.raises(Exception, match="has run already"):  # (the backward overwrote f's operand images: once per forward)
        eng.step_backward()
    eng.step_tail(1e-3, 1.0)
    idx, val, nnz = eng.encode_relu(x)
    assert eng.decode_rows(idx, val, nnz).shape == (8, 1, 16) and eng.scatter_rows(idx, val, nnz).shape == (8, 64)
    assert eng.scratch_bytes() > 8 * 64 * 4


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
    from saev_amd import nn
    from saev_amd.framework import train as T
    from saev_amd.nn import modeling as M

    g = load_golden("g9_train_b")
    relu = _cfg(tmp_path, g, M.Relu(sparsity=M.L1Sparsity(coeff=2e-3)), optim=optim)
    topk = _cfg(tmp_path, g, M.TopK(top_k=int(g["k"]), aux=M.AuxK(k_aux=int(g["k_aux"]))), optim=optim)

    def run(cfgs):
        saes, objs, log, steps = T.train(cfgs, train_pool=g["acts"])
        ev = T.evaluate(cfgs, saes, objs, val_pool=g["val"])
        return saes, [{k_: v.detach().cpu().clone() for k_, v in s_.state_dict().items()} for s_ in saes], log, ev, steps

    saes, alone, log, ev, steps = run([relu])
    assert steps == int(g["n_steps"])
    recs = [m for _, m in log.records[0]]
    assert recs and all(math.isfinite(r["loss/mse"]) for r in recs) and recs[-1]["loss/mse"] < recs[0]["loss/mse"]
    for r in recs:
        assert r["loss/sparsity"] == pytest.approx(2e-3 * r["loss/l1"], rel=1e-6) and r["loss/sparsity"] > 0
        assert r["loss/loss"] == pytest.approx(r["loss/mse"] + r["loss/sparsity"], rel=1e-12) and r["loss/aux"] == 0
        assert 0 < r["loss/l0"] < int(g["s"]) and math.isfinite(r["metrics/explained_variance"]) and 0 <= r["metrics/dead_unit_pct"] < 1
    # (24 steps, most of them warm-up: nothing is claimed about how good the SAE is by then, only that the pass is consistent)
    assert 0 < ev[0].l0 < int(g["s"]) and math.isfinite(ev[0].mse) and ev[0].mse > 0 and ev[0].l1 > 0
    assert ev[0].normalized_mse == pytest.approx(ev[0].sse_sae / ev[0].sse_baseline, rel=1e-12)
    assert ev[0].freqs.shape == (int(g["s"]),) and float(ev[0].freqs.max()) > 0
    # the checkpoint in the reference's format: four state keys, the sparsity preserved
    nn.dump(tmp_path / "ckpt" / "sae.pt", saes[0])
    back = nn.load(tmp_path / "ckpt" / "sae.pt")
    assert list(back.state_dict()) == list(R.PARAM_ORDER) and back.cfg == saes[0].cfg
    assert back.cfg.activation == M.Relu(sparsity=M.L1Sparsity(coeff=2e-3), aux=M.NoAux())
    for k_, v in alone[0].items():
        assert torch.equal(back.state_dict()[k_], v)
    _, again, *_ = run([relu])
    for k_ in alone[0]:
        assert torch.equal(alone[0][k_], again[0][k_]), f"{k_} differs between identical runs"
    _, topk_alone, _, ev_t, _ = run([topk])
    # In a group every member is initialised from one RNG stream, so only the FIRST member starts where it starts alone: it must
    # end bit for bit where it ends alone, whoever else trains on its batches.  (A ReLU engine shares nothing with the others; a
    # TopK one that follows it neither borrows from it nor draws its batch inside its step.)
    for order, first_alone, ev_alone in (((topk, relu), topk_alone, ev_t), ((relu, topk), alone, ev)):
        _, both, _, ev_b, _ = run(list(order))
        for k_ in first_alone[0]:
            assert torch.equal(both[0][k_], first_alone[0][k_]), f"{type(order[0].sae.activation).__name__} first, {k_}: differs from training it alone"
        assert ev_b[0].mse == ev_alone[0].mse
        assert all(math.isfinite(e.mse) and e.mse > 0 and 0 < e.l0 < int(g["s"]) for e in ev_b)
