"""The bf16 encoder (BASELINE.json configs[3]) at every dispatch class, route and image hand-over (needs -m gpu).  bf16 is not one of
the arithmetics the suite is collected for three-fold (tests/conftest.py: ENCODER_MODES), so it runs only where a test names it;
tests/test_gpu_bf16.py holds it to the oracle's bf16 model at a few fused shapes.  Here:

  A. codes -- encode_topk, the evaluation forward, encode_dense -- at every row of tests/step_restatement.py: SHAPES and the shapes
     of tests/bf16_cases.py: exact against the fp64 product of the bf16-ROUNDED operands to tol_b of tests/topk_exactness.py (the
     product of two bf16 numbers is exact in fp32: the kernel's only error is its fp32 accumulation), and, once per shape, more than
     2 tol_b away from the product of the unrounded ones;
  B. the four gradients of one step at every SHAPES row against the fp64 bf16 restatement (restated_gradients(bf16_codes=True):
     values of the bf16 product, gradient of the fp32 formula, AuxK on the unrounded h), teacher-forced on the step's own selection,
     every element within the row's bound -- tests/test_gpu_step_geometry.py, part A, for the fourth arithmetic;
  C. predicted bounds: the bf16 instantiation of the predicted-bounds kernel, a failed prediction caught and repeated;
  D. candidate-list overflow falling to the exact dense route, on ties and on real weights;
  E. the hand-over of the images the fused Adam leaves: bit identity with a fresh split at nks = 1, on the 64-group kernel, at
     d_model 1280 with ragged d_sae and at a width without hand-over; the late tile checksums, the only thing between an
     unannounced W_enc write and steps run silently on stale images (bf16 has no early sampled check).

tests/test_bf16_cases_host_cpu.py fixes, without a GPU, that the references discriminate."""

import math

import pytest
import torch

from bf16_cases import (EXTRA_CODE_SHAPES, HANDOVER_SHAPES, LATE_CHECK_SHAPE, OVERFLOW_SHAPE, assert_bf16_codes_exact,
                        assert_bf16_codes_exact_to_output_rounding, bf16r, extra_inputs, overflow_inputs, pre_activations, tol_b,
                        worst_value_error)
from step_restatement import DEAD_THR, SHAPES, assert_grads_close, input_conditions, restated_gradients, row_inputs
from test_gpu_parity import make_engine, rand_params
from test_gpu_step_geometry import _batches as _cpu_batches
from test_gpu_stream import _batches, _engine, _same
from topk_exactness import assert_topk_exact

pytestmark = [pytest.mark.gpu, pytest.mark.encoder_modes("f32")]  # bf16 tests pick their own encoder mode: collected once

ALPHA = 1 / 32

# ------------------------------------------------------------------------------------------------
# A. codes in every class
# ------------------------------------------------------------------------------------------------

_CODE_CASES = [((r.n, r.d, r.s, r.k, 1.0), r) for r in SHAPES] + [(c, None) for c in EXTRA_CODE_SHAPES]


def _ascending_in_range(idx, s, what):
    assert (idx[:, 1:] > idx[:, :-1]).all(), f"{what}: codes come out in strictly ascending latent order"
    assert (idx >= 0).all() and (idx < s).all(), f"{what}: a latent index outside 0..{s - 1}"


@pytest.mark.parametrize("shape,row", _CODE_CASES, ids=[r.id if r else "{}x{}x{}k{}-x{:g}".format(*c) for c, r in _CODE_CASES])
def test_bf16_codes_in_every_class(shape, row):
    """Beyond SHAPES: (2049, 64, 516, 8) nine row blocks, so both branches of the encoder's XCD swizzle; (257, 32, 260, 4) nks = 1 and
    a second row block of one row; (65, 64 / 96, 260, 8) nks = 2 / 3; (300, 128, 1028, 16) with x scaled by 3e5 and by 1e-6 (bf16
    carries no x scale: its exponent range is fp32's)."""
    n, d, s, k, _ = shape
    if row is not None:
        p, x, _ = row_inputs(row)
    else:
        p, x = extra_inputs(*shape)
    what = f"({n}, {d}, {s}, {k})"
    kk = min(k, s)
    eng = make_engine(d, s, k, max_batch=n, encoder="bf16")
    eng.load_params(p)
    xg, W, b = x.cuda(), p["W_enc"].cuda(), p["b_enc"].cuda()
    idx, val = eng.encode_topk(xg)
    assert idx.shape == (n, kk) and val.shape == (n, kk)
    api = assert_bf16_codes_exact(xg, idx, val, W, b, what=f"{what} encode_topk: ")
    _ascending_in_range(idx, s, f"{what} encode_topk")
    # the evaluation forward: the same codes by the step's entry, and the route it took
    eng.step_forward(xg, training=False)
    st = eng.read_stats()
    idx2, val2, _ = eng.last_codes(n)
    fwd = assert_bf16_codes_exact(xg, idx2, val2, W, b, what=f"{what} step_forward: ")
    _ascending_in_range(idx2, s, f"{what} step_forward")
    assert st.n_overflow_rows == 0, st
    assert st.dense_route == (1 if k > 64 else 0), (k, st)  # (fused_supported: top_k <= 64; above, the dense kernel and select_dense)
    # encode_dense: every element to the same per-row tolerance
    h = eng.encode_dense(xg)
    err = (h.double() - pre_activations(bf16r(xg), bf16r(W), b)).abs() / tol_b(bf16r(xg), bf16r(W))[:, None]
    assert (err <= 1.0).all(), f"{what} encode_dense: element {int(err.argmax())} is {err.max().item():.2f} tol_b off the product of the rounded operands"
    # negative control: it really is the bf16 product -- the same values fail against the unrounded operands
    off = worst_value_error(xg, idx, val, W, b)
    off_dense = ((h.double() - pre_activations(xg, W, b)).abs() / tol_b(xg, W)[:, None]).max().item()
    print(f"{what}: encode_topk {api[0]:.2f} / {api[1]:.2f} tol_b, step_forward {fwd[0]:.2f} / {fwd[1]:.2f} tol_b, encode_dense {err.max().item():.2f} tol_b; "
          f"against the unrounded operands: codes {off:.0f} tol_b, dense {off_dense:.0f} tol_b")
    assert off > 2.0 and off_dense > 2.0, (off, off_dense)
    with pytest.raises(AssertionError, match="value error|left-out"):
        assert_topk_exact(xg, idx, val, W, b)  # (the checker itself, fed the unrounded operands, rejects these codes)
    eng.close()


# ------------------------------------------------------------------------------------------------
# B. gradients in every class
# ------------------------------------------------------------------------------------------------

_REFERENCES = {}  # row.id -> (mask, W_dec as the step normalised it, dead mask, (mse, aux, gradients)): computed once per row


def _reference(row, params, x, toks, mask):
    """The fp64 bf16 restatement on the step's own selection and its own (renormalised) W_dec -- shared by the two weight-gradient
    routes of a row as long as they hand in the same mask and parameters."""
    hit = _REFERENCES.get(row.id)
    if hit is not None and torch.equal(hit[0], mask) and torch.equal(hit[1], params["W_dec"]):
        return hit[2], hit[3]
    # (the AuxK selection reads the unrounded h: the dead gap is the one input_conditions asserts; its top-k mask is the EXACT one and
    # not compared -- the bf16 selection differs from it on most rows, tests/test_bf16_cases_host_cpu.py)
    _, dead, _ = input_conditions(row, params["W_enc"], params["b_enc"], x, toks)
    assert not mask[:, dead].any(), f"{row.id}: a dead latent is among the step's codes"
    out = restated_gradients(params, x, mask, dead, row.prefixes, row.k_aux, ALPHA, bf16_codes=True)
    _REFERENCES[row.id] = (mask, params["W_dec"], dead, out)
    return dead, out


@pytest.mark.parametrize("dw", ["default", "rows"])  # (without slices -- d_model % 32 != 0, Matryoshka -- the two are the same code)
@pytest.mark.parametrize("row", SHAPES, ids=lambda r: r.id)
def test_bf16_gradients_in_every_dispatch_class_match_fp64(row, dw, monkeypatch):
    if dw == "rows":
        monkeypatch.setenv("SAEV_AMD_DW", "rows")
    p, x, toks = row_inputs(row)
    k = min(row.k, row.s)
    eng = make_engine(row.d, row.s, row.k, k_aux=row.k_aux, alpha=ALPHA, thr=DEAD_THR, max_batch=row.n, remove_parallel_grads=False, encoder="bf16")
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
    # (near ties among the bf16 pre-activations: the cut is checked, not set equality with a reference's top-k)
    worst = assert_bf16_codes_exact(xg, idx, val, eng.view("W_enc"), eng.view("b_enc"), what=f"{row.id}: ")
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
        ratios = assert_grads_close(got, ref, row.bound, what=f"{row.id} {dw} bf16: ")
    finally:
        print(f"{row.id} {dw} bf16: codes {worst[0]:.2f} / {worst[1]:.2f} tol_b; mse {st.mse:.9e} (fp64 {mse:.9e}) aux {st.aux:.9e} "
              f"(fp64 {aux:.9e}); worst |difference| / max|fp64|: " + "  ".join(f"{k_} {v:.2e}" for k_, v in ratios.items()))
    assert math.isclose(st.mse, mse, rel_tol=1e-4), (st.mse, mse)
    assert math.isclose(st.aux, aux, rel_tol=1e-4, abs_tol=1e-9), (st.aux, aux)
    assert (aux > 0) == (row.n_dead > 0)
    assert st.l0 == float(k)
    eng.close()


# ------------------------------------------------------------------------------------------------
# C. predicted bounds
# ------------------------------------------------------------------------------------------------


def test_bf16_failed_bound_prediction_is_caught_and_repeated():
    """tests/test_gpu_parity.py::test_failed_bound_prediction_is_caught_and_repeated on the bf16 instantiation of the predicted-bounds
    kernel: the same construction, the same bound_state() assertions; the codes are exact for the rounded operands."""
    d, s, k, n = 128, 4096, 16, 300
    p = rand_params(d, s, seed=70)
    p["b_enc"][:256] = 50.0 * (1.0 - 2.0 * (torch.arange(256) % 2).float())
    x = torch.randn(n, d, generator=torch.Generator().manual_seed(71))
    eng = make_engine(d, s, k, k_aux=0, max_batch=n, bounds="predicted", encoder="bf16")
    eng.load_params(p)
    before = eng.bound_state()
    idx, val = eng.encode_topk(x.cuda())
    after = eng.bound_state()
    assert after["launches"] == before["launches"] + 1 and after["repeats"] == before["repeats"] + 1
    assert after["z"] < before["z"]
    worst = assert_bf16_codes_exact(x.cuda(), idx, val, p["W_enc"].cuda(), p["b_enc"].cuda())
    _ascending_in_range(idx, s, "after the repeat")
    print(f"repeated launch: worst value error {worst[0]:.2f} tol_b, worst cut excess {worst[1]:.2f} tol_b")
    # an ordinary launch afterwards predicts fine again (z dropped, the lists are just longer)
    p2 = rand_params(d, s, seed=72)
    eng.load_params(p2)
    idx, val = eng.encode_topk(x.cuda())
    again = eng.bound_state()
    assert again["launches"] == after["launches"] + 1 and again["repeats"] == after["repeats"]
    assert_bf16_codes_exact(x.cuda(), idx, val, p2["W_enc"].cuda(), p2["b_enc"].cuda())
    eng.close()


def test_bf16_guaranteed_and_predicted_bounds_give_the_same_codes():
    d, s, k, n = 256, 8192, 32, 700
    p = rand_params(d, s, seed=73)
    x = (torch.randn(n, d, generator=torch.Generator().manual_seed(74)) + 0.5).cuda()
    out = []
    for bounds in ("guaranteed", "predicted"):
        eng = make_engine(d, s, k, k_aux=0, max_batch=n, bounds=bounds, encoder="bf16")
        eng.load_params(p)
        codes = [eng.encode_topk(x) for _ in range(3)]  # (a failed prediction lowers z: later launches predict again)
        out.append(([c[0].clone() for c in codes], [c[1].clone() for c in codes], eng.bound_state()))
        eng.close()
    for a, b in zip(out[0][0] + out[0][1], out[1][0] + out[1][1]):
        assert torch.equal(a, b)
    assert out[0][2]["launches"] == 0 and out[1][2]["launches"] == 3 and out[1][2]["repeats"] <= 1
    assert 32 <= out[1][2]["mean_candidates"] < 2000
    assert_bf16_codes_exact(x, out[1][0][-1], out[1][1][-1], p["W_enc"].cuda(), p["b_enc"].cuda())  # (and both are right)


# ------------------------------------------------------------------------------------------------
# D. overflow to the dense route
# ------------------------------------------------------------------------------------------------


def test_bf16_candidate_overflow_takes_the_exact_dense_route():
    """tests/test_gpu_parity.py::test_candidate_overflow_takes_the_exact_dense_route, word for word: zeros and the biases 1, 2 and 3 are
    exact in bf16."""
    n, d, s, k = 40, 32, 16384, 16
    p = rand_params(d, s, seed=3)
    p["W_enc"] = torch.zeros(d, s)
    p["b_enc"] = torch.ones(s)
    p["b_enc"][7], p["b_enc"][9000] = 2.0, 3.0
    x = torch.randn(n, d, generator=torch.Generator().manual_seed(4))
    eng = make_engine(d, s, k, max_batch=64, encoder="bf16")
    eng.load_params(p)
    eng.step_forward(x.cuda(), training=False)
    st = eng.read_stats()
    assert st.n_overflow_rows == n and st.cand_max > 4096
    assert st.dense_route == 1
    idx, val, x_hat = (t.cpu() for t in eng.last_codes(n))
    assert (idx[:, 1:] > idx[:, :-1]).all()
    for row in range(n):
        got = dict(zip(idx[row].tolist(), val[row].tolist()))
        assert got.get(7) == 2.0 and got.get(9000) == 3.0, "the two strict maxima are always selected"
        assert sorted(got.values())[:k - 2] == [1.0] * (k - 2), "the rest are ties at 1.0 (any k of them)"
    # the step's loss is the loss of exactly those codes
    want_hat = p["b_dec"] + torch.einsum("bk,bkd->bd", val, p["W_dec"][idx.long()])
    torch.testing.assert_close(x_hat, want_hat, rtol=1e-5, atol=1e-5)
    assert math.isclose(st.mse, ((want_hat - x) ** 2).mean().item(), rel_tol=1e-4)
    eng.train_step(x.cuda(), 1e-3, 1.0)
    st = eng.read_stats()
    assert st.n_overflow_rows == n and math.isfinite(st.grad_norm) and st.grad_norm > 0
    eng.close()


@pytest.mark.parametrize("k", [33, 64])
def test_bf16_candidate_overflow_on_real_weights(k):
    """Real weights behind b_enc = 1: W_enc of rand_params scaled by 1e-3, two strict maxima.  The pre-activations of a row all lie
    within 1e-2 of 1 and are all different; the lists overflow in every row, and the dense route's codes are those of the bf16
    product.  (Values to tol_b plus the half ulp of the fp32 they are stored as: bf16_cases.assert_bf16_codes_exact_to_output_rounding.)

    k > 32, the 64-group kernel: its bound is the top_k-th largest of 64 group maxima kept as 16-bit keys (a float's upper half,
    rounded down).  Every maximum but two lies in [1, 1 + 2^-7) and has the key of 1.0, so the bound is 1.0 and half of the 16384
    values pass it: 8192 > 4096 entries (k = 33 walks the key search, k = 64 takes its minimum).  At k <= 32 the bound is a full
    fp32 value -- the minimum of 32 group maxima, refined on the first tile -- and tells values that differ apart: the same
    inputs at k = 16 leave lists of at most 1794 entries, no overflow, and nothing for this test to see."""
    n, d, s, _ = OVERFLOW_SHAPE
    p, x = overflow_inputs()
    eng = make_engine(d, s, k, max_batch=64, encoder="bf16")
    eng.load_params(p)
    xg = x.cuda()
    eng.step_forward(xg, training=False)
    st = eng.read_stats()
    print(f"k = {k}: n_overflow_rows {st.n_overflow_rows} of {n}, cand_max {st.cand_max}, dense_route {st.dense_route}")
    assert st.n_overflow_rows == n and st.cand_max > 4096 and st.dense_route == 1, st
    idx, val, _ = eng.last_codes(n)
    _ascending_in_range(idx, s, "overflow")
    assert ((idx == 7).any(dim=1) & (idx == 9000).any(dim=1)).all(), "the two strict maxima are always selected"
    worst = assert_bf16_codes_exact_to_output_rounding(xg, idx, val, p["W_enc"].cuda(), p["b_enc"].cuda())
    off = worst_value_error(xg, idx, val, p["W_enc"].cuda(), p["b_enc"].cuda())
    print(f"k = {k}: worst value error {worst[0]:.2f}, worst cut excess {worst[1]:.2f} of tol_b + half an ulp; {off:.0f} tol_b off the unrounded product")
    half_ulp = 3.0 * 2.0 ** -24 / tol_b(xg, p["W_enc"].cuda()).min().item()  # of a value <= 3, in units of the smallest tol_b
    assert off > 2.0 * (1.0 + half_ulp), (off, half_ulp)  # negative control: twice what the check above allows
    eng.close()


# ------------------------------------------------------------------------------------------------
# E. the image hand-over
# ------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n,d,s,k", HANDOVER_SHAPES)
def test_bf16_images_left_by_adam_equal_a_fresh_split_at_every_geometry(n, d, s, k):
    """tests/test_gpu_step_geometry.py::test_bf16_images_left_by_adam_at_ragged_d_sae_equal_a_fresh_split (prep_route 0 against 1, four
    steps, bit identity of parameters, moments and tracker) at nks = 1, on the 64-group kernel, at d_model = 1280 with ragged d_sae,
    and at d_model % 32 != 0 where nothing is handed over -- and both routes RIGHT, not only equal: the last step's codes are exact
    against the W_enc and b_enc that step started from."""
    p = rand_params(d, s, seed=s + n + 1)
    engs = [make_engine(d, s, k, k_aux=32, thr=3 * n, max_batch=n, encoder="bf16", prep_route=r) for r in (0, 1)]
    for eng in engs:
        eng.load_params(p)
    xs = _cpu_batches(n, d, seed=s + 1)
    for i, x in enumerate(xs):
        if i == len(xs) - 1:
            W_enc, b_enc = engs[0].view("W_enc").clone(), engs[0].view("b_enc").clone()
            assert torch.equal(W_enc, engs[1].view("W_enc")) and not torch.equal(W_enc.cpu(), p["W_enc"])
        for eng in engs:
            eng.train_step(x, 1e-3, 1.0)
            assert eng.read_stats().n_overflow_rows == 0, i
        a, c = (e.read_stats() for e in engs)
        assert a.mse == c.mse and a.dense_route == c.dense_route == 0, (i, a, c)
    torch.cuda.synchronize()
    _same(*engs)
    for eng in engs:
        idx, val, _ = eng.last_codes(n)
        worst = assert_bf16_codes_exact(xs[-1], idx, val, W_enc, b_enc, what=f"prep_route {eng.cfg.prep_route}: ")
        _ascending_in_range(idx, s, f"prep_route {eng.cfg.prep_route}")
        print(f"({n}, {d}, {s}, {k}) prep_route {eng.cfg.prep_route}: worst value error {worst[0]:.2f} tol_b, worst cut excess {worst[1]:.2f} tol_b")
    for eng in engs:
        eng.step_forward(xs[0], training=False)  # (a pending SAEV_STALE_PARAMS would raise here: none on an honest run)
        torch.cuda.synchronize()
        eng.close()


@pytest.mark.parametrize("what", ["one_element", "one_column", "b_enc_one"])
def test_bf16_sparse_unannounced_write_is_never_silent(what):
    """tests/test_gpu_stream.py::test_a_sparse_unannounced_write_is_never_silent on a bf16 engine.  A bf16 forward reads b_enc from the
    parameters: a b_enc write needs no announcement -- no error, no dense route, right codes at once.  A W_enc write meets no early
    check here; the fused Adam's tile checksums find it at the end of the first step that used the stale images, the next call
    fails with SAEV_STALE_PARAMS, once, and the run continues from a fresh split."""
    from saev_amd import _lib

    d, s, k, b = LATE_CHECK_SHAPE
    eng = _engine(d, s, k, b, 0, seed=61, encoder="bf16")
    xs = _batches(d, b, 9, seed=62)
    for x in xs[:3]:
        eng.train_step(x, 1e-4, 1.0)
    torch.cuda.synchronize()
    if what == "one_element":
        eng.view("W_enc").data[17, 1234] += 0.25
    elif what == "one_column":
        eng.view("W_enc").data[:, 77] = torch.randn(d, device="cuda") / d**0.5
    else:
        eng.view("b_enc").data[5] += 1.0
    raised, dense = 0, []
    for i, x in enumerate(xs[3:]):
        W_enc, b_enc = eng.view("W_enc").clone(), eng.view("b_enc").clone()
        try:
            eng.train_step(x, 1e-4, 1.0)
            torch.cuda.synchronize()
            dense.append(eng.read_stats().dense_route)
        except _lib.SaevError as e:
            raised += 1
            assert "saev_params_touched" in str(e) and "tiles" in str(e), str(e)
            continue
        if what == "b_enc_one" or raised == 1:  # (every step that has no stale image behind it: its codes are those of its parameters)
            idx, val, _ = eng.last_codes(b)
            assert_bf16_codes_exact(x, idx, val, W_enc, b_enc, what=f"{what}, step {i} after the write: ")
    if what == "b_enc_one":
        assert raised == 0 and sum(dense) == 0, (raised, dense)
    else:
        assert raised == 1, (raised, dense)
        assert dense[-1] == 0
    # ... and the run goes on: the codes agree with an engine that was told
    told = _engine(d, s, k, b, 0, seed=61, encoder="bf16")
    told.load_params({n: eng.view(n).clone() for n in ("W_dec", "b_dec", "W_enc", "b_enc")})
    i0, v0 = eng.encode_topk(xs[0])
    i1, v1 = told.encode_topk(xs[0])
    assert torch.equal(i0, i1) and torch.equal(v0, v1)
    assert_bf16_codes_exact(xs[0], i0, v0, eng.view("W_enc"), eng.view("b_enc"))


def test_bf16_tile_checksums_stay_quiet_on_an_honest_run():
    """tests/test_gpu_stream.py::test_tile_checksums_stay_quiet_on_an_honest_run's schedule without its x1000 batch (which exists for
    fp16's range): evaluation forwards in between, announced writes, a smaller batch -- the late check never fires."""
    d, s, k, b = LATE_CHECK_SHAPE
    eng = _engine(d, s, k, b, 0, seed=71, k_aux=32, dead_threshold_tokens=3 * b, encoder="bf16")
    xs = _batches(d, b, 14, seed=72)
    other = _batches(d, 300, 2, seed=73)
    for i, x in enumerate(xs):
        if i == 3:
            eng.step_forward(other[0], training=False)
        if i == 5:
            eng.view("W_enc").data[:, 3] *= 2.0
            eng.params_touched()
        if i == 7:
            eng.view("W_enc").mul_(1.001)  # the version counter announces it
        W_enc, b_enc = eng.view("W_enc").clone(), eng.view("b_enc").clone()
        x = x[:400].contiguous() if i == 11 else x
        eng.train_step(x, 1e-4, 1.0)
        assert eng.read_stats().dense_route == 0, i
        if i in (5, 7, 11, 13):  # (after each intervention and at the end: the codes are those of the parameters the step started from)
            idx, val, _ = eng.last_codes(x.shape[0])
            assert_bf16_codes_exact(x, idx, val, W_enc, b_enc, what=f"step {i}: ")
    torch.cuda.synchronize()
    eng.step_forward(other[1], training=False)  # (would raise)
