"""Norm-predicted TopK bounds (EngineConfig(bounds="norm")) change which candidates the fused encoder lists, never
what the step computes: the exact refinement makes the codes independent of the filter, a prediction that fails is caught by the
select stage and the step repeated on the device with guaranteed bounds.

  a. ~30 training steps with bounds="norm" and bounds="guaranteed" from the same state agree bit for bit (codes, values,
     statistics, parameters, Adam moments) on mean-like and on low-rank data;
  b. a batch built so that the prediction must fail still gives the fp64 top-k of its pre-activations, bound_state()["repeats"]
     counts the repeat, and the step after it is right too (tests/test_rho_bounds_host_cpu.py: the reference has no ties at the cut);
  c. the first steps of a context, a step after params_touched, another batch size and an evaluation forward in between all take
     the guaranteed kernel (bound_state()["launches"] stands still);
  d. rows past n_rows in the last tile and a ragged d_sae do not disturb the ratio the next bounds scale from;
  e. prediction that does not pay is paused: entered after three such steps in a row, 256 steps long, resumed, and four times as
     long the next time."""

import pytest
import torch

import rho_bounds_cases as C

pytestmark = [pytest.mark.gpu, pytest.mark.encoder_modes("f16r")]  # the streamed step belongs to the f16r encoder

LR = 1e-3
STATS = ("mse", "l0", "l1", "aux", "grad_norm", "n_dead", "dense_route", "n_overflow_rows", "sse", "sum_sq", "upper")


def _engine(p, k, b, bounds):
    from saev_amd.engine import EngineConfig, SaeEngine

    s, d = p["W_dec"].shape
    eng = SaeEngine(EngineConfig(d_model=d, d_sae=s, top_k=k, max_batch=b, k_aux=0, bounds=bounds))
    for name, t in p.items():
        eng.view(name).copy_(t.cuda())
    return eng


def _same_runs(p, k, b, batches, steps):
    """`steps` train steps over `batches` (cycled) on a "norm" and a "guaranteed" engine, compared after every step."""
    a, g = _engine(p, k, b, "norm"), _engine(p, k, b, "guaranteed")
    xs = [x.cuda() for x in batches]
    for i in range(steps):
        x = xs[i % len(xs)]
        n = x.shape[0]
        a.train_step(x, LR, 1.0)
        g.train_step(x, LR, 1.0)
        (ia, va, xa), (ig, vg, xg) = a.last_codes(n), g.last_codes(n)
        assert torch.equal(ia, ig) and torch.equal(va, vg), f"step {i}: codes differ"
        assert torch.equal(xa, xg), f"step {i}: x_hat differs"
        sa, sg = a.read_stats(), g.read_stats()
        for name in STATS:
            assert getattr(sa, name) == getattr(sg, name), f"step {i}: read_stats().{name} {getattr(sa, name)!r} != {getattr(sg, name)!r}"
    for name in ("params", "adam_m", "adam_v"):
        assert torch.equal(getattr(a, name), getattr(g, name)), f"{name} differ after {steps} steps"
    st = a.bound_state()
    print(f"norm bounds: {st}; guaranteed: {g.bound_state()}; longest lists {a.read_stats().cand_max} / {g.read_stats().cand_max}")
    assert g.bound_state()["launches"] == 0
    return st


@pytest.mark.parametrize("data", ["mean", "lowrank"])
@pytest.mark.parametrize("k", [8, 32])
def test_norm_and_guaranteed_bounds_train_alike(data, k):
    d, s, n, steps = 256, 4096, 1024, 30
    make = C.mean_batches if data == "mean" else C.lowrank_batches
    st = _same_runs(C.params(d, s, seed=5), k, n, make(d, n, 6, seed=6), steps)
    # (the first step prepares in full, the second is the first streamed one and only leaves its ratios: steps - 2 predictions unless
    # the controller switched them off, which takes three steps in a row that failed or left long lists)
    assert 3 <= st["launches"] <= steps - 2
    assert st["repeats"] <= st["launches"]


@pytest.mark.parametrize("seed", C.FAIL_SEEDS)
def test_failed_norm_prediction_is_repeated(seed):
    p, warm, bad, after = C.failing_case(seed)
    eng = _engine(p, C.K, C.N, "norm")

    def step_and_check(x, what):
        # (lr = 0: W_enc and b_enc stay the ones the CPU reference was formed with)
        eng.train_step(x.cuda(), 0.0, 1.0)
        idx, val, _ = eng.last_codes(x.shape[0])
        want = C.fp64_reference(p, x, C.K)
        assert torch.equal(idx.long().sort(dim=1).values.cpu(), want.indices[:, : C.K].sort(dim=1).values), f"{what}: codes are not the fp64 top-k"
        h = x.double() @ p["W_enc"].double() + p["b_enc"].double()
        torch.testing.assert_close(val.cpu().double(), h.gather(1, idx.long().cpu()), rtol=1e-5, atol=1e-5 * float(x.abs().max()))

    for i, x in enumerate(warm):
        step_and_check(x, f"warm-up step {i}")
    before = eng.bound_state()
    assert before["launches"] == len(warm) - 2 and before["repeats"] == 0, before
    step_and_check(bad, "failing batch")
    mid = eng.bound_state()
    dense_failed = eng.read_stats().dense_route != 0
    print(f"before {before}\nafter the failing batch {mid}; dense route {dense_failed}")
    assert mid["launches"] == before["launches"] + 1 and mid["repeats"] == before["repeats"] + 1
    assert mid["z"] < before["z"]
    # (the repeat itself may end on the exact dense route: the rows at 1e-3 x the batch scale overflow the survivor lists of the
    # guaranteed-bound kernel just as well -- tools/experiments/README.md, "Rows far below their batch")
    # ... and a step that ended there has no final select to take ratios from: the step after it runs on guaranteed bounds, the
    # one after that predicts again
    step_and_check(after, "step after the failing batch")
    dense = eng.read_stats().dense_route
    assert eng.bound_state()["launches"] == mid["launches"] + (0 if dense_failed else 1)
    assert dense == 0
    step_and_check(warm[0], "second step after the failing batch")
    end = eng.bound_state()
    assert end["launches"] == mid["launches"] + (1 if dense_failed else 2) and end["repeats"] == mid["repeats"], end


def test_guaranteed_kernel_where_the_prediction_has_no_footing():
    d, s, k, n = 256, 2048, 16, 512
    p = C.params(d, s, seed=9)
    xs = [x.cuda() for x in C.mean_batches(d, n, 16, seed=10)]
    eng, ref = _engine(p, k, n, "norm"), _engine(p, k, n, "guaranteed")
    it = iter(xs)

    def step(x=None):
        x = next(it) if x is None else x
        eng.train_step(x, LR, 1.0)
        ref.train_step(x, LR, 1.0)
        (ia, va, _), (ig, vg, _) = eng.last_codes(x.shape[0], x_hat=False), ref.last_codes(x.shape[0], x_hat=False)
        assert torch.equal(ia, ig) and torch.equal(va, vg)
        return eng.bound_state()["launches"]

    assert step() == 0  # the first step of a context: full preparation
    assert step() == 0  # the first streamed step: nothing to scale a bound from yet
    assert step() == 1
    # parameters written from outside and announced: full preparation, then a step that only leaves its ratios
    for e in (eng, ref):
        e.view("b_enc").add_(0.001)
        e.params_touched()
    assert step() == 1
    assert step() == 1
    assert step() == 2
    # a smaller batch: its ratios are another batch's
    assert step(next(it)[: n // 2].contiguous()) == 2
    assert step(next(it)[: n // 2].contiguous()) == 3
    assert step() == 3  # ... and back
    assert step() == 4
    # an evaluation forward in between
    for e in (eng, ref):
        e.step_forward(xs[0], training=False)
    assert step() == 4
    assert [step() for _ in range(3)] == [5, 6, 7]  # ... and prediction resumes with the very next step
    assert eng.bound_state()["repeats"] == 0 and ref.bound_state()["launches"] == 0


@pytest.mark.parametrize("s, n", [(4000, 1000), (2048 + 40, 513)])
def test_ragged_rows_and_latents_leave_the_ratio_alone(s, n):
    """n_rows is no multiple of the encoder's 256-row tile and d_sae none of its 256-latent tile: rows past n_rows and padded latents
    must take no part in the ratio.  After every streamed step the device's rho_lo is the minimum over the batch's OWN rows of (exact
    k-th largest pre-activation) / ||x_b - mu||, mu the previous batch's column mean, recomputed here in fp64 from the parameters
    the step started with.  The bound of the comparison, 1e-2 relative: which recent batch's column mean the streamed preparation
    centres on is its own business; two such means differ by about sqrt(2 d / n) in norm, which moves ||x_b - mu|| (about sqrt(2 d))
    by up to ~(d / n) / (2 d) * 2 = 1 / n relative, 1-2e-3 here (measured: 1.6e-3 both ways), and fp32 against fp64 is far below
    that.  A stray row would be an all-zero image row, whose ratio is that of the biases alone: twenty times smaller than the
    batch's (the pause test below builds exactly that row).  Codes and parameters equal the guaranteed engine's, as in (a)."""
    d, k, steps = 256, 32, 8
    p = C.params(d, s, seed=12)
    xs = [x.cuda() for x in C.mean_batches(d, n, 4, seed=13)]
    a, g = _engine(p, k, 1024, "norm"), _engine(p, k, 1024, "guaranteed")
    for i in range(steps):
        x = xs[i % len(xs)]
        W, b = a.view("W_enc").double().clone(), a.view("b_enc").double().clone()
        a.train_step(x, LR, 1.0)
        g.train_step(x, LR, 1.0)
        (ia, va, _), (ig, vg, _) = a.last_codes(n, x_hat=False), g.last_codes(n, x_hat=False)
        assert torch.equal(ia, ig) and torch.equal(va, vg), f"step {i}: codes differ"
        st = a.bound_state()
        if i == 0:
            assert st["rho_lo"] != st["rho_lo"]  # (NaN: a full preparation leaves no ratio)
            continue
        assert a.read_stats().dense_route == 0
        T = torch.topk(x.double() @ W + b, k, dim=1).values[:, -1]
        mu = xs[(i - 1) % len(xs)].double().mean(dim=0)
        want = (T / (x.double() - mu).norm(dim=1)).min().item()
        print(f"step {i}: rho_lo {st['rho_lo']!r}, from the batch's own rows {want!r}; {st}")
        assert abs(st["rho_lo"] - want) <= 1e-2 * abs(want), f"step {i}: rho_lo {st['rho_lo']!r}, expected {want!r}"
        assert st["launches"] == i - 1
    assert torch.equal(a.params, g.params)


def test_prediction_that_does_not_pay_is_paused_and_resumed():
    """Every batch holds an all-zero row.  Its k-th largest pre-activation is that of the biases alone, so its ratio is tiny: it
    sets rho_lo, and the bounds scaled from it keep about half of all latents per row -- far more than max(12 k, 256).  Whether such
    a step passes its verification or is repeated, it does not pay.  After three of them in a row the controller pauses prediction
    for 256 steps (bound_state is read after every step here, so the host sees the pause before the next step: those 256 steps
    are plain guaranteed steps), then tries three more and pauses for 1 024.  Codes stay those of the guaranteed engine throughout."""
    d, s, k, n = 256, 2048, 8, 512
    p = C.params(d, s, seed=21)
    xs = [x.cuda() for x in C.mean_batches(d, n, 8, seed=22)]
    for x in xs:
        x[5] = 0.0
    eng, ref = _engine(p, k, n, "norm"), _engine(p, k, n, "guaranteed")
    launches, states = [], []
    for i in range(2 + 3 + 256 + 3 + 300):
        x = xs[i % len(xs)]
        eng.train_step(x, LR, 1.0)
        states.append(eng.bound_state())
        launches.append(states[-1]["launches"])
    # the same run on guaranteed bounds, compared at the end: one differing code anywhere would have moved the parameters apart
    for i in range(len(launches)):
        ref.train_step(xs[i % len(xs)], LR, 1.0)
    assert torch.equal(eng.params, ref.params) and torch.equal(eng.adam_m, ref.adam_m)
    st = eng.bound_state()
    print(f"launches by step: {launches[:8]} ... {launches[258:268]} ... {launches[-3:]}; {st}")
    assert launches[:5] == [0, 0, 1, 2, 3]
    assert launches[5:5 + 256] == [3] * 256  # paused: 256 steps, not one prediction
    assert launches[261:264] == [4, 5, 6]  # resumed; three more that do not pay ...
    assert launches[264:] == [6] * 300  # ... and the next pause is longer than the first
    # the device's own counter: set to 256 by the third such step, counted down by every step without prediction, then 1 024
    assert [t["pause_left"] for t in states[3:8]] == [0, 256, 255, 254, 253]
    assert states[260]["pause_left"] == 0 and states[263]["pause_left"] == 1024 and states[-1]["pause_left"] == 1024 - 300
    # ... and why: the three predicted steps left lists far longer than max(12 k, 256) candidates per row
    assert all(t["mean_candidates"] > 256 > 12 * k for t in states[2:5]), [t["mean_candidates"] for t in states[2:5]]


def test_pause_with_the_host_running_ahead():
    """The same data as above with nothing read back in between, which is how a training loop runs: the host enqueues steps ahead of
    the device, so the steps between the controller's decision and the host's noticing it are held back by the device's own gate, and
    the host's pause begins -- and ends -- that many steps later than the device's.  Whatever the lag, the parameters are the
    guaranteed engine's, the first three predictions are made, and no more than the three after the first pause can follow."""
    d, s, k, n = 256, 2048, 8, 512
    p = C.params(d, s, seed=21)
    xs = [x.cuda() for x in C.mean_batches(d, n, 8, seed=22)]
    for x in xs:
        x[5] = 0.0
    eng, ref = _engine(p, k, n, "norm"), _engine(p, k, n, "guaranteed")
    steps = 2 + 3 + 256 + 3 + 40
    for e in (eng, ref):
        for i in range(steps):
            e.train_step(xs[i % len(xs)], LR, 1.0)
    assert torch.equal(eng.params, ref.params) and torch.equal(eng.adam_m, ref.adam_m) and torch.equal(eng.adam_v, ref.adam_v)
    st = eng.bound_state()
    print(f"host running ahead: {st}")
    assert 3 <= st["launches"] <= 6 and st["repeats"] <= st["launches"], st
    # (three predictions, the pause of 256; if the three after it were made, the pause of 1 024 is running)
    assert (st["launches"] == 6) == (st["pause_left"] > 256), st
