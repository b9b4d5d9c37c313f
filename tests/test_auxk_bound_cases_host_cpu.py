"""The AuxK bound table without a GPU: every row of tests/auxk_bound_cases.py reaches the bound, the count, the route and the kernel
family it names -- from the library's constants as the cases file restates them and from an fp64 replay of the scenario (the
selection, the fired set and the tracker of every step).  This is where the rows' seeds are fixed."""

import math

import pytest
import torch

import sae_ref as R
from auxk_bound_cases import (AUX_FUSED_MAX, AUX_MFMA_MAX, AUX_SMALL_D_MAX, AUX_SMALL_DEFAULT, AUX_SMALL_MAX, CASES, DEAD_LAG, DENSE_CASES,
                              SMALL_CASES, STALE_CASES, VARIANTS, aux_fused_supported, aux_mfma_supported, dispatch, measured_conditions,
                              replay, scenario)
from step_restatement import BOUND, assert_grads_close, restated_gradients

ALPHA = 1 / 32

RUNS = [(c, v) for c in CASES for v in c.variants]


def _ids(run):
    return f"{run[0].id}-{run[1]}"


def test_the_constants_are_the_librarys():
    """The restated constants against the sources they point to (a changed constant must change the table, not pass it by)."""
    import pathlib
    import re

    csrc = pathlib.Path(__file__).resolve().parent.parent / "saev_amd" / "csrc"
    kernels, ctx, auxk, step = ((csrc / f).read_text() for f in ("kernels.h", "ctx.h", "auxk.hip", "ctx_auxk.hip"))
    for name, value in (("AUX_SMALL_MAX", AUX_SMALL_MAX), ("AUX_SMALL_DEFAULT", AUX_SMALL_DEFAULT), ("AUX_FUSED_MAX", AUX_FUSED_MAX),
                        ("AUX_MFMA_MAX", AUX_MFMA_MAX)):
        assert re.search(rf"constexpr int {name} = {value};", kernels), name
    assert re.search(rf"constexpr int DEAD_LAG = {DEAD_LAG};", ctx)
    assert "bool aux_fused_supported(int D) { return D % 256 == 0 && D >= 256 && D <= 1024; }" in auxk
    assert "bool aux_mfma_supported(int D) { return D % 128 == 0 && D >= 128; }" in auxk
    assert f"bound <= small_max && c->cfg.d_model <= {AUX_SMALL_D_MAX}" in step
    assert aux_fused_supported(256) and aux_fused_supported(1024) and not aux_fused_supported(1280) and not aux_fused_supported(128)
    assert aux_mfma_supported(128) and not aux_mfma_supported(100) and not aux_mfma_supported(2044)


def test_the_table_is_well_formed():
    assert len({c.id for c in CASES}) == len(CASES) == 19
    assert len(DENSE_CASES) == 5 and len(SMALL_CASES) == 14
    # variant B (and the fused-entry test): one row per family
    assert [(c.n_dead, c.n_sleepy) for c in STALE_CASES] == [(0, 40), (10, 30), (33, 67), (65, 63), (0, 128), (4, 4)]
    for c in CASES:
        assert c.d % 4 == 0 and c.s % 4 == 0 and c.n_sleepy > 0 and c.bound <= c.s - c.k
        assert c.n_sleepy + c.k <= c.s


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_every_row_takes_the_route_and_kernels_it_claims(case):
    got = dispatch(case.d, case.s, case.k_aux, case.bound)
    assert tuple(sorted(got.items())) == case.claim, (got, dict(case.claim))
    claim = dict(case.claim)
    assert case.bound > case.n_dead, "the row is about a bound above the count"
    if claim["family"] == "dense":
        assert claim["ndp"] >= case.bound > case.n_dead  # padding columns past the count
        assert claim["aux_all"] == (case.bound <= case.k_aux) and min(case.k_aux, case.n_dead) <= claim["ku"]  # ku_dev, at most the host's ku
    if claim["family"] == "mfma":
        assert not aux_fused_supported(case.d) or case.bound > AUX_FUSED_MAX
        assert (case.n_dead > 0) + (case.n_dead > 32) + (case.n_dead > 64) <= claim["windows"]  # the count's window is among those enqueued
    if claim["family"] == "valu":
        assert not aux_mfma_supported(case.d) and case.bound == claim["cap"]  # at the cap: one more near latent and the step is dense
    if claim["family"] == "fused":
        assert case.n_dead <= claim["latents"]


@pytest.mark.parametrize("run", RUNS, ids=_ids)
def test_the_scenario_reaches_its_bound_and_count(run):
    case, variant = run
    wake, measured = VARIANTS[variant]
    p, toks0, xs, dead, sleepy = scenario(case, variant)
    steps = replay(case, variant)
    assert len(steps) == len(xs) == measured and measured - DEAD_LAG >= 1
    planted = torch.zeros(case.s, dtype=torch.bool)
    planted[dead] = True
    both = planted.clone()
    both[sleepy] = True
    assert int(planted.sum()) == case.n_dead and int(both.sum()) == case.bound
    # the record that sizes the measured step: n_near by its definition
    rec = steps[measured - DEAD_LAG - 1]
    assert rec.n_near == case.bound
    assert torch.equal(rec.toks >= case.thr - DEAD_LAG * case.n, both)
    # the dead set of every step: the planted D, and in variant B the sleepy ones too on step 4 alone
    for i, st in enumerate(steps, 1):
        want = both if (variant == "B" and i == 4) else planted
        assert torch.equal(st.dead, want), f"step {i}: {int(st.dead.sum())} dead"
        # the planted latents fire in the wake batch only, all of them that are meant to
        assert bool(st.mask[:, sleepy].any(dim=0).all()) == (i == wake) and bool(st.mask[:, sleepy].any()) == (i == wake), f"step {i}"
        assert not st.mask[:, dead].any()
        # nobody else comes near the threshold: the bound and the count are the planted latents' alone
        assert int(st.toks[~both].max()) < case.thr - DEAD_LAG * case.n
        # the fired set -- and so the tracker the GPU test compares exactly -- does not hang on fp32 rounding
        assert st.undecided == 0, f"step {i}: the firing of {st.undecided} latents is within fp32 rounding of the cut"
    # steps 1-4 read the count back; none of them may see more than the compact buffers are meant to have held
    if variant == "A":
        assert all(int(st.dead.sum()) == case.n_dead for st in steps)
    # the measured step: fp32 and fp64 select alike (top-k on every row; among the dead where there is a selection)
    mask, dmask, gaps = measured_conditions(case, variant)
    print(f"{case.id} {variant}: bound {rec.n_near}, count {int(dmask.sum())}; smallest top-k gap {gaps[0]:.1f} tol_b, smallest dead gap {gaps[1]:.1f} tol_b")
    assert torch.equal(mask, steps[-1].mask) and torch.equal(dmask, planted)
    assert not mask[:, both].any(), "a planted latent is in the measured step's top-k"
    assert gaps[0] > 2.0 and (case.n_dead <= case.k_aux or gaps[1] > 2.0)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_the_gpu_check_rejects_a_count_that_is_off(case):
    """What the GPU test's comparison is for: the fp64 gradients of the measured step with the BOUND taken for the count (every
    padding / stale row treated as a dead latent) or with the last dead latent left out (a window or loop predicate off by one)
    miss the row's bound against the true ones; so does the auxiliary loss at its 1e-4."""
    p, _, xs, dead, sleepy = scenario(case, "A")
    steps = replay(case, "A")
    p = dict(p, W_dec=R.normalize_w_dec(p["W_dec"]))
    planted = torch.zeros(case.s, dtype=torch.bool)
    planted[dead] = True
    _, aux, ref = restated_gradients(p, xs[-1], steps[-1].mask, planted, None, case.k_aux, ALPHA)
    assert_grads_close(ref, ref, 0.0)
    wrong = {"bound for count": planted.clone()}
    wrong["bound for count"][sleepy] = True
    if case.n_dead:
        wrong["last dead latent dropped"] = planted.clone()
        wrong["last dead latent dropped"][dead.max()] = False
    for what, dmask in wrong.items():
        _, aux_bad, bad = restated_gradients(p, xs[-1], steps[-1].mask, dmask, None, case.k_aux, ALPHA)
        with pytest.raises(AssertionError, match=r"\.grad: flat index \d+ = \(row, column\)"):
            assert_grads_close(bad, ref, BOUND, what=f"{what}: ")
        assert not math.isclose(aux_bad, aux, rel_tol=1e-4), (what, aux_bad, aux)
