"""The per-latent logistic probes on the MI355X (include/saev_amd.h: PROBE1D): prepare, the event sums, one solver
iteration, evaluate, the whole fit and worker_fn against the fp64 numpy restatement of the contract (tests/probe1d_restatement.py,
itself held against the reference's recorded results on the CPU) and against fixtures G23 and G25, recorded from the reference.

Bands.  Event sums: every term is formed in fp64 from exp, log1p and one division -- a dozen roundings of 2^-53 each -- and the sums
add them in a fixed order, so a sum may differ from the restatement's by about 1e-15 of the sum of the terms' magnitudes; the band
is 1e-12 of that sum (+ 1e-300 for terms that underflow), four orders above fp64 rounding and four below any fp32 slip.  The solver
step: 1e-13 relative, with every synthetic input at least 1e-6 relative away from each threshold it is compared with, so that both
sides take the same branch.  End to end: the bands recorded with the fixture from the reference's own float32 / float64 difference."""

import dataclasses

import numpy as np
import pytest
import scipy.sparse
import torch

import probe1d_restatement as R
from conftest import GOLDEN
from probe1d_cases import CASES, CHUNK, make_design, make_labels
from probe1d_cases import coefficients as _coefficients

pytestmark = [pytest.mark.gpu, pytest.mark.encoder_modes("f32")]


def _engine():
    from saev_amd import engine

    assert engine.Probe1D.CHUNK == CHUNK
    return engine


class Case:
    def __init__(self, n, s, c, full, seed):
        engine = _engine()
        self.n, self.s, self.c = n, s, c
        self.indptr, self.indices, self.data = make_design(n, s, seed, full=full)
        self.ids = make_labels(n, c, seed)
        self.ymat = R.labels_matrix(self.ids, c)
        self.ref = R.prepare(self.indptr, self.indices, self.data, s)
        dev = torch.device("cuda")
        self.csr = [torch.from_numpy(a).to(dev) for a in (self.indptr, self.indices, self.data)]
        self.p = engine.Probe1D(n, s, c, self.data.size, dev).prepare(*self.csr, labels=torch.from_numpy(self.ids).to(dev))

    def matrix_form(self):
        engine = _engine()
        p = engine.Probe1D(self.n, self.s, self.c, self.data.size, "cuda")
        return p.prepare(*self.csr, y=torch.from_numpy(self.ymat).cuda())


@pytest.fixture(scope="module")
def cases():
    built = {}

    def get(i):
        if i not in built:
            built[i] = Case(*CASES[i], seed=50 + i)
        return built[i]

    return get


@pytest.mark.parametrize("i", range(len(CASES)), ids=[f"n{n}_s{s}_c{c}" for n, s, c, _ in CASES])
def test_prepare_matches_a_stable_sort_and_both_label_forms_give_the_same_bits(cases, i):
    k = cases(i)
    starts, rows, vals, qx = k.ref
    counts = np.diff(starts)
    if k.n == 5000 and k.s >= 6:
        assert counts[:5].tolist() == [0, 1, CHUNK - 1, CHUNK, CHUNK + 1]
    np.testing.assert_array_equal(k.p.starts.cpu().numpy(), starts)
    np.testing.assert_array_equal(k.p.chunk_starts.cpu().numpy(), np.concatenate([[0], np.cumsum(-(-counts // CHUNK))]))
    got_rows, got_vals = k.p.row.cpu().numpy(), k.p.val.cpu().numpy()
    np.testing.assert_array_equal(got_rows, rows)  # ascending inside every latent: the stable order
    np.testing.assert_array_equal(got_vals.view(np.uint32), vals.view(np.uint32))
    np.testing.assert_allclose(k.p.qx.cpu().numpy(), qx, rtol=1e-14, atol=0)
    np.testing.assert_array_equal(k.p.pos.cpu().numpy(), k.ymat.sum(axis=0))
    bits = k.p.ybits.cpu().numpy().view(np.uint32)
    np.testing.assert_array_equal(bits, R.pack_bits(k.ymat))
    m = k.matrix_form()
    np.testing.assert_array_equal(m.ybits.cpu().numpy().view(np.uint32), bits)
    np.testing.assert_array_equal(m.pos.cpu().numpy(), k.p.pos.cpu().numpy())
    np.testing.assert_array_equal(m.row.cpu().numpy(), rows)


def test_prepare_reports_bad_labels_and_columns_from_the_device(cases):
    engine = _engine()
    k = cases(1)
    ids = torch.from_numpy(k.ids.copy()).cuda()
    ids[5] = k.c
    with pytest.raises(ValueError, match="class id"):
        engine.Probe1D(k.n, k.s, k.c, k.data.size, "cuda").prepare(*k.csr, labels=ids)
    y = torch.from_numpy(k.ymat.astype(np.uint8)).cuda()
    y[7, 3] = 2
    with pytest.raises(ValueError, match="neither 0 nor 1"):
        engine.Probe1D(k.n, k.s, k.c, k.data.size, "cuda").prepare(*k.csr, y=y)
    cols = k.csr[1].clone()
    cols[0] = k.s
    with pytest.raises(ValueError, match="column index"):
        engine.Probe1D(k.n, k.s, k.c, k.data.size, "cuda").prepare(k.csr[0], cols, k.csr[2], labels=torch.from_numpy(k.ids).cuda())
    with pytest.raises(ValueError, match="one of the two"):
        engine.Probe1D(k.n, k.s, k.c, k.data.size, "cuda").prepare(*k.csr)


@pytest.mark.parametrize("i", range(len(CASES)), ids=[f"n{n}_s{s}_c{c}" for n, s, c, _ in CASES])
def test_event_sums_match_the_restatement(cases, i):
    k = cases(i)
    starts, rows, vals, _ = k.ref
    b, w = _coefficients(k.s, k.c, 7 + i)
    want, mag = R.event_sums(starts, rows, vals, k.ymat, b, w)
    got = k.p.stats(torch.from_numpy(b).cuda(), torch.from_numpy(w).cuda()).cpu().numpy()
    assert np.isfinite(want).all() and (k.s * k.c < 100 or ((np.abs(b) > 40).any() and (np.abs(w) > 800).any()))
    err = np.abs(got - want)
    band = 1e-12 * mag + 1e-300
    worst = (err / band).max(axis=(0, 2))
    print("largest error / band per sum:", dict(zip(R.SUM_NAMES, worst.round(6))))
    for q, name in enumerate(R.SUM_NAMES):
        assert (err[:, q] <= band[:, q]).all(), name
    again = k.p.stats(torch.from_numpy(b).cuda(), torch.from_numpy(w).cuda()).cpu().numpy()
    np.testing.assert_array_equal(again.view(np.uint64), got.view(np.uint64))


@pytest.mark.parametrize("among,cls", [(6, 37), (6, 150), (4, 40), (1, 9), (2, 31)])
def test_a_class_alone_and_among_others_gives_identical_bits(cases, among, cls):
    """One class prepared on its own (eight sub-chunks side by side in a wave) against the same class among the others (one to
    eight side by side, or lane = class over several groups): the order of the adds is the same, hence the bits."""
    engine = _engine()
    k = cases(among)
    b, w = _coefficients(k.s, k.c, 90 + among)
    full = k.p.stats(torch.from_numpy(b).cuda(), torch.from_numpy(w).cuda()).cpu().numpy()
    alone = engine.Probe1D(k.n, k.s, 1, k.data.size, "cuda").prepare(*k.csr, y=torch.from_numpy(k.ymat[:, cls:cls + 1].copy()).cuda())
    one = alone.stats(torch.from_numpy(b[:, cls:cls + 1].copy()).cuda(), torch.from_numpy(w[:, cls:cls + 1].copy()).cuda()).cpu().numpy()
    np.testing.assert_array_equal(one[:, :, 0].view(np.uint64), full[:, :, cls].view(np.uint64))


# ---- one solver iteration on synthetic gradients ------------------------------------------------------------------------------------------
# columns: g0, g1, h0, h1, h2, lam, prev_pred, prev_loss, prev_clipped, qx; the loss of every pair is 0.4.  Every value is at least
# 1e-6 relative away from each threshold it meets (tol, |det| = 1e-18, norm = delta_logit, pred = 0, rho = 0.25 / 0.75, the clamps).
NAN = float("nan")
STEPS = {
    "inactive": (1e-9, -2e-9, 0.2, 0.01, 0.3, 1e-3, NAN, NAN, 0, 1.0),
    "accepted_first_try": (0.1, 0.05, 0.2, 0.01, 0.3, 1e-3, NAN, NAN, 0, 1.3),
    "clipped": (0.1, 0.02, 1e-3, 0.0, 1e-3, 1e-3, NAN, NAN, 0, 0.7),
    "singular_three_tries": (0.1, 0.0, 0.0, 0.0, 0.0, 3e-12, NAN, NAN, 0, 1.0),
    "pred_negative_1_try": (0.1, 0.0, -0.05, 0.0, 1.0, 1e-2, NAN, NAN, 0, 1.0),
    "pred_negative_2_tries": (0.1, 0.0, -0.05, 0.0, 1.0, 1e-3, NAN, NAN, 0, 1.0),
    "pred_negative_3_tries": (0.1, 0.0, -0.05, 0.0, 1.0, 1e-4, NAN, NAN, 0, 1.0),
    "pred_negative_4_tries": (0.1, 0.0, -0.05, 0.0, 1.0, 1e-5, NAN, NAN, 0, 1.0),
    "five_failures_fallback": (0.1, 0.03, -0.05, 0.0, 1.0, 1e-6, NAN, NAN, 0, 2.0),
    "nan_prev_pred_skips_the_rule": (0.1, 0.05, 0.2, 0.01, 0.3, 1e-3, NAN, 0.5, 1, 1.0),
    "rho_small_grows": (0.1, 0.05, 0.2, 0.01, 0.3, 1e-3, 0.1, 0.41, 0, 1.0),
    "rho_large_shrinks": (0.1, 0.05, 0.2, 0.01, 0.3, 1e-3, 0.1, 0.49, 0, 1.0),
    "rho_large_but_clipped_grows": (0.1, 0.05, 0.2, 0.01, 0.3, 1e-3, 0.1, 0.49, 1, 1.0),
    "lam_at_the_upper_clamp": (0.1, 0.05, 0.2, 0.01, 0.3, 1e12, 0.1, 0.41, 0, 1.0),
    "lam_at_the_lower_clamp": (0.1, 0.05, 0.2, 0.01, 0.3, 1e-12, 0.1, 0.49, 0, 1.0),
    "empty_latent": (0.3, 0.3, 0.2, 0.0, 0.3, 5.0, NAN, 0.41, 1, None),
}
WANT_FLAGS = {"inactive": (R.INACTIVE, 0), "accepted_first_try": (0, 1), "clipped": (R.CLIPPED, 1), "singular_three_tries": (R.SINGULAR | R.CLIPPED, 4),
              "pred_negative_1_try": (0, 2), "pred_negative_2_tries": (0, 3), "pred_negative_3_tries": (0, 4), "pred_negative_4_tries": (0, 5),
              "five_failures_fallback": (R.FALLBACK_FLAG | R.CLIPPED, 5), "nan_prev_pred_skips_the_rule": (0, 1), "rho_small_grows": (R.GROWN, 1),
              "rho_large_shrinks": (R.SHRUNK, 1), "rho_large_but_clipped_grows": (R.GROWN, 1), "lam_at_the_upper_clamp": (R.GROWN, 1),
              "lam_at_the_lower_clamp": (R.SHRUNK, 1), "empty_latent": (R.EMPTY | R.INACTIVE, 0)}


def test_update_takes_every_branch_as_the_restatement_does():
    engine = _engine()
    names = list(STEPS)
    s, n = len(names), 8
    table = np.array([[np.nan if v is None else v for v in STEPS[k]] for k in names])
    # every latent but the last fires on all 8 rows with the constant value qx (so zf = 0 and qx is that value); 4 of 8 rows are positive
    rows, cols = np.meshgrid(np.arange(n), np.arange(s - 1), indexing="ij")
    csr = scipy.sparse.csr_matrix((table[cols.ravel(), 9].astype(np.float32), (rows.ravel(), cols.ravel())), shape=(n, s))
    ids = np.array([0, 1] * 4, dtype=np.uint8)  # class 1 of 2: pi = 0.5, base = 0
    c = 2
    p = engine.Probe1D(n, s, c, csr.nnz, "cuda").prepare(torch.from_numpy(csr.indptr.astype(np.int64)).cuda(), torch.from_numpy(csr.indices.astype(np.int32)).cuda(),
                                                         torch.from_numpy(csr.data).cuda(), labels=torch.from_numpy(ids).cuda())
    hp = engine.Probe1DHyper(ridge=0.0, max_iter=1, class_slab_size=1)
    rhp = R.Hyper(ridge=0.0, max_iter=1, class_slab_size=1)
    starts, _, _, qx = R.prepare(csr.indptr, csr.indices, csr.data, s)
    pos = np.array([4, 4])
    g0, g1, h0, h1, h2 = (np.repeat(table[:, q:q + 1], c, axis=1) for q in range(5))
    sums = np.stack([n * (g0 + 0.5), n * g1, n * h0, n * h1, n * h2, np.full((s, c), n * 0.4), np.full((s, c), 4.0)], axis=1)
    state = R.init_state(s, pos, n, rhp)
    state["lam"] = np.repeat(table[:, 5:6], c, axis=1)
    state["prev_pred"] = np.repeat(table[:, 6:7], c, axis=1)
    state["prev_loss"] = np.repeat(table[:, 7:8], c, axis=1)
    state["clipped"] = np.repeat(table[:, 8:9], c, axis=1) != 0
    p.init(hp)
    np.testing.assert_array_equal(p.state("b").cpu().numpy(), state["b"])
    for name in ("lam", "prev_pred", "prev_loss"):
        p.state(name).copy_(torch.from_numpy(state[name]))
    p.state("clipped").copy_(torch.from_numpy(state["clipped"].astype(np.int32)))
    step, flags = p.update(hp, torch.from_numpy(sums).cuda(), debug=True)
    new, info = R.update(sums, state, np.diff(starts), qx, pos, n, rhp)
    step, flags = step.cpu().numpy(), flags.cpu().numpy()
    for i, name in enumerate(names):
        want_flags, want_tries = WANT_FLAGS[name]
        assert (info["flags"][i] == want_flags).all() and (info["tries"][i] == want_tries).all(), (name, info["flags"][i], info["tries"][i])
        assert (flags[i] & 0xff == want_flags).all() and (flags[i] >> 8 == want_tries).all(), (name, flags[i])
    for q, key in enumerate(("db", "dw", "pred", "lam")):
        np.testing.assert_allclose(step[:, :, q], info[key], rtol=1e-13, atol=0, equal_nan=True, err_msg=key)
    for key in ("b", "w", "lam", "prev_pred", "prev_loss"):
        np.testing.assert_allclose(p.state(key).cpu().numpy(), new[key], rtol=1e-13, atol=1e-300, equal_nan=True, err_msg=key)
    np.testing.assert_array_equal(p.state("clipped").cpu().numpy() != 0, new["clipped"])
    assert new["lam"][names.index("lam_at_the_upper_clamp"), 0] == 1e12 and new["lam"][names.index("lam_at_the_lower_clamp"), 0] == 1e-12
    assert np.isnan(new["prev_pred"][names.index("five_failures_fallback")]).all()
    assert (new["b"][-1] == 0).all() and (new["w"][-1] == 0).all() and (new["lam"][-1] == hp.lam_init).all()


# ---- fixtures G23 and G25 (the tags groups and wide) ------------------------------------------------------------------------------------------------------------------------

def _g23(tag):
    with np.load(GOLDEN / f"{'g25' if tag in ('groups', 'wide') else 'g23'}_probe1d_{tag}.npz") as z:
        return {k: z[k] for k in z.files}


def _csr(g):
    return scipy.sparse.csr_matrix((g["data"], g["indices"], g["indptr"]), shape=(int(g["n_rows"]), int(g["n_latents"])))


def _probe(g, **kw):
    from saev_amd import probe1d

    return probe1d.Sparse1DProbe(n_latents=int(g["n_latents"]), n_classes=int(g["n_classes"]), class_slab_size=int(g["class_slab_size"]),
                                 **{k: type(d)(g[k]) for k, d in (("ridge", 0.0), ("tol", 0.0), ("max_iter", 0), ("lam_init", 0.0), ("lam_shrink", 0.0),
                                                                  ("lam_grow", 0.0), ("delta_logit", 0.0))}, **kw)


@pytest.mark.parametrize("tag", ["plain", "absent", "groups", "wide"])
def test_evaluate_at_the_references_coefficients(tag):
    engine = _engine()
    g = _g23(tag)
    n, s, c = int(g["n_rows"]), int(g["n_latents"]), int(g["n_classes"])
    p = engine.Probe1D(n, s, c, g["data"].size, "cuda").prepare(*(torch.from_numpy(g[k]).cuda() for k in ("indptr", "indices", "data")),
                                                                labels=torch.from_numpy(g["labels"]).cuda())
    b, w = torch.from_numpy(g["r64_intercept"]).cuda(), torch.from_numpy(g["r64_coef"]).cuda()
    loss, tp, fp, tn, fn = (t.cpu().numpy() for t in p.evaluate(b, w, 0.5, dtype=torch.float64))
    for name, got in (("tp", tp), ("fp", fp), ("tn", tn), ("fn", fn)):
        np.testing.assert_array_equal(got, g[f"r64_{name}"], err_msg=name)  # exact integers, the reference's on every pair
    want = R.evaluate(g["indptr"], g["indices"], g["data"], s, g["labels"], c, g["r64_intercept"], g["r64_coef"])
    assert (np.abs(loss - want[0]) <= 1e-12 * want[5] + 1e-300).all()
    f32 = p.evaluate(b, w, 0.5)  # the same, rounded once to float32 on the way out
    np.testing.assert_array_equal(f32[0].cpu().numpy(), loss.astype(np.float32))
    np.testing.assert_array_equal(f32[1].cpu().numpy(), tp.astype(np.float32))
    with pytest.raises(ValueError, match="between 0 and 1"):
        p.evaluate(b, w, 1.0)


@pytest.fixture(scope="module")
def fits():
    """One fit per (fixture, dtype), shared: (probe, x, labels, metrics)."""
    done = {}

    def get(tag, dtype):
        if (tag, dtype) not in done:
            g = _g23(tag)
            probe, x, y = _probe(g, dtype=dtype), _csr(g), g["labels"]
            probe.fit(x, y)
            done[tag, dtype] = (g, probe, x, y, probe.loss_matrix_with_aux(x, y))
        return done[tag, dtype]

    return get


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["float32", "float64"])
@pytest.mark.parametrize("tag", ["plain", "absent", "groups", "wide"])
def test_fit_end_to_end_against_the_reference(fits, tag, dtype):
    """fit, then loss_matrix_with_aux, on the reference's recorded results (R64: dtype=float64, R32: its default float32):
    n_iter equal to R64's; every loss within loss_band = max |L_R32 - L_R64| of R64's; coefficient and intercept of every well-posed
    pair within coef_band (4 x R32's largest distance over those pairs) of R64's, and at most 1 % of all pairs outside it."""
    g, probe, x, y, metrics = fits(tag, dtype)
    n, c = int(g["n_rows"]), int(g["n_classes"])
    assert probe.coef_.dtype == dtype and probe.intercept_.dtype == dtype and probe.latent_qx_.dtype == dtype
    np.testing.assert_array_equal(probe.n_iter_.cpu().numpy(), g["r64_n_iter"])
    np.testing.assert_allclose(probe.latent_qx_.double().cpu().numpy(), g["r64_qx"], rtol=1e-14 if dtype == torch.float64 else 2.0 ** -24)
    coef, icpt = probe.coef_.double().cpu().numpy(), probe.intercept_.double().cpu().numpy()
    dist = np.maximum(np.abs(coef - g["r64_coef"]) / (1 + np.abs(g["r64_coef"])), np.abs(icpt - g["r64_intercept"]) / (1 + np.abs(g["r64_intercept"])))
    loss, tp, fp, tn, fn = (m.cpu().numpy() for m in metrics)
    assert loss.dtype == np.float32 and loss.shape == g["r64_loss"].shape
    dl = np.abs(loss.astype(np.float64) - g["r64_loss"].astype(np.float64))
    print(f"{tag} {dtype}: largest distance {dist.max():.3g}, well-posed {dist[g['well_posed']].max():.3g}, coef_band {float(g['coef_band']):.3g}, "
          f"outside {(dist > g['coef_band']).mean():.4f}; largest loss difference {dl.max():.3g}, loss_band {float(g['loss_band']):.3g}")
    assert (dl <= g["loss_band"]).all()
    assert (dist[g["well_posed"]] <= g["coef_band"]).all()
    assert (dist > g["coef_band"]).mean() <= 0.01
    np.testing.assert_array_equal(tp + fp + tn + fn, np.float32(n))
    np.testing.assert_array_equal(tp + fn, np.broadcast_to(np.bincount(g["labels"], minlength=c).astype(np.float32), tp.shape))
    np.testing.assert_array_equal(probe.loss_matrix(x, y).cpu().numpy(), loss)


def test_label_matrix_and_torch_csr_inputs_give_the_same_fit(fits):
    g, probe, x, y, metrics = fits("plain", torch.float32)
    other = _probe(g)
    xt = torch.sparse_csr_tensor(torch.from_numpy(g["indptr"]), torch.from_numpy(g["indices"].astype(np.int64)), torch.from_numpy(g["data"]),
                                 size=x.shape)
    ymat = torch.from_numpy(R.labels_matrix(y, int(g["n_classes"])).astype(np.float32))
    other.fit(xt, ymat)
    assert torch.equal(other.coef_, probe.coef_) and torch.equal(other.intercept_, probe.intercept_) and torch.equal(other.n_iter_, probe.n_iter_)
    for a, b in zip(other.loss_matrix_with_aux(xt, ymat.bool()), metrics):
        assert torch.equal(a, b)


@pytest.mark.parametrize("tag", ["plain", "absent", "groups", "wide"])
def test_two_fits_and_a_polled_fit_give_identical_bits(tag):
    engine = _engine()
    g = _g23(tag)
    n, s, c = int(g["n_rows"]), int(g["n_latents"]), int(g["n_classes"])
    hp = engine.Probe1DHyper(max_iter=30, class_slab_size=int(g["class_slab_size"]))
    outs = []
    for poll in (0, 0, 1, 7):
        p = engine.Probe1D(n, s, c, g["data"].size, "cuda").prepare(*(torch.from_numpy(g[k]).cuda() for k in ("indptr", "indices", "data")),
                                                                    labels=torch.from_numpy(g["labels"]).cuda())
        coef, icpt, n_iter = p.fit(hp, dtype=torch.float64, poll_every=poll)
        outs.append((coef.cpu().numpy().view(np.uint64), icpt.cpu().numpy().view(np.uint64), n_iter.cpu().numpy(), p.done.cpu().numpy().copy()))
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(outs[0][2], g["r64_n_iter"])
    n_slabs = -(-c // hp.class_slab_size)
    assert (outs[0][3][:n_slabs] == 1).all()  # every slab met its tolerance before max_iter in these designs


def test_worker_fn_writes_the_references_files(tmp_path):
    from saev_amd import disk, probe1d
    from saev_amd.data import write_shards

    rng = np.random.default_rng(11)
    d_sae, n_cls, shards, acts, labels = 24, 5, [], [], []
    for i in range(2):
        n_ex = 40 + 10 * i
        lab = rng.integers(0, n_cls, size=(n_ex, 6)).astype(np.uint8)
        shards.append(write_shards(tmp_path / f"s{i}", rng.standard_normal((n_ex, 1, 6, 8)).astype(np.float32), labels=lab))
        x = scipy.sparse.random(n_ex * 6, d_sae, density=0.2, format="csr", dtype=np.float32, random_state=i)
        x.data += (lab.reshape(-1)[x.nonzero()[0]] == (x.nonzero()[1] % n_cls)).astype(np.float32)
        acts.append(x)
        labels.append(lab.reshape(-1))
    run = disk.Run.new("probe0001", train_shards_dir=shards[0], val_shards_dir=shards[1], runs_root=tmp_path / "saev" / "runs")
    for sh, x in zip(shards, acts):
        (run.inference / sh.name).mkdir()
        scipy.sparse.save_npz(run.inference / sh.name / "token_acts.npz", x)
    cfg = probe1d.Config(run=run.run_dir, train_shards=shards[0], test_shards=shards[1], max_iter=12)
    assert probe1d.worker_fn(cfg) == 0
    probe = probe1d.Sparse1DProbe(n_latents=d_sae, n_classes=n_cls, ridge=cfg.ridge, max_iter=cfg.max_iter)
    probe.fit(acts[0], labels[0])
    for sh, x, lab in zip(shards, acts, labels):
        with np.load(run.inference / sh.name / "probe1d_metrics.npz") as z:
            assert sorted(z.files) == sorted(("loss", "weights", "biases", "tp", "fp", "tn", "fn"))
            want = dict(zip(("loss", "tp", "fp", "tn", "fn"), probe.loss_matrix_with_aux(x, lab)), weights=probe.coef_, biases=probe.intercept_)
            for key, t in want.items():
                assert z[key].shape == (d_sae, n_cls) and z[key].dtype == np.float32, key
                np.testing.assert_array_equal(z[key], t.cpu().numpy(), err_msg=key)
    assert dataclasses.replace(cfg, max_iter=3).max_iter == 3
