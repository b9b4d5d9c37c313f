"""GPU tests of SPARSE LINEAR (include/saev_amd.h): engine.pool_images and engine.l1_logistic against the numpy
restatement (tests/sparse_linear_restatement.py) and fixture G27 (the reference's pooling, scikit-learn's fits), and the audit end to
end from files this project wrote.

Tolerances (derived, not tuned).

POOLING is exact: np.array_equal with the restatement and with the reference's recorded output.

KKT.  Recomputed on the host in float64 from the returned coef_ / intercept_, the residual is <= kkt_tol + (n + K + 4) 2^-52 C
max_j sum_i |x_ij|: the second term is the rounding of one gradient element's float64 sum of n products of |r| <= 1 with x.

OBJECTIVE.  F is convex: for any subgradient s at a,  F(a) - F(b) <= <s, a - b> <= ||s||_inf (||W_a - W_b||_1 + ||b_a - b_b||_1),
and the KKT residual eps_a (host-recomputed) is the smallest ||s||_inf.  Applied in both directions to (ours, restatement) and (ours,
G27's converged fit).  Both objectives are themselves float64 evaluations, so the comparison allows their rounding
(R.objective_rounding: the n + S K term sum of non-negative terms, and the dot products inside the logits through the loss, which
is 2-Lipschitz in the logits' largest error).  F(ours) <= F(the reference's default fit) is a condition, not a tolerance.

W = 0 DESIGNS.  With W = 0 the problem is the intercept-only one, whose optimum is the closed form b* (log(n_1 / n_0) for K = 2,
log(n_k / n) minus its mean for K >= 3).  Its Hessian in b at b* is C n (diag(p) - p p^T); on the mean-zero subspace the
intercepts live in (or on the line, for K = 2, where it is C n p (1 - p)) its smallest eigenvalue is at least
mu = C n min_k p_k (1 - p_k).  A point with gradient norm eps is then within eps / mu of b* if the curvature stayed mu along the
way; it changes inside that neighbourhood, which the factor 2 covers: |b - b*|_inf <= 2 eps / (C n min_k p_k (1 - p_k)), eps the
host-recomputed residual.

SCALED X.  X * 1e-3 at the same C: every |g| is 1e-3 of what it was, the optimum is W = 0 and L never leaves 1-8.  X * 1e3 is run at
C / 1e3: with C kept it is the (nearly) unpenalised, nearly separable problem, whose conditioning between the intercept (curvature
C n / 4) and the coefficients (1e6 times the original) no first-order method resolves -- the float64 restatement stops at max_iter
with residuals of 1e-4 to 5e-2 on every design tried -- while C / 1e3 keeps the gradients of the coefficients and takes L to 1e3 times its original
value, ten more doublings (the intercept's gradient shrinks with C, so its residual is met early and the optimum found is not the
original one rescaled: the bounds above are what is asserted, not the support)."""

import json
import pickle
import warnings

import numpy as np
import pytest
import scipy.sparse
import torch

import sparse_linear_restatement as R
from sparse_linear_cases import N_CLS, c_keeping_features, closed_form_intercepts, cls_design, golden, make_design, pool_design

pytestmark = [pytest.mark.gpu, pytest.mark.encoder_modes("f32")]
DEV = "cuda"


# ---------------------------------------------------------------- pooling --------------------------------------------------------------

def _pool(indptr, indices, data, n_img, tpi, s, agg):
    from saev_amd import engine

    args = (torch.from_numpy(np.asarray(indptr, np.int64)).to(DEV), torch.from_numpy(np.asarray(indices, np.int32)).to(DEV),
            torch.from_numpy(np.asarray(data, np.float32)).to(DEV))
    return engine.pool_images(*args, n_img, tpi, s, agg)


@pytest.mark.parametrize("tpi", [1, 3, 64, 257])
@pytest.mark.parametrize("s", [1, 63, 64, 65, 1000, 70001])
def test_pooling_equals_the_restatement(tpi, s):
    n_img = 300 if (tpi, s) == (3, 65) else 5
    indptr, indices, data = pool_design(n_img, tpi, s, 100 * tpi + s % 97)
    for agg in ("max", "mean"):
        res = _pool(indptr, indices, data, n_img, tpi, s, agg)
        got = res.pooled.cpu().numpy()
        want = R.pool_images(indptr, indices, data, n_img, tpi, s, agg)
        assert got.dtype == np.float32 and got.shape == (n_img, s) and np.array_equal(got, want), agg
        assert res.ranges == -(-s // res.range_len) and (res.ranges > 1) == (s == 70001)  # the last S is past one workgroup's range
    mx = _pool(indptr, indices, data, n_img, tpi, s, "max").pooled.cpu().numpy()
    assert mx[0, 0] == -1.0  # stored in every patch, negative values only: a negative maximum
    if s > 1 and tpi > 1:
        assert mx[0, s - 1] == 0.0  # stored in tpi - 1 patches: the implicit 0 wins
    if n_img > 1:
        assert not mx[1].any()


@pytest.mark.parametrize("i", range(4))
def test_pooling_equals_the_references_recorded_output(i):
    g = golden()
    n_img, tpi, s = (int(v) for v in g[f"pool{i}_shape"])
    for agg in ("max", "mean"):
        got = _pool(g[f"pool{i}_indptr"], g[f"pool{i}_indices"], g[f"pool{i}_data"], n_img, tpi, s, agg).pooled.cpu().numpy()
        assert np.array_equal(got, g[f"pool{i}_{agg}"]), agg
    if i == 0:  # the order-sensitive mean: 1e8, 1, -1e8, 1 in float32 patch order
        assert got[0, 2] == np.float32(0.25)


def test_pooling_errors_and_determinism():
    indptr, indices, data = pool_design(6, 3, 1000, 5)
    a = _pool(indptr, indices, data, 6, 3, 1000, "mean").pooled
    b = _pool(indptr, indices, data, 6, 3, 1000, "mean").pooled
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    bad = indices.copy()
    bad[len(bad) // 2] = 1000
    res = _pool(indptr, bad, data, 6, 3, 1000, "max")
    with pytest.raises(ValueError, match="column index"):
        res.pooled
    with pytest.raises(ValueError, match="column index"):  # every read raises, not just the first
        res.pooled
    for v in (np.inf, -np.inf, np.nan):
        d = data.copy()
        d[3] = v
        with pytest.raises(ValueError, match="not finite"):
            _pool(indptr, indices, d, 6, 3, 1000, "max").pooled
    _pool(indptr, indices, data, 6, 3, 1000, "max").pooled  # and a good call after them is good


# ---------------------------------------------------------------- the solver -----------------------------------------------------------

def _fit(x, y, c, **kw):
    from saev_amd import engine

    return engine.l1_logistic(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(DEV), torch.from_numpy(np.asarray(y)).to(DEV), c, **kw)


def _host(res):
    return res.coef_.cpu().numpy(), res.intercept_.cpu().numpy()


def check_fit(x, y, c, res, *, other=None, kkt_tol=1e-4, label=""):
    """The KKT bound of a fit and, against ``other`` = (coef, intercept) of another solver, the objective bound in both directions.
    Returns (host KKT residual, host objective)."""
    classes, yi = R.class_indices(y)
    k, n = len(classes), len(y)
    w, b = _host(res)
    assert res.converged_ and w.shape == ((1 if k == 2 else k), x.shape[1]) and w.dtype == np.float64 and b.shape == (w.shape[0],)
    assert res.classes_.cpu().numpy().tolist() == classes.tolist()
    eps = R.kkt_residual(x, yi, k, w, b, c)
    slack = R.gradient_rounding(x, n, k, c)
    f = R.objective(x, yi, k, w, b, c)
    print(f"{label}: n {n} S {x.shape[1]} K {k} C {c:.4g}: {res.n_iter_} iterations, L {res.lipschitz_:g}, rejected {res.n_rejected_}, restarts {res.n_restarts_}, "
          f"kkt host {eps:.4g} device {res.kkt_residual_:.4g} (tol + {slack:.2g}), F host {f:.17g} device {res.objective_:.17g}")
    assert eps <= kkt_tol + slack
    assert abs(res.kkt_residual_ - eps) <= slack + 1e-12 * eps and abs(res.objective_ - f) <= R.objective_rounding(x, w, b, c, f)
    if k > 2:
        assert abs(b.mean()) <= 8 * 2.0 ** -52 * np.abs(b).max()
    if other is not None:
        wo, bo = other
        eps_o, f_o = R.kkt_residual(x, yi, k, wo, bo, c), R.objective(x, yi, k, wo, bo, c)
        dist = float(np.abs(w - wo).sum() + np.abs(b - bo).sum())
        rounding = R.objective_rounding(x, w, b, c, f) + R.objective_rounding(x, wo, bo, c, f_o)
        print(f"    F ours - other {f - f_o:.3g} (bound {eps * dist:.3g}), other - ours {f_o - f:.3g} (bound {eps_o * dist:.3g}), rounding {rounding:.2g}")
        assert f - f_o <= eps * dist + rounding and f_o - f <= eps_o * dist + rounding
    return eps, f


def check_zero(x, y, c, res, eps):
    """W = 0 exactly and the intercepts within 2 eps / (C n min p (1 - p)) of the closed form (the module's docstring)."""
    w, b = _host(res)
    assert (w == 0.0).all()
    want, curv = closed_form_intercepts(y)
    tol = 2 * eps / (c * len(y) * curv)
    print(f"    intercepts: largest distance from the closed form {np.abs(b - want).max():.3g}, tolerance {tol:.3g}")
    assert np.abs(b - want).max() <= tol + 4 * 2.0 ** -52 * np.abs(want).max()


@pytest.fixture(scope="module")
def g27():
    return golden()


@pytest.mark.parametrize("tag", ["sparse", "zero"])
@pytest.mark.parametrize("i", range(N_CLS))
def test_g27_designs(g27, i, tag):
    x, y, k = cls_design(g27, i)
    n, tpi, s, _ = (int(v) for v in g27[f"cls{i}_shape"])
    pooled = _pool(g27[f"cls{i}_indptr"], g27[f"cls{i}_indices"], g27[f"cls{i}_data"], n, tpi, s, "max").pooled.cpu().numpy()
    assert np.array_equal(pooled, x)  # X is the device's own pooling of the stored tokens
    c = float(g27[f"cls{i}_{tag}_C"])
    res = _fit(pooled, y, c)
    own = R.fista(x, y, c)
    eps, f = check_fit(x, y, c, res, other=(own["coef"], own["intercept"]), label=f"cls{i} {tag} vs the restatement")
    centre = (lambda b: b - b.mean()) if k > 2 else (lambda b: b)
    wo, bo = g27[f"cls{i}_{tag}_opt_coef"], centre(g27[f"cls{i}_{tag}_opt_intercept"])
    check_fit(x, y, c, res, other=(wo, bo), label=f"cls{i} {tag} vs G27's converged fit")
    _, yi = R.class_indices(y)
    f_ref = R.objective(x, yi, k, g27[f"cls{i}_{tag}_ref_coef"].astype(np.float64), g27[f"cls{i}_{tag}_ref_intercept"].astype(np.float64), c)
    print(f"    F(the reference's default fit) - F(ours) = {f_ref - f:.3g}")
    assert f <= f_ref
    w, _ = _host(res)
    assert np.array_equal(w != 0, wo != 0)
    assert np.array_equal(R.ranked_support(w), R.ranked_support(wo))
    if tag == "zero":
        check_zero(x, y, c, res, eps)
    else:
        assert 5 <= len(R.ranked_support(w)) <= 15


# every n of {2, 63, 65, 257, 1025}, every S of {1, 31, 33, 255, 257, 4097} and every K of {2, 3, 7, 33, 64} at least once
RAGGED = [(2, 1, 2), (2, 4097, 2), (63, 31, 3), (63, 1, 7), (65, 33, 7), (65, 255, 33), (257, 255, 33), (257, 4097, 2), (257, 31, 64), (1025, 257, 64),
          (1025, 33, 3), (1025, 4097, 7)]


@pytest.mark.parametrize("shape", RAGGED, ids=["x".join(map(str, s)) for s in RAGGED])
def test_ragged_shapes(shape):
    n, s, k = shape
    x, y = make_design(n, s, k, 7 * n + s + k)
    c = c_keeping_features(x, y)
    res = _fit(x, y, c)
    own = R.fista(x, y, c)
    assert own["converged"]
    check_fit(x, y, c, res, other=(own["coef"], own["intercept"]), label="ragged")
    if not (n, s) == (2, 1):
        assert len(R.ranked_support(_host(res)[0])) >= 1


def test_zero_optimum_at_ragged_shapes():
    for n, s, k in [(63, 33, 3), (257, 31, 2), (1025, 255, 7)]:
        x, y = make_design(n, s, k, n + k)
        c = c_keeping_features(x, y, factor=0.5)
        res = _fit(x, y, c)
        eps, _ = check_fit(x, y, c, res, label="zero optimum")
        check_zero(x, y, c, res, eps)


def test_duplicate_columns():
    """W is not unique: the objective and the KKT residual only."""
    x, y = make_design(96, 40, 3, 11)
    x = np.concatenate([x, x[:, :12]], axis=1)
    c = c_keeping_features(x, y)
    res = _fit(x, y, c)
    own = R.fista(x, y, c)
    check_fit(x, y, c, res, other=(own["coef"], own["intercept"]), label="duplicate columns")


@pytest.mark.parametrize("k", [2, 5])
def test_scaled_x(k):
    x, y = make_design(200, 60, k, 21 + k)
    c = c_keeping_features(x, y)
    base = _fit(x, y, c)
    check_fit(x, y, c, base, label="scale 1")
    up, c_up = x * np.float32(1e3), c / 1e3
    res = _fit(up, y, c_up)
    own = R.fista(up, y, c_up)
    check_fit(up, y, c_up, res, other=(own["coef"], own["intercept"]), label="scale 1e3 at C / 1e3")
    assert res.lipschitz_ >= 256 * base.lipschitz_  # 1e3 times the curvature: at least eight more doublings
    down = x * np.float32(1e-3)
    res = _fit(down, y, c)
    eps, _ = check_fit(down, y, c, res, label="scale 1e-3")
    check_zero(down, y, c, res, eps)


def test_class_ids_absent_from_y_and_refusals():
    x, y = make_design(120, 33, 3, 5)
    ids = np.asarray([0, 2, 5])[y]
    c = c_keeping_features(x, y)
    res = _fit(x, ids, c)
    assert res.classes_.cpu().numpy().tolist() == [0, 2, 5] and res.coef_.shape == (3, 33)
    same = _fit(x, y, c)
    assert torch.equal(res.coef_, same.coef_) and torch.equal(res.intercept_, same.intercept_)
    check_fit(x, ids, c, res, label="ids 0, 2, 5")
    # two classes: one row, the positive class is classes_[1]
    two = _fit(x, np.where(y == 0, 9, 4), c)
    assert two.classes_.cpu().numpy().tolist() == [4, 9] and two.coef_.shape == (1, 33)
    check_fit(x, np.where(y == 0, 9, 4), c, two, label="ids 4, 9")
    with pytest.raises(ValueError, match="only one class"):
        _fit(x, np.zeros(120, dtype=np.int64), c)
    with pytest.raises(ValueError, match="at most 64"):
        _fit(x, np.arange(120) % 65, c)
    bad = x.copy()
    bad[7, 3] = np.inf
    with pytest.raises(ValueError, match="not finite"):
        _fit(bad, y, c)
    bad[7, 3] = np.nan
    with pytest.raises(ValueError, match="not finite"):
        _fit(bad, y, c)


def test_max_iter_determinism_and_check_every():
    x, y = make_design(257, 255, 7, 3)
    c = c_keeping_features(x, y)
    with pytest.warns(RuntimeWarning, match="not converged"):
        short = _fit(x, y, c, max_iter=3)
    assert short.converged_ is False and short.n_iter_ == 3
    w, b = _host(short)
    _, yi = R.class_indices(y)
    # what an unfinished fit reports is the residual and the objective of the iterate it returns
    assert abs(short.kkt_residual_ - R.kkt_residual(x, yi, 7, w, b, c)) <= R.gradient_rounding(x, 257, 7, c) + 1e-12 * short.kkt_residual_
    assert abs(short.objective_ - R.objective(x, yi, 7, w, b, c)) <= R.objective_rounding(x, w, b, c, short.objective_)
    with warnings.catch_warnings():
        warnings.filterwarnings("error", category=RuntimeWarning)
        a = _fit(x, y, c)
        b25 = _fit(x, y, c, check_every=25)
        b1 = _fit(x, y, c, check_every=1)
    for other in (b25, b1):
        assert torch.equal(a.coef_.view(torch.int64), other.coef_.view(torch.int64)) and torch.equal(a.intercept_.view(torch.int64), other.intercept_.view(torch.int64))
        assert (a.n_iter_, a.kkt_residual_, a.objective_, a.lipschitz_) == (other.n_iter_, other.kkt_residual_, other.objective_, other.lipschitz_)


# ---------------------------------------------------------------- end to end -----------------------------------------------------------

def test_the_audit_runs_from_files_this_project_wrote(tmp_path):
    from saev_amd import classification as cl
    from saev_amd import disk
    from saev_amd.data import write_shards

    rng = np.random.default_rng(8)
    d_sae, tpi, habitats = 48, 6, ["demersal", "pelagic", "reef-associated"]

    def split(n_ex, seed):
        r = np.random.default_rng(seed)
        img_y = r.integers(0, 3, size=n_ex)
        img_y[:3] = np.arange(3)
        seg = r.choice(np.array([0, 2, 3, 7], dtype=np.uint8), size=(n_ex, tpi))
        shards = write_shards(tmp_path / f"s{n_ex}", r.standard_normal((n_ex, 1, tpi, 8)).astype(np.float32), labels=seg)
        x = scipy.sparse.random(n_ex * tpi, d_sae, density=0.15, format="lil", dtype=np.float32, random_state=seed)
        for i in range(n_ex):
            for j in range(2):
                x[i * tpi + int(r.integers(tpi)), 3 * img_y[i] + j] = 2.0 + r.random()
        x = x.tocsr().astype(np.float32)
        x.sort_indices()
        with open(shards / "image_labels.csv", "w") as fd:
            fd.write("stem,habitat,water\n" + "".join(f"img{i},{habitats[img_y[i]]},salt\n" for i in range(n_ex)))
        return shards, x, img_y

    (train_shards, train_x, train_y), (test_shards, test_x, test_y) = split(60, 1), split(40, 2)
    run = disk.Run.new("audit0002", train_shards_dir=train_shards, val_shards_dir=test_shards, runs_root=tmp_path / "saev" / "runs")
    for shards, x in ((train_shards, train_x), (test_shards, test_x)):
        (run.inference / shards.name).mkdir()
        scipy.sparse.save_npz(run.inference / shards.name / "token_acts.npz", x)
    pooled = cl.aggregate_to_images(train_x, 60, tpi, cl.PatchAgg.MAX)
    c = c_keeping_features(pooled, train_y)
    cfg = cl.TrainConfig(run=run.run_dir, train_shards=train_shards, test_shards=test_shards, task=cl.LabelGrouping(name="habitat", source_col="habitat"),
                         cls=cl.SparseLinear(C=c))
    assert cl.train_worker_fn(cfg) == 0
    ckpt = run.inference / test_shards.name / f"cls_habitat_max_C{c}.pkl"
    with open(ckpt, "rb") as fd:
        header = json.loads(fd.readline())
        payload = pickle.load(fd)
    assert sorted(header) == ["cfg", "class_names", "n_classes", "test_acc"] and header["class_names"] == habitats and header["n_classes"] == 3
    assert header["cfg"]["cls"] == {"key": "sparse-linear", "C": c, "max_iter": 90, "kkt_tol": 1e-4, "solver_iters": 5000} and header["cfg"]["patch_agg"] == "max"
    clf = payload["classifier"]
    assert isinstance(clf, cl.SparseLinearClassifier) and clf.converged_ and clf.coef_.shape == (3, d_sae) and clf.classes_.tolist() == [0, 1, 2]
    _, yi = R.class_indices(train_y)
    assert R.kkt_residual(pooled, yi, 3, clf.coef_, clf.intercept_, c) <= 1e-4 + R.gradient_rounding(pooled, 60, 3, c)
    test_pooled = R.pool_images(test_x.indptr, test_x.indices, test_x.data, 40, tpi, d_sae, "max")
    assert np.array_equal(payload["test_y"], test_y) and np.array_equal(payload["test_pred"], clf.predict(test_pooled))
    assert header["test_acc"] == float((payload["test_pred"] == test_y).mean()) and header["test_acc"] > 0.5
    support = int((np.abs(clf.coef_).sum(axis=0) > 0).sum())
    assert 1 <= support < d_sae

    ecfg = cl.EvalConfig(run=run.run_dir, test_shards=test_shards, cls_checkpoints=(ckpt,), max_budget=10, budgets=(1, 3, 10), tau=0.3)
    assert cl.eval_worker_fn(ecfg) == 0
    out = json.loads((run.inference / test_shards.name / "audit_results.json").read_text())
    assert out["d_sae"] == d_sae and len(out["classifiers"]) == 1
    entry = out["classifiers"][0]
    assert entry["cls_type"] == "sparse-linear" and entry["n_nonzero_importance"] == support and entry["cls_checkpoint"] == str(ckpt)

    # a grouped task masks the unlisted label out, and the mean pooling goes through the same path
    gcfg = cl.TrainConfig(run=run.run_dir, train_shards=train_shards, test_shards=test_shards, patch_agg=cl.PatchAgg.MEAN,
                          task=cl.LabelGrouping(name="open", source_col="habitat", groups={"open": ["pelagic"], "floor": ["demersal"]}), cls=cl.SparseLinear(C=4 * c))
    assert cl.train_worker_fn(gcfg) == 0
    with open(run.inference / test_shards.name / f"cls_open_mean_C{4 * c}.pkl", "rb") as fd:
        gheader = json.loads(fd.readline())
        gpayload = pickle.load(fd)
    assert gheader["class_names"] == ["floor", "open"] and gpayload["classifier"].coef_.shape == (1, d_sae)
    assert len(gpayload["test_y"]) == int((test_y != 2).sum()) and set(gpayload["test_y"].tolist()) == {0, 1}
