"""GPU tests of the k-means baseline (include/saev_amd.h: K-MEANS; saev_amd/baselines.py).

Tolerance.  tol(D) = (D + 3) 2^-24, relative, on squared distances: one rounding per difference, one per square and at most D - 1
per sum over non-negative terms.  Every dist2 lies within tol(D) of the fp64 row optimum, the fp64 value of the returned pair
within 2 tol(D) of it, and the index equals the fp64 arg-optimum on the rows whose fp64 runner-up differs from the best by more than
4 tol(D) times itself; a test that asserts equality for every row asserts that gap first.  Shapes are the smallest that reach each
class of the 128 x 128 tile, of the 64-wide k stage and of the 64 x 64 exact tile.

Route.  Where the filter is expected to answer, the test says so: route == "filter", no overflow, and the number of candidates the
device reports lies inside the bracket (sure, maybe) that the restated candidate rule gives for the same device tensors
(kmeans_restatement.candidate_bracket; test_kmeans_host_cpu.py holds the same inputs below half the capacity on the CPU).  Without
that, a filter that always fell back to the exact route would pass every comparison of the two routes."""

import json

import numpy as np
import pytest
import scipy.sparse
import torch

import kmeans_cases as K
import kmeans_restatement as R
from conftest import GOLDEN

pytestmark = [pytest.mark.gpu, pytest.mark.encoder_modes("f32")]

DEV = "cuda:0"
ASSIGN_SHAPES = K.ASSIGN_SHAPES


def tol(D):
    return (D + 3) * 2.0 ** -24


def d2_64(X, C):
    """(n, k) fp64 squared distances, difference form, on the device."""
    return torch.cdist(X.double(), C.double(), compute_mode="donot_use_mm_for_euclid_dist").pow(2)


def check_assign(res, X, C, farthest, label=""):
    """The three rules of the module docstring; returns the number of rows whose index the gap rule decides."""
    D = X.shape[1]
    d = d2_64(X, C)
    best, arg = (d.max(dim=1) if farthest else d.min(dim=1))
    got, idx = res.dist2.double(), res.indices.long()
    assert idx.min() >= 0 and idx.max() < C.shape[0]
    err = ((got - best).abs() / best.clamp_min(1e-300)).max().item() if best.max() > 0 else (got - best).abs().max().item()
    pair = d[torch.arange(X.shape[0], device=X.device), idx]
    perr = ((pair - best).abs() / pair.clamp_min(1e-300)).max().item()
    if C.shape[0] > 1:
        two = d.topk(2, dim=1, largest=farthest).values
        decided = (two[:, 0] - two[:, 1]).abs() > 4 * tol(D) * two[:, 1].abs()
    else:
        decided = torch.ones(X.shape[0], dtype=torch.bool, device=X.device)
    print(f"{label} farthest={farthest}: dist2 err {err:.3g} (tol {tol(D):.3g}), pair err {perr:.3g}, decided rows {int(decided.sum())}/{X.shape[0]}, "
          f"route {res.route}, overflow {res.overflow}, candidates/row {res.candidates / X.shape[0]:.2f}, tiles {res.tiles_refiltered}")
    assert err <= tol(D) and perr <= 2 * tol(D)
    assert torch.equal(idx[decided], arg[decided])
    return int(decided.sum())


def same_bits(a, b):
    return torch.equal(a.dist2.view(torch.int32), b.dist2.view(torch.int32)) and torch.equal(a.indices, b.indices)


def check_filter(res, bracket, label=""):
    """The filter answered, with a number of candidates inside the restated rule's bracket (assign and collapsed alike)."""
    sure, maybe = bracket
    print(f"{label}: route {res.route}, overflow {res.overflow}, candidates {res.candidates} in [{sure}, {maybe}] of {res.capacity}")
    assert res.route == "filter" and not res.overflow
    assert sure <= res.candidates <= maybe


@pytest.mark.parametrize("n,k,D", ASSIGN_SHAPES)
def test_assign_against_fp64_on_both_routes(n, k, D):
    from saev_amd.engine import kmeans_assign

    X, C = (t.to(DEV) for t in K.gaussian(n, k, D))
    brackets = R.candidate_brackets(X, C) if k > 1 else None
    for farthest in (False, True):
        auto = kmeans_assign(X, C, farthest=farthest)
        check_assign(auto, X, C, farthest, f"({n}, {k}, {D})")
        if k > 1:
            check_filter(auto, brackets[farthest], f"({n}, {k}, {D}) farthest={farthest}")
        exact = kmeans_assign(X, C, farthest=farthest, route="exact")
        assert exact.route == "exact" and not exact.overflow
        assert same_bits(auto, exact), "both routes return the same bits"
        assert same_bits(auto, kmeans_assign(X, C, farthest=farthest)), "two calls give the same bits"
        assert auto.capacity == min(n * k, max(4096, 8 * n))
        if k == 1:  # nothing to filter: the exact route, and no overflow to report
            assert auto.route == "exact" and not auto.overflow and auto.candidates == 0


def test_assign_returns_the_refined_value_bit_for_bit():
    from saev_amd.engine import kmeans_assign

    g = torch.Generator().manual_seed(5)
    X, C = torch.randn(70, 68, generator=g) + 2, torch.randn(45, 68, generator=g) + 2
    r = torch.from_numpy(R.r_fp32(X.numpy(), C.numpy()))
    for farthest in (False, True):
        res = kmeans_assign(X.to(DEV), C.to(DEV), farthest=farthest)
        want = r.max(dim=1) if farthest else r.min(dim=1)
        assert torch.equal(res.dist2.cpu(), want.values)
        assert torch.equal(r[torch.arange(70), res.indices.cpu().long()], want.values)


def test_assign_ties_go_to_the_smallest_index():
    from saev_amd.engine import kmeans_assign

    g = torch.Generator().manual_seed(7)
    C = 4 * torch.randn(50, 16, generator=g)
    C[40] = C[5]
    C[17] = C[5]
    X = C[5] + 0.01 * torch.randn(20, 16, generator=g)
    d = d2_64(X.to(DEV), C.to(DEV))
    others = d[:, [j for j in range(50) if j not in (5, 17, 40)]].min(dim=1).values
    assert bool((others > 100 * d[:, 5]).all()), "the gap: every other centre is far"
    for route in ("auto", "exact"):
        res = kmeans_assign(X.to(DEV), C.to(DEV), route=route)
        assert res.indices.tolist() == [5] * 20


def test_assign_identical_centres_overflow_to_the_exact_route():
    from saev_amd.engine import kmeans_assign

    X, C = (t.to(DEV) for t in K.identical_centres())
    res = kmeans_assign(X, C)
    assert res.overflow and res.route == "exact"
    assert res.candidates > res.capacity, "overflow by count, not for want of a unit image"
    assert same_bits(res, kmeans_assign(X, C, route="exact"))
    assert res.indices.tolist() == [0] * 65
    check_assign(res, X, C, False, "identical centres")


def test_assign_far_from_the_origin():
    """Activations with a large mean: rows = 100 + 0.01 randn.  The centring on the mean of the centres is what lets the filter
    answer here: it does, with the candidates the restated rule counts (about 1.03 per row)."""
    from saev_amd.engine import kmeans_assign

    X, C = (t.to(DEV) for t in K.far_from_the_origin())
    brackets = R.candidate_brackets(X, C)
    for farthest in (False, True):
        res = kmeans_assign(X, C, farthest=farthest)
        check_assign(res, X, C, farthest, "far from the origin")
        check_filter(res, brackets[farthest], f"far from the origin farthest={farthest}")
        assert same_bits(res, kmeans_assign(X, C, farthest=farthest, route="exact"))


def test_assign_refuses_non_finite_input():
    from saev_amd.engine import kmeans_assign

    g = torch.Generator().manual_seed(13)
    X, C = torch.randn(130, 16, generator=g).to(DEV), torch.randn(70, 16, generator=g).to(DEV)
    bad = X.clone()
    bad[129, 15] = float("nan")
    with pytest.raises(ValueError, match="inf or a NaN"):
        kmeans_assign(bad, C)
    bad = C.clone()
    bad[3, 0] = float("inf")
    for route in ("auto", "exact"):
        with pytest.raises(ValueError, match="inf or a NaN"):
            kmeans_assign(X, bad, route=route)


def _index_cases():
    g = torch.Generator().manual_seed(17)
    yield "every centre once", torch.randperm(257, generator=g).to(torch.int32), 257, 4
    idx = torch.full((3000,), 11, dtype=torch.int32)
    yield "one centre takes all", idx, 37, 68
    yield "most centres empty", torch.randint(0, 5000, (300,), generator=g).to(torch.int32) // 100 * 100, 5000, 4096
    long = torch.where(torch.rand(9000, generator=g) < 0.6, torch.tensor(3), torch.randint(0, 7, (9000,), generator=g))
    yield "a segment sorted in place", long.to(torch.int32), 7, 4  # more rows in one centre than the LDS sort holds
    two = torch.where(torch.arange(12345) % 3 == 1, torch.tensor(1), torch.tensor(4))  # 4 115 and 8 228 rows: both past the LDS sort,
    two[12340:] = torch.tensor([0, 5, 1, 4, 1])  # n no multiple of the 4 096-entry compaction step, its last entries mixed
    yield "two long segments", two.to(torch.int32), 6, 4
    yield "ragged", torch.randint(0, 40, (5000,), generator=g).to(torch.int32) ** 2 // 40, 40, 68


def check_group(idx, k):
    """counts, starts and the grouped rows against bincount, cumsum and a stable sort over the entries inside [0, k) -- the others
    are ignored; (counts, starts, rows) of the device and the CPU's counts."""
    from saev_amd.engine import kmeans_group

    counts, starts, rows = kmeans_group(idx.to(DEV), k)
    valid = torch.nonzero((idx >= 0) & (idx < k)).flatten()
    want_counts = torch.bincount(idx[valid].long(), minlength=k)
    assert torch.equal(counts.cpu().long(), want_counts)
    assert torch.equal(starts.cpu().long(), torch.cat([torch.zeros(1, dtype=torch.long), want_counts.cumsum(0)]))
    want_rows = valid[torch.sort(idx[valid].long(), stable=True).indices]
    assert torch.equal(rows.cpu().long()[:valid.numel()], want_rows), "ascending within each centre"
    assert torch.equal(rows[:valid.numel()], kmeans_group(idx.to(DEV), k)[2][:valid.numel()])
    return counts, starts, rows, want_counts


@pytest.mark.parametrize("name,idx,k,D", list(_index_cases()), ids=lambda v: v if isinstance(v, str) else None)
def test_group_and_update_against_a_one_thread_index_add(name, idx, k, D):
    check_group_and_update(name, idx, k, D)


def check_group_and_update(name, idx, k, D):
    from saev_amd.engine import kmeans_update

    n = idx.shape[0]
    g = torch.Generator().manual_seed(19 + k)
    X = torch.randn(n, D, generator=g) + 1
    centers = torch.randn(k, D, generator=g)
    prev = torch.randint(0, 4, (k,), generator=g).float() * torch.randint(1, 900, (k,), generator=g).float()  # zeros among them
    counts, starts, rows, want_counts = check_group(idx, k)
    valid = (idx >= 0) & (idx < k)  # (the rows of the others contribute nothing)

    empty = torch.nonzero(want_counts == 0).flatten()
    repl = torch.full((k,), -1, dtype=torch.int32)
    repl[empty[::2]] = torch.randint(0, n, (empty[::2].numel(),), generator=g).to(torch.int32)  # some empty centres, not all
    dist2 = torch.rand(n, generator=g)
    threads = torch.get_num_threads()
    torch.set_num_threads(1)  # index_add_ on the CPU: one thread, one order
    try:
        sums = torch.zeros(k, D).index_add_(0, idx[valid].long(), X[valid])
    finally:
        torch.set_num_threads(threads)
    batch = want_counts.float()
    took = repl >= 0
    sums[took] = X[repl[took].long()]
    batch[took] = 1.0
    tot = prev + batch
    m = batch > 0
    want_c = centers.clone()
    want_c[m] = (centers[m] * prev[m].unsqueeze(1) + sums[m]) / tot[m].unsqueeze(1)
    for use_repl in (True, False):
        c_dev, n_dev = centers.to(DEV), prev.to(DEV)
        inertia = kmeans_update(X.to(DEV), starts, rows, c_dev, n_dev, repl_rows=repl.to(DEV) if use_repl else None, dist2=dist2.to(DEV))
        if use_repl:
            assert torch.equal(c_dev.cpu(), want_c), name
            assert torch.equal(n_dev.cpu(), tot), name
        else:  # without replacements the empty centres stay as they are
            keep = want_counts > 0
            assert torch.equal(c_dev.cpu()[keep], want_c[keep]) and torch.equal(c_dev.cpu()[~keep], centers[~keep])
            assert torch.equal(n_dev.cpu(), prev + want_counts.float())
        assert abs(inertia.item() - dist2.double().mean().item()) <= 1e-12
        c2, n2 = centers.to(DEV), prev.to(DEV)
        again = kmeans_update(X.to(DEV), starts, rows, c2, n2, repl_rows=repl.to(DEV) if use_repl else None, dist2=dist2.to(DEV))
        assert torch.equal(c2, c_dev) and torch.equal(again.view(torch.int64), inertia.view(torch.int64))


_planted = K.planted


@pytest.mark.parametrize("k,D", K.COLLAPSED_SHAPES)
def test_collapsed_against_fp64(k, D):
    from saev_amd.engine import kmeans_collapsed

    tol_ = 0.5
    C, counts = _planted(k, D, tol_, 23 + k + D)
    want = torch.from_numpy(R.collapsed(C.numpy(), counts.numpy(), tol_))
    if k > 1:
        p2 = d2_64(C.to(DEV), C.to(DEV))[tuple(torch.triu_indices(k, k, 1).to(DEV))]
        gap = ((p2 - tol_ * tol_).abs() / torch.maximum(p2, torch.tensor(tol_ * tol_, device=DEV))).min().item()
        print(f"collapsed ({k}, {D}): smallest relative gap to tol^2 {gap:.3g} against 4 tol(D) = {4 * tol(D):.3g}")
        assert gap > 4 * tol(D), "the gap: fp64 decides every pair"
    if k >= 20:
        # (0,1) equal counts: 0; (2,k-1) and (8,15) beyond tol: none; (3,7) 9 > 2: 7; (4,9) 2 <= 9: 4; (5,11) at 0, equal: 5;
        # (6,13) at 0, 4 > 1: 13; (17,k-2) both 0: 17
        assert want.tolist()[:10] == [True, False, False, False, True, True, False, True, False, False]
        assert bool(want[13]) and not bool(want[11]) and bool(want[17]) and not bool(want[k - 2]) and not bool(want[k - 1])
        assert int(want.sum()) == 6
    auto = kmeans_collapsed(C.to(DEV), counts.to(DEV), tol_)
    exact = kmeans_collapsed(C.to(DEV), counts.to(DEV), tol_, route="exact")
    print(f"collapsed ({k}, {D}): route {auto.route}, overflow {auto.overflow}, candidates {auto.candidates} of {auto.capacity}")
    assert torch.equal(auto.losers.cpu(), want) and torch.equal(exact.losers.cpu(), want)
    assert auto.losers.dtype == torch.bool and exact.route == "exact"
    if k == 1:
        assert not auto.losers.any() and auto.route == "exact" and not auto.overflow
    else:
        check_filter(auto, R.collapsed_bracket(C.to(DEV), tol_), f"collapsed ({k}, {D})")


def test_collapsed_identical_centres_overflow():
    from saev_amd.engine import kmeans_collapsed

    C = torch.randn(1, 68, generator=torch.Generator().manual_seed(29)).repeat(300, 1).to(DEV)
    counts = torch.ones(300, device=DEV)
    auto, exact = kmeans_collapsed(C, counts, 0.5), kmeans_collapsed(C, counts, 0.5, route="exact")
    assert auto.overflow and auto.route == "exact" and auto.candidates > auto.capacity
    assert auto.losers.tolist() == [True] * 299 + [False] and torch.equal(auto.losers, exact.losers)
    with pytest.raises(ValueError, match="inf or a NaN"):
        bad = C.clone()
        bad[7, 3] = float("nan")
        kmeans_collapsed(bad, counts, 0.5)


def _g24(tag):
    with np.load(GOLDEN / f"g24_kmeans_{tag}.npz") as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("tag", ["clustered", "events"])
def test_trajectories_equal_the_references_bit_for_bit(tag, monkeypatch):
    from saev_amd import baselines

    g = _g24(tag)
    D = int(g["D"])
    draws = [(str(g["draw_kinds"][i]), torch.from_numpy(g[f"draw{i}"])) for i in range(int(g["n_draws"]))]

    def replay(fn, *args, **kwargs):
        kind, value = draws.pop(0)
        assert kind == fn, (kind, fn)
        if fn == "randint":
            assert args[2] == (value.numel(),), "as many replacement rows as the reference drew"
        return value.to(kwargs["device"])

    monkeypatch.setattr(baselines, "_draw", replay)
    model = baselines.MiniBatchKMeans(int(g["k"]), device=DEV, collapse_tol=float(g["collapse_tol"]))
    for t in range(int(g["n_steps"])):
        model.partial_fit(torch.from_numpy(g[f"batch{t}"]))
        assert torch.equal(model.cluster_centers_.cpu(), torch.from_numpy(g[f"centers{t}"])), (tag, t)
        assert torch.equal(model.cluster_counts_.cpu(), torch.from_numpy(g[f"counts{t}"])), (tag, t)
        want = float(g["inertia64"][t])
        print(f"{tag} step {t}: inertia {model.last_batch_inertia_!r} fp64 {want!r} reference {float(g['ref_inertia'][t])!r}, assign {model.last_assign_}")
        assert abs(model.last_batch_inertia_ - want) <= tol(D) * want + 1e-12
        assert abs(float(g["ref_inertia"][t]) - want) <= float(g["inertia_band"])
    assert not draws and model.n_steps_ == int(g["n_steps"]) and model.n_features_in_ == D


def test_partial_fit_leaves_the_state_alone_on_a_non_finite_batch():
    from saev_amd import baselines

    g = torch.Generator().manual_seed(31)
    model = baselines.MiniBatchKMeans(8, device=DEV)
    model.partial_fit(torch.randn(64, 16, generator=g))
    c, n = model.cluster_centers_.clone(), model.cluster_counts_.clone()
    model.partial_fit(torch.randn(64, 16, generator=g))  # (a second good step: no zero counts left, the one-read-back path)
    c, n, steps = model.cluster_centers_.clone(), model.cluster_counts_.clone(), model.n_steps_
    bad = torch.randn(64, 16, generator=g)
    bad[5, 5] = float("nan")
    with pytest.raises(ValueError, match="inf or a NaN"):
        model.partial_fit(bad)
    assert torch.equal(model.cluster_centers_, c) and torch.equal(model.cluster_counts_, n) and model.n_steps_ == steps


def test_partial_fit_commits_nothing_on_a_non_finite_first_batch():
    """The first batch seeds the centres; a NaN row among them must not become state.  k = n, so the bad row is certainly drawn."""
    from saev_amd import baselines

    g = torch.Generator().manual_seed(33)
    model = baselines.MiniBatchKMeans(64, device=DEV)
    bad = torch.randn(64, 16, generator=g)
    bad[5, 5] = float("nan")
    with pytest.raises(ValueError, match="inf or a NaN"):
        model.partial_fit(bad)
    assert model.cluster_centers_ is None and model.cluster_counts_ is None and model.n_features_in_ is None and model.n_steps_ == 0
    model.partial_fit(torch.randn(64, 20, generator=g))  # (another width is fine too: nothing was fitted)
    assert model.n_steps_ == 1 and model.n_features_in_ == 20 and bool(torch.isfinite(model.cluster_centers_).all())


def test_workers_train_then_infer(tmp_path):
    from saev_amd import baselines, data, disk

    rng = np.random.default_rng(37)
    k, D, T, n_ex = 32, 68, 12, 250
    points = 3 * rng.standard_normal((k, D))
    acts = (points[rng.integers(0, k, size=n_ex * T)] + 0.3 * rng.standard_normal((n_ex * T, D))).astype(np.float32)
    shards = data.write_shards(tmp_path, acts.reshape(n_ex, 1, T, D))
    runs_root = tmp_path / "saev" / "runs"
    runs_root.mkdir(parents=True)
    dcfg = data.ShuffledConfig(shards=shards, layer=0, batch_size=512, seed=5)
    cfg = baselines.TrainConfig(k=k, train_data=dcfg, val_data=dcfg, n_train=3000, n_val=1500, runs_root=runs_root, log_every=2, track=False)
    run = baselines.train_worker_fn(cfg)
    assert isinstance(run, disk.Run) and (run.run_dir / "checkpoint" / "baseline.pt").exists() and run.config["k"] == k
    model = baselines.load(run, device=DEV)
    assert model.cluster_centers_.shape == (k, D) and 5 <= model.n_steps_ <= 7 and float(model.cluster_counts_.sum()) > 0
    ev = baselines.eval_kmeans(cfg, model)
    assert set(ev) == {"eval/inertia", "eval/utilization", "eval/mean_pop", "eval/max_pop"}
    assert 0 < ev["eval/utilization"] <= 1 and abs(ev["eval/mean_pop"] * k - 1500) <= 512 and ev["eval/max_pop"] >= ev["eval/mean_pop"]

    icfg = baselines.InferenceConfig(run=run.run_dir, data=data.OrderedConfig(shards=shards, layer=0, batch_size=1000), n_dists=5)
    metrics = baselines.inference_worker_fn(icfg)
    root = run.inference / data.Metadata.load(shards).hash
    ta = scipy.sparse.load_npz(root / "token_acts.npz").tocsr()
    n = n_ex * T
    assert ta.shape == (n, k) and ta.nnz == n and np.array_equal(np.diff(ta.indptr), np.ones(n)), "exactly one entry per row"
    X, C = torch.from_numpy(acts).to(DEV), model.cluster_centers_
    d = d2_64(X, C)
    best, arg = d.min(dim=1)
    two = d.topk(2, dim=1, largest=False).values
    decided = ((two[:, 1] - two[:, 0]) > 4 * tol(D) * two[:, 1]).cpu().numpy()
    assert decided.mean() > 0.99
    cols = ta.indices.astype(np.int64)
    assert np.array_equal(cols[decided], arg.cpu().numpy()[decided])
    pair = d[torch.arange(n, device=DEV), torch.from_numpy(cols).to(DEV)]
    want_val = (1.0 / (1.0 + pair.sqrt())).cpu().numpy()
    # v = 1 / (1 + sqrt r): dv / v = (dr / r) s / (2 (1 + s)) <= tol(D) / 2 with s = sqrt r, and sqrtf, the addition and the division add
    # at most 3 x 2^-24 relative, so tol(D), relative, holds the values for every D >= 3
    verr = (np.abs(ta.data - want_val) / want_val).max()
    print(f"workers: values rel err {verr:.3g} (tol {tol(D):.3g})")
    assert verr <= tol(D)
    pop = np.bincount(cols, minlength=k)
    sparsity = torch.load(root / "sparsity.pt")
    assert sparsity.dtype == torch.float32 and np.abs(sparsity.double().numpy() - pop / n).max() <= 2.0 ** -24  # pop / n rounded once
    mv = torch.load(root / "mean_values.pt").numpy()
    want_mv = np.bincount(cols, weights=want_val, minlength=k) / np.maximum(pop, 1)
    # (a mean of positive values, each within tol(D) / 2 + 3 x 2^-24 relative, summed in fp64 and rounded to fp32 once)
    merr = (np.abs(mv[pop > 0] - want_mv[pop > 0]) / want_mv[pop > 0]).max()
    print(f"workers: mean_values rel err {merr:.3g} (tol {tol(D):.3g})")
    assert mv.dtype == np.float32 and merr <= tol(D) and np.isnan(mv[pop == 0]).all()
    dist = torch.load(root / "distributions.pt")
    assert dist.shape == (n, 5)
    got = json.loads((root / "metrics.json").read_text())
    sse = pair.sum().item()
    x64 = X.double()
    base = (x64 * x64).sum().item() - (x64.sum(dim=0) ** 2).sum().item() / n
    from saev_amd.metrics import Metrics

    want = Metrics.from_accumulators(sse_recon=sse, sse_baseline=base, n_tokens=n, d_model=D).to_dict()
    assert set(got) == set(want) and metrics is not None
    for key, value in want.items():  # every r_i is within tol(D) of the fp64 value of its pair, hence so is their sum and what follows from it
        print(f"workers: metrics {key} got {got[key]!r} want {value!r}")
        assert abs(got[key] - value) <= tol(D) * abs(value) + 1e-12, key

    stamp = {p.name: p.stat().st_mtime_ns for p in root.iterdir()}
    assert baselines.inference_worker_fn(icfg) is None, "a second call without force writes nothing"
    assert stamp == {p.name: p.stat().st_mtime_ns for p in root.iterdir()}
