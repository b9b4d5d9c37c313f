"""Host-side checks of the k-means baseline (include/saev_amd.h: K-MEANS; saev_amd/baselines.py) that need no GPU: the entries are
declared, exported and bound with the header's types and refuse bad arguments before touching a device; the numpy restatement
of the step's contract reproduces both G24 trajectories of the reference bit for bit; the reference's own checkpoint file loads
on the CPU and ``dump`` writes the same format; the configs take the reference's field names; PCA and Semi-NMF raise.

The last block runs the restated candidate rule of the fp16 filter (kmeans_restatement.filter_values / candidate_bracket) on the
CPU: its bound E holds against the refined value for every pair of every input family the GPU tests use, and those inputs
(kmeans_cases, same functions, same seeds) meet the conditions the GPU tests take for granted."""

import ctypes as C
import dataclasses
import io
import json
import re
import subprocess

import numpy as np
import pytest
import torch

import kmeans_cases as K
import kmeans_restatement as R
from conftest import GOLDEN, ROOT
from saev_amd import baselines, disk

ENTRIES = ("saev_kmeans_workspace_bytes", "saev_kmeans_assign", "saev_kmeans_group", "saev_kmeans_update", "saev_kmeans_collapsed")
CTYPES = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float}
INVALID = -1
FIXTURES = ("clustered", "events")


def _lib():
    subprocess.run(["make", "-C", str(ROOT)], check=True, capture_output=True)
    from saev_amd import _lib

    return _lib, _lib.load()


def test_entries_are_declared_exported_and_bound_with_the_headers_types():
    lib_mod, lib = _lib()
    raw = (ROOT / "include" / "saev_amd.h").read_text()
    assert re.search(r"/\* K-MEANS \(", raw), "the K-MEANS comment block"
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in ENTRIES:
        m = re.search(r"(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, f"{name} is not declared"
        args = [C.c_void_p if "*" in a else CTYPES[a.replace("const", "").split()[0]] for a in m.group(2).split(",")]
        want_res, want_args = lib_mod._SIGNATURES[name]
        assert want_res is CTYPES[m.group(1)], name
        assert list(want_args) == args, name
        assert hasattr(lib, name) and name in lib_mod.EXPORTED_SYMBOLS
    assert lib.saev_abi_version() == 12 and lib_mod.ABI_VERSION == 12  # additive entries: the version stays


def test_workspace_bytes_and_refusals_without_a_device():
    _, lib = _lib()
    ws = lib.saev_kmeans_workspace_bytes
    assert ws(1, 1, 4) > 0 and ws(2**20, 2**20, 4) > 0
    for bad in ((0, 1, 4), (1, 0, 4), (2**20 + 1, 1, 4), (1, 2**20 + 1, 4), (1, 1, 0), (1, 1, 6), (1, 1, 4100)):
        assert ws(*bad) == -1, bad
    # n = k = 16 384, D = 1 024: both centred fp32 copies and fp16 images, 128 x 16 384 doubles, the list -- never n x k floats
    big = ws(16384, 16384, 1024)
    assert 2 * 16384 * 1024 * 6 < big < 16384 * 16384 * 4 // 4
    assert ws(300, 4097, 256) % 256 == 0
    a = 4096  # a fake, aligned, non-null "pointer": every call below must be refused before it is used
    assert lib.saev_kmeans_assign(a, 8, a, 8, 6, 0, 0, a, 1 << 30, a, a, a, None) == INVALID      # D % 4
    assert lib.saev_kmeans_assign(a, 8, a, 8, 8, 0, 2, a, 1 << 30, a, a, a, None) == INVALID      # route
    assert lib.saev_kmeans_assign(a, 8, a, 8, 8, 0, 0, a, 16, a, a, a, None) == INVALID           # workspace too small
    assert lib.saev_kmeans_assign(a + 4, 8, a, 8, 8, 0, 0, a, 1 << 30, a, a, a, None) == INVALID  # alignment
    assert lib.saev_kmeans_assign(a, 8, None, 8, 8, 0, 0, a, 1 << 30, a, a, a, None) == INVALID   # null
    assert lib.saev_kmeans_group(None, 8, 8, a, a, a, None) == INVALID
    assert lib.saev_kmeans_group(a, 0, 8, a, a, a, None) == INVALID
    assert lib.saev_kmeans_update(a, 8, 6, 8, a, a, None, a, a, None, None, None) == INVALID
    assert lib.saev_kmeans_update(a, 8, 8, 8, a, a, None, None, a, None, None, None) == INVALID
    assert lib.saev_kmeans_collapsed(a, 8, 8, 0.5, a, 3, a, 1 << 30, a, a, None) == INVALID
    assert lib.saev_kmeans_collapsed(a, 8, 8, 0.5, a, 0, a, 16, a, a, None) == INVALID


def test_python_entries_refuse_bad_arguments():
    from saev_amd import engine

    x = torch.zeros(8, 8)
    with pytest.raises(ValueError, match="route"):
        engine.kmeans_assign(x, x, route="fast")
    with pytest.raises(ValueError, match="float32 device"):
        engine.kmeans_assign(x, x)
    with pytest.raises(ValueError, match="matrices"):
        engine.kmeans_assign(x[0], x)
    with pytest.raises(ValueError, match="int32 device"):
        engine.kmeans_group(torch.zeros(8, dtype=torch.int32), 4)
    with pytest.raises(RuntimeError, match="HIP device"):
        baselines.MiniBatchKMeans(4, device="cpu").partial_fit(x)


def _g24(tag):
    with np.load(GOLDEN / f"g24_kmeans_{tag}.npz") as z:
        return {k: z[k] for k in z.files}


def test_fixture_g24_holds_the_designs_the_tests_rely_on():
    c, e = _g24("clustered"), _g24("events")
    for g in (c, e):
        assert int(g["k"]) == 96 and int(g["D"]) == 68 and float(g["collapse_tol"]) == 0.5
        assert float(g["min_gap"]) >= 16 * R.tol(68)
        assert float(np.abs(g["ref_inertia"] - g["inertia64"]).max()) <= float(g["inertia_band"])
    assert [c[f"batch{t}"].shape[0] for t in range(6)] == [512] * 6
    assert not any(c[f"losers{t}"].any() or int(c[f"n_empty{t}"]) for t in range(6))
    assert list(c["draw_kinds"]) == ["randperm"]
    assert [e[f"batch{t}"].shape[0] for t in range(5)] == [64, 300, 512, 512, 512]
    assert int(e["losers0"].sum()) == 32 and int(e["n_empty0"]) == 32  # the duplicated centres: replaced, collapsed, re-seeded
    assert int(e["n_empty1"]) > 0 and all(k == "randint" for k in e["draw_kinds"])


@pytest.mark.parametrize("tag", FIXTURES)
def test_the_restatement_reproduces_g24_bit_for_bit(tag):
    g = _g24(tag)
    st = R.State(k=int(g["k"]), collapse_tol=float(g["collapse_tol"]))
    draws = [g[f"draw{i}"] for i in range(int(g["n_draws"]))]
    for t in range(int(g["n_steps"])):
        log = R.step(st, g[f"batch{t}"], draws)
        assert np.array_equal(st.centers, g[f"centers{t}"]), (tag, t)
        assert np.array_equal(st.counts, g[f"counts{t}"]), (tag, t)
        assert st.centers.dtype == np.float32 and st.counts.dtype == np.float32
        assert np.array_equal(log.assign, g[f"assign{t}"]) and np.array_equal(log.losers, g[f"losers{t}"])
        assert log.inertia64 == float(g["inertia64"][t]) and log.n_empty == int(g[f"n_empty{t}"])
    assert not draws, "every recorded draw is consumed"


def test_the_refined_value_restated_meets_its_tolerance():
    rng = np.random.default_rng(0)
    X, Cn = rng.standard_normal((37, 68)).astype(np.float32) + 3, rng.standard_normal((29, 68)).astype(np.float32) + 3
    r, d = R.r_fp32(X, Cn).astype(np.float64), R.dist2_64(X, Cn)
    assert r.dtype == np.float64 and float((np.abs(r - d) / d).max()) <= R.tol(68)


def _fake_run(tmp_path):
    return disk.Run.new("r0", train_shards_dir=tmp_path, val_shards_dir=tmp_path, runs_root=tmp_path / "saev" / "runs")


def test_load_reads_the_references_file_and_dump_writes_its_format(tmp_path):
    g = _g24("clustered")
    run = _fake_run(tmp_path)
    ckpt = run.ckpt.parent / "baseline.pt"
    ckpt.write_bytes((GOLDEN / "g24_kmeans_baseline.pt").read_bytes())
    model = baselines.load(run, device="cpu")
    assert isinstance(model, baselines.MiniBatchKMeans) and model.k == 96 and model.n_features_in_ == 68 and model.n_steps_ == 6
    assert torch.equal(model.cluster_centers_, torch.from_numpy(g["centers5"])) and model.cluster_centers_.dtype == torch.float32
    assert torch.equal(model.cluster_counts_, torch.from_numpy(g["counts5"])) and model.collapse_tol == 0.5
    x = torch.from_numpy(g["batch0"][:7])
    assert torch.equal(model.transform(x), -torch.cdist(x, model.cluster_centers_))

    with open(ckpt, "rb") as fd:  # what the reference wrote: the yardstick for dump below
        ref_header = json.loads(fd.readline())
        ref_state = torch.load(io.BytesIO(fd.read()), weights_only=False)
    cfg = baselines.TrainConfig(k=96, device="cpu", runs_root=tmp_path)
    path = baselines.dump(run, cfg, model)
    assert path == ckpt
    with open(path, "rb") as fd:
        header = json.loads(fd.readline())
        state = torch.load(io.BytesIO(fd.read()), weights_only=False)
    assert set(header) == set(ref_header) == {"method", "schema", "commit", "lib"} and header["method"] == "kmeans" and header["schema"] == 1
    assert list(state) == list(ref_state) == ["cluster_centers", "cluster_counts", "n_steps", "n_features_in", "collapse_tol"]
    for key, want in ref_state.items():
        got = state[key]
        assert type(got) is type(want), key
        if isinstance(want, torch.Tensor):
            assert got.dtype == want.dtype and got.device.type == "cpu" and torch.equal(got, want), key
        else:
            assert got == want, key
    assert json.loads((ckpt.parent / "config.json").read_text())["k"] == 96
    again = baselines.load(run)
    assert torch.equal(again.cluster_centers_, model.cluster_centers_) and again.n_steps_ == 6


def test_the_configs_take_the_references_field_names():
    train = ["method", "train_data", "val_data", "n_train", "n_val", "k", "collapse_tol", "z_iters", "encode_iters", "ridge", "eps",
             "forget_factor", "d_update_every", "device", "seed", "runs_root", "slurm_acct", "slurm_partition", "n_hours", "mem_gb", "log_to",
             "debug", "track", "wandb_project", "tag", "log_every"]
    infer = ["run", "data", "device", "seed", "n_dists", "n_iters", "save", "force", "slurm_acct", "slurm_partition", "n_hours", "mem_gb",
             "log_to"]
    assert [f.name for f in dataclasses.fields(baselines.TrainConfig)] == train
    assert [f.name for f in dataclasses.fields(baselines.InferenceConfig)] == infer
    cfg = baselines.TrainConfig()
    assert cfg.method == "kmeans" and cfg.k == 16384 and cfg.collapse_tol == 0.5 and cfg.log_every == 50 and cfg.n_val == 10_000_000
    assert baselines.InferenceConfig().n_dists == 25 and baselines.InferenceConfig().force is False


@pytest.mark.parametrize("method", ["pca", "semi-nmf"])
def test_the_other_methods_are_not_built(method, tmp_path):
    with pytest.raises(NotImplementedError, match=method):
        baselines.train_worker_fn(baselines.TrainConfig(method=method, runs_root=tmp_path))
    run = _fake_run(tmp_path)
    (run.ckpt.parent / "baseline.pt").write_bytes(json.dumps({"method": method, "schema": 1, "commit": "x", "lib": "x"}).encode() + b"\n")
    with pytest.raises(NotImplementedError, match=method):
        baselines.load(run)


def test_draw_is_the_one_source_of_randomness(monkeypatch):
    seen = []
    monkeypatch.setattr(baselines, "_draw", lambda fn, *a, **k: seen.append((fn, a)) or torch.arange(a[0]))
    m = baselines.MiniBatchKMeans(3, device="cpu")
    centers, counts = m._initial_centers(torch.arange(20.0).reshape(5, 4))
    assert seen == [("randperm", (5,))] and torch.equal(centers, torch.arange(12.0).reshape(3, 4)) and torch.equal(counts, torch.zeros(3))
    centers, _ = m._initial_centers(torch.arange(8.0).reshape(2, 4))  # fewer rows than k: repeated, no draw
    assert len(seen) == 1 and torch.equal(centers[2], centers[0])
    assert m.cluster_centers_ is None and m.n_features_in_ is None, "seeding alone commits nothing"


# ---- the restated candidate rule ------------------------------------------------------------------------------
def _slices(make, n, k, scale=1.0):
    X, C = make()
    return X[:n] * scale, C[:k] * scale


def _collapsed_pair(k, D):
    C = K.collapsed_case(k, D)[0]
    return C, C


# every input family of the GPU tests at a few hundred rows (slices of the same tensors where the function has one size)
BOUND_FAMILIES = {
    "gaussian D=68": lambda: K.gaussian(129, 37, 68),
    "gaussian D=128": lambda: K.gaussian(257, 300, 128),
    "gaussian D=4096": lambda: K.gaussian(60, 50, 4096),
    "grid D=16": lambda: K.gaussian(300, 300, 16),
    "far from the origin": lambda: K.far_from_the_origin(400, 100),
    "identical centres": K.identical_centres,
    "three centres": lambda: K.three_centres(3000),
    "many centres": lambda: K.many_centres(5000),
    "tied tiles": lambda: (K.tied_tiles()[0], K.tied_tiles()[1][350:650]),
    "mixed norms 10^U(-1, 1)": lambda: _slices(lambda: K.mixed_norms(1), 300, 400),
    "mixed norms 10^U(-3, 3)": lambda: _slices(lambda: K.mixed_norms(3), 300, 400),
    "scaled by 2^-40": lambda: _slices(lambda: K.gaussian(*K.SCALED_SHAPE), 200, 300, K.SCALES[0]),
    "scaled by 2^50": lambda: _slices(lambda: K.gaussian(*K.SCALED_SHAPE), 200, 300, K.SCALES[1]),
    "no image: a row of X": K.no_image_row_of_x,
    "no image: a centre": K.no_image_centre,
    "collapsed (129, 16)": lambda: _collapsed_pair(129, 16),
    "collapsed (129, 68)": lambda: _collapsed_pair(129, 68),
}


def _bound_ratio(X, C):
    """max |s~ - r| / E over the pairs whose rows both have a unit image, r the refined value bit for bit."""
    st, E = R.filter_values(X, C)
    r = torch.from_numpy(R.r_fp32(X.numpy(), C.numpy())).double()
    mu = R.centring_vector(C)
    live = R.filter_rows(X, mu).has_image[:, None] & R.filter_rows(C, mu).has_image[None, :]
    assert bool(torch.isfinite(E[live]).all()) and bool((E[live] > 0).all())
    return ((st - r).abs() / E)[live].max().item(), int(live.sum())


@pytest.mark.parametrize("name", list(BOUND_FAMILIES))
def test_the_restated_bound_holds_against_the_refined_value(name):
    ratio, pairs = _bound_ratio(*BOUND_FAMILIES[name]())
    print(f"{name}: max |s~ - r| / E = {ratio:.3f} over {pairs} pairs")
    assert ratio <= 1.0


def test_the_bound_test_fails_with_a_quarter_of_E():
    """The sensitivity of the test above: with E divided by 4 it fails on Gaussian rows at D = 68 (largest ratio 0.26), and at D = 4
    with E divided by 1.2 (0.88: few columns leave the Cauchy-Schwarz step of the bound little slack), so a constant of the bound that
    is too small by such a factor cannot hide in it."""
    assert 0.25 < _bound_ratio(*K.gaussian(129, 37, 68))[0] <= 1.0
    assert 1 / 1.2 < _bound_ratio(*K.three_centres(3000))[0] <= 1.0


def _scaled(s):
    X, C = K.gaussian(*K.SCALED_SHAPE)
    return X * s, C * s


# every GPU assign test that asserts route == "filter" (in both directions): the same function, the same seed
FILTER_CASES = {f"gaussian ({n}, {k}, {D})": (lambda n=n, k=k, D=D: K.gaussian(n, k, D)) for n, k, D in K.ASSIGN_SHAPES if k > 1}
FILTER_CASES.update({
    "far from the origin": K.far_from_the_origin,
    "grid": lambda: K.gaussian(*K.GRID),
    "many centres": K.many_centres,
    "tied tiles": K.tied_tiles,
    "mixed norms 10^U(-1, 1)": lambda: K.mixed_norms(1),
    "scaled by 2^-40": lambda: _scaled(K.SCALES[0]),
    "scaled by 2^50": lambda: _scaled(K.SCALES[1]),
})


@pytest.mark.parametrize("name", list(FILTER_CASES))
def test_the_filter_can_answer_the_inputs_the_gpu_tests_expect_it_to(name):
    X, C = FILTER_CASES[name]()
    n, cap = X.shape[0], K.assign_capacity(X.shape[0], C.shape[0])
    for farthest, (sure, maybe) in R.candidate_brackets(X, C).items():
        print(f"{name} farthest={farthest}: sure {sure} maybe {maybe} ({maybe / n:.3f} per row) of {cap}")
        assert n <= sure <= maybe <= cap // 2
        if name == "tied tiles":
            assert sure >= 2 * n, "every optimum and its exact copy"


def test_the_largest_n_case_meets_its_conditions():
    """n = 2^20 from a 2^17-row sample of the same distribution: the candidates per row stay below half the capacity per row
    (capacity = n k = 3 n here), and the whole input has more candidates than the refinement has threads."""
    X, C = K.three_centres(2 ** 17)
    for farthest, (sure, maybe) in R.candidate_brackets(X, C).items():
        print(f"three centres, 2^17 rows, farthest={farthest}: sure {sure} maybe {maybe} ({maybe / 2 ** 17:.4f} per row)")
        assert 2 ** 17 <= sure <= maybe and 8 * maybe <= K.assign_capacity(2 ** 20, 3) // 2
    r = R.r_fp32(X[:2000].numpy(), C.numpy())
    assert np.array_equal(r[:, 0], r[:, 1]), "the first 2 000 rows tie centres 0 and 1 bit for bit"
    sure = R.candidate_bracket(X[:2000], C, False)[0]
    assert sure >= 2000 + int((r[:, 0] <= r[:, 2]).sum())
    # every row keeps its optimum, the tied rows whose optimum is the tie keep both: 2^20 + these > 4 096 x 256 threads
    assert 2 ** 20 + int((r[:, 0] <= r[:, 2]).sum()) > 4096 * 256
    assert bool((X.abs() < 8).all())


@pytest.mark.parametrize("k,D", [kd for kd in K.COLLAPSED_SHAPES if kd[0] > 1] + [K.GRID[1:]])
def test_the_collapsed_filter_can_answer_the_planted_centres(k, D):
    C, _ = K.collapsed_case(k, D)
    sure, maybe = R.collapsed_bracket(C, K.COLLAPSED_TOL)
    print(f"collapsed ({k}, {D}): sure {sure} maybe {maybe} of {K.collapsed_capacity(k)}")
    assert 6 <= sure <= maybe <= K.collapsed_capacity(k) // 2  # (the six planted pairs below tol are candidates)


def test_the_overflow_cases_overflow_by_count_and_the_no_image_cases_by_a_zero_row():
    X, C = K.identical_centres()
    assert R.candidate_bracket(X, C, False)[0] > K.assign_capacity(65, 65)
    C300 = torch.randn(1, 68, generator=torch.Generator().manual_seed(29)).repeat(300, 1)
    assert R.collapsed_bracket(C300, 0.5)[0] > K.collapsed_capacity(300)
    assert R.candidate_bracket(*K.mixed_norms(3), False)[0] > K.assign_capacity(1000, 3000)

    X, C = K.no_image_row_of_x()
    mu = R.centring_vector(C)
    x, c = R.filter_rows(X, mu), R.filter_rows(C, mu)
    assert torch.equal(mu.double(), C.double().mean(dim=0)) and bool(c.has_image.all())
    assert (~x.has_image).nonzero().flatten().tolist() == [K.NO_IMAGE_ROW] and bool((X[K.NO_IMAGE_ROW] == mu).all())
    X, C = K.no_image_centre()
    mu = R.centring_vector(C)
    x, c = R.filter_rows(X, mu), R.filter_rows(C, mu)
    assert torch.equal(mu, C[64]) and bool(x.has_image.all()) and (~c.has_image).nonzero().flatten().tolist() == [64]


def test_group_edges_has_the_segments_it_names():
    idx, k = K.group_edges()
    valid = (idx >= 0) & (idx < k)
    assert torch.bincount(idx[valid].long(), minlength=k).tolist() == [4096, 4097, 2, 1, 0]
    assert idx.numel() % 4096 != 0 and int((~valid).sum()) == 300 and {-1, k, 2 ** 31 - 1} <= set(idx[~valid].tolist())
    assert idx[:64].unique().numel() > 1, "interleaved"
