"""Host-side checks of the k-means baseline (include/saev_amd.h: K-MEANS; saev_amd/baselines.py) that need no GPU: the entries are
declared, exported and bound with the header's types and refuse bad arguments before touching a device; the numpy restatement
of the step's contract reproduces both G24 trajectories of the reference bit for bit; the reference's own checkpoint file loads
on the CPU and ``dump`` writes the same format; the configs take the reference's field names; PCA and Semi-NMF raise."""

import ctypes as C
import dataclasses
import io
import json
import re
import subprocess

import numpy as np
import pytest
import torch

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
