"""GPU tests of the latent operating points (include/saev_amd.h: LATENT OPERATING POINTS) against the numpy restatement
(tests/latent_operating_restatement.py, itself held against the subset definition and ``sklearn.metrics.roc_curve`` by
tests/test_latent_operating_host_cpu.py) on the designs of tests/latent_operating_cases.py.

What is asserted, and there is no tolerance anywhere: the confusion counts, ``j2``, ``n_pos``, ``n_neg`` and the class counts ON THE
INTEGERS; ``f1``, ``youden`` and both thresholds ON THE BITS, NaN exactly where the contract says (``f1`` when n_pos = 0, ``youden``
when n_pos n_neg = 0)."""

import ctypes as C
import importlib.util

import numpy as np
import pytest
import scipy.sparse
import torch

import latent_auroc_cases as AK
import latent_operating_cases as OK
import latent_operating_restatement as OR
from conftest import GOLDEN, ROOT

pytestmark = [pytest.mark.gpu, pytest.mark.encoder_modes("f32")]
DEV = "cuda"
PAIRS = OR.PAIRS_F64 + OR.PAIRS_F32 + OR.PAIRS_INT
KEYS = PAIRS + ("n_pos", "n_neg", "class_counts")


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _args(d, labels=None, remap=None, roles=None):
    return ((_dev(d["indptr"]), _dev(d["indices"]), _dev(d["data"]), d["n"], d["s"], d["c"]),
            dict(labels=_dev(d["cls"] if labels is None else labels), remap=None if remap is None else _dev(remap), roles=_dev(d["roles"] if roles is None else roles)))


def _run(d, *, reuse=None, **kw):
    from saev_amd import engine

    args, kwargs = _args(d, **kw)
    return engine.latent_operating(*args, **kwargs, reuse=reuse)


def _host(res):
    return {k: getattr(res, k).cpu().numpy() for k in KEYS}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same(a, b, keys=KEYS):
    return all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in keys)


def _restate(d):
    return OR.operating(d["indptr"], d["indices"], d["data"], d["n"], d["s"], d["cls"], d["roles"])


def _check(got, want, name=""):
    for key in OR.PAIRS_INT + ("n_pos", "n_neg"):
        np.testing.assert_array_equal(got[key], want[key], err_msg=f"{name}: {key}")
    np.testing.assert_array_equal(got["class_counts"], want["pos"])
    for key in OR.PAIRS_F32 + OR.PAIRS_F64:
        assert got[key].dtype == want[key].dtype and np.array_equal(np.isnan(got[key]), np.isnan(want[key])), f"{name}: {key} NaN"
        ok = ~np.isnan(want[key])
        assert np.array_equal(_bits(got[key])[ok], _bits(want[key])[ok]), f"{name}: {key}"
    nan_bits = np.uint64(0x7ff8000000000000)
    assert (_bits(got["f1"])[:, want["n_pos"] == 0] == nan_bits).all() and not np.isnan(got["f1"][:, want["n_pos"] > 0]).any()
    void = (want["n_pos"] == 0) | (want["n_neg"] == 0)
    assert (_bits(got["youden"])[:, void] == nan_bits).all() and not np.isnan(got["youden"][:, ~void]).any()
    assert not np.isnan(got["f1_thr"]).any() and not np.isnan(got["j_thr"]).any() and (got["j2"] >= 0).all()


@pytest.fixture(scope="module")
def restated():
    """The restatement of every small design, computed once and left unchanged."""
    out = {}
    for name, make in OK.SMALL.items():
        d = make()
        out[name] = (d, _restate(d))
    return out


@pytest.mark.parametrize("name", list(OK.SMALL))
def test_small_designs_against_the_restatement(restated, name):
    d, want = restated[name]
    _check(_host(_run(d)), want, name)


@pytest.mark.parametrize("name", list(OK.LARGE))
def test_large_designs_against_the_restatement(name):
    d = OK.LARGE[name]()
    _check(_host(_run(d)), _restate(d), name)


def test_the_sorts_second_trip_and_long_latents():
    """The ``past_cap`` design of the analysis tests (70 000 rows, 2.24 M entries, every latent tens of thousands of events in a few
    dozen tie groups, every third latent signed) with three tasks."""
    import analysis_scale_cases as A

    d = dict(A.past_cap(), roles=AK.PAST_CAP_ROLES)
    _check(_host(_run(d)), _restate(d), "past_cap")


def test_both_label_forms_and_two_calls_give_the_same_bits(restated):
    for name in ("kinds", "grid_5x11x130", "planted"):
        d, want = restated[name]
        labels, remap = AK.as_bytes(d)
        got = _host(_run(d, labels=labels, remap=remap))
        _check(got, want, name)
        assert _same(got, _host(_run(d, labels=d["cls"].astype(np.int64)))) and _same(got, _host(_run(d))) and _same(got, _host(_run(d)))


def test_a_task_alone_and_a_latent_alone_give_the_bits_they_have_among_others(restated):
    for name, tasks, latents in (("kinds", (0, 2, 4, 5), (6, 7, 10, 11)), ("grid_5x300x65", (0, 63, 64), (1, 2)), ("chunks", (1,), (0, 4)),
                                 ("planted", (0, 1), (1, 2, 9))):
        d, _ = restated[name]
        full = _host(_run(d))
        for t in tasks:
            alone = _host(_run(d, roles=d["roles"][t:t + 1]))
            assert all(np.array_equal(_bits(alone[k][:, 0]), _bits(full[k][:, t])) for k in PAIRS), (name, t)
            assert alone["n_pos"][0] == full["n_pos"][t] and alone["n_neg"][0] == full["n_neg"][t]
        for j in latents:
            alone = _host(_run(AK.one_latent(d, j)))
            assert all(np.array_equal(_bits(alone[k][0]), _bits(full[k][j])) for k in PAIRS), (name, j)


def test_a_shuffled_row_order_gives_the_same_outputs(restated):
    for name in ("kinds", "chunks", "grid_5x11x130"):
        d, want = restated[name]
        perm = np.random.default_rng(3).permutation(d["n"])  # new row i is old row perm[i]
        csr = scipy.sparse.csr_matrix((d["data"], d["indices"], d["indptr"]), shape=(d["n"], d["s"]))[perm]
        csr.sort_indices()
        moved = dict(d, indptr=csr.indptr.astype(np.int64), indices=csr.indices.astype(np.int32), data=csr.data.astype(np.float32), cls=d["cls"][perm])
        assert len(moved["data"]) == len(d["data"])
        _check(_host(_run(moved)), want, name + " shuffled")


def test_reuse_after_either_entry_equals_a_fresh_call_and_leaves_the_auroc_outputs_alone(restated):
    from saev_amd import engine

    au_keys = ("auroc", "u2", "n_pos", "n_neg", "fire_pos", "fire_neg", "sum_pos", "sum_neg", "class_counts")
    for name in ("kinds", "chunks", "grid_5x300x65", "grid_1x4096x130", "planted"):
        d, want = restated[name]
        args, kwargs = _args(d)
        fresh = _host(_run(d))
        ranked = engine.latent_auroc(*args, **kwargs)
        before = {k: getattr(ranked, k).clone() for k in au_keys}
        ws_before = ranked._ws.clone()
        after_auroc = engine.latent_operating(*args, **kwargs, reuse=ranked)
        assert after_auroc._ws is ranked._ws and after_auroc.n_pos is ranked.n_pos
        got = _host(after_auroc)
        _check(got, want, name + " reused")
        assert _same(got, fresh)
        again = engine.latent_operating(*args, **kwargs, reuse=after_auroc)
        assert _same(_host(again), fresh) and _same(_host(engine.latent_operating(*args, **kwargs, reuse=_run(d))), fresh)
        assert all(torch.equal(before[k].view(torch.int64), getattr(ranked, k).view(torch.int64)) for k in au_keys)
        assert torch.equal(ws_before, ranked._ws)  # the sorted events, the role table and the error word: nothing is written
    d, _ = restated["kinds"]
    with pytest.raises(ValueError, match="the result to reuse has"):
        _run(d, reuse=_run(d, roles=d["roles"][:3]))


def test_derived_rates(restated):
    d, want = restated["kinds"]
    res = _run(d)
    with np.errstate(divide="ignore", invalid="ignore"):
        tp, fp, jtp, jfp = (want[k].astype(np.float64) for k in ("f1_tp", "f1_fp", "j_tp", "j_fp"))
        n_pos, n_neg = want["n_pos"][None, :].astype(np.float64), want["n_neg"][None, :].astype(np.float64)
        for key, value in (("precision_f1", tp / (tp + fp)), ("recall_f1", tp / n_pos), ("tpr_j", jtp / n_pos), ("fpr_j", jfp / n_neg)):
            got = getattr(res, key)
            assert got.is_cuda and got.dtype == torch.float64
            assert np.array_equal(got.cpu().numpy(), np.broadcast_to(value, tp.shape), equal_nan=True), key


@pytest.mark.parametrize("what, message", [("role", "a role byte is above 2"), ("class", "a class id lies outside"), ("latent", "a column index lies outside")])
def test_the_error_word(restated, what, message):
    d, _ = restated["grid_5x11x130"]
    d = dict(d)
    if what == "role":
        d["roles"] = d["roles"].copy()
        d["roles"][129, 10] = 3
    elif what == "class":
        d["cls"] = d["cls"].copy()
        d["cls"][17] = d["c"]
    else:
        d["indices"] = d["indices"].copy()
        d["indices"][5] = d["s"]
    res = _run(d)
    with pytest.raises(ValueError, match=message):
        res.f1
    with pytest.raises(ValueError, match=message):
        res.check()
    with pytest.raises(ValueError, match=message):  # the word stays what the first call left
        _run(d, reuse=res).j_thr


def test_the_c_entry_with_an_exact_workspace_and_poisoned_outputs(restated):
    from saev_amd import _lib

    lib = _lib.load()
    for name in ("kinds", "grid_5x300x65"):
        d, want = restated[name]
        n, s, c, t, nnz = d["n"], d["s"], d["c"], d["roles"].shape[0], len(d["data"])
        need = lib.saev_latent_operating_workspace_bytes(n, s, c, t, nnz)
        guard = 4096
        ws = torch.full((need + guard,), 0xA5, device=DEV, dtype=torch.uint8)
        assert ws.data_ptr() % 256 == 0
        dtypes = dict(f1=torch.float64, youden=torch.float64, f1_thr=torch.float32, j_thr=torch.float32)
        out = {k: torch.full((s, t), -7, device=DEV, dtype=dtypes.get(k, torch.int64)) for k in ("f1", "f1_thr", "f1_tp", "f1_fp", "j2", "youden", "j_thr", "j_tp", "j_fp")}
        counts = dict(n_pos=torch.full((t,), -7, device=DEV, dtype=torch.int64), n_neg=torch.full((t,), -7, device=DEV, dtype=torch.int64),
                      pos=torch.full((c,), -7, device=DEV, dtype=torch.int64))
        x = [_dev(d["indptr"]), _dev(d["indices"]), _dev(d["data"])]
        cls, roles = _dev(d["cls"]), _dev(d["roles"])
        ptr = lambda v: C.c_void_p(v.data_ptr())  # noqa: E731

        def call(flags):
            rc = lib.saev_latent_operating(*map(ptr, x), nnz, n, s, c, None, None, ptr(cls), ptr(roles), t, flags, *map(ptr, out.values()), *map(ptr, counts.values()),
                                           ptr(ws), need, C.c_void_p(torch.cuda.current_stream().cuda_stream))
            assert rc == 0, lib.saev_last_error(None)
            torch.cuda.synchronize()
            got = {k: v.cpu().numpy() for k, v in out.items()}
            got.update(n_pos=counts["n_pos"].cpu().numpy(), n_neg=counts["n_neg"].cpu().numpy(), class_counts=counts["pos"].cpu().numpy())
            return got

        first = call(0)
        _check(first, want, name + " through the C entry")
        assert (ws[need:] == 0xA5).all() and int(ws[:4].view(torch.int32).item()) == 0
        kept = ws.clone()
        for v in out.values():
            v.fill_(-7)
        assert _same(call(_lib.OPERATING_SORTED), first) and torch.equal(ws, kept)


# ---------------------------------------------------------------- the Python modules -----------------------------------------------------

@pytest.mark.parametrize("as_negative", [False, True])
def test_latent_operating_matrix_against_the_restatement(as_negative):
    from saev_amd import classification as cl

    rng = np.random.default_rng(9)
    n, s = 400, 12
    labels = rng.choice(np.array([0, 2, 3, 7, 255], dtype=np.uint8), size=n)
    x = scipy.sparse.random(n, s, density=0.3, format="csr", dtype=np.float32, random_state=3)
    x.data = (np.ceil(x.data * 8) / 8 * rng.choice([-1.0, 1.0], size=x.nnz, p=[0.2, 0.8])).astype(np.float32)
    points, classes, n_pos, n_neg = cl.latent_operating_matrix(x, labels, ignore_label_ids=(0, 255), ignored_as_negative=as_negative)
    assert classes.tolist() == [2, 3, 7] and points["f1"].shape == (s, 3)
    cls = np.select([labels == 2, labels == 3, labels == 7], [0, 1, 2], default=3 if as_negative else -1).astype(np.int32)
    roles = np.ones((3, 4 if as_negative else 3), dtype=np.uint8)
    roles[np.arange(3), np.arange(3)] = 2
    want = OR.operating(x.indptr, x.indices, x.data, n, s, cls, roles)
    _check(dict(points, n_pos=n_pos, n_neg=n_neg, class_counts=want["pos"]), want, "matrix")
    with np.errstate(divide="ignore", invalid="ignore"):
        assert np.array_equal(points["precision_f1"], want["f1_tp"] / (want["f1_tp"] + want["f1_fp"]).astype(np.float64), equal_nan=True)
        assert np.array_equal(points["fpr_j"], want["j_fp"] / want["n_neg"][None, :].astype(np.float64), equal_nan=True)


def _tool():
    spec = importlib.util.spec_from_file_location("latent_thresholds_tool", ROOT / "tools" / "latent_thresholds.py")
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def test_worker_fn_and_the_tool_at_image_level(tmp_path, capsys):
    from saev_amd import mimics, operating

    with np.load(GOLDEN / "g29_latent_auroc.npz") as z:
        d = AK.g29_designs({k: z[k] for k in z.files})[0]
    run_root, shards = AK.g29_run(tmp_path, d)
    cfg = operating.Config(run_root_dpath=run_root, shards_dpath=shards, run_ids=["mimic001"], level="image", pair_specs=d["pair_specs"], views=d["views"],
                           min_samples=d["min_samples"])
    operating.worker_fn(cfg)
    fpath = operating.operating_fpath(run_root, run_id="mimic001", shard_id=shards.name)
    assert fpath == run_root / "mimic001" / "inference" / shards.name / "latent_operating.npz" and not (fpath.parent / mimics.NPZ_FNAME).exists()
    specs = mimics.build_task_specs(d["sv"], pair_specs=d["pair_specs"], views=d["views"], min_samples=d["min_samples"])
    cls, roles = mimics.task_classes(specs, d["n_images"])
    p = scipy.sparse.csr_matrix(d["pooled"])
    want = OR.operating(p.indptr, p.indices, p.data, d["n_images"], d["s"], cls, roles)
    with np.load(fpath) as z:
        got = {k: z[k] for k in z.files}
    assert tuple(got) == operating.KEYS and str(got["level"]) == "image" and got["task"].tolist() == [s.name for s in specs]
    _check({**{k: got[k].T for k in PAIRS}, "n_pos": got["n_pos"], "n_neg": got["n_neg"], "class_counts": want["pos"]}, want, "image level")
    assert np.array_equal(got["auroc"].astype(np.float32).reshape(-1).view(np.uint32), d["col_auroc"].view(np.uint32))  # the reference's AUROC, beside it
    # the thresholds do to the pooled codes what the file says
    for t in range(len(specs)):
        thr = operating.thresholds(fpath, specs[t].name, "f1")
        fires = d["pooled"][specs[t].include] > thr[None, :]
        ok = np.isfinite(got["f1_thr"][t]) | (got["f1_tp"][t] + got["f1_fp"][t] == 0)
        assert np.array_equal(fires[specs[t].melp_mask].sum(axis=0)[ok], got["f1_tp"][t][ok]) and np.array_equal(fires[specs[t].erato_mask].sum(axis=0)[ok], got["f1_fp"][t][ok])
    # the cache is honoured; a file of the other level is not
    marked = dict(got, f1=np.full_like(got["f1"], 0.25))
    np.savez(fpath, **marked)
    assert (operating.score_run("mimic001", cfg)["f1"] == 0.25).all()
    tool = _tool()
    out = tool.main(["--run", str(run_root / "mimic001"), "--shards", str(shards), "--level", "image", "--force", "--min-samples", str(d["min_samples"]),
                     "--pairs", *[f"{e}:{m}" for e, m in d["pair_specs"]], "--views", *d["views"]])
    text = capsys.readouterr().out
    assert out["level"] == "image" and list(out["tasks"]) == [s.name for s in specs] and out["n_latents"] == d["s"] and "predict nothing" in text
    first = out["tasks"][specs[0].name]
    assert len(first["f1_quantiles"]) == 7 and len(first["best_by_f1"]) == min(10, d["s"]) and first["n_pos"] == specs[0].n_pos
    best = first["best_by_f1"][0]
    assert best[1] == np.nanmax(want["f1"][:, 0]) and best[2] == want["f1_thr"][best[0], 0]
    out = tool.main(["--run", str(run_root / "mimic001"), "--shards", str(shards), "--level", "image", "--latent", "3", "--min-samples", str(d["min_samples"]),
                     "--pairs", *[f"{e}:{m}" for e, m in d["pair_specs"]], "--views", *d["views"]])
    assert out["latent"] == 3 and out["tasks"][specs[1].name]["f1"] == want["f1"][3, 1] and specs[1].name in capsys.readouterr().out


def test_worker_fn_at_token_level(tmp_path):
    from saev_amd import operating
    from saev_amd.data import write_shards

    rng = np.random.default_rng(4)
    n_img, tpi, s = 12, 9, 10
    labels = rng.choice(np.array([0, 1, 4, 9], dtype=np.uint8), size=(n_img, tpi))
    shards = write_shards(tmp_path / "shards", np.zeros((n_img, 1, tpi, 4), dtype=np.float32), labels=labels)
    x = scipy.sparse.random(n_img * tpi, s, density=0.35, format="csr", dtype=np.float32, random_state=5)
    x.data = (np.ceil(x.data * 4) / 4).astype(np.float32)
    inference = tmp_path / "runs" / "tok001" / "inference" / shards.name
    inference.mkdir(parents=True)
    scipy.sparse.save_npz(inference / "token_acts.npz", x)
    cfg = operating.Config(run_root_dpath=tmp_path / "runs", shards_dpath=shards, run_ids=["tok001"], level="token", ignore_label_ids=(0,))
    operating.worker_fn(cfg)
    with np.load(inference / "latent_operating.npz") as z:
        got = {k: z[k] for k in z.files}
    assert tuple(got) == operating.KEYS and str(got["level"]) == "token" and got["task"].tolist() == ["label_1", "label_4", "label_9"]
    flat = labels.reshape(-1)
    cls = np.select([flat == 1, flat == 4, flat == 9], [0, 1, 2], default=-1).astype(np.int32)
    roles = np.ones((3, 3), dtype=np.uint8)
    roles[np.arange(3), np.arange(3)] = 2
    want = OR.operating(x.indptr, x.indices, x.data, n_img * tpi, s, cls, roles)
    _check({**{k: got[k].T for k in PAIRS}, "n_pos": got["n_pos"], "n_neg": got["n_neg"], "class_counts": want["pos"]}, want, "token level")
    card = operating.scorecard(inference / "latent_operating.npz")
    assert len(card["f1"]) == 3 * s and np.array_equal(card["f1"], got["f1"].reshape(-1), equal_nan=True) and ((card["auroc"] >= 0) & (card["auroc"] <= 1)).all()
    # the rows of label 0 as negatives of every task, computed again over the file that is there
    again = operating.score_run("tok001", operating.Config(**{**cfg.__dict__, "ignored_as_negative": True, "force_recompute": True}))
    assert str(again["level"]) == "token" and np.array_equal(again["n_pos"], got["n_pos"]) and (again["n_neg"] == n_img * tpi - again["n_pos"]).all()
