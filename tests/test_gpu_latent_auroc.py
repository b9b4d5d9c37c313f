"""GPU tests of the latent AUROC (include/saev_amd.h: LATENT AUROC) against its numpy restatement
(tests/latent_auroc_restatement.py, itself held against the pair-counting definition and the reference's recorded values by
tests/test_latent_auroc_host_cpu.py) on the designs of tests/latent_auroc_cases.py.

What is asserted: ``u2``, ``n_pos``, ``n_neg``, ``fire_*`` and the class counts ON THE INTEGERS; ``auroc`` equal to
u2 / (2.0 * n_pos * n_neg) on the fp64 bits (NaN where a task has no positives or no negatives); ``sum_*`` equal to the restatement's
sequential fp64 sum on the bits and within (m + 1) 2^-53 sum |a| of ``math.fsum`` (m additions, each within 2^-53 relative of a
partial sum that is at most sum |a|); ``mimics.score_run`` on the float32 bits of the reference's ``auroc`` and supports and within
(n + 2) 2^-24 (sum |a|) / n of its means."""

import numpy as np
import pytest
import scipy.sparse
import torch

import analysis_scale_cases as A
import latent_auroc_cases as AK
import latent_auroc_restatement as AR
from conftest import GOLDEN

pytestmark = [pytest.mark.gpu, pytest.mark.encoder_modes("f32")]
DEV = "cuda"


def _run(d, *, labels=None, remap=None, roles=None):
    from saev_amd import engine

    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)  # noqa: E731
    return engine.latent_auroc(t(d["indptr"]), t(d["indices"]), t(d["data"]), d["n"], d["s"], d["c"], labels=t(d["cls"] if labels is None else labels),
                               remap=None if remap is None else t(remap), roles=t(d["roles"] if roles is None else roles))


def _host(res):
    return {k: getattr(res, k).cpu().numpy() for k in ("auroc", "u2", "n_pos", "n_neg", "fire_pos", "fire_neg", "sum_pos", "sum_neg", "class_counts")}


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


def _check(got, want, name=""):
    for key in ("u2", "n_pos", "n_neg", "fire_pos", "fire_neg"):
        np.testing.assert_array_equal(got[key], want[key], err_msg=f"{name}: {key}")
    np.testing.assert_array_equal(got["class_counts"], want["pos"])
    void = (want["n_pos"] == 0) | (want["n_neg"] == 0)
    assert np.isnan(got["auroc"][:, void]).all() and (got["u2"][:, void] == 0).all()
    assert _same_bits(got["auroc"][:, ~void], want["auroc"][:, ~void]), f"{name}: auroc"
    for role in ("pos", "neg"):
        mine, seq = got[f"sum_{role}"], want[f"sum_{role}"]
        nan = np.isnan(seq)
        assert np.array_equal(np.isnan(mine), nan) and _same_bits(mine[~nan], seq[~nan]), f"{name}: sum_{role}"
        finite = np.isfinite(want[f"fsum_{role}"]) & np.isfinite(seq)
        bound = (want[f"n_ev_{role}"] + 1) * 2.0 ** -53 * want[f"abs_{role}"]
        assert (np.abs(mine[finite] - want[f"fsum_{role}"][finite]) <= bound[finite]).all(), f"{name}: sum_{role} against fsum"


@pytest.fixture(scope="module")
def restated():
    """The restatement of every small design, computed once and left unchanged."""
    out = {}
    for name, make in AK.SMALL.items():
        d = make()
        out[name] = (d, AR.one_walk(d["indptr"], d["indices"], d["data"], d["n"], d["s"], d["cls"], d["roles"]))
    return out


@pytest.mark.parametrize("name", list(AK.SMALL))
def test_small_designs_against_the_restatement(restated, name):
    d, want = restated[name]
    got = _host(_run(d))
    _check(got, want, name)
    n_events = np.bincount(d["indices"][d["data"] != 0], minlength=d["s"])
    ok = (want["n_pos"] > 0) & (want["n_neg"] > 0)
    assert (got["auroc"][n_events == 0][:, ok] == 0.5).all()


def test_both_label_forms_give_the_same_bits(restated):
    for name in ("kinds", "grid_5x11x130"):
        d, want = restated[name]
        labels, remap = AK.as_bytes(d)
        got = _host(_run(d, labels=labels, remap=remap))
        _check(got, want, name)
        wide = _host(_run(d, labels=d["cls"].astype(np.int64)))
        assert all(np.array_equal(got[k].view(np.int64), wide[k].view(np.int64)) for k in got)
    d, want = restated["chunks"]  # bytes without a remap: the identity (a design without rows of class -1)
    cls = np.where(d["cls"] < 0, 0, d["cls"]).astype(np.int32)
    plain = AR.one_walk(d["indptr"], d["indices"], d["data"], d["n"], d["s"], cls, d["roles"])
    _check(_host(_run(d, labels=cls.astype(np.uint8))), plain, "chunks as bytes")


def test_two_calls_a_task_alone_and_a_latent_alone_give_the_same_bits(restated):
    for name, tasks, latents in (("kinds", (0, 2, 5), (6, 7, 11)), ("grid_5x300x65", (0, 63, 64), (1, 2)), ("chunks", (1,), (0, 4))):
        d, _ = restated[name]
        full, again = _host(_run(d)), _host(_run(d))
        assert all(np.array_equal(full[k].view(np.int64), again[k].view(np.int64)) for k in full)
        per_pair = ("auroc", "u2", "fire_pos", "fire_neg", "sum_pos", "sum_neg")
        for t in tasks:
            alone = _host(_run(d, roles=d["roles"][t:t + 1]))
            assert all(np.array_equal(alone[k][:, 0].view(np.int64), full[k][:, t].view(np.int64)) for k in per_pair), (name, t)
            assert alone["n_pos"][0] == full["n_pos"][t] and alone["n_neg"][0] == full["n_neg"][t]
        for j in latents:
            alone = _host(_run(AK.one_latent(d, j)))
            assert all(np.array_equal(alone[k][0].view(np.int64), full[k][j].view(np.int64)) for k in per_pair), (name, j)


def test_large_counts_where_the_sort_takes_its_second_trip():
    """The ``past_cap`` design (70 000 rows, 2.24 M entries) with three tasks.  2 n_pos n_neg is at most 2 x 35 000^2 < 2^32 on 70 000
    rows, so u2 stays below 2^32 here whatever the tasks (the next test passes it); what this design has is counts past 2^29, every
    latent tens of thousands of events long and the sort's second trip."""
    d = dict(A.past_cap(), roles=AK.PAST_CAP_ROLES)
    assert len(d["data"]) > A.GRID_CAP_ENTRIES and d["c"] == AK.PAST_CAP_ROLES.shape[1]
    want = AR.by_ranks(d["indptr"], d["indices"], d["data"], d["n"], d["s"], d["cls"], d["roles"])
    print("past_cap: n_pos", want["n_pos"].tolist(), "n_neg", want["n_neg"].tolist(), "largest u2", int(want["u2"].max()))
    assert (want["u2"].max(axis=0) > 1 << 27).all() and (want["u2"] > 1 << 29).any()
    _check(_host(_run(d)), want, "past_cap")


def test_u2_past_2_32():
    d = AK.wide_counts()
    want = AR.one_walk(d["indptr"], d["indices"], d["data"], d["n"], d["s"], d["cls"], d["roles"])
    assert (want["u2"] > 1 << 32).all() and (want["u2"][:, 0] + want["u2"][:, 1] == 2 * want["n_pos"][0] * want["n_neg"][0]).all()  # the roles swapped
    _check(_host(_run(d)), want, "wide_counts")


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
        res.auroc
    with pytest.raises(ValueError, match=message):
        res.check()


def test_sorted_events_are_left_where_latent_aps_layout_says(restated):
    from latent_ap_restatement import sorted_events, value_key

    d, _ = restated["kinds"]
    starts, key, latent, row = _run(d).sorted_events()
    w_starts, w_lat, w_val, w_rows = sorted_events(d["indptr"], d["indices"], d["data"], d["s"])
    np.testing.assert_array_equal(starts.cpu().numpy(), w_starts)
    np.testing.assert_array_equal(key.cpu().numpy().view(np.uint32), value_key(w_val))
    np.testing.assert_array_equal(latent.cpu().numpy(), w_lat)
    np.testing.assert_array_equal(row.cpu().numpy(), w_rows)


# ---------------------------------------------------------------- the Python modules -----------------------------------------------------

@pytest.mark.parametrize("as_negative", [False, True])
def test_latent_auroc_matrix_against_the_restatement(as_negative):
    from saev_amd import classification as cl

    rng = np.random.default_rng(9)
    n, s = 400, 12
    labels = rng.choice(np.array([0, 2, 3, 7, 255], dtype=np.uint8), size=n)
    x = scipy.sparse.random(n, s, density=0.3, format="csr", dtype=np.float32, random_state=3)
    x.data = (np.ceil(x.data * 8) / 8 * rng.choice([-1.0, 1.0], size=x.nnz, p=[0.2, 0.8])).astype(np.float32)
    auroc, classes, n_pos = cl.latent_auroc_matrix(x, labels, ignore_label_ids=(0, 255), ignored_as_negative=as_negative)
    assert classes.tolist() == [2, 3, 7] and auroc.shape == (s, 3) and auroc.dtype == np.float64
    cls = np.select([labels == 2, labels == 3, labels == 7], [0, 1, 2], default=3 if as_negative else -1).astype(np.int32)
    roles = np.ones((3, 4 if as_negative else 3), dtype=np.uint8)
    roles[np.arange(3), np.arange(3)] = 2
    want = AR.one_walk(x.indptr, x.indices, x.data, n, s, cls, roles)
    assert _same_bits(auroc, want["auroc"]) and np.array_equal(n_pos, want["n_pos"])
    assert (want["n_neg"] == (n if as_negative else int((cls >= 0).sum())) - want["n_pos"]).all()


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN / "g29_latent_auroc.npz") as z:
        return {k: z[k] for k in z.files}


def _against_reference(cols, d, specs):
    bits = lambda x: np.ascontiguousarray(x).view(np.uint32)  # noqa: E731
    assert [cols[k].dtype for k in ("feature_id", "auroc", "support_erato", "support_melpomene", "mean_act_erato", "mean_act_melpomene")] == [np.int32] + [np.float32] * 5
    assert cols["task"].tolist() == d["col_task"].tolist() and np.array_equal(cols["feature_id"], d["col_feature_id"])
    for key in ("auroc", "support_erato", "support_melpomene"):
        assert np.array_equal(bits(cols[key]), bits(d[f"col_{key}"])), key
    for side, mask in (("erato", "erato_mask"), ("melpomene", "melp_mask")):
        for t, spec in enumerate(specs):
            acts = d["pooled"][spec.include][getattr(spec, mask)].astype(np.float64)
            at = slice(t * d["s"], (t + 1) * d["s"])
            miss = np.abs(cols[f"mean_act_{side}"][at].astype(np.float64) - d[f"col_mean_act_{side}"][at].astype(np.float64))
            assert (miss <= AR.mean_bound(len(acts), np.abs(acts).sum(axis=0))).all(), (side, spec.name)


def test_score_run_and_worker_fn_reproduce_the_references_columns(golden, tmp_path):
    from saev_amd import mimics

    for i, d in enumerate(AK.g29_designs(golden)):
        run_root, shards = AK.g29_run(tmp_path / f"d{i}", d)
        np.testing.assert_array_equal(mimics.max_pool_csr(scipy.sparse.csr_matrix((d["data"], d["indices"], d["indptr"]), shape=(d["n_images"] * d["tpi"], d["s"])),
                                                          d["n_images"], d["tpi"]), d["pooled"])
        cfg = mimics.Config(run_root_dpath=run_root, shards_dpath=shards, run_ids=["mimic001"], pair_specs=d["pair_specs"], views=d["views"],
                            min_samples=d["min_samples"], feature_chunk=d["feature_chunk"])
        mimics.worker_fn(cfg)
        npz = run_root / "mimic001" / "inference" / shards.name / "cambridge-mimics.npz"
        assert npz.exists()
        with np.load(npz) as z:
            cols = {k: z[k] for k in z.files}
        assert tuple(cols) == mimics.COLUMNS and set(cols["run_id"].tolist()) == {"mimic001"}
        specs = mimics.build_task_specs(d["sv"], pair_specs=d["pair_specs"], views=d["views"], min_samples=d["min_samples"])
        _against_reference(cols, d, specs)
        if i:
            continue
        # the cache is honoured: a marked file comes back as it is; force_recompute writes the scores again
        marked = dict(cols, auroc=np.full_like(cols["auroc"], 0.25))
        np.savez(npz, **marked)
        kw = dict(run_root_dpath=run_root, shard_id=shards.name, task_specs=specs, n_images=d["n_images"], feature_chunk=d["feature_chunk"])
        assert (mimics.score_run("mimic001", **kw)["auroc"] == 0.25).all()
        again = mimics.score_run("mimic001", force_recompute=True, **kw)
        assert np.array_equal(again["auroc"].view(np.uint32), cols["auroc"].view(np.uint32))
        with np.load(npz) as z:
            assert np.array_equal(z["auroc"].view(np.uint32), cols["auroc"].view(np.uint32))


def test_score_run_writes_the_parquet_when_pyarrow_is_there(golden, tmp_path):
    pq = pytest.importorskip("pyarrow.parquet")
    pytest.importorskip("pyarrow")
    from saev_amd import mimics

    d = AK.g29_designs(golden)[0]
    run_root, shards = AK.g29_run(tmp_path, d)
    specs = mimics.build_task_specs(d["sv"], pair_specs=d["pair_specs"], views=d["views"], min_samples=d["min_samples"])
    cols = mimics.score_run("mimic001", run_root_dpath=run_root, shard_id=shards.name, task_specs=specs, n_images=d["n_images"])
    table = pq.read_table(mimics.get_scores_fpath(run_root, run_id="mimic001", shard_id=shards.name))
    assert tuple(table.column_names) == mimics.COLUMNS and table.num_rows == len(cols["auroc"])
    assert np.array_equal(np.asarray(table["auroc"]).view(np.uint32), cols["auroc"].view(np.uint32)) and str(table.schema.field("feature_id").type) == "int32"
