"""The latent AP on the MI355X (include/saev_amd.h: LATENT AP): the kernels against the high-precision evaluation of
the contract (tests/latent_ap_restatement.py: ``decimal`` at 80 digits, rounded once) on the designs of tests/latent_ap_cases.py, the
sorted arrays against numpy's lexsort, fixture G26 recorded from the reference, determinism and independence, the error word, and
``classification.eval_worker_fn`` on a small run directory.

Tolerances (derived, not tuned): in AP units every piece of a term is at most 1, a pair has n_{j,c} + 1 terms (n_{j,c} = events of
latent j in class c) and a term at most about 16 roundings of 2^-53 given the relative accuracy of H_{t+n} - H_t, so
|ap - exact| <= (n_{j,c} + 2) 2^-49.  Against the reference's float32 ``ref_ap``: both are far inside half a float32 ulp of the exact
value, so they round to the same float or to neighbours (<= 1 ulp).  best_class is compared with np.argmax of the kernel's own ap."""

import json
import pickle
import types

import numpy as np
import pytest
import scipy.sparse
import torch

import csr_cases
import latent_ap_cases as K
import latent_ap_restatement as R
from conftest import GOLDEN

pytestmark = [pytest.mark.gpu, pytest.mark.encoder_modes("f32")]
DEV = "cuda"


def _run(d, cls=None, c=None, *, labels=None, remap=None):
    from saev_amd import engine

    cls = d["cls"] if cls is None else cls
    lab = torch.from_numpy(np.ascontiguousarray(cls)).to(DEV) if labels is None else labels
    res = engine.latent_ap(*(torch.from_numpy(d[k]).to(DEV) for k in ("indptr", "indices", "data")), d["n"], d["s"], d["c"] if c is None else c,
                           labels=lab, remap=remap, nnz=int(d["indptr"][-1] - d["indptr"][0]))
    assert res.layout.direct_max == K.DIRECT_MAX == R.DIRECT_MAX
    return res


def _host(res):
    return res.ap.cpu().numpy(), res.n_pos.cpu().numpy(), res.best_ap.cpu().numpy(), res.best_class.cpu().numpy()


@pytest.fixture(scope="module")
def designs():
    """name -> (design, kernel outputs on the host, exact ap, events per pair): built once, shared, left unchanged."""
    built = {}

    def get(name):
        if name not in built:
            d = {**K.SMALL, **K.LARGE}[name]()
            exact, pos, n_ev = R.exact_ap(d["indptr"], d["indices"], d["data"], d["n"], d["s"], d["cls"], d["c"])
            built[name] = (d, _host(_run(d)), exact, pos, n_ev)
        return built[name]

    return get


@pytest.mark.parametrize("name", list(K.SMALL) + list(K.LARGE))
def test_ap_against_the_exact_evaluation(designs, name):
    d, (ap, pos, best_ap, best_class), exact, pos_x, n_ev = designs(name)
    assert ap.shape == (d["s"], d["c"]) and ap.dtype == np.float64
    assert (pos == pos_x).all()
    miss = np.abs(ap - exact) / R.bound(n_ev)
    j, c = np.unravel_index(np.argmax(miss), miss.shape)
    print(f"{name}: largest |ap - exact| / bound = {miss.max():.3g} at latent {j}, class {c} ({n_ev[j, c]} events)")
    assert (miss <= 1.0).all()
    assert (ap[:, pos == 0] == 0).all()
    assert (best_class == np.argmax(ap, axis=1)).all() and best_class.dtype == np.int32
    assert (best_ap == ap.max(axis=1)).all()


def test_designs_reach_what_they_are_meant_to_reach(designs):
    d = designs("deep")[0]
    m = np.diff(R.sorted_events(d["indptr"], d["indices"], d["data"], d["s"])[0])
    assert d["n"] == 70_000 and m.tolist() == [60, 64_999, 3000]
    d = designs("ragged")[0]
    m = np.diff(R.sorted_events(d["indptr"], d["indices"], d["data"], d["s"])[0])
    assert d["indptr"][0] == 37 and m.max() == 5000 and (np.delete(m, 517) <= 3).all() and (m == 0).any()
    d = designs("wide_4096")[0]
    assert d["c"] == 4096 and (np.bincount(d["cls"][d["cls"] >= 0], minlength=4096) == 0).sum() > 4000 and (d["cls"] == 4095).any()
    d, (ap, pos, _, _), *_ = designs("zero_groups")
    assert pos[2] == 1 and pos[3] == 4  # a class with one row; a class whose rows lie in the zero group


def test_both_label_forms_give_the_same_bits(designs):
    d, (ap, pos, best_ap, best_class), *_ = designs("kinds")
    to_byte = (np.arange(d["c"]) * 23 + 5) % 251           # a column's byte (distinct: 23 is coprime to 251)
    bytes_n = np.where(d["cls"] >= 0, to_byte[np.maximum(d["cls"], 0)], 253).astype(np.uint8)
    remap = np.full(256, -1, dtype=np.int32)
    remap[to_byte] = np.arange(d["c"], dtype=np.int32)
    got = _host(_run(d, labels=torch.from_numpy(bytes_n).to(DEV), remap=torch.from_numpy(remap).to(DEV)))
    for a, b in zip(got, (ap, pos, best_ap, best_class)):
        np.testing.assert_array_equal(a, b)
    # bytes without a remap are the columns themselves (no byte says "no class": every row gets one)
    full = np.where(d["cls"] >= 0, d["cls"], 3).astype(np.int32)
    a_i32 = _host(_run(d, cls=full))
    a_u8 = _host(_run(d, labels=torch.from_numpy(full.astype(np.uint8)).to(DEV)))
    for a, b in zip(a_u8, a_i32):
        np.testing.assert_array_equal(a, b)
    assert a_i32[1].sum() == d["n"] and not np.array_equal(a_i32[0], ap)


def test_golden_g26_within_one_float32_ulp_of_the_reference():
    with np.load(GOLDEN / "g26_latent_ap.npz") as z:
        g = {k: z[k] for k in z.files}
    d = dict(indptr=g["indptr"], indices=g["indices"], data=g["data"], n=int(g["n_rows"]), s=int(g["n_latents"]), c=int(g["n_classes"]), cls=g["labels"])
    ap, pos, _, best_class = _host(_run(d))
    ulps = R.ulps32(ap.astype(np.float32), g["ref_ap"])
    print(f"G26: largest distance to ref_ap {ulps.max()} float32 ulps; |ap - exact| / bound {(np.abs(ap - g['exact_ap']) / R.bound(g['n_events'])).max():.3g}")
    assert ulps.max() <= 1
    assert (np.abs(ap - g["exact_ap"]) <= R.bound(g["n_events"])).all()
    assert (best_class == np.argmax(ap, axis=1)).all()


def test_two_calls_give_the_same_bits_and_latents_and_classes_stand_alone(designs):
    d, (ap, pos, best_ap, best_class), *_ = designs("kinds")
    again = _host(_run(d))
    for a, b in zip(again, (ap, pos, best_ap, best_class)):
        np.testing.assert_array_equal(a, b)
    dense = scipy.sparse.csr_matrix((d["data"], d["indices"], d["indptr"]), shape=(d["n"], d["s"]))
    stored = scipy.sparse.csr_matrix((np.ones_like(d["data"]), d["indices"], d["indptr"]), shape=(d["n"], d["s"])).toarray() != 0
    for j in (2, 7, 15):  # a signed latent, the dense one with both signs, the one with stored zeros
        one = K._pack(dense.toarray()[:, [j]], stored[:, [j]], d["cls"], d["c"])
        np.testing.assert_array_equal(_host(_run(one))[0][0], ap[j])
    for c in (0, 4, d["c"] - 2):
        alone = np.where(d["cls"] == c, 0, -1).astype(np.int32)
        got = _host(_run(d, cls=alone, c=1))
        np.testing.assert_array_equal(got[0][:, 0], ap[:, c])
        assert got[1][0] == pos[c]


@pytest.mark.parametrize("name", ["value_images", "kinds", "ragged"])
def test_sorted_events_equal_numpys_lexsort(designs, name):
    d = designs(name)[0]
    starts, key, latent, row = (t.cpu().numpy() for t in _run(d).sorted_events())
    w_starts, w_lat, w_val, w_row = R.sorted_events(d["indptr"], d["indices"], d["data"], d["s"])
    np.testing.assert_array_equal(starts, w_starts)
    np.testing.assert_array_equal(latent, w_lat.astype(np.int32))
    np.testing.assert_array_equal(key.view(np.uint32), R.value_key(w_val))
    np.testing.assert_array_equal(row, w_row.astype(np.int32))


@pytest.mark.parametrize("shift", [0, 333])
def test_sorted_rows_across_empty_rows_and_a_block_that_does_not_start_at_0(shift):
    """The row of a stored entry where indptr repeats (empty rows first, last and three in a run) and where it starts at ``shift``."""
    d = csr_cases.empty_rows_block(shift)
    res = _run(dict(d, c=3, cls=np.arange(d["n"], dtype=np.int32) % 3))
    starts, key, latent, row = (t.cpu().numpy() for t in res.sorted_events())
    order = csr_cases.by_latent(d, by_value=True)
    np.testing.assert_array_equal(starts, np.concatenate([[0], np.cumsum(np.bincount(d["cols"], minlength=d["s"]))]))
    np.testing.assert_array_equal(row, d["rows"][order])
    np.testing.assert_array_equal(latent, d["cols"][order])
    np.testing.assert_array_equal(key.view(np.uint32), R.value_key(d["vals"][order]))
    res.ap  # (the error word is 0: the entries in front of the block were not read)


def test_the_error_word_is_set_and_python_raises():
    d = K.kinds()
    bad = d["cls"].copy()
    bad[17] = d["c"]
    with pytest.raises(ValueError, match="class id"):
        _run(d, cls=bad).ap
    bad[17] = -2
    with pytest.raises(ValueError, match="class id"):
        _run(d, cls=bad).best_class
    e = dict(d, indices=d["indices"].copy())
    e["indices"][len(e["indices"]) // 2] = d["s"]
    res = _run(e)
    with pytest.raises(ValueError, match="column index"):
        res.n_pos
    with pytest.raises(ValueError, match="column index"):  # every read raises, not just the first
        res.ap
    _run(d).ap  # and a good call after them is good


def test_dense_entries_equal_the_rows_of_the_matrix_entry():
    from saev_amd import classification as cl

    d = K.kinds()
    x = scipy.sparse.csr_matrix((d["data"], d["indices"], d["indptr"]), shape=(d["n"], d["s"]))
    labels = (d["cls"] + 1).astype(np.uint8)  # byte 0 = no class, ignored by default
    ap_sc, classes, n_pos = cl.latent_ap_matrix(x, labels)
    assert classes.tolist() == sorted(set(labels.tolist()) - {0}) and ap_sc.dtype == np.float64
    one_hot = (labels[:, None] == classes[None, :]).astype(np.float32)
    assert (n_pos == one_hot.sum(axis=0)).all()
    dense = x.toarray()
    batch = cl.compute_ap_batched(dense[:, 2:9], one_hot, one_hot.sum(axis=0))
    assert batch.dtype == np.float32 and batch.shape == (7, len(classes))
    np.testing.assert_array_equal(batch, ap_sc[2:9].astype(np.float32))
    one = cl.compute_ap_for_latent(dense[:, 7], one_hot, one_hot.sum(axis=0))
    np.testing.assert_array_equal(one, ap_sc[7].astype(np.float32))
    with pytest.raises(ValueError, match="column sums"):
        cl.compute_ap_batched(dense[:, :1], one_hot, one_hot.sum(axis=0) + 1)


def test_eval_worker_fn_writes_the_references_files(tmp_path):
    from saev_amd import classification as cl
    from saev_amd import disk
    from saev_amd.data import write_shards

    rng = np.random.default_rng(12)
    d_sae, n_ex, T = 24, 50, 6
    lab = rng.choice(np.array([0, 2, 3, 7, 200], dtype=np.uint8), size=(n_ex, T))
    shards = write_shards(tmp_path / "s0", rng.standard_normal((n_ex, 1, T, 8)).astype(np.float32), labels=lab)
    x = scipy.sparse.random(n_ex * T, d_sae, density=0.2, format="csr", dtype=np.float32, random_state=3)
    x.data = (np.ceil(x.data * 4) / 4).astype(np.float32)
    x.data += (lab.reshape(-1)[x.nonzero()[0]] == np.array([2, 3, 7, 200])[x.nonzero()[1] % 4]).astype(np.float32)
    run = disk.Run.new("audit0001", train_shards_dir=shards, val_shards_dir=shards, runs_root=tmp_path / "saev" / "runs")
    out = run.inference / shards.name
    out.mkdir()
    scipy.sparse.save_npz(out / "token_acts.npz", x)
    payloads = [("sparse-linear", types.SimpleNamespace(coef_=rng.standard_normal((3, d_sae)) * (rng.random((3, d_sae)) < 0.4))),
                ("decision-tree", types.SimpleNamespace(feature_importances_=rng.random(d_sae) * (rng.random(d_sae) < 0.5)))]
    ckpts = []
    for i, (key, obj) in enumerate(payloads):
        ckpts.append(tmp_path / f"cls_{i}.pkl")
        with open(ckpts[-1], "wb") as fd:
            fd.write(json.dumps({"cfg": {"cls": {"key": key}}, "test_acc": 0.5}).encode() + b"\n")
            pickle.dump({"classifier": obj}, fd)
    cfg = cl.EvalConfig(run=run.run_dir, test_shards=shards, cls_checkpoints=tuple(ckpts), max_budget=5, budgets=(1, 3, 5), tau=0.3)
    assert cl.eval_worker_fn(cfg) == 0

    labels_flat = lab.reshape(-1)
    classes = np.array([2, 3, 7, 200])
    cls = np.full(len(labels_flat), -1, dtype=np.int32)
    for k, c in enumerate(classes):
        cls[labels_flat == c] = k
    want, _, _ = R.latent_ap(x.indptr.astype(np.int64), x.indices.astype(np.int32), x.data, n_ex * T, d_sae, cls, 4)
    ap_sc = np.load(out / "audit_ap_sc.npy")
    assert ap_sc.shape == (d_sae, 4) and ap_sc.dtype == np.float32 and R.ulps32(ap_sc, want.astype(np.float32)).max() <= 1
    device_ap, device_classes, _ = cl.latent_ap_matrix(x, labels_flat)
    assert device_classes.tolist() == classes.tolist()
    np.testing.assert_array_equal(ap_sc, device_ap.astype(np.float32))

    rankings = [cl.extract_feature_ranking(obj, key)[0] for key, obj in payloads]
    union = sorted(set(rankings[0][:5].tolist()) | set(rankings[1][:5].tolist()))
    assert 5 <= len(union) < d_sae
    best_ap_s, best_class_s = np.load(out / "audit_ap_s.npy"), np.load(out / "audit_best_class_s.npy")
    assert best_ap_s.dtype == np.float32 and best_class_s.dtype == np.int32 and best_ap_s.shape == best_class_s.shape == (d_sae,)
    outside = np.setdiff1d(np.arange(d_sae), union)
    assert np.isnan(best_ap_s[outside]).all() and (best_class_s[outside] == -1).all()
    np.testing.assert_array_equal(best_ap_s[union], device_ap.max(axis=1).astype(np.float32)[union])
    np.testing.assert_array_equal(best_class_s[union], classes[np.argmax(device_ap, axis=1)][union])  # original label ids
    assert R.ulps32(best_ap_s[union], want.max(axis=1).astype(np.float32)[union]).max() <= 1

    res = json.loads((out / "audit_results.json").read_text())
    assert sorted(res) == sorted(("run", "test_shards", "max_budget", "n_features_evaluated", "n_seg_classes", "ignore_label_ids", "d_sae", "classifiers"))
    assert res["n_features_evaluated"] == len(union) and res["n_seg_classes"] == 4 and res["d_sae"] == d_sae and res["ignore_label_ids"] == [0]
    for entry, ckpt, (key, obj), ranked in zip(res["classifiers"], ckpts, payloads, rankings):
        assert sorted(entry) == sorted(("cls_checkpoint", "cls_type", "n_nonzero_importance", "tau", "budgets", "yield_at_b", "auc_b"))
        assert entry["cls_checkpoint"] == str(ckpt) and entry["cls_type"] == key and entry["budgets"] == [1, 3, 5] and entry["tau"] == 0.3
        y = {str(b): float(int(np.nansum(best_ap_s[ranked[:b]] >= 0.3)) / b) for b in (1, 3, 5)}
        assert entry["yield_at_b"] == y and entry["auc_b"] == sum(y.values()) / 3
        assert entry["n_nonzero_importance"] == int((cl.extract_feature_ranking(obj, key)[1] > 0).sum())
