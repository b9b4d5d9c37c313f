"""The probe AP on the MI355X (include/saev_amd.h: PROBE AP): the kernel against the high-precision evaluation of the
contract (tests/probe_ap_restatement.py: ``decimal`` at 80 digits, rounded once) on the designs of tests/probe_ap_cases.py in both
score dtypes, cross-checks against the kernels that exist (``latent_ap``, ``csr_topk``), determinism and independence on the bits,
void pairs, the error word, and ``probe_metrics.worker_fn`` on the run directory of fixture G28, recorded from the reference.

Tolerances (derived, not tuned): in AP units every piece of a term is at most 1, a pair has at most n_{j,c} + 1 non-zero terms
(n_{j,c} = events of latent j in class c; a group without a row of the class adds nothing, and only the zero block holds rows of the
class that are no events) and a term at most about 16 roundings of 2^-53, so |ap - exact| <= (n_{j,c} + 2) 2^-49, as for LATENT AP.
Counts are integers and compared as such.  Against the reference's float32 ``ap`` of G28: (2 N + 4) 2^-24, the reference's own error
bound, which the fixture's generator asserts."""

import numpy as np
import pytest
import scipy.sparse
import torch

import latent_ap_cases as K
import probe_ap_cases as PK
import probe_ap_restatement as PR
from conftest import GOLDEN

pytestmark = [pytest.mark.gpu, pytest.mark.encoder_modes("f32")]
DEV = "cuda"
DTYPES = {"fp32": np.float32, "fp64": np.float64}


def _run(d, dtype, *, w=None, b=None, cls=None, c=None, top_k=0):
    from saev_amd import engine

    w, b = (d["w"] if w is None else w), (d["b"] if b is None else b)
    cls = d["cls"] if cls is None else cls
    res = engine.probe_ap(*(torch.from_numpy(d[k]).to(DEV) for k in ("indptr", "indices", "data")), d["n"], d["s"], d["c"] if c is None else c,
                          labels=torch.from_numpy(np.ascontiguousarray(cls)).to(DEV), weights=torch.from_numpy(np.ascontiguousarray(w, dtype=dtype)).to(DEV),
                          biases=torch.from_numpy(np.ascontiguousarray(b, dtype=dtype)).to(DEV), top_k=top_k, nnz=int(d["indptr"][-1] - d["indptr"][0]))
    assert res.layout.direct_max == PK.DIRECT_MAX
    return res


def _host(res):
    return {k: getattr(res, k).cpu().numpy() for k in ("ap", "n_pos", "tp", "n_pred_pos")}


def _args(d, dtype):
    return (d["indptr"], d["indices"], d["data"], d["n"], d["s"], d["cls"], d["c"], d["w"].astype(dtype), d["b"].astype(dtype))


@pytest.fixture(scope="module")
def designs():
    """(name, dtype) -> (design, kernel outputs on the host, the exact evaluation): built once, shared, left unchanged."""
    built = {}

    def get(name, dt):
        if (name, dt) not in built:
            d = {**PK.SMALL, **PK.LARGE}[name]()
            built[name, dt] = (d, _host(_run(d, DTYPES[dt])), PR.exact_ap(*_args(d, DTYPES[dt])))
        return built[name, dt]

    return get


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("name", list(PK.SMALL) + list(PK.LARGE))
def test_ap_and_counts_against_the_exact_evaluation(designs, name, dt):
    d, got, x = designs(name, dt)
    assert got["ap"].shape == (d["s"], d["c"]) and got["ap"].dtype == np.float64 and got["tp"].dtype == got["n_pred_pos"].dtype == np.int64
    np.testing.assert_array_equal(got["n_pos"], x["pos"])
    miss = np.abs(got["ap"] - x["ap"]) / PR.bound(x["n_ev"])
    j, c = np.unravel_index(np.argmax(miss), miss.shape)
    print(f"{name} {dt}: largest |ap - exact| / bound = {miss.max():.3g} at latent {j}, class {c} ({x['n_ev'][j, c]} events)")
    assert (miss <= 1.0).all()
    assert (got["ap"][:, x["pos"] == 0] == 0).all()
    np.testing.assert_array_equal(got["tp"], x["tp"])
    np.testing.assert_array_equal(got["n_pred_pos"], x["pred_pos"])


def test_designs_reach_what_they_are_meant_to_reach(designs):
    r32, r64 = designs("kinds", "fp32")[2]["reach"], designs("kinds", "fp64")[2]["reach"]
    assert r32["inf_ties"] > 0 and r32["collapsed"] > r64["collapsed"] > 0 and r32["merged"] > r64["merged"] > 0
    assert r32["zero_first"] > 0 and r32["zero_inside"] > 0
    d, got, x = designs("kinds", "fp32")
    m = np.diff(PR.sorted_events(d["indptr"], d["indices"], d["data"], d["s"])[0])
    assert (m == 0).any() and (m == d["n"]).any() and x["pos"][d["c"] - 1] == 0 and (d["cls"] == -1).any()
    assert (np.signbit(d["w"][:, 3]) & (d["w"][:, 3] == 0)).all() and (d["w"][:, 2] == 0).all() and (d["b"][:, 7] == 0).all()
    for dt in DTYPES:
        r = designs("middle", dt)[2]["reach"]
        assert r["merged"] == 6 and r["zero_inside"] == 16  # both sides, one side, the other side (x 2 signs of w); never without b
    d = designs("wide70", "fp32")[0]
    assert d["c"] == 70 and all((d["w"][:, lo:hi] > 0).any() and (d["w"][:, lo:hi] < 0).any() for lo, hi in ((0, 64), (64, 70)))
    d = designs("chunks", "fp32")[0]
    assert np.diff(PR.sorted_events(d["indptr"], d["indices"], d["data"], d["s"])[0]).tolist() == [63, 64, 65, 129] and (d["w"][:, 0] < 0).all()
    assert designs("created", "fp32")[2]["reach"]["merged"] > 0
    d = designs("deep", "fp32")[0]
    assert d["n"] == 70_000 and np.diff(PR.sorted_events(d["indptr"], d["indices"], d["data"], d["s"])[0]).tolist() == [60, 64_999, 3000]
    assert (d["w"] > 0).any() and (d["w"] < 0).any()


def test_a_latent_silent_on_positive_rows_against_the_exact_evaluation_only(designs):
    """Every latent of ``silent`` fires on about half the rows of its class; the others lie in the zero block, tied at score b with
    every other silent row.  The reference ranks such a tie in whatever order its unstable argsort leaves (in practice by row
    number), so its AP for such a pair is an accident of the row order, not a property of the probe: it is not consulted here.  The
    contract's value is the mean over all orders of the tied rows (tests/test_probe_ap_host_cpu.py checks that against an
    enumeration), and that is what the kernel must give."""
    for dt in DTYPES:
        d, got, x = designs("silent", dt)
        in_block = x["pos"] - x["n_ev"].diagonal()
        assert (in_block > 0).all() and (x["n_ev"].diagonal() > 0).all()
        assert (np.abs(got["ap"] - x["ap"]) <= PR.bound(x["n_ev"])).all()


@pytest.mark.parametrize("dt", list(DTYPES))
def test_unit_weights_give_the_bits_of_latent_ap(dt):
    from saev_amd import engine

    d = K.kinds()
    ones, zeros = np.ones((d["s"], d["c"])), np.zeros((d["s"], d["c"]))
    dev = [torch.from_numpy(d[k]).to(DEV) for k in ("indptr", "indices", "data")]
    lab = torch.from_numpy(d["cls"]).to(DEV)
    want = engine.latent_ap(*dev, d["n"], d["s"], d["c"], labels=lab)
    got = _run(d, DTYPES[dt], w=ones, b=zeros)
    np.testing.assert_array_equal(got.ap.cpu().numpy(), want.ap.cpu().numpy())
    np.testing.assert_array_equal(got.n_pos.cpu().numpy(), want.n_pos.cpu().numpy())
    for a, b in zip(got.sorted_events(), want.sorted_events()):  # the same sort, the same arrays left behind
        np.testing.assert_array_equal(a.cpu().numpy(), b.cpu().numpy())
    negated = engine.latent_ap(dev[0], dev[1], -dev[2], d["n"], d["s"], d["c"], labels=lab)
    np.testing.assert_array_equal(_run(d, DTYPES[dt], w=-ones, b=zeros).ap.cpu().numpy(), negated.ap.cpu().numpy())


def test_top_rows_equal_csr_topk_and_numpys_lexsort():
    from saev_amd import helpers

    d = PK.kinds()
    x = scipy.sparse.csr_matrix((d["data"], d["indices"], d["indptr"]), shape=(d["n"], d["s"]))
    got = _run(d, np.float32, top_k=64).top_rows.cpu().numpy()
    assert got.shape == (d["s"], 64) and got.dtype == np.int64
    np.testing.assert_array_equal(got, helpers.csr_topk(x, k=64, axis=0).indices.T)
    got = _run(d, np.float32, top_k=256).top_rows.cpu().numpy()
    np.testing.assert_array_equal(got, PR.top_rows(d["indptr"], d["indices"], d["data"], d["s"], 256))
    m = np.diff(PR.sorted_events(d["indptr"], d["indices"], d["data"], d["s"])[0])
    assert (m < 64).any() and (m == 0).any() and (m > 256).any() and d["n"] >= 256
    assert _run(d, np.float32).top_rows is None


@pytest.mark.parametrize("dt", list(DTYPES))
def test_two_calls_give_the_same_bits_and_a_pair_stands_alone(designs, dt):
    d, got, _ = designs("kinds", dt)
    again = _host(_run(d, DTYPES[dt]))
    for k in got:
        np.testing.assert_array_equal(again[k], got[k])
    dense = scipy.sparse.csr_matrix((d["data"], d["indices"], d["indptr"]), shape=(d["n"], d["s"])).toarray()
    stored = scipy.sparse.csr_matrix((np.ones_like(d["data"]), d["indices"], d["indptr"]), shape=(d["n"], d["s"])).toarray() != 0
    for j, c in ((2, 0), (7, 1), (7, 8), (15, 5), (9, 6), (0, 4), (6, 9)):  # signed, dense with both signs, stored zeros, one value, no events
        one = K._pack(dense[:, [j]], stored[:, [j]], np.where(d["cls"] == c, 0, -1).astype(np.int32), 1)
        alone = _host(_run(one, DTYPES[dt], w=d["w"][[j]][:, [c]], b=d["b"][[j]][:, [c]]))
        for k, v in (("ap", got["ap"][j, c]), ("tp", got["tp"][j, c]), ("n_pred_pos", got["n_pred_pos"][j, c]), ("n_pos", got["n_pos"][c])):
            assert alone[k].reshape(-1)[0] == v, (j, c, k)


@pytest.mark.parametrize("dt", list(DTYPES))
def test_void_pairs_give_nan_and_touch_no_other_pair(designs, dt):
    d, got, _ = designs("kinds", dt)
    w, b = d["w"].copy(), d["b"].copy()
    void = np.zeros(w.shape, dtype=bool)
    w[3, 0], b[7, 1], w[20, 9], b[20, 10], w[0, 2] = np.nan, np.inf, -np.inf, np.nan, np.inf
    for j, c in ((3, 0), (7, 1), (20, 9), (20, 10), (0, 2)):
        void[j, c] = True
    res = _run(d, DTYPES[dt], w=w, b=b)
    res.check()  # a diverged probe does not set the error word
    out = _host(res)
    assert np.isnan(out["ap"][void]).all() and (out["tp"][void] == 0).all() and (out["n_pred_pos"][void] == 0).all()
    for k in ("ap", "tp", "n_pred_pos"):
        np.testing.assert_array_equal(out[k][~void], got[k][~void])
    np.testing.assert_array_equal(out["n_pos"], got["n_pos"])


def test_the_error_word_is_set_and_python_raises():
    d = PK.kinds()
    bad = d["cls"].copy()
    bad[17] = d["c"]
    with pytest.raises(ValueError, match="class id"):
        _run(d, np.float32, cls=bad).ap
    bad[17] = -2
    with pytest.raises(ValueError, match="class id"):
        _run(d, np.float64, cls=bad).check()
    e = dict(d, indices=d["indices"].copy())
    e["indices"][len(e["indices"]) // 2] = d["s"]
    res = _run(e, np.float32)
    with pytest.raises(ValueError, match="column index"):
        res.tp
    with pytest.raises(ValueError, match="column index"):  # every read raises, not just the first
        res.ap
    for value in (np.inf, -np.inf, np.nan):
        e = dict(d, data=d["data"].copy())
        e["data"][len(e["data"]) // 3] = value
        with pytest.raises(ValueError, match="not finite"):
            _run(e, np.float32, top_k=4).top_rows
    _run(d, np.float32).ap  # and a good call after them is good


def test_worker_fn_on_the_run_directory_of_g28(tmp_path):
    from saev_amd import probe_metrics

    with np.load(GOLDEN / "g28_probe_metrics.npz") as z:
        g = {k: z[k] for k in z.files}
    run_dir, train_shards, test_shards = PK.g28_run(tmp_path, g)
    probe_metrics.worker_fn(probe_metrics.Config(run=run_dir, train_shards=train_shards, test_shards=test_shards, max_k=int(g["max_k"])))
    out = run_dir / "inference" / test_shards.name
    with np.load(out / f"probe1d_metrics__train-{train_shards.name}.npz") as z:
        got = {k: z[k] for k in z.files}
    assert sorted(got) == ["ap", "f1", "precision", "recall", "top_labels"]
    n, s, c = len(g["labels"]), int(g["n_latents"]), int(g["n_classes"])
    for k in got:
        assert got[k].dtype == g["ref_" + k].dtype and got[k].shape == g["ref_" + k].shape, k
    assert got["top_labels"].shape == (s, int(g["max_k"])) and got["top_labels"].dtype == np.uint8 and got["ap"].shape == (c,)
    distance = np.abs(got["ap"].astype(np.float64) - g["ref_ap"].astype(np.float64))
    print(f"G28: |ap - ref ap| {distance.tolist()} against {(2 * n + 4) * 2.0 ** -24:.3g}; ulps {PR.ulps32(got['ap'], g['ref_ap']).tolist()}")
    assert (distance <= (2 * n + 4) * 2.0 ** -24).all()  # every class
    for k in ("precision", "recall", "f1", "top_labels"):
        assert np.array_equal(got[k], g["ref_" + k]), k
    assert (np.abs(got["ap"].astype(np.float64) - g["exact_ap"]) <= 2.0 ** -24).all()  # one float32 rounding of the exact value
    ap_lc = np.load(out / f"probe1d_ap_lc__train-{train_shards.name}.npy")
    assert ap_lc.shape == (s, c) and ap_lc.dtype == np.float32
    np.testing.assert_array_equal(ap_lc[np.argmin(g["loss"], axis=0), np.arange(c)], got["ap"])
