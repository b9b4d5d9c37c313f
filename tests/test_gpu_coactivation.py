"""GPU tests of COACTIVATION (include/saev_amd.h): engine.coactivation_match on every case of
tests/coactivation_cases.py against the integer restatement (tests/coactivation_restatement.py), the error word, determinism and
independence of the row order, and saev_amd.alignment / tools/align_latents.py end to end on run directories the test writes.

No tolerance anywhere: index, intersection, support_a and support_b are integers and must EQUAL the restatement; jaccard and
containment are one float64 division of those integers on either side, so they must be equal too."""

import functools
import importlib.util
import json

import numpy as np
import pytest
import scipy.sparse
import torch

import coactivation_cases as K
import coactivation_restatement as R
from conftest import ROOT

pytestmark = [pytest.mark.gpu, pytest.mark.encoder_modes("f32")]
DEV = "cuda"
CASES = {c.name: c for c in K.all_cases()}


@functools.lru_cache(maxsize=None)
def _expected(name):
    c = CASES[name]
    return R.match(c.A, c.B, **c.settings)


def _dev(m):
    if m is None:
        return None
    m = scipy.sparse.csr_matrix(m)
    return (torch.from_numpy(m.indptr.astype(np.int64)).to(DEV), torch.from_numpy(m.indices.astype(np.int32)).to(DEV),
            torch.from_numpy(np.ascontiguousarray(m.data, dtype=np.float32)).to(DEV))


def _run(A, B, **settings):
    from saev_amd import engine

    return engine.coactivation_match(_dev(A), _dev(B), n_rows=A.shape[0], n_latents_a=A.shape[1], n_latents_b=None if B is None else B.shape[1],
                                     **settings)


INTEGERS = ("index", "intersection", "support_a", "support_b")


def _assert_equal(res, want, what=INTEGERS):
    for k in what:
        got = getattr(res, k).cpu().numpy()
        assert got.dtype == want[k].dtype or k in ("jaccard", "containment", "mutual"), k
        bad = np.argwhere(~((got == want[k]) | ((got != got) & (want[k] != want[k]))))
        assert got.shape == want[k].shape and bad.size == 0, (k, bad[:5].tolist(), got[tuple(bad[0])] if bad.size else None,
                                                            want[k][tuple(bad[0])] if bad.size else None)


@pytest.mark.parametrize("name", list(CASES))
def test_equals_the_restatement(name):
    c = CASES[name]
    res = _run(c.A, c.B, **c.settings)
    _assert_equal(res, _expected(name), INTEGERS + ("jaccard", "containment", "mutual"))
    if c.B is not None:
        K._eq(res.reverse.index[:, 0].cpu().numpy(), _expected(name)["reverse_index"])


@pytest.mark.parametrize("name", ["random_jaccard", "random_self", "heavy_lists", "window_sb_%d" % (K.WINDOW + 1), "random_long_rows"])
def test_two_calls_and_a_shuffled_row_order_give_the_same_bits(name):
    c = CASES[name]
    first, second = _run(c.A, c.B, **c.settings), _run(c.A, c.B, **c.settings)
    perm = np.random.default_rng(0).permutation(c.A.shape[0])
    shuffled = _run(c.A[perm], None if c.B is None else c.B[perm], **c.settings)
    for k in INTEGERS:
        assert torch.equal(getattr(first, k), getattr(second, k)), k
        assert torch.equal(getattr(first, k), getattr(shuffled, k)), k
    _assert_equal(first, _expected(name))


def _broken(kind):
    rng = np.random.default_rng(1)
    A, B = K.random_csr(rng, 100, 20, 5), K.random_csr(rng, 100, 30, 4)
    a, b = [list(x) for x in (_dev(A), _dev(B))]
    if kind == "column_a":
        a[1] = a[1].clone()
        a[1][17] = 20
    elif kind == "column_b_negative":
        b[1] = b[1].clone()
        b[1][3] = -1
    elif kind == "value_nan":
        a[2] = a[2].clone()
        a[2][40] = float("nan")
    elif kind == "value_inf_b":
        b[2] = b[2].clone()
        b[2][7] = float("inf")
    elif kind == "indptr_decreasing":
        a[0] = a[0].clone()
        a[0][50] = a[0][49] - 1
    elif kind == "indptr_past_nnz":
        b[0] = b[0].clone()
        b[0][-1] = b[1].numel() + 1000
    elif kind == "indptr_negative":
        a[0] = a[0].clone()
        a[0][0] = -4
    return A, B, tuple(a), tuple(b)


@pytest.mark.parametrize("kind,code", [("column_a", 1), ("column_b_negative", 1), ("value_nan", 2), ("value_inf_b", 2), ("indptr_decreasing", 3),
                                       ("indptr_past_nnz", 3), ("indptr_negative", 3)])
def test_error_word(kind, code):
    """Bad input is reported, never followed out of bounds (the kernels check every index they use); the outputs are void, the call
    returns, and the next call on good input is right."""
    from saev_amd import engine

    A, B, a, b = _broken(kind)
    res = engine.coactivation_match(a, b, n_rows=100, n_latents_a=20, n_latents_b=30, top_m=2)
    assert int(res._err.item()) == code
    with pytest.raises(ValueError, match="found on the device"):
        res.index
    with pytest.raises(ValueError):
        res.support_a
    good = _run(A, B, top_m=2)
    _assert_equal(good, R.match(A, B, top_m=2))


def test_largest_error_code_wins():
    from saev_amd import engine

    A, B, a, _ = _broken("column_a")
    _, _, _, b = _broken("indptr_past_nnz")
    res = engine.coactivation_match(a, b, n_rows=100, n_latents_a=20, n_latents_b=30)
    assert int(res._err.item()) == 3


def test_c_entry_writes_padding_and_supports_without_a_read_back():
    """The C entry itself, with a workspace exactly as large as the size function says and poisoned outputs."""
    from saev_amd import _lib
    from saev_amd.engine import _ptr, _stream

    lib = _lib.load()
    c = CASES["top_m_8"]
    a, b = _dev(c.A), _dev(c.B)
    n, sa, sb = c.A.shape[0], c.A.shape[1], c.B.shape[1]
    need = lib.saev_coactivation_workspace_bytes(n, sa, sb, a[1].numel(), b[1].numel())
    ws = torch.full((need,), 0xAB, device=DEV, dtype=torch.uint8)
    out = [torch.full(shape, -77, device=DEV, dtype=torch.int32) for shape in ((sa,), (sb,), (sa, 8), (sa, 8), (1,))]
    rc = lib.saev_coactivation(*map(_ptr, a), a[1].numel(), sa, *map(_ptr, b), b[1].numel(), sb, n, 0.0, 0.0, 0, 8, *map(_ptr, out), _ptr(ws), need,
                               _stream())
    assert rc == 0, lib.saev_last_error(None)
    want = _expected("top_m_8")
    for got, k in zip(out, ("support_a", "support_b", "index", "intersection")):
        K._eq(got.cpu().numpy(), want[k])
    assert out[4].item() == 0
    assert lib.saev_coactivation(*map(_ptr, a), a[1].numel(), sa, *map(_ptr, b), b[1].numel(), sb, n, 0.0, 0.0, 0, 8, *map(_ptr, out), _ptr(ws), need - 1,
                                 _stream()) == -1


# ---------------------------------------------------------------- alignment ----------------------------------------------------------

N_IMG, TPI, S_A, S_B = 64, 4, 96, 128


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """Two run directories with token_acts.npz of 64 images x 4 tokens: run b's first 96 latents are run a's, permuted, with a tenth of
    the entries dropped; its other 32 are noise."""
    root = tmp_path_factory.mktemp("runs")
    rng = np.random.default_rng(31)
    ta_a = K.random_csr(rng, N_IMG * TPI, S_A, 6)
    dense = ta_a.toarray()
    dense[rng.random(dense.shape) < 0.1] = 0
    ta_b = scipy.sparse.csr_matrix(np.concatenate([dense[:, rng.permutation(S_A)], K.random_csr(rng, N_IMG * TPI, S_B - S_A, 2).toarray()], axis=1),
                                   dtype=np.float32)
    for run, ta in (("run_a", ta_a), ("run_b", ta_b)):
        d = root / run / "inference" / "shard0"
        d.mkdir(parents=True)
        scipy.sparse.save_npz(str(d / "token_acts.npz"), ta)
    return root, ta_a, ta_b


def _pooled(ta):
    """Max over each image's tokens, clamped at 0 (the values are positive here, so the clamp changes nothing)."""
    d = ta.toarray().reshape(N_IMG, TPI, -1).max(axis=1)
    return scipy.sparse.csr_matrix(np.maximum(d, 0.0).astype(np.float32))


def _top_k(m, k):
    """Per latent its k highest rows (value descending, row ascending: csr_topk's rule), as a CSR matrix."""
    d = m.toarray()
    out = np.zeros_like(d)
    for j in range(d.shape[1]):
        rows = np.flatnonzero(d[:, j] > 0)
        best = rows[np.argsort(-d[rows, j], kind="stable")][:k]
        out[best, j] = d[best, j]
    return scipy.sparse.csr_matrix(out)


SETS = {"token": lambda ta: ta, "image": _pooled, "token_top5": lambda ta: _top_k(ta, 5), "image_top5": lambda ta: _top_k(_pooled(ta), 5)}


@pytest.mark.parametrize("self_mode", [False, True], ids=["pair", "self"])
@pytest.mark.parametrize("kind", list(SETS))
def test_alignment_worker(runs, kind, self_mode):
    from saev_amd import alignment

    root, ta_a, ta_b = runs
    cfg = alignment.Config(run_a=root / "run_a", run_b=None if self_mode else root / "run_b", shards="shard0", level=kind.split("_")[0],
                           tokens_per_image=TPI, top_k=5 if kind.endswith("top5") else None, top_m=3, device=DEV)
    fpath = alignment.worker_fn(cfg)
    assert fpath == root / "run_a" / "inference" / "shard0" / ("latent_alignment__self.npz" if self_mode else "latent_alignment__run_b.npz")
    e = R.match(SETS[kind](ta_a), None if self_mode else SETS[kind](ta_b), top_m=3)
    want = alignment.arrays_of(e["index"], e["intersection"], e["support_a"], e["support_b"], e["reverse_index"])
    with np.load(fpath) as z:
        assert tuple(z.files) == alignment.KEYS
        for k in alignment.KEYS:
            assert z[k].dtype == want[k].dtype and np.array_equal(z[k], want[k], equal_nan=True), k
        if not self_mode and kind == "token":
            assert z["mutual"].mean() > 0.9  # the planted permutation is found


def test_tool_main(runs, capsys):
    root, ta_a, ta_b = runs
    spec = importlib.util.spec_from_file_location("align_latents", ROOT / "tools" / "align_latents.py")
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    out = tool.main([str(root / "run_a"), str(root / "run_b"), "--shards", "shard0", "--level", "image", "--tokens-per-image", str(TPI), "--top-m", "2",
                     "--device", DEV])
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == json.loads(json.dumps(out))
    e = R.match(_pooled(ta_a), _pooled(ta_b), top_m=2)
    assert out["mode"] == "pair" and out["n_latents_a"] == S_A and out["n_latents_b"] == S_B
    assert out["mutual_fraction"] == float(e["mutual"].mean()) and out["matched_fraction"] == float((e["index"][:, 0] >= 0).mean())
    best = int(np.argmax(np.where(e["index"][:, 0] >= 0, e["jaccard"][:, 0], -1.0)))
    assert out["closest"][0] == [best, int(e["index"][best, 0]), float(e["jaccard"][best, 0]), int(e["intersection"][best, 0])]
    assert len(out["jaccard_quantiles"]) == 7 and out["jaccard_quantiles"][-1] == float(np.nanmax(e["jaccard"][:, 0]))
    out = tool.main([str(root / "run_a"), "--shards", "shard0", "--measure", "containment", "--device", DEV])
    assert out["mode"] == "self" and out["out"].endswith("latent_alignment__self.npz")
