"""The per-latent top-k on the MI355X (include/saev_amd.h: LATENT TOP-K): fixture G21, recorded from the
reference's ``csr_topk(axis=0)``, and the numpy restatement of the contract (tests/latent_topk_restatement.py, itself checked
against G21 on the CPU) -- every comparison exact: values bit for bit, rows and counts equal."""

import numpy as np
import pytest
import scipy.sparse
import torch

import csr_cases
import sae_ref as R
from conftest import GOLDEN, load_golden
from latent_topk_restatement import restate, restate_csr, restate_padded

pytestmark = [pytest.mark.gpu, pytest.mark.encoder_modes("f16r")]

BIG = 2**33  # a row_base whose row ids need more than 32 bits
FOUR = np.array([-1.5, 0.25, 2.0, 7.0], dtype=np.float32)


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def lists(d_sae, k):
    from saev_amd.engine import LatentTopK

    return LatentTopK(d_sae, k, "cuda")


def same(got, want):
    """got: LatentTopKHost or NumpyTopK (+ counts); want: (values, indices, counts) of the restatement."""
    values = got.values.numpy() if isinstance(got.values, torch.Tensor) else got.values
    indices = got.indices.numpy() if isinstance(got.indices, torch.Tensor) else got.indices
    assert values.dtype == np.float32 and indices.dtype == np.int64 and values.shape == want[0].shape
    np.testing.assert_array_equal(values.view(np.int32), want[0].view(np.int32))  # bit for bit (+0 padding, infinities)
    np.testing.assert_array_equal(indices, want[1])
    if hasattr(got, "counts"):
        np.testing.assert_array_equal(got.counts.numpy(), want[2])


def bits(acc):
    return acc.top_val.view(torch.int32).clone(), acc.top_row.clone(), acc.top_cnt.clone()


def g21():
    with np.load(GOLDEN / "g21_csr_topk.npz") as z:
        return {name: z[name] for name in z.files}


@pytest.mark.parametrize("k", [1, 5, 20])
@pytest.mark.parametrize("case", ["a", "b", "ties"])
def test_fixture_g21_the_references_csr_topk(case, k):
    from saev_amd import helpers

    g = g21()
    n_rows, n_cols = g[f"{case}_shape"].tolist()
    indptr, indices, data = g[f"{case}_indptr"], g[f"{case}_indices"], g[f"{case}_data"]
    acc = lists(n_cols, k)
    acc.add_csr(dev(indptr, torch.int64), dev(indices, torch.int32), dev(data), row_base=0)
    got = acc.read()
    top = helpers.csr_topk(scipy.sparse.csr_array((data, indices, indptr), shape=(n_rows, n_cols)), k=k, axis=0)
    for values, rows in ((got.values.numpy(), got.indices.numpy()), (top.values, top.indices)):
        assert values.dtype == np.float32 and rows.dtype == np.int64
        np.testing.assert_array_equal(values.view(np.int32), g[f"{case}_k{k}_values"].view(np.int32))  # tolerance 0
        if case != "ties":  # among equal values the reference's rows follow no fixed rule
            np.testing.assert_array_equal(rows, g[f"{case}_k{k}_indices"])
    same(got, restate_csr(indptr, indices, data, n_cols, k))


def scenario(k, S, values, seed=0, n=3000, cap=5):
    """Padded rows with one latent (0) in every row, a latent without entries, one with k - 1 entries, latents outside [0, S),
    zeros of both signs, infinities, negatives, a keep mask and row counts from 0 to above cap.  At most one entry per
    (row, latent)."""
    rng = np.random.default_rng(seed + 1000 * k + S)
    pool = np.concatenate([[-2, -1], np.arange(1, S + 2)]).astype(np.int32)  # never 0: slot 0 holds it
    idx = np.empty((n, cap), dtype=np.int32)
    idx[:, 0] = 0
    if pool.size <= 64:
        idx[:, 1:] = pool[np.argsort(rng.random((n, pool.size)), axis=1)[:, :cap - 1]]
    else:  # distinct latents per row: a random start and distinct strides through the pool
        start = rng.integers(0, pool.size, n)
        idx[:, 1:] = pool[(start[:, None] + np.arange(cap - 1)[None, :] * rng.integers(1, 50, n)[:, None]) % pool.size]
    if values == "four":
        val = rng.choice(FOUR, size=(n, cap))
    else:
        val = rng.standard_normal((n, cap)).astype(np.float32)
    special = rng.random((n, cap))
    val[special < 0.02] = np.inf
    val[(special >= 0.02) & (special < 0.04)] = -np.inf
    val[(special >= 0.04) & (special < 0.07)] = 0.0
    val[(special >= 0.07) & (special < 0.10)] = -0.0
    keep = rng.random(n) < 0.8
    row_nnz = rng.integers(0, cap + 3, n).astype(np.int32)
    if S >= 60:
        empty, few = S - 1, S - 2
        idx[np.isin(idx, (empty, few))] = -1
        idx[:k - 1, 1] = few  # exactly k - 1 entries, all of them kept, counted and nonzero
        val[:k - 1, 1] = FOUR[rng.integers(0, 4, k - 1)]
        keep[:k - 1] = True
        row_nnz[:k - 1] = np.maximum(row_nnz[:k - 1], 2)
    for r in range(0, n, 97):  # canonical: no latent twice in a row
        inside = idx[r][(idx[r] >= 0) & (idx[r] < S)]
        assert np.unique(inside).size == inside.size
    return idx, val.astype(np.float32), row_nnz, keep


@pytest.mark.parametrize("values", ["four", "normal"])
@pytest.mark.parametrize("S", [1, 60, 1004])
@pytest.mark.parametrize("k", [1, 5, 64])
def test_streamed_updates_equal_the_restatement(k, S, values):
    idx, val, row_nnz, keep = scenario(k, S, values)
    n = idx.shape[0]
    want = restate_padded(idx, val, S, k, row_nnz=row_nnz, keep=keep, row_base=BIG)
    assert want[2][0] == k  # the latent of every row filled its list from thousands of candidates
    if S >= 60:
        assert want[2][S - 1] == 0 and want[2][S - 2] == k - 1
    if values == "four":  # ties straddle the cut: the first entry left out of latent 0's list equals the last one in it
        assert restate_padded(idx, val, S, k + 1, row_nnz=row_nnz, keep=keep, row_base=BIG)[0][k, 0] == want[0][k - 1, 0]
    acc = lists(S, k)
    cuts = [0, 1, 130, 131, 700, 1900, 1964, 2999, n]
    for lo, hi in reversed(list(zip(cuts[:-1], cuts[1:]))):  # descending row_base: the tie rule does not depend on arrival
        acc.add(dev(idx[lo:hi]), dev(val[lo:hi]), dev(row_nnz[lo:hi]), dev(keep[lo:hi]), row_base=BIG + lo)
        acc.add(dev(idx[:0]), dev(val[:0]), dev(row_nnz[:0]), dev(keep[:0]), row_base=BIG + lo)  # n = 0 writes nothing
    same(acc.read(), want)
    assert int(acc.read().indices.max()) >= BIG


@pytest.mark.parametrize("S", [1025, 2100, 5000])
def test_more_latents_than_the_scan_has_threads(S):
    """Above 1 024 latents the scan takes more than one round (2, 3 and 5 here, the last one partly filled)."""
    k = 3
    idx, val, row_nnz, keep = scenario(k, S, "four", n=1200)
    acc = lists(S, k)
    for lo, hi in ((600, 1200), (0, 600)):
        acc.add(dev(idx[lo:hi]), dev(val[lo:hi]), dev(row_nnz[lo:hi]), dev(keep[lo:hi]), row_base=lo)
    same(acc.read(), restate_padded(idx, val, S, k, row_nnz=row_nnz, keep=keep))


@pytest.mark.parametrize("shift", [0, 333])
def test_csr_rows_across_empty_rows_and_a_block_that_does_not_start_at_0(shift):
    """The row of a stored entry where indptr repeats (empty rows first, last and three in a run) and where it starts at ``shift``:
    with k = 64 every entry of a latent is in its list, so top_row names the row of each."""
    d = csr_cases.empty_rows_block(shift)
    acc = lists(d["s"], 64)
    acc.add_csr(dev(d["indptr"]), dev(d["indices"]), dev(d["data"]), row_base=0)
    got = acc.read()
    order = csr_cases.by_latent(d, by_value=True)
    counts = np.bincount(d["cols"], minlength=d["s"])
    np.testing.assert_array_equal(got.counts.numpy(), counts)
    starts = np.concatenate([[0], np.cumsum(counts)])
    for j in range(d["s"]):
        mine = order[starts[j]:starts[j + 1]]
        np.testing.assert_array_equal(got.indices.numpy()[:counts[j], j], d["rows"][mine])
        np.testing.assert_array_equal(got.values.numpy()[:counts[j], j].view(np.int32), d["vals"][mine].view(np.int32))


def test_eight_updates_one_update_and_the_csr_form_give_the_same_bits():
    k, S = 5, 60
    idx, val, row_nnz, keep = scenario(k, S, "four", seed=3)
    n, cap = idx.shape
    one = lists(S, k)
    one.add(dev(idx), dev(val), dev(row_nnz), dev(keep), row_base=7)
    again = lists(S, k)
    again.add(dev(idx), dev(val), dev(row_nnz), dev(keep), row_base=7)
    eight = lists(S, k)
    for part in np.array_split(np.arange(n), 8):
        lo, hi = int(part[0]), int(part[-1]) + 1
        eight.add(dev(idx[lo:hi]), dev(val[lo:hi]), dev(row_nnz[lo:hi]), dev(keep[lo:hi]), row_base=7 + lo)
    # the same entries as CSR: what the first min(row_nnz, cap) slots of a row hold (the mask stays an argument)
    on = np.arange(cap)[None, :] < row_nnz[:, None]
    indptr = np.concatenate([[0], np.cumsum(on.sum(axis=1))]).astype(np.int64)
    csr = lists(S, k)
    csr.add_csr(dev(indptr), dev(idx[on]), dev(val[on]), dev(keep), row_base=7)
    ref = bits(one)
    for other in (again, eight, csr):
        for a, b in zip(ref, bits(other)):
            assert torch.equal(a, b)
    same(one.read(), restate_padded(idx, val, S, k, row_nnz=row_nnz, keep=keep, row_base=7))
    # unwritten slots keep the caller's zeros
    cnt = one.top_cnt.cpu().long()
    past = torch.arange(k)[None, :] >= cnt[:, None]
    assert (one.top_val.cpu()[past].view(torch.int32) == 0).all() and (one.top_row.cpu()[past] == 0).all()


def test_a_batch_below_every_full_list_leaves_the_state_identical():
    k, S, n = 5, 60, 64
    rng = np.random.default_rng(11)
    idx = np.tile(np.arange(S, dtype=np.int32), (n, 1))
    high = (10 + rng.random((n, S))).astype(np.float32)
    acc = lists(S, k)
    acc.add(dev(idx), dev(high), row_base=0)
    assert (acc.top_cnt == k).all()
    before = bits(acc)
    low = rng.random((n, S)).astype(np.float32) - 0.5
    acc.add(dev(idx), dev(low), row_base=n)
    for a, b in zip(before, bits(acc)):
        assert torch.equal(a, b)
    # equal to the last value but in a later row: passes the filter, loses the merge
    last = acc.top_val[:, k - 1].cpu().numpy()
    acc.add(dev(idx[:1]), dev(last[None, :]), row_base=2 * n)
    for a, b in zip(before, bits(acc)):
        assert torch.equal(a, b)
    # ... and in an earlier row it takes the place
    low_row = lists(S, k)
    low_row.add(dev(idx), dev(high), row_base=10)
    low_row.add(dev(idx[:1]), dev(last[None, :]), row_base=0)
    both_idx, both_val = np.concatenate([idx, idx[:1]]), np.concatenate([high, last[None, :]])
    rows = np.concatenate([np.arange(n) + 10, [0]])
    same(low_row.read(), restate(np.repeat(rows, S), both_idx.reshape(-1), both_val.reshape(-1), S, k))
    assert (low_row.top_row[:, k - 1] == 0).all()


def _params(d, s, k, seed):
    gen = torch.Generator().manual_seed(seed)
    params = R.init_params(R.RefConfig(d_model=d, d_sae=s, top_k=k), gen)
    params["b_enc"] = 0.01 * torch.randn(s, generator=gen)
    return params, gen


def test_engine_feeds_the_codes_of_a_topk_forward():
    from saev_amd.engine import EngineConfig, SaeEngine

    d, s, k, b = 64, 512, 8, 96
    params, gen = _params(d, s, k, 0)
    eng = SaeEngine(EngineConfig(d_model=d, d_sae=s, top_k=k, max_batch=b), "cuda")
    eng.load_params(params)
    acc = lists(s, 6)
    all_idx, all_val, all_keep = [], [], []
    for step in range(3):
        x = torch.randn(b, d, generator=gen).cuda()
        keep = None if step == 1 else (torch.rand(b, generator=gen) < 0.7).cuda()
        eng.step_forward(x, training=False)
        eng.add_latent_topk(acc, keep, row_base=step * b)
        idx, val, _ = eng.last_codes(b, x_hat=False)
        all_idx.append(idx.cpu().numpy()); all_val.append(val.cpu().numpy())
        all_keep.append(np.ones(b, dtype=bool) if keep is None else keep.cpu().numpy())
    want = restate_padded(np.concatenate(all_idx), np.concatenate(all_val), s, 6, keep=np.concatenate(all_keep))
    assert want[2].max() == 6 and want[2].min() < 6
    same(acc.read(), want)
    eng.train_step(x, 1e-3)
    with pytest.raises(RuntimeError, match="no step_forward"):
        eng.add_latent_topk(acc, row_base=0)
    eng.step_forward(x, training=False)
    with pytest.raises(RuntimeError, match="another shape"):
        eng.add_latent_topk(lists(s + 1, 6), row_base=0)


def test_relu_and_batch_topk_rows():
    from saev_amd.engine import EngineConfig, SaeEngine

    d, s, k, b = 64, 512, 8, 96
    params, gen = _params(d, s, k, 1)
    x = torch.randn(2 * b, d, generator=gen).cuda()
    relu = SaeEngine(EngineConfig(d_model=d, d_sae=s, k_aux=0, max_batch=b, activation="relu"), "cuda", with_optim=False)
    relu.load_params(params)
    btk = SaeEngine(EngineConfig(d_model=d, d_sae=s, top_k=k, k_aux=0, max_batch=b, activation="batch_topk"), "cuda")
    btk.load_params(params)
    for eng, encode in ((relu, relu.encode_relu), (btk, lambda xb: btk.encode_batch_topk(xb, training=True))):
        acc = lists(s, 7)
        entries = []
        for part in range(2):
            idx, val, row_nnz = encode(x[part * b:(part + 1) * b])
            acc.add(idx, val, row_nnz, row_base=part * b)
            dense = eng.scatter_rows(idx, val, row_nnz).cpu().numpy()  # the scattered dense codes of the batch
            r, c = np.nonzero(dense)
            entries.append((r + part * b, c, dense[r, c]))
        want = restate(*(np.concatenate([e[i] for e in entries]) for i in range(3)), s, 7)
        assert want[2].sum() > 0
        same(acc.read(), want)
    # a BatchTopK step: the context's rows, padded with idx = -1
    acc = lists(s, 7)
    btk.step_forward(x[:b], training=True)
    btk.add_latent_topk(acc, row_base=5)
    idx, val, _, row_nnz = btk.last_codes(b, x_hat=False, row_nnz=True)
    same(acc.read(), restate_padded(idx.cpu().numpy(), val.cpu().numpy(), s, 7, row_nnz=row_nnz.cpu().numpy(), row_base=5))


def test_helpers_csr_topk_does_not_depend_on_the_blocks(monkeypatch):
    from saev_amd import helpers
    from saev_amd.engine import LatentTopK

    rng = np.random.default_rng(2)
    dense = rng.choice(np.concatenate([FOUR, np.zeros(12, np.float32)]), size=(500, 37)).astype(np.float32)
    dense[:, 4] = 0
    dense[200:300] = 0  # blocks without an entry
    arr = scipy.sparse.csr_array(dense)
    want = restate_csr(arr.indptr, arr.indices, arr.data, 37, 9)
    calls = []
    orig = LatentTopK.add_csr
    monkeypatch.setattr(LatentTopK, "add_csr", lambda self, *a, **kw: (calls.append(kw["row_base"]), orig(self, *a, **kw))[1])
    monkeypatch.setattr(helpers, "_BLOCK_ENTRIES", 1)  # blocks of batch_size rows
    small = helpers.csr_topk(arr, k=9, batch_size=7)
    n_small = len(calls)
    large = helpers.csr_topk(arr, k=9, batch_size=1024)
    assert n_small > 50 and len(calls) == n_small + 1
    for got in (small, large, helpers.csr_topk(scipy.sparse.csr_matrix(arr), k=9, axis=0)):
        assert isinstance(got, helpers.NumpyTopK)
        same(got, want)
    f64 = helpers.csr_topk(arr.astype(np.float64), k=9)
    assert f64.values.dtype == np.float64
    np.testing.assert_array_equal(f64.values, want[0].astype(np.float64))
    with pytest.raises(ValueError, match="float32"):
        helpers.csr_topk(scipy.sparse.csr_array(np.array([[0.1, 0.0], [0.0, 1.0]])), k=1)


def _run_dir(tmp_path, tag):
    from saev_amd import disk, nn
    from test_inference_host_cpu import write_cache

    g = load_golden(tag)
    d = write_cache(tmp_path, g)
    runs_root = tmp_path / "saev" / "runs"
    runs_root.mkdir(parents=True)
    run = disk.Run.new("gpu000lt", train_shards_dir=d, val_shards_dir=d, runs_root=runs_root)
    if "ckpt" in g:
        run.ckpt.parent.mkdir(parents=True, exist_ok=True)
        run.ckpt.write_bytes(g["ckpt"].numpy().tobytes())
    else:
        S, D = g["p_W_dec"].shape
        sae = nn.SparseAutoencoder(nn.SparseAutoencoderConfig(
            d_model=D, d_sae=S, activation=nn.modeling.TopK(top_k=int(g["k"]), aux=nn.modeling.AuxK(k_aux=int(g["k_aux"])))))
        with torch.no_grad():
            for name in R.PARAM_ORDER:
                getattr(sae, name).copy_(g["p_" + name])
        nn.dump(run.ckpt, sae)
    return g, d, run


def _snapshot(out):
    return {p.name: p.read_bytes() for p in sorted(out.iterdir())}


def _contents(out):
    """What the artifacts hold (a rewritten .npz differs in its archive's time stamps): arrays as bytes, metrics as text."""
    got = {}
    for p in sorted(out.iterdir()):
        if p.name == "token_acts.npz":
            csr = scipy.sparse.load_npz(p)
            got[p.name] = (csr.shape, csr.indptr.tobytes(), csr.indices.tobytes(), csr.data.tobytes())
        elif p.suffix == ".pt" and p.name != "top_tokens.pt":
            t = torch.load(p)
            got[p.name] = (t.dtype, tuple(t.shape), t.numpy().tobytes())
        elif p.name == "metrics.json":
            got[p.name] = p.read_text()
    return got


@pytest.mark.parametrize("tag", ["g14_inference_plain", "g14_inference_labels", "g19_inference_relu_labels", "g20_inference_batch_topk_plain"])
def test_inference_writes_top_tokens(tmp_path, tag):
    from saev_amd.data import Metadata, OrderedConfig
    from saev_amd.framework import inference

    g, d, run = _run_dir(tmp_path, tag)
    out = run.inference / Metadata.load(d).hash
    cfg = inference.Config(run=run.run_dir, data=OrderedConfig(shards=d, layer=11, batch_size=int(g["batch_size"])),
                           n_dists=int(g["n_dists"]), ignore_labels=g["ignore_labels"].tolist())
    # top_k_tokens = 0: the pass as it was
    inference.worker_fn(cfg, top_k_tokens=0)
    assert sorted(p.name for p in out.iterdir()) == ["config.json", "distributions.pt", "mean_values.pt", "metrics.json", "sparsity.pt",
                                                      "token_acts.npz"]
    plain = _contents(out)
    assert len(plain) == 5

    k = 8
    forced = inference.Config(run=cfg.run, data=cfg.data, n_dists=cfg.n_dists, ignore_labels=cfg.ignore_labels, force_recompute=True)
    inference.worker_fn(forced, top_k_tokens=k)
    with_lists = _snapshot(out)
    assert sorted(with_lists) == sorted(list(plain) + ["config.json", "top_tokens.pt"])
    assert _contents(out) == plain  # every existing artifact holds what it held
    csr = scipy.sparse.load_npz(out / "token_acts.npz")
    want = restate_csr(csr.indptr, csr.indices, csr.data, csr.shape[1], k)
    top = torch.load(out / "top_tokens.pt")
    assert sorted(top) == ["counts", "indices", "values"]
    assert top["values"].dtype == torch.float32 and top["indices"].dtype == torch.int64 and top["counts"].dtype == torch.int64
    assert tuple(top["values"].shape) == (k, csr.shape[1]) and want[2].max() == k
    np.testing.assert_array_equal(top["values"].numpy().view(np.int32), want[0].view(np.int32))
    np.testing.assert_array_equal(top["indices"].numpy(), want[1])
    np.testing.assert_array_equal(top["counts"].numpy(), want[2])

    # the pass is up to date and only the lists are missing: rebuilt from token_acts.npz, identically
    (out / "top_tokens.pt").unlink()
    assert not inference.need_compute(cfg)[0]
    inference.worker_fn(cfg, top_k_tokens=k)
    again = torch.load(out / "top_tokens.pt")
    for name in ("values", "indices", "counts"):
        assert again[name].dtype == top[name].dtype and torch.equal(again[name], top[name]), name
    rest = _snapshot(out)
    rest.pop("top_tokens.pt")
    with_lists.pop("top_tokens.pt")
    assert rest == with_lists

    # lists kept for another k are not handed out as this k's: rebuilt from the artifact, the file of the right k left alone
    inference.worker_fn(cfg, top_k_tokens=3)
    three = torch.load(out / "top_tokens.pt")
    assert tuple(three["values"].shape) == (3, csr.shape[1])
    assert torch.equal(three["values"], top["values"][:3]) and torch.equal(three["indices"], top["indices"][:3])
    assert torch.equal(three["counts"], top["counts"].clamp(max=3))
    stamp = (out / "top_tokens.pt").stat().st_mtime_ns
    inference.worker_fn(cfg, top_k_tokens=3)
    assert (out / "top_tokens.pt").stat().st_mtime_ns == stamp
    # a pass that rewrites token_acts.npz without lists does not leave the old ones beside it
    inference.worker_fn(forced, top_k_tokens=0)
    assert not (out / "top_tokens.pt").exists()
