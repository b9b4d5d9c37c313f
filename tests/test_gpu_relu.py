"""ReLU SAE forward on the MI355X (needs -m gpu): the sparse ReLU encoder against fp64, the decode of variable-length rows,
the module API of a reference-written checkpoint against the reference's own outputs (fixtures G19_relu_forward_*), and
framework.inference.worker_fn against the reference's artifacts (fixtures G19_inference_relu_*; tools/gen_relu_golden.py)."""

import io
import json
import math

import numpy as np
import pytest
import scipy.sparse
import torch

from conftest import load_golden
from test_inference_host_cpu import write_cache

pytestmark = pytest.mark.gpu


def ckpt_params(g) -> dict:
    """The four tensors of the reference-written checkpoint a fixture carries (header line, then torch.save)."""
    raw = g["ckpt"].numpy().tobytes()
    return torch.load(io.BytesIO(raw[raw.index(b"\n") + 1 :]), weights_only=True, map_location="cpu")


def relu_engine(d, s, b, params=None):
    from saev_amd.engine import EngineConfig, SaeEngine

    eng = SaeEngine(EngineConfig(d_model=d, d_sae=s, k_aux=0, max_batch=b, activation="relu"), "cuda", with_optim=False)
    if params is not None:
        eng.load_params(params)
    return eng


def check_rows(eng, x, idx, val, row_nnz, slab=512):
    """Every row against fp64: ascending latents, values = the pre-activations, membership = {h64 > 0} except where |h64| is
    within tol_b = 8 * 2^-24 * ||x_b|| * max_s ||W_enc[:, s]|| + 2^-23 |b_enc|_max (the d-term fp32 dot-product bound of
    test_gpu_fullsize.py plus the bias rounding), and row_nnz between the counts above +tol and above -tol.  Returns the
    largest row count."""
    n, cap = idx.shape
    S = eng.cfg.d_sae
    W, be = eng.view("W_enc").double(), eng.view("b_enc").double()
    wmax = W.norm(dim=0).max().item()
    nnz = row_nnz.long()
    assert nnz.min() >= 0 and nnz.max() <= cap
    slot = torch.arange(cap, device=idx.device)[None, :]
    for lo in range(0, n, slab):
        rows = slice(lo, min(n, lo + slab))
        m = slot < nnz[rows, None]
        ii, vv = idx[rows].long(), val[rows].double()
        assert ((ii >= 0) & (ii < S) | ~m).all()
        # ascending within the valid entries
        asc = (ii[:, 1:] > ii[:, :-1]) | ~m[:, 1:]
        assert asc.all(), "latents of a row are not in ascending order"
        h = x[rows].double() @ W + be
        tol = (8.0 * 2.0 ** -24 * x[rows].double().norm(dim=1) * wmax + 2.0 ** -23 * be.abs().max()).clamp_min(1e-30)
        hs = h.gather(1, ii.clamp(0, S - 1))
        err = torch.where(m, (hs - vv).abs(), 0.0).amax(dim=1)  # (slots past row_nnz are unspecified: NaN is fine there)
        assert (err <= tol).all(), f"rows {lo}..: value error {err.max().item():.3e}"
        assert ((vv > 0) | ~m).all(), "an emitted value is not positive"
        got = torch.zeros_like(h, dtype=torch.bool)
        got.scatter_(1, torch.where(m, ii, 0), m)  # (index 0 of masked-out slots: scattered with False)
        got[:, 0] = (ii == 0).logical_and(m).any(dim=1)
        sure_pos, maybe_pos = h > tol[:, None], h > -tol[:, None]
        assert (got | ~sure_pos).all(), f"rows {lo}..: a clearly positive latent is missing"
        assert (~got | maybe_pos).all(), f"rows {lo}..: a clearly negative latent was emitted"
        assert (nnz[rows] == got.sum(dim=1)).all()
        del h, got
    return int(nnz.max())


def test_encoder_sparse_fixture_with_an_empty_row(encoder_mode):
    g = load_golden("g19_relu_forward_sparse")
    params = ckpt_params(g)
    S, D = params["W_dec"].shape
    eng = relu_engine(D, S, 128, params)
    x = g["x"].cuda()
    idx, val, nnz = eng.encode_relu(x)
    assert x.shape[0] % 32 != 0
    assert eng.relu_second_launches == 0
    assert int(nnz[int(g["zero_row"])]) == 0  # the all-zero input row: h = b_enc < 0 everywhere
    assert 0 < check_rows(eng, x, idx, val, nnz) < eng.relu_row_cap
    # the reference's f_x (first rows), through the variable-length scatter
    r = g["f_x"].shape[0]
    torch.testing.assert_close(eng.scatter_rows(idx, val, nnz)[:r].cpu(), g["f_x"], rtol=1e-5, atol=1e-5)
    # one row alone, and a tiny capacity that every other row overflows: the same rows
    i1, v1, n1 = eng.encode_relu(x[:1].contiguous())
    assert int(n1[0]) == int(nnz[0])
    torch.testing.assert_close(v1[0, : int(n1[0])], val[0, : int(nnz[0])], rtol=0, atol=0)
    i2, v2, n2 = eng.encode_relu(x, row_cap=4)
    assert eng.relu_second_launches == 1 and i2.shape[1] == int(nnz.max())
    torch.testing.assert_close(n2, nnz, rtol=0, atol=0)
    m = torch.arange(i2.shape[1], device="cuda")[None, :] < n2[:, None]
    torch.testing.assert_close(torch.where(m, i2, -1), torch.where(m, idx[:, : i2.shape[1]], -1), rtol=0, atol=0)


def test_encoder_dense_fixture_takes_the_overflow_route(encoder_mode):
    g = load_golden("g19_relu_forward_dense")
    params = ckpt_params(g)
    S, D = params["W_dec"].shape
    eng = relu_engine(D, S, 128, params)
    x = g["x"].cuda()
    cap0 = eng.relu_row_cap
    idx, val, nnz = eng.encode_relu(x)
    assert int(nnz.max()) > cap0, "this fixture must overflow the default capacity"
    assert eng.relu_second_launches == 1 and idx.shape[1] == int(nnz.max())
    assert eng.relu_row_cap >= int(nnz.max())  # the next call starts wide enough
    check_rows(eng, x, idx, val, nnz)
    eng.encode_relu(x)
    assert eng.relu_second_launches == 1


def test_encoder_at_configs1_shape(encoder_mode):
    """configs[1]: d_model 1024, d_sae 32768, 16 384 rows, a sparse active set (tens of positives per row)."""
    d, s, b = 1024, 32768, 16384
    eng = relu_engine(d, s, b)
    gen = torch.Generator(device="cuda").manual_seed(19)
    W = (torch.rand(s, d, device="cuda", generator=gen) * 2 - 1) * math.sqrt(6.0 / d)
    W /= W.norm(dim=1, keepdim=True)
    eng.view("W_dec").copy_(W)
    eng.view("W_enc").copy_(W.t() + 0.01 * torch.randn(d, s, device="cuda", generator=gen))
    x = torch.randn(b, d, device="cuda", generator=gen) + torch.randn(d, device="cuda", generator=gen)
    h_sample = (x[:64] @ eng.view("W_enc")).flatten()
    thr = torch.quantile(h_sample[:: 2], 0.999).item()
    eng.view("b_enc").copy_(-thr + 0.05 * torch.randn(s, device="cuda", generator=gen))
    eng.params_touched()
    idx, val, nnz = eng.encode_relu(x)
    top = check_rows(eng, x, idx, val, nnz)
    mean = nnz.float().mean().item()
    print(f"configs[1] ReLU: mean {mean:.1f} positives per row, max {top}, second launches {eng.relu_second_launches}")
    assert 5 < mean < 200
    # the decode of these rows against the dense-code decode of the same codes
    rows = torch.randperm(b, device="cuda")[:256]
    xh = eng.decode_rows(idx[rows], val[rows], nnz[rows])[:, 0].double()
    f = eng.scatter_rows(idx[rows], val[rows], nnz[rows]).double()
    want = f @ eng.view("W_dec").double() + eng.view("b_dec").double()
    torch.testing.assert_close(xh, want, rtol=1e-4, atol=1e-4)


@pytest.mark.encoder_modes("f32")
@pytest.mark.parametrize("prefixes", [None, (100, 700, 2048), (1, 2, 3, 2048)])
def test_decode_rows_against_fp64(prefixes, encoder_mode):
    d, s, n, cap = 256, 2048, 77, 300
    gen = torch.Generator().manual_seed(20)
    eng = relu_engine(d, s, n)
    eng.view("W_dec").copy_(torch.randn(s, d, generator=gen).cuda())
    eng.view("b_dec").copy_(torch.randn(d, generator=gen).cuda())
    nnz = torch.randint(0, cap + 1, (n,), generator=gen, dtype=torch.int32)
    nnz[[0, 5, 76]] = 0
    nnz[3] = cap
    idx = torch.full((n, cap), s + 1000, dtype=torch.int32)  # padding: out of range and never read
    val = torch.full((n, cap), float("nan"))
    for r in range(n):
        k = int(nnz[r])
        idx[r, :k] = torch.randperm(s, generator=gen)[:k].sort().values.to(torch.int32)
        val[r, :k] = torch.rand(k, generator=gen) * 2
    pre = [s] if prefixes is None else list(prefixes)
    got = eng.decode_rows(idx.cuda(), val.cuda(), nnz.cuda(), prefixes=prefixes).cpu().double()
    assert got.shape == (n, len(pre), d)
    W, bd = eng.view("W_dec").double().cpu(), eng.view("b_dec").double().cpu()
    for r in range(n):
        k = int(nnz[r])
        ii, vv = idx[r, :k].long(), val[r, :k].double()
        for p, cut in enumerate(pre):
            m = ii < cut
            want = bd + vv[m] @ W[ii[m]]
            torch.testing.assert_close(got[r, p], want, rtol=1e-5, atol=1e-4 * (1 + k) ** 0.5)


@pytest.mark.parametrize("tag", ["sparse", "dense"])
def test_module_api_of_the_reference_checkpoint(tmp_path, tag, encoder_mode):
    from saev_amd import nn

    g = load_golden(f"g19_relu_forward_{tag}")
    path = tmp_path / "sae.pt"
    path.write_bytes(g["ckpt"].numpy().tobytes())
    sae = nn.load(path, device="cuda")
    x = g["x"].cuda()
    r = g["f_x"].shape[0]  # the fixture keeps the dense h_x / f_x of its first r rows, the reconstructions of all
    out = sae(x)
    torch.testing.assert_close(out.x_hats.cpu(), g["x_hats"], rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(out.f_x[:r].cpu(), g["f_x"], rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(out.h_x[:r].cpu(), g["h_x"], rtol=1e-5, atol=1e-5)
    enc = sae.encode(x)
    torch.testing.assert_close(enc.h_x[:r].cpu(), g["h_x"], rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(enc.f_x[:r].cpu(), g["f_x"], rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(enc.f_x, out.f_x, rtol=0, atol=0)
    # decode of dense latents: the forward's own f_x for every row, the reference's f_x for its first rows
    torch.testing.assert_close(sae.decode(out.f_x).cpu(), g["x_hats"], rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(sae.decode(out.f_x, prefixes=g["prefixes"]).cpu(), g["x_hats_p"], rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(sae.decode(g["f_x"].cuda()).cpu(), g["x_hats"][:r], rtol=1e-4, atol=1e-5)
    # the Matryoshka reconstructions of the forward's own rows
    idx, val, nnz = sae.encode_sparse(x)
    xp = sae._eng().decode_rows(idx, val, nnz, prefixes=g["prefixes"].tolist())
    torch.testing.assert_close(xp.cpu(), g["x_hats_p"], rtol=1e-4, atol=1e-5)


@pytest.mark.encoder_modes("f32")
def test_relu_engine_refuses_training_and_bf16(encoder_mode):
    from saev_amd.engine import EngineConfig, SaeEngine

    g = load_golden("g19_relu_forward_sparse")
    params = ckpt_params(g)
    S, D = params["W_dec"].shape
    eng = relu_engine(D, S, 128, params)
    x = g["x"].cuda()
    for call in (lambda: eng.step_forward(x, training=False), lambda: eng.train_step(x, 1e-3), lambda: eng.encode_topk(x)):
        with pytest.raises(NotImplementedError):
            call()
    bf = SaeEngine(EngineConfig(d_model=D, d_sae=S, k_aux=0, max_batch=128, activation="relu", encoder="bf16"), "cuda",
                   with_optim=False)
    with pytest.raises(NotImplementedError):
        bf.encode_relu(x)


@pytest.mark.parametrize("tag", ["plain", "labels"])
def test_inference_artifacts_match_the_reference(tmp_path, tag, encoder_mode):
    from saev_amd import disk
    from saev_amd.data import Metadata, OrderedConfig
    from saev_amd.framework import inference

    g = load_golden(f"g19_inference_relu_{tag}")
    d = write_cache(tmp_path, g)
    md = Metadata.load(d)
    runs_root = tmp_path / "saev" / "runs"
    runs_root.mkdir(parents=True)
    run = disk.Run.new("gpu00019", train_shards_dir=d, val_shards_dir=d, runs_root=runs_root)
    run.ckpt.parent.mkdir(parents=True, exist_ok=True)
    run.ckpt.write_bytes(g["ckpt"].numpy().tobytes())  # the reference's own nn.dump of the ReLU SAE
    cfg = inference.Config(run=run.run_dir, data=OrderedConfig(shards=d, layer=11, batch_size=int(g["batch_size"])),
                           n_dists=int(g["n_dists"]), ignore_labels=g["ignore_labels"].tolist())
    assert inference.need_compute(cfg)[0]
    inference.worker_fn(cfg)
    out = run.inference / md.hash
    assert sorted(p.name for p in out.iterdir()) == ["config.json", "distributions.pt", "mean_values.pt", "metrics.json",
                                                      "sparsity.pt", "token_acts.npz"]

    csr = scipy.sparse.load_npz(out / "token_acts.npz")
    assert csr.shape == tuple(g["csr_shape"].tolist())
    assert csr.indices.dtype == np.int32 and csr.indptr.dtype == np.int32 and csr.data.dtype == np.float32
    np.testing.assert_array_equal(csr.indptr, g["csr_indptr"].numpy())
    np.testing.assert_array_equal(csr.indices, g["csr_indices"].numpy())  # no near-ties at the cut in this fixture
    np.testing.assert_allclose(csr.data, g["csr_data"].numpy(), rtol=1e-5, atol=1e-6)

    torch.testing.assert_close(torch.load(out / "mean_values.pt"), g["mean_values"], rtol=1e-5, atol=1e-6, equal_nan=True)
    torch.testing.assert_close(torch.load(out / "sparsity.pt"), g["sparsity"], rtol=1e-6, atol=0)
    torch.testing.assert_close(torch.load(out / "distributions.pt"), g["distributions"], rtol=1e-5, atol=1e-6)
    got = json.loads((out / "metrics.json").read_text())
    want = dict(zip(g["metrics_keys"].tolist(), g["metrics_vals"].tolist()))
    assert list(got) == list(want)
    for k, v in want.items():
        assert got[k] == pytest.approx(v, rel=1e-5), k
    assert isinstance(got["n_tokens"], int) and got["n_tokens"] == int(want["n_tokens"])
