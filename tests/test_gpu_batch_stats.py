"""saev_batch_stats / saev_row_norm_mean on the MI355X (include/saev_amd.h: BATCH STATISTICS) against fp64 torch recomputations
on the same device tensors, and the three host paths that use them -- the log block of train(), evaluate() and the inference
pass -- against recomputations from the codes and reconstructions the engine hands out.

Tolerances of the fp64 sums are derived, not tuned: two fp64 summations of the same m exact terms in different orders differ by
at most 2 (m - 1) u sum |t_i|, u = 2^-53 (each is within (m - 1) u sum |t_i| of the exact sum, to first order).  The terms of
col_sum, sum x and sum x^2 are exact in fp64 (an fp32 value, or the 48-bit square of one); r = x - x_hat is the same single fp64
rounding on both sides; r^2 is one more rounding in the torch restatement (the kernel's fma does not round it), which moves each
term by at most u |t_i|: that sum's bound is (2 (m - 1) + 1) u sum |t_i|.  n_pos and live are exact."""

import dataclasses
import json
import math

import numpy as np
import pytest
import torch

import sae_ref as R
from conftest import load_golden

pytestmark = [pytest.mark.gpu, pytest.mark.encoder_modes("f16r")]

U = 2.0 ** -53
EPS = 1e-12
SHAPES = [(1, 256, 512, 8), (1000, 768, 6144, 32), (4099, 1280, 8192, 64), (257, 4096, 1024, 16), (16384, 1024, 32768, 32)]
MASKS = ("none", "all", "no_rows", "third")


def E():
    from saev_amd import engine

    return engine


def make_x(n, D, kind, gen):
    x = torch.randn(n, D, generator=gen, device="cuda")
    x_hat = x + 0.3 * torch.randn(n, D, generator=gen, device="cuda")
    if kind == "offset":  # the f16r centring test's regime: a large common offset, two columns three hundred times larger
        x = x + 30.0
        x[:, :2] *= 300.0
        x_hat = x + 0.3 * torch.randn(n, D, generator=gen, device="cuda")
    return x.contiguous(), x_hat.contiguous()


def make_codes(n, S, cap, pattern, gen):
    idx = torch.randint(0, S, (n, cap), generator=gen, device="cuda", dtype=torch.int32)
    val = torch.randn(n, cap, generator=gen, device="cuda")
    flat_i, flat_v = idx.view(-1), val.view(-1)
    m = flat_v.numel()
    special = torch.tensor([0.0, -0.0, 1e-12, -1e-12, 2e-12, -2e-12], device="cuda")
    for j, v in enumerate(special.tolist()):  # exact zeros and values around live_eps, spread over the slots
        flat_v[j::max(1, 13 + j)][: max(1, m // 40)] = v
    flat_i[5::17] = -1   # indices outside [0, S): ignored
    flat_i[11::19] = S
    row_nnz = None
    if pattern == "rows":  # variable rows: empty ones, counts above cap, slots past the count hold poison
        row_nnz = torch.randint(0, cap + 4, (n,), generator=gen, device="cuda", dtype=torch.int32)
        row_nnz[::7] = 0
        past = torch.arange(cap, device="cuda")[None, :] >= row_nnz[:, None]
        val[past] = float("nan")
    return idx, val, row_nnz


def make_keep(n, mask):
    if mask == "none":
        return None
    if mask == "all":
        return torch.ones(n, dtype=torch.bool, device="cuda")
    if mask == "no_rows":
        return torch.zeros(n, dtype=torch.bool, device="cuda")
    k = torch.zeros(n, dtype=torch.bool, device="cuda")
    k[::3] = True
    return k


def reference(x, x_hat, idx, val, row_nnz, keep, S):
    """fp64 torch restatement: the values and, for every sum, its number of terms m and sum |t_i|."""
    n, D = x.shape
    kp = torch.ones(n, dtype=torch.bool, device=x.device) if keep is None else keep
    x64 = x[kp].double()
    out = {"n_kept": float(kp.sum()), "col_sum": x64.sum(0), "col_abs": x64.abs().sum(0), "sx": x64.sum(), "sx_abs": x64.abs().sum(),
           "sxx": (x64 * x64).sum(), "m_rows": int(kp.sum())}
    if x_hat is not None:
        r = x64 - x_hat[kp].double()
        out.update(sr=r.sum(), sr_abs=r.abs().sum(), srr=(r * r).sum())
    cap = idx.shape[1]
    valid = kp[:, None] & (idx >= 0) & (idx < S)
    if row_nnz is not None:
        valid &= torch.arange(cap, device=x.device)[None, :] < row_nnz[:, None]
    ii = idx.long().clamp(0, S - 1)
    pos, nz = valid & (val > 0), valid & (val != 0)
    out["n_pos"] = torch.bincount(ii[pos], minlength=S)
    out["value_sum"] = torch.zeros(S, dtype=torch.float64, device=x.device).index_add_(0, ii[nz], val[nz].double())
    out["value_abs"] = torch.zeros(S, dtype=torch.float64, device=x.device).index_add_(0, ii[nz], val[nz].double().abs())
    out["value_m"] = torch.bincount(ii[nz], minlength=S)
    lv = valid & (val.abs() > EPS)
    out["live"] = torch.zeros(S, dtype=torch.int32, device=x.device)
    out["live"][ii[lv]] = 1
    return out


def t64(v):
    return v.detach().cpu().double() if torch.is_tensor(v) else torch.tensor(v, dtype=torch.float64)


def check(acc, ref, D, with_r=True, label=""):
    got = acc.read()
    m, md = ref["m_rows"], ref["m_rows"] * D
    assert got.n_kept == ref["n_kept"], label
    print(f"{label}: n_kept {got.n_kept:.0f}")

    def close(name, g, w, bound):
        g, w, bound = t64(g), t64(w), t64(bound)
        err = (g - w).abs()
        print(f"{label}: {name} max err {err.max().item():.3e} (bound at that entry {bound.reshape(-1)[err.reshape(-1).argmax()].item():.3e})")
        assert bool((err <= bound).all()), f"{label}: {name} err {err.max().item():.3e}"

    close("col_sum", got.col_sum, ref["col_sum"], 2 * max(m - 1, 0) * U * ref["col_abs"])
    close("sum_x", got.sum_x, ref["sx"], 2 * max(md - 1, 0) * U * ref["sx_abs"])
    close("sum_xx", got.sum_xx, ref["sxx"], 2 * max(md - 1, 0) * U * ref["sxx"])
    if with_r:
        close("sum_r", got.sum_r, ref["sr"], 2 * max(md - 1, 0) * U * ref["sr_abs"])
        close("sum_rr", got.sum_rr, ref["srr"], (2 * max(md - 1, 0) + 1) * U * ref["srr"])
    else:
        assert got.sum_r == 0.0 and got.sum_rr == 0.0
    assert torch.equal(got.n_pos, ref["n_pos"].cpu()), f"{label}: n_pos"
    assert torch.equal(got.live, ref["live"].cpu()), f"{label}: live"
    close("value_sum", got.value_sum, ref["value_sum"], 2 * (ref["value_m"] - 1).clamp_min(0).double() * U * ref["value_abs"])
    return got


@pytest.mark.parametrize("kind", ["normal", "offset"])
@pytest.mark.parametrize("pattern", ["topk", "rows"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_output_against_fp64_torch(shape, pattern, kind):
    n, D, S, cap = shape
    gen = torch.Generator(device="cuda").manual_seed(n + D)
    x, x_hat = make_x(n, D, kind, gen)
    idx, val, row_nnz = make_codes(n, S, cap, pattern, gen)
    for mask in MASKS:
        keep = make_keep(n, mask)
        ref = reference(x, x_hat, idx, val, row_nnz, keep, S)
        acc = E().BatchStats(D, S, "cuda:0")
        acc.add(x, x_hat, idx, val, row_nnz, keep)
        label = f"{shape} {pattern} {kind} mask={mask}"
        got = check(acc, ref, D, label=label)
        # bit-reproducible fp64 sums: a second run into fresh accumulators
        acc2 = E().BatchStats(D, S, "cuda:0")
        acc2.add(x, x_hat, idx, val, row_nnz, keep)
        got2 = acc2.read()
        assert torch.equal(got.col_sum, got2.col_sum), label
        assert (got.sum_x, got.sum_xx, got.sum_r, got.sum_rr) == (got2.sum_x, got2.sum_xx, got2.sum_r, got2.sum_rr), label
        if kind == "offset" and ref["m_rows"] > 0 and ref["m_rows"] * D > 1:  # explained variance from the sums vs two passes in fp64
            kp = slice(None) if keep is None else keep
            x64, r64 = x[kp].double(), x[kp].double() - x_hat[kp].double()
            want = 1 - (r64.var() / x64.var()).item()
            mm = ref["m_rows"] * D
            ev = 1 - ((got.sum_rr - got.sum_r ** 2 / mm) / (mm - 1)) / ((got.sum_xx - got.sum_x ** 2 / mm) / (mm - 1))
            print(f"{label}: explained variance {ev!r} vs two-pass {want!r}")
            assert math.isclose(ev, want, rel_tol=1e-9), (label, ev, want)


def test_without_x_hat_and_with_a_subset_of_outputs():
    n, D, S, cap = 1000, 768, 6144, 32
    gen = torch.Generator(device="cuda").manual_seed(1)
    x, _ = make_x(n, D, "normal", gen)
    idx, val, _ = make_codes(n, S, cap, "topk", gen)
    ref = reference(x, None, idx, val, None, None, S)
    acc = E().BatchStats(D, S, "cuda:0")
    acc.add(x, None, idx, val)
    check(acc, ref, D, with_r=False, label="no x_hat")
    only = E().BatchStats(D, S, "cuda:0", want=("n_pos",))
    only.add(x, None, idx, val)
    got = only.read()
    assert torch.equal(got.n_pos, ref["n_pos"].cpu()) and got.col_sum is None and got.live is None and got.n_kept == 0.0


def test_eight_batches_accumulate_to_one_call_on_their_concatenation():
    n, D, S, cap = 520, 1280, 8192, 64
    gen = torch.Generator(device="cuda").manual_seed(2)
    parts = [(make_x(n + 3 * b, D, "offset", gen), make_codes(n + 3 * b, S, cap, "rows", gen)) for b in range(8)]
    acc = E().BatchStats(D, S, "cuda:0")
    for (x, x_hat), (idx, val, nnz) in parts:
        acc.add(x, x_hat, idx, val, nnz)
    cat = lambda j, k: torch.cat([p[j][k] for p in parts])  # noqa: E731
    x, x_hat, idx, val, nnz = cat(0, 0), cat(0, 1), cat(1, 0), cat(1, 1), cat(1, 2)
    ref = reference(x, x_hat, idx, val, nnz, None, S)
    check(acc, ref, D, label="eight batches vs the concatenation's reference")
    one = E().BatchStats(D, S, "cuda:0")
    one.add(x, x_hat, idx, val, nnz)
    a, b = acc.read(), one.read()
    m, md = x.shape[0], x.shape[0] * D
    assert bool(((a.col_sum - b.col_sum).abs() <= 2 * (m - 1) * U * ref["col_abs"].cpu()).all())
    assert abs(a.sum_xx - b.sum_xx) <= 2 * (md - 1) * U * ref["sxx"].item()
    assert abs(a.sum_rr - b.sum_rr) <= 2 * (md - 1) * U * ref["srr"].item()
    assert torch.equal(a.n_pos, b.n_pos) and torch.equal(a.live, b.live)


def test_overwrite_ignores_old_contents_and_live_is_never_cleared():
    n, D, S, cap = 300, 256, 512, 8
    gen = torch.Generator(device="cuda").manual_seed(3)
    x, x_hat = make_x(n, D, "normal", gen)
    idx, val, _ = make_codes(n, S, cap, "topk", gen)
    ref = reference(x, x_hat, idx, val, None, None, S)
    acc = E().BatchStats(D, S, "cuda:0")
    acc.sums.fill_(1e300)
    acc.extra.zero_()
    acc.value_sum.fill_(float("nan"))
    acc.n_pos.fill_(12345)
    acc.add(x, x_hat, idx, val, overwrite=True)
    check(acc, ref, D, label="overwrite")
    acc.live.fill_(1)
    acc.add(x, x_hat, idx, val, overwrite=True)
    assert bool((acc.live == 1).all())
    # accumulate mode on top: exactly twice the integer counts
    acc.add(x, x_hat, idx, val)
    assert torch.equal(acc.n_pos.cpu(), 2 * ref["n_pos"].cpu())


def test_nan_in_one_row_poisons_its_column_and_the_scalar_sums_only():
    n, D, S, cap = 1000, 768, 6144, 32
    gen = torch.Generator(device="cuda").manual_seed(4)
    x, x_hat = make_x(n, D, "normal", gen)
    idx, val, _ = make_codes(n, S, cap, "topk", gen)
    x[123, 45] = float("nan")
    acc = E().BatchStats(D, S, "cuda:0")
    acc.add(x, x_hat, idx, val)
    got = acc.read()
    nan_cols = torch.isnan(got.col_sum).nonzero().flatten().tolist()
    assert nan_cols == [45]
    assert all(math.isnan(v) for v in (got.sum_x, got.sum_xx, got.sum_r, got.sum_rr)) and got.n_kept == n
    assert not torch.isnan(got.value_sum).any()
    # masked out, the row poisons nothing
    keep = torch.ones(n, dtype=torch.bool, device="cuda")
    keep[123] = False
    acc2 = E().BatchStats(D, S, "cuda:0")
    acc2.add(x, x_hat, idx, val, keep=keep)
    check(acc2, reference(x, x_hat, idx, val, None, keep, S), D, label="NaN row masked out")


def test_empty_batch_and_empty_rows_write_nothing():
    acc = E().BatchStats(256, 512, "cuda:0")
    acc.buf.fill_(7)
    before = acc.buf.clone()
    z = lambda *s, dt=torch.float32: torch.zeros(*s, device="cuda", dtype=dt)  # noqa: E731
    acc.add(z(0, 256), z(0, 256), z(0, 8, dt=torch.int32), z(0, 8))
    assert torch.equal(acc.buf, before)
    acc2 = E().BatchStats(256, 512, "cuda:0")
    acc2.add(z(5, 256) + 1, None, None, None)  # cap = 0: no codes at all
    got = acc2.read()
    assert got.n_kept == 5 and got.sum_x == 5 * 256 and int(got.n_pos.sum()) == 0


@pytest.mark.parametrize("shape", [(1, 256), (7, 4), (1000, 768), (4097, 1280), (300, 4096), (32768, 1024)], ids=lambda s: "x".join(map(str, s)))
def test_row_norm_mean(shape):
    S, D = shape
    gen = torch.Generator(device="cuda").manual_seed(S)
    W = torch.randn(S, D, generator=gen, device="cuda") * torch.rand(S, 1, generator=gen, device="cuda") * 3
    want = W.double().norm(dim=1).mean().item()
    got = E().row_norm_mean(W)
    print(f"row_norm_mean {shape}: {got!r} vs {want!r}, rel {abs(got - want) / want:.3e}")
    assert math.isclose(got, want, rel_tol=1e-7)
    assert E().row_norm_mean(W) == got  # fixed order: the same bits


# ---- through the public interface ------------------------------------------------------------------------------------------


def M():
    from saev_amd.nn import modeling

    return modeling


def O():
    from saev_amd.nn import objectives

    return objectives


def small_cfg(tmp_path, g, **kw):
    from saev_amd import data
    from saev_amd.framework import train as T

    m, o = M(), O()
    d, s, k, bsz = int(g["d"]), int(g["s"]), int(g["k"]), int(g["bsz"])
    dc = data.ShuffledConfig(batch_size=bsz, seed=3)
    return T.Config(
        train_data=dc, val_data=dc, n_train=int(g["n_train"]), n_val=10**9,
        sae=m.SparseAutoencoderConfig(d_model=d, d_sae=s, reinit_blend=0.0,
                                      activation=m.TopK(top_k=k, aux=m.AuxK(k_aux=int(g["k_aux"]), alpha=1 / 32))),
        objective=o.Matryoshka(n_prefixes=1, dead_threshold_tokens=int(g["thr"])),
        lr=float(g["lr"]), n_lr_warmup=int(g["n_warm"]), track=False, log_every=1, runs_root=tmp_path / "runs", **kw)


@pytest.fixture
def spy(monkeypatch):
    """Records what every statistics call of the host paths was given: copies of x, of the engine's codes and reconstruction
    (eng.last_codes) or of the padded ReLU rows, the row mask and the step's own statistics."""
    eng_mod = E()
    calls = []
    real_eng, real_add = eng_mod.SaeEngine.add_batch_stats, eng_mod.BatchStats.add

    def add_batch_stats(self, acc, x, keep=None, **kw):
        idx, val, x_hat = self.last_codes(x.shape[0])
        calls.append(dict(x=x.clone(), idx=idx, val=val, x_hat=x_hat, row_nnz=None, keep=None if keep is None else keep.clone(),
                          st=self.read_stats(), eng=self))
        return real_eng(self, acc, x, keep, **kw)

    def add(self, x, x_hat, idx, val, row_nnz=None, keep=None, **kw):
        calls.append(dict(x=x.clone(), idx=idx.clone(), val=val.clone(), x_hat=x_hat.clone(), row_nnz=row_nnz.clone(),
                          keep=None if keep is None else keep.clone(), st=None, eng=None))
        return real_add(self, x, x_hat, idx, val, row_nnz, keep, **kw)

    monkeypatch.setattr(eng_mod.SaeEngine, "add_batch_stats", add_batch_stats)
    monkeypatch.setattr(eng_mod.BatchStats, "add", add)
    return calls


def test_train_log_records_equal_an_fp64_recomputation(tmp_path, spy, monkeypatch):
    from saev_amd.framework import train as T

    g = load_golden("g9_train_a")
    cfg = small_cfg(tmp_path, g, log_coherence=False)
    norms = []
    real_dec = T._decoder_metrics

    def dec(sae, c):
        norms.append(sae.W_dec.detach().double().norm(dim=1).mean().item())
        return real_dec(sae, c)

    monkeypatch.setattr(T, "_decoder_metrics", dec)
    saes, objs, run, steps = T.train([cfg], train_pool=g["acts"])
    logs = [rec for _, rec in run.records[0]]
    assert len(logs) == steps == len(spy) == len(norms) and steps >= 5
    S, D = int(g["s"]), int(g["d"])
    keys = {"loss/loss", "loss/mse", "loss/l0", "loss/l1", "loss/sparsity", "loss/aux", "loss/n_dead", "progress/n_patches_seen",
            "progress/learning_rate", "metrics/explained_variance", "metrics/dead_unit_pct", "metrics/grad_norm", "metrics/sse_sae",
            "metrics/sse_baseline", "metrics/normalized_mse", "loader/buffer_fill", "metrics/avg_decoder_row_norm"}
    for rec, c, norm in zip(logs, spy, norms):
        assert keys <= set(rec), keys - set(rec)
        x64, xh64, st = c["x"].double(), c["x_hat"].double(), c["st"]
        n = x64.shape[0]
        r64 = x64 - xh64
        # from the new kernels
        assert math.isclose(rec["metrics/explained_variance"], 1 - (r64.var() / x64.var()).item(), rel_tol=1e-9)
        live = torch.zeros(S, dtype=torch.int32, device="cuda")
        live[c["idx"][c["val"].abs() > EPS].long()] = 1
        assert abs(rec["metrics/dead_unit_pct"] - int((live == 0).sum()) / S) < 0.5 / S  # the exact count of dead flags
        base = (x64 * x64).sum().item() - (x64.sum(0) ** 2).sum().item() / n
        assert math.isclose(rec["metrics/sse_baseline"], base, rel_tol=1e-9)
        assert math.isclose(rec["metrics/avg_decoder_row_norm"], norm, rel_tol=1e-7)
        # from the step's own statistics (read_stats), unchanged: the same numbers, and the fp64 restatement to the accuracy
        # of the step's fp32 reconstruction
        assert rec["metrics/sse_sae"] == st.sse and rec["loss/n_dead"] == st.n_dead
        for key, want in (("loss/mse", st.mse), ("loss/l0", st.l0), ("loss/l1", st.l1), ("loss/aux", st.aux), ("loss/loss", st.mse + st.aux)):
            assert math.isclose(rec[key], want, rel_tol=1e-12, abs_tol=1e-300), key  # (x n / n on the host)
        assert rec["metrics/grad_norm"] == st.grad_norm and rec["loss/sparsity"] == 0.0 and rec["loader/buffer_fill"] == 1.0
        assert math.isclose(rec["metrics/sse_sae"], (r64 * r64).sum().item(), rel_tol=1e-4)
        assert math.isclose(rec["metrics/normalized_mse"], st.sse / base, rel_tol=1e-9)


def test_evaluate_equals_an_fp64_recomputation(tmp_path, spy):
    from saev_amd.framework import train as T

    g = load_golden("g9_train_a")
    cfg = small_cfg(tmp_path, g)
    sae = M().SparseAutoencoder(cfg.sae)
    sae.load_state_dict({k: g["final_" + k] for k in R.PARAM_ORDER})
    saes = torch.nn.ModuleList([sae]).cuda()
    objs = torch.nn.ModuleList([O().get_objective(cfg.objective)])
    ev = T.evaluate([cfg], saes, objs, val_pool=g["val"])[0]
    assert len(spy) >= 1
    S, D = int(g["s"]), int(g["d"])
    n_pos = torch.zeros(S, dtype=torch.int64, device="cuda")
    vsum = torch.zeros(S, dtype=torch.float64, device="cuda")
    sum_vec = torch.zeros(D, dtype=torch.float64, device="cuda")
    n = 0
    tot = dict(sum_sq=0.0, sse=0.0, l0=0.0, l1=0.0, mse=0.0)
    for c in spy:
        b = c["x"].shape[0]
        n += b
        idx, val = c["idx"].long().view(-1), c["val"].view(-1)
        n_pos += torch.bincount(idx[val > 0], minlength=S)
        vsum.index_add_(0, idx, val.double())
        sum_vec += c["x"].double().sum(0)
        st = c["st"]
        tot["sum_sq"] += st.sum_sq; tot["sse"] += st.sse; tot["l0"] += st.l0 * b; tot["l1"] += st.l1 * b; tot["mse"] += st.mse * b
    base = tot["sum_sq"] - (sum_vec ** 2).sum().item() / n
    assert ev.freqs.dtype == torch.float32 and ev.mean_values.dtype == torch.float32
    assert torch.equal(ev.freqs, (n_pos.cpu().to(torch.float32) / n))
    torch.testing.assert_close(ev.mean_values, (vsum / n_pos.double()).to(torch.float32).cpu(), rtol=2e-7, atol=0, equal_nan=True)
    assert bool(torch.isnan(ev.mean_values[n_pos.cpu() == 0]).all())
    assert math.isclose(ev.sse_baseline, base, rel_tol=1e-9) and math.isclose(ev.sse_sae, tot["sse"], rel_tol=1e-12)
    assert math.isclose(ev.normalized_mse, tot["sse"] / base, rel_tol=1e-9)
    assert math.isclose(ev.l0, tot["l0"] / n, rel_tol=1e-12) and math.isclose(ev.l1, tot["l1"] / n, rel_tol=1e-12)
    assert math.isclose(ev.mse, tot["mse"] / n, rel_tol=1e-12)
    fr = n_pos.cpu().to(torch.float32) / n
    assert (ev.n_dead, ev.n_almost_dead, ev.n_dense) == (int((fr == 0).sum()), int((fr < 1e-7).sum()), int((fr > 1e-2).sum()))


@pytest.mark.parametrize("tag", ["g14_inference_plain", "g14_inference_labels", "g19_inference_relu_plain", "g19_inference_relu_labels"])
def test_inference_artifacts_equal_an_fp64_recomputation(tmp_path, spy, tag):
    import scipy.sparse

    from saev_amd import disk, nn
    from saev_amd.data import Metadata, OrderedConfig
    from saev_amd.framework import inference
    from saev_amd.metrics import Metrics
    from test_inference_host_cpu import write_cache

    g = load_golden(tag)
    d = write_cache(tmp_path, g)
    md = Metadata.load(d)
    runs_root = tmp_path / "saev" / "runs"
    runs_root.mkdir(parents=True)
    run = disk.Run.new("gpu000bs", train_shards_dir=d, val_shards_dir=d, runs_root=runs_root)
    relu = "relu" in tag
    if relu:
        run.ckpt.parent.mkdir(parents=True, exist_ok=True)
        run.ckpt.write_bytes(g["ckpt"].numpy().tobytes())
    else:
        S, D = g["p_W_dec"].shape
        sae = nn.SparseAutoencoder(nn.SparseAutoencoderConfig(
            d_model=D, d_sae=S, activation=nn.modeling.TopK(top_k=int(g["k"]), aux=nn.modeling.AuxK(k_aux=int(g["k_aux"])))))
        with torch.no_grad():
            for k in R.PARAM_ORDER:
                getattr(sae, k).copy_(g["p_" + k])
        nn.dump(run.ckpt, sae)
    n_dists = int(g["n_dists"])
    cfg = inference.Config(run=run.run_dir, data=OrderedConfig(shards=d, layer=11, batch_size=int(g["batch_size"])),
                           n_dists=n_dists, ignore_labels=g["ignore_labels"].tolist())
    inference.worker_fn(cfg)
    out = run.inference / md.hash
    assert len(spy) >= 1
    if "labels" in tag:
        assert any(c["keep"] is not None for c in spy)  # the masked route ran
    S, D = nn.load(run.ckpt).cfg.d_sae, spy[0]["x"].shape[1]
    n_pos = torch.zeros(S, dtype=torch.int64, device="cuda")
    vsum = torch.zeros(S, dtype=torch.float64, device="cuda")
    sum_vec = torch.zeros(D, dtype=torch.float64, device="cuda")
    sse = sum_sq = 0.0
    n_tok, rows = 0, []
    for c in spy:
        x, idx, val = c["x"], c["idx"], c["val"]
        b, cap = idx.shape
        kp = torch.ones(b, dtype=torch.bool, device="cuda") if c["keep"] is None else c["keep"].bool()
        n_tok += int(kp.sum())
        entries = kp[:, None] & ((torch.arange(cap, device="cuda")[None, :] < c["row_nnz"][:, None]) if relu else (val != 0))
        dense = torch.zeros(b, S, dtype=torch.float64, device="cuda")
        rr = torch.arange(b, device="cuda")[:, None].expand_as(idx)[entries]
        dense[rr, idx[entries].long()] = val[entries].double()
        rows.append(dense)
        n_pos += (dense > 0).sum(0)
        vsum += dense.sum(0)
        x64 = x[kp].double()
        r64 = x64 - c["x_hat"][kp].double()
        sum_vec += x64.sum(0)
        if relu or c["keep"] is not None:
            sse += (r64 * r64).sum().item(); sum_sq += (x64 * x64).sum().item()
        else:  # unmasked TopK batches: the step's own reductions, as before
            sse += c["st"].sse; sum_sq += c["st"].sum_sq
            assert math.isclose(c["st"].sse, (r64 * r64).sum().item(), rel_tol=1e-4)
    dense = torch.cat(rows)
    csr = scipy.sparse.load_npz(out / "token_acts.npz")
    n_samples = csr.shape[0]  # every token of the cache (a batch without a kept row makes no statistics call)
    mean_values, sparsity = torch.load(out / "mean_values.pt"), torch.load(out / "sparsity.pt")
    assert mean_values.dtype == torch.float32 and sparsity.dtype == torch.float32
    torch.testing.assert_close(mean_values, (vsum / n_pos.double()).to(torch.float32).cpu(), rtol=2e-7, atol=0, equal_nan=True)
    assert bool(torch.isnan(mean_values[n_pos.cpu() == 0]).all())
    assert torch.equal(sparsity, n_pos.cpu().to(torch.float32) / n_samples)
    if dense.shape[0] == n_samples:
        np.testing.assert_array_equal(csr.toarray(), dense.to(torch.float32).cpu().numpy())
    np.testing.assert_allclose(np.asarray(csr.sum(axis=0)).reshape(-1), vsum.cpu().numpy(), rtol=1e-5, atol=1e-6)
    dist = torch.load(out / "distributions.pt")
    assert dist.shape[1] == n_dists and dist.dtype == torch.float32
    got = json.loads((out / "metrics.json").read_text())
    base = sum_sq - (sum_vec ** 2).sum().item() / n_tok
    want = Metrics.from_accumulators(sse_recon=sse, sse_baseline=base, n_tokens=n_tok, d_model=D).to_dict()
    assert list(got) == list(want)
    for k, v in want.items():
        assert got[k] == pytest.approx(v, rel=1e-9), k


def test_a_log_step_allocates_no_batch_sized_temporary(tmp_path):
    from saev_amd.framework import train as T
    from saev_amd.framework.ddp import DataParallelStepper

    n, D, S, k = 4096, 1024, 8192, 32
    m, o = M(), O()
    g = load_golden("g9_train_a")
    cfg = dataclasses.replace(small_cfg(tmp_path, g), log_coherence=False,
                              sae=m.SparseAutoencoderConfig(d_model=D, d_sae=S, reinit_blend=0.0, activation=m.TopK(top_k=k, aux=m.AuxK(k_aux=64, alpha=1 / 32))))
    torch.manual_seed(0)
    sae = m.SparseAutoencoder(cfg.sae).cuda().train()
    obj = o.get_objective(cfg.objective).train()
    st = DataParallelStepper(obj._bind(sae, n))
    x = torch.randn(n, D, device="cuda")
    pre = {}
    st.train_step(x, 1e-4, cfg.grad_clip, pre_tail=lambda: pre.update(T._decoder_metrics(sae, cfg)))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    rec = T._log_metrics(sae, st.engine, x, 1e-4, n, cfg, pre)
    torch.cuda.synchronize()
    growth = torch.cuda.max_memory_allocated() - before
    print(f"log step at ({n}, {D}): peak growth {growth} bytes, n D 4 = {n * D * 4}")
    assert growth < n * D * 4, growth
    assert 0.0 <= rec["metrics/dead_unit_pct"] <= 1.0 and math.isfinite(rec["metrics/explained_variance"])
