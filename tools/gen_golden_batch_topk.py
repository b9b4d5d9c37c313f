"""Generate the BatchTopK golden vectors (G20) by RUNNING the upstream reference on the CPU (build container only).

Test infrastructure beside ``oracle/`` (it imports ``oracle/gen_golden.py`` for its helpers and the reference import shim and
changes nothing there).  The reference is read from its own location at generation time only; the outputs are data under
``tests/golden/``:

  g20_batch_topk_forward     a BatchTopK SAE written by the reference's nn.dump with a NON-ZERO ``activation.threshold`` (the raw
                             bytes), x, and what the reference makes of it: a training-mode forward (h_x, f_x, x_hats, the
                             objective's losses, the threshold before and after), the same with four Matryoshka prefixes, and
                             eval-mode forwards with the stored threshold (> 0) and with threshold = 0
  g20_batch_topk_train_p1    a 4-step Adam trajectory of the reference's loop body (renormalise, objective, backward,
                             remove_parallel_grads, clip, fused Adam; train.py:332-460) in which latents die and the AuxK term is
                             non-zero from step 2: per step the batch, losses, n_dead, gradient norm, threshold and f_x; initial and
                             final parameters, the biases after every step
  g20_batch_topk_train_p4    the same with n_prefixes = 4 (fixed cut points)
  g20_inference_batch_topk_{plain,labels}
                             the reference's framework/inference.worker_fn artifacts of a BatchTopK SAE over a small cache, with
                             the module in EVAL mode.  (The reference's inference pass never calls ``eval()``, so as written it would
                             run the batch-wide select per inference batch and move the threshold while doing so; the eval-mode
                             threshold is what the activation's own documentation prescribes for inference, and what saev_amd runs.
                             The generator therefore hands the reference's worker an ``nn.load`` that returns ``.eval()``.)

No near-tie at a cut: seeds are searched until, at EVERY recorded training-mode forward, the gap in fp64 between the (n top_k)-th
largest pre-activation and the next one is at least 16 x the fp32 dot-product bound 8 * 2^-24 * max_b ||x_b|| * max_s ||W_enc[:, s]||
(the bound tests/test_gpu_relu.py uses) -- a selection computed in fp32 in any summation order is then the reference's.  The gaps
and bounds are stored in the fixtures.

    python tools/gen_golden_batch_topk.py
"""

import importlib
import json
import pathlib
import shutil
import sys
import tempfile

import numpy as np
import torch

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "oracle"))
sys.path.insert(0, str(ROOT))
import gen_golden as G  # noqa: E402

D, S, B, K = 64, 256, 96, 8
K_AUX, ALPHA, MOMENTUM = 16, 1 / 32, 0.1
PREFIXES = (5, 40, 120, 256)
GAP_FACTOR = 16.0


def make_sae(ref, d, s, k, seed, k_aux=K_AUX, momentum=MOMENTUM):
    torch.manual_seed(seed)
    cfg = ref.modeling.SparseAutoencoderConfig(
        d_model=d, d_sae=s, reinit_blend=0.0,
        activation=ref.modeling.BatchTopK(top_k=k, momentum=momentum, aux=ref.modeling.AuxK(k_aux=k_aux, alpha=ALPHA)))
    sae = ref.modeling.SparseAutoencoder(cfg)
    with torch.no_grad():
        sae.b_enc.copy_(0.05 * torch.randn(s))
        sae.b_dec.copy_(0.1 * torch.randn(d))
        sae.W_enc.add_(0.02 * torch.randn(d, s))
    return sae


def cut_gap(sae, x, k):
    """(gap, bound, cut): fp64 gap between the (n k)-th largest pre-activation and the next, the fp32 dot-product bound, the cut."""
    with torch.no_grad():
        h = x.double() @ sae.W_enc.double() + sae.b_enc.double()
        n, s = h.shape
        t = min(k * n, s * n)
        v = h.flatten().sort(descending=True).values
        gap = float(v[t - 1] - v[t]) if t < v.numel() else float("inf")
        bound = 8.0 * 2.0 ** -24 * float(x.double().norm(dim=1).max()) * float(sae.W_enc.double().norm(dim=0).max())
    return gap, bound, float(v[t - 1])


def dump_bytes(ref, sae):
    tmp = pathlib.Path(tempfile.mkdtemp(prefix="g20_"))
    try:
        ref.modeling.dump(tmp / "sae.pt", sae)
        return (tmp / "sae.pt").read_bytes()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def with_fixed_prefixes(ref, fixed):
    class _Ctx:
        def __enter__(self):
            self.orig = ref.objectives.sample_prefixes
            if fixed is not None:
                ref.objectives.sample_prefixes = lambda d_sae, n_prefixes, *a, **kw: torch.tensor(fixed, dtype=torch.int64)

        def __exit__(self, *exc):
            ref.objectives.sample_prefixes = self.orig

    return _Ctx()


def forward_fixture(ref):
    for seed in range(200, 400):
        sae = make_sae(ref, D, S, K, seed=seed)
        x = G.lowrank_data(B, D, seed=seed + 1000)
        gap, bound, cut = cut_gap(sae, x, K)
        if gap >= GAP_FACTOR * bound and cut > 0:
            break
    else:
        raise RuntimeError("no seed without a near-tie at the cut")
    thr0 = float(np.float32(0.8 * cut))  # a stored threshold of the size training would have left
    with torch.no_grad():
        sae.activation.threshold.fill_(thr0)
    ckpt = dump_bytes(ref, sae)
    out = {}
    # training mode: the plain objective, then four nested reconstructions
    for tag, fixed in (("p1", None), ("p4", PREFIXES)):
        with torch.no_grad():
            sae.activation.threshold.fill_(thr0)
        sae.train()
        obj = ref.objectives.get_objective(ref.objectives.Matryoshka(n_prefixes=1 if fixed is None else len(fixed)))
        obj.train()
        with with_fixed_prefixes(ref, fixed), torch.no_grad():
            loss, o = obj(sae, x)
        out.update({f"{tag}_mse": loss.mse, f"{tag}_aux": loss.aux, f"{tag}_l0": loss.l0, f"{tag}_l1": loss.l1,
                    f"{tag}_x_hats": o.x_hats, f"{tag}_thr_after": sae.activation.threshold.clone()})
        if fixed is None:
            out.update(h_x=o.h_x, f_x=o.f_x)
        else:
            assert torch.equal(o.f_x, out["f_x"])
    nnz = (out["f_x"] != 0).sum(dim=1)
    assert int(nnz.sum()) == B * K
    print(f"forward: seed {seed}, gap {gap:.3e} vs bound {bound:.3e}, cut {cut:.4f}, codes per row {int(nnz.min())}..{int(nnz.max())}")
    # eval mode: the stored threshold, then zero
    sae.eval()
    for tag, thr in (("thr", thr0), ("zero", 0.0)):
        with torch.no_grad():
            sae.activation.threshold.fill_(thr)
            o = sae(x)
        en = (o.f_x != 0).sum(dim=1)
        print(f"eval {tag}: codes per row {int(en.min())}..{int(en.max())} (mean {float(en.float().mean()):.1f})")
        out.update({f"eval_{tag}_f_x": o.f_x, f"eval_{tag}_x_hats": o.x_hats})
    G.npz("g20_batch_topk_forward", ckpt=np.frombuffer(ckpt, dtype=np.uint8), x=x, k=K, momentum=MOMENTUM, thr_before=thr0,
          prefixes=np.array(PREFIXES, dtype=np.int64), gap=gap, bound=bound, cut=cut, **out)


def train_fixture(ref, tag, fixed, n_steps=4, lr=1e-3):
    thr_tokens = 2 * B  # a latent that stays silent for two batches is dead: the AuxK term switches on inside the trajectory
    for seed in range(400, 1400):
        torch.manual_seed(seed)
        sae = make_sae(ref, D, S, K, seed=seed)
        sae.train()
        obj = ref.objectives.get_objective(ref.objectives.Matryoshka(n_prefixes=1 if fixed is None else len(fixed),
                                                                     dead_threshold_tokens=thr_tokens))
        obj.train()
        init = {k_: v.detach().clone() for k_, v in sae.state_dict().items()}
        acts = G.lowrank_data(n_steps * B, D, seed=seed + 5000)
        # the clip threshold: half of the first step's gradient norm (measured on a throw-away copy), so every step is clipped
        opt = torch.optim.Adam([{"params": list(sae.parameters()), "lr": lr}], fused=True)
        rec = {k_: [] for k_ in ("mse", "aux", "l0", "l1", "n_dead", "grad_norm", "thr", "gap", "bound", "f_x", "b_enc", "b_dec")}
        clip, ok = None, True
        with with_fixed_prefixes(ref, fixed):
            for i in range(n_steps):
                x = acts[i * B:(i + 1) * B]
                sae.normalize_w_dec()
                gap, bound, _ = cut_gap(sae, x, K)
                if gap < GAP_FACTOR * bound:
                    ok = False
                    break
                loss, o = obj(sae, x)
                loss.loss.backward()
                sae.remove_parallel_grads()
                if clip is None:
                    total = torch.sqrt(sum((p.grad.double() ** 2).sum() for p in sae.parameters()))
                    clip = float(np.float32(0.5 * float(total)))
                gn = torch.nn.utils.clip_grad_norm_(sae.parameters(), max_norm=clip)
                opt.step()
                opt.zero_grad()
                for k_, v in (("mse", loss.mse), ("aux", loss.aux), ("l0", loss.l0), ("l1", loss.l1), ("n_dead", loss.n_dead),
                              ("grad_norm", gn), ("thr", sae.activation.threshold), ("gap", gap), ("bound", bound)):
                    rec[k_].append(float(v))
                rec["f_x"].append(o.f_x.detach().clone())
                rec["b_enc"].append(sae.b_enc.detach().clone())
                rec["b_dec"].append(sae.b_dec.detach().clone())
        if not ok:
            continue
        if max(rec["n_dead"]) >= 1 and max(rec["aux"]) > 0 and min(rec["grad_norm"]) > clip:
            break
    else:
        raise RuntimeError("no seed with dead latents, a non-zero AuxK term and clean gaps")
    print(f"train {tag}: seed {seed}, n_dead {rec['n_dead']}, aux {rec['aux']}, grad_norm {rec['grad_norm']} (clip {clip:.4g}), "
          f"thr {rec['thr']}, gap/bound {[g_ / b_ for g_, b_ in zip(rec['gap'], rec['bound'])]}")
    final = {k_: v.detach().clone() for k_, v in sae.state_dict().items()}
    G.npz(f"g20_batch_topk_train_{tag}", acts=acts, d=D, s=S, k=K, bsz=B, k_aux=K_AUX, alpha=ALPHA, momentum=MOMENTUM,
          thr_tokens=thr_tokens, lr=lr, grad_clip=clip, n_steps=n_steps,
          prefixes=np.array(fixed if fixed is not None else (S,), dtype=np.int64),
          toks_final=obj.toks_since_active,
          **{"init_" + k_.replace(".", "_"): v for k_, v in init.items()},
          **{"final_" + k_.replace(".", "_"): v for k_, v in final.items()},
          **{"log_" + k_: np.array(rec[k_], dtype=np.float64) for k_ in ("mse", "aux", "l0", "l1", "n_dead", "grad_norm", "thr", "gap", "bound")},
          f_x=torch.stack(rec["f_x"]), b_enc_steps=torch.stack(rec["b_enc"]), b_dec_steps=torch.stack(rec["b_dec"]))


def inference_fixture(ref, tag, with_labels):
    """framework/inference.worker_fn of the reference on a BatchTopK SAE in eval mode (as G19 does for ReLU)."""
    import scipy.sparse

    from saev_amd.data import shards as my_shards

    ordered = importlib.import_module("saev.data.ordered")
    ref.data.OrderedConfig, ref.data.OrderedDataLoader = ordered.Config, ordered.DataLoader
    inf = importlib.import_module("saev.framework.inference")
    rshards = importlib.import_module("saev.data.shards")

    d, s, n_ex, n_tok, layers = 32, 256, 13, 6, (5, 11)
    thr = 0.125
    rows = G.lowrank_data(n_ex * len(layers) * (n_tok + 1), d, seed=205 + with_labels)
    acts = rows.reshape(n_ex, len(layers), n_tok + 1, d).numpy()
    labels = None
    if with_labels:
        labels = np.random.default_rng(20).integers(0, 4, (n_ex, n_tok)).astype(np.uint8)
    tmp = pathlib.Path(tempfile.mkdtemp(prefix="g20_"))
    orig_load = inf.nn.load
    try:
        shards_dir = my_shards.write_shards(tmp, acts, layers=layers, cls_token=True,
                                            max_tokens_per_shard=4 * (n_tok + 1) * len(layers), labels=labels)
        md = rshards.Metadata.load(shards_dir)
        sae = make_sae(ref, d, s, 8, seed=207)
        # the first bias draw with no pre-activation within 2e-5 of the threshold (in fp64, on every token of the layer), so that
        # the CSR structure is the same under any fp32 summation order
        x_layer = torch.from_numpy(acts[:, layers.index(11), 1:, :].reshape(-1, d)).double()
        for bias_seed in range(208, 408):
            b_enc = -0.45 + 0.05 * torch.randn(s, generator=torch.Generator().manual_seed(bias_seed))
            if ((x_layer @ sae.W_enc.detach().double() + b_enc.double()) - thr).abs().min() >= 2e-5:
                break
        else:
            raise RuntimeError("no bias draw without a near-tie at the threshold")
        with torch.no_grad():
            sae.b_enc.copy_(b_enc)
            sae.b_dec.copy_(rows.mean(dim=0))
            sae.activation.threshold.fill_(thr)
        run = G.ref_disk_new(tmp, shards_dir)
        ref.modeling.dump(run / "checkpoint" / "sae.pt", sae)
        inf.nn.load = lambda *a, **kw: orig_load(*a, **kw).eval()  # (see the module docstring)
        cfg = inf.Config(run=run, data=ordered.Config(shards=shards_dir, layer=11, batch_size=4 * n_tok + 1),
                         n_dists=5, ignore_labels=[2] if with_labels else [], device="cpu")
        inf.worker_fn(cfg)
        out = run / "inference" / md.hash
        csr = scipy.sparse.load_npz(out / "token_acts.npz")
        metrics = json.loads((out / "metrics.json").read_text())
        print(f"inference {tag}: {csr.nnz} codes over {csr.shape[0]} tokens")
        assert csr.nnz > 0
        G.npz(f"g20_inference_batch_topk_{tag}", acts=acts, labels=labels if labels is not None else np.zeros((0, 0), np.uint8),
              layers=np.array(layers), n_dists=5, batch_size=4 * n_tok + 1,
              max_tokens_per_shard=4 * (n_tok + 1) * len(layers),
              ignore_labels=np.array([2] if with_labels else [], dtype=np.int64),
              ckpt=np.frombuffer((run / "checkpoint" / "sae.pt").read_bytes(), dtype=np.uint8),
              csr_data=csr.data, csr_indices=csr.indices, csr_indptr=csr.indptr, csr_shape=np.array(csr.shape),
              mean_values=torch.load(out / "mean_values.pt"), sparsity=torch.load(out / "sparsity.pt"),
              distributions=torch.load(out / "distributions.pt"),
              metrics_keys=np.array(list(metrics.keys())), metrics_vals=np.array([float(v) for v in metrics.values()]),
              threshold=thr)
    finally:
        inf.nn.load = orig_load
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ref = G._refshim.install()
    forward_fixture(ref)
    train_fixture(ref, "p1", None)
    train_fixture(ref, "p4", PREFIXES)
    inference_fixture(ref, "plain", False)
    inference_fixture(ref, "labels", True)


if __name__ == "__main__":
    main()
