"""Generate the ReLU training golden vectors (G22) by RUNNING the upstream reference on the CPU (build container only).

Test infrastructure beside ``oracle/`` (it imports ``oracle/gen_golden.py`` for its helpers and the reference import shim and
changes nothing there).  The reference is read from its own location at generation time only; the outputs are data under
``tests/golden/``:

  g22_relu_train_l1           a 4-step Adam trajectory of the reference's loop body (renormalise, objective, backward,
                              remove_parallel_grads, clip, fused Adam; train.py:332-460) of ``Relu(sparsity=L1Sparsity(coeff=1e-2))``
                              with the plain objective (n_prefixes = 1), every step clipped: per step the batch, mse, sparsity, l0,
                              l1, n_dead, the gradient norm, f_x and the biases; initial and final parameters; the four gradients of
                              step 1 (as autograd leaves them: before remove_parallel_grads and the clip)
  g22_relu_train_nosparsity   the same with ``Relu(sparsity=NoSparsity())``

A few latents start with b_enc = -6 and dead_threshold_tokens = 2 B: they never fire, n_dead > 0 from step 2, and their gradient
rows are exactly zero.

No pre-activation near zero: seeds are searched until, at EVERY recorded forward, min |h| in fp64 is at least 16 x the fp32 bound
8 * 2^-24 * max_b ||x_b|| * max_s ||W_enc[:, s]|| + 2^-23 * max |b_enc| (the bound of tests/test_gpu_relu.py) -- the mask f > 0
computed in fp32 in any summation order is then the reference's.  Gaps and bounds are stored in the fixtures.  (D = 32, S = 128,
B = 64: at D = 64, S = 256, B = 96 no seed in 600 reaches the factor 16 -- four times as many entries per step.)

    python tools/gen_golden_relu_train.py
"""

import pathlib
import sys

import numpy as np
import torch

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "oracle"))
sys.path.insert(0, str(ROOT))
import gen_golden as G  # noqa: E402

D, S, B = 32, 128, 64
N_SILENT = 3          # latents with b_enc = -6
GAP_FACTOR = 16.0


def make_sae(ref, sparsity, seed):
    torch.manual_seed(seed)
    cfg = ref.modeling.SparseAutoencoderConfig(d_model=D, d_sae=S, reinit_blend=0.0,
                                               activation=ref.modeling.Relu(sparsity=sparsity, aux=ref.modeling.NoAux()))
    sae = ref.modeling.SparseAutoencoder(cfg)
    silent = torch.randperm(S)[:N_SILENT].sort().values
    with torch.no_grad():
        sae.b_enc.copy_(0.05 * torch.randn(S))
        sae.b_dec.copy_(0.1 * torch.randn(D))
        sae.W_enc.add_(0.02 * torch.randn(D, S))
        sae.b_enc[silent] = -6.0
    return sae, silent


def zero_gap(sae, x):
    """(gap, bound): min |h| in fp64 and the fp32 bound of a pre-activation's error."""
    with torch.no_grad():
        h = x.double() @ sae.W_enc.double() + sae.b_enc.double()
        gap = float(h.abs().min())
        bound = (8.0 * 2.0 ** -24 * float(x.double().norm(dim=1).max()) * float(sae.W_enc.double().norm(dim=0).max())
                 + 2.0 ** -23 * float(sae.b_enc.abs().max()))
    return gap, bound


def train_fixture(ref, tag, sparsity, n_steps=4, lr=1e-3):
    thr_tokens = 2 * B
    for seed in range(2200, 3200):
        sae, silent = make_sae(ref, sparsity, seed)
        sae.train()
        obj = ref.objectives.get_objective(ref.objectives.Matryoshka(n_prefixes=1, dead_threshold_tokens=thr_tokens))
        obj.train()
        init = {k_: v.detach().clone() for k_, v in sae.state_dict().items()}
        acts = G.lowrank_data(n_steps * B, D, seed=seed + 5000)
        opt = torch.optim.Adam([{"params": list(sae.parameters()), "lr": lr}], fused=True)
        keys = ("mse", "sparsity", "l0", "l1", "n_dead", "grad_norm", "gap", "bound")
        rec = {k_: [] for k_ in keys + ("f_x", "b_enc", "b_dec")}
        clip, ok, grads1 = None, True, None
        for i in range(n_steps):
            x = acts[i * B:(i + 1) * B]
            sae.normalize_w_dec()
            gap, bound = zero_gap(sae, x)
            if gap < GAP_FACTOR * bound:
                ok = False
                break
            loss, o = obj(sae, x)
            loss.loss.backward()
            if i == 0:
                grads1 = {k_: p.grad.detach().clone() for k_, p in sae.named_parameters()}
            sae.remove_parallel_grads()
            if clip is None:  # half of the first step's gradient norm: every step is clipped
                total = torch.sqrt(sum((p.grad.double() ** 2).sum() for p in sae.parameters()))
                clip = float(np.float32(0.5 * float(total)))
            gn = torch.nn.utils.clip_grad_norm_(sae.parameters(), max_norm=clip)
            opt.step()
            opt.zero_grad()
            for k_, v in (("mse", loss.mse), ("sparsity", loss.sparsity), ("l0", loss.l0), ("l1", loss.l1), ("n_dead", loss.n_dead),
                          ("grad_norm", gn), ("gap", gap), ("bound", bound)):
                rec[k_].append(float(v))
            rec["f_x"].append(o.f_x.detach().clone())
            rec["b_enc"].append(sae.b_enc.detach().clone())
            rec["b_dec"].append(sae.b_dec.detach().clone())
        if not ok:
            continue
        f_all = torch.stack(rec["f_x"])
        if rec["n_dead"][1] >= 1 and min(rec["grad_norm"]) > clip and float(f_all[:, :, silent].abs().max()) == 0.0:
            break
    else:
        raise RuntimeError("no seed with clean gaps, dead latents from step 2 and every step clipped")
    nnz = (f_all > 0).sum(dim=2)
    print(f"train {tag}: seed {seed}, codes per row {int(nnz.min())}..{int(nnz.max())}, n_dead {rec['n_dead']}, "
          f"grad_norm {rec['grad_norm']} (clip {clip:.4g}), gap/bound {[g_ / b_ for g_, b_ in zip(rec['gap'], rec['bound'])]}")
    final = {k_: v.detach().clone() for k_, v in sae.state_dict().items()}
    coeff = float(sparsity.coeff) if hasattr(sparsity, "coeff") else 0.0
    G.npz(f"g22_relu_train_{tag}", acts=acts, d=D, s=S, bsz=B, l1_coeff=coeff, thr_tokens=thr_tokens, lr=lr, grad_clip=clip,
          n_steps=n_steps, silent=silent, toks_final=obj.toks_since_active,
          **{"init_" + k_: v for k_, v in init.items()},
          **{"final_" + k_: v for k_, v in final.items()},
          **{"grad1_" + k_: v for k_, v in grads1.items()},
          **{"log_" + k_: np.array(rec[k_], dtype=np.float64) for k_ in keys},
          f_x=f_all, b_enc_steps=torch.stack(rec["b_enc"]), b_dec_steps=torch.stack(rec["b_dec"]))


def main():
    ref = G._refshim.install()
    train_fixture(ref, "l1", ref.modeling.L1Sparsity(coeff=1e-2))
    train_fixture(ref, "nosparsity", ref.modeling.NoSparsity())


if __name__ == "__main__":
    main()
