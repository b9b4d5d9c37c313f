"""Generate the intervention golden vectors (G30) by RUNNING the upstream reference's SparseAutoencoder (build container only).

Test infrastructure beside ``oracle/gen_golden.py`` (imported for its helpers and the reference import shim, left unchanged).
The reference's own intervention module (contrib/interactive_interp/semseg) imports packages that no longer exist, so its
experiment is restated here on the reference's SAE: ``(x - x_hats[:, -1]) + sae.decode(f_mod)[:, -1]`` with ``f_mod`` the dense
``f_x`` after one global SET and a per-class SET list.  Output: ``tests/golden/g30_interventions.npz`` with, for a TopK (k = 4)
and a ReLU SAE (D = 32, S = 128, 48 rows): the parameters, x, the reference's dense f_x, row labels (0..5, some outside), the
edits, the reference's output and

    bound_ref = 2 (K + 3) 2^-24 (|x_d| + |b_dec,d| + sum_j |f_j| |W_j,d| + sum_e |t_e| |W_l_e,d|)

K the largest non-zero count of an edited row: the standard bound for the two rounded sums (x_hat and the modified decode, in any
order), plus the two element-wise roundings.  The generator asserts that the reference's output lies within it of fp64.

    python tools/gen_golden_interventions.py
"""

import pathlib
import sys

import numpy as np
import torch

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "oracle"))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT))
import gen_golden as G  # noqa: E402
import interventions_restatement as IR  # noqa: E402

D, S, N, C = 32, 128, 48, 6


def make(ref, kind: str):
    torch.manual_seed(300 + (kind == "relu"))
    if kind == "topk":
        act = ref.modeling.TopK(top_k=4)
    else:
        act = ref.modeling.Relu()
    sae = ref.modeling.SparseAutoencoder(ref.modeling.SparseAutoencoderConfig(d_model=D, d_sae=S, reinit_blend=0.0, activation=act))
    x = G.lowrank_data(N, D, seed=302 + (kind == "relu"))
    with torch.no_grad():
        sae.b_dec.copy_(0.1 * torch.randn(D))
        sae.W_enc.add_(0.02 * torch.randn(D, S))
        if kind == "relu":  # a few positives per row
            sae.b_enc.copy_(-torch.quantile((x @ sae.W_enc).flatten(), 0.93) + 0.02 * torch.randn(S))
        else:
            sae.b_enc.copy_(0.05 * torch.randn(S))
    return sae, x


def fixture(ref, kind: str) -> dict:
    sae, x = make(ref, kind)
    rng = np.random.default_rng(304 + (kind == "relu"))
    labels = rng.integers(0, C, N).astype(np.int32)
    labels[[3, 17]] = -1
    labels[[8, 40]] = C + 1
    with torch.no_grad():
        out = sae(x)
        f_x = out.f_x.clone()
        fired = (f_x != 0).sum(dim=0)
        # the global edit sets a latent that fires in some rows and not in others; the class edits one latent each
        order = torch.argsort(fired, descending=True)
        g_lat = int(order[0])
        c_lat = [int(order[1 + c]) for c in range(C - 1)] + [S - 1]
        edits = [(g_lat, IR.SET, 2.5, -1)] + [(c_lat[c], IR.SET, float(-1.0 + 0.75 * c), c) for c in range(C)]
        f_mod = f_x.clone()
        f_mod[:, g_lat] = 2.5
        for b in range(N):
            if 0 <= labels[b] < C:
                f_mod[b, c_lat[labels[b]]] = float(-1.0 + 0.75 * labels[b])
        ref_out = (x - out.x_hats[:, -1]) + sae.decode(f_mod)[:, -1]
    W, b_dec = sae.W_dec.detach().numpy(), sae.b_dec.detach().numpy()
    K = int((f_mod != 0).sum(dim=1).max())
    absW = np.abs(W).astype(np.float64)
    sum_f = np.abs(f_x.numpy()).astype(np.float64) @ absW
    sum_t = np.zeros((N, D))
    for b in range(N):
        sum_t[b] += 2.5 * absW[g_lat]
        if 0 <= labels[b] < C:
            sum_t[b] += abs(-1.0 + 0.75 * labels[b]) * absW[c_lat[labels[b]]]
    bound = 2 * (K + 3) * 2.0 ** -24 * (np.abs(x.numpy()).astype(np.float64) + np.abs(b_dec)[None] + sum_f + sum_t)
    # fp64 from the reference's own codes
    nz = f_x != 0
    cap = int(nz.sum(dim=1).max())
    idx = np.full((N, cap), -1, dtype=np.int32)
    val = np.zeros((N, cap), dtype=np.float32)
    nnz = nz.sum(dim=1).numpy().astype(np.int32)
    for b in range(N):
        cols = torch.nonzero(nz[b]).flatten().numpy()
        idx[b, :len(cols)] = cols
        val[b, :len(cols)] = f_x[b, cols].numpy()
    exact = IR.intervene(x.numpy(), W, idx, val, nnz, edits, C, row_group=labels)
    err = np.abs(ref_out.numpy().astype(np.float64) - exact["out"])
    assert (err <= bound).all(), f"{kind}: the reference lies outside its own bound ({(err / bound).max():.3f} of it)"
    print(f"{kind}: K {K}, row capacity {cap}, reference error at most {(err / bound).max():.3f} of bound_ref")
    return {f"{kind}_{k}": v for k, v in dict(
        W_dec=W, b_dec=b_dec, W_enc=sae.W_enc.detach().numpy(), b_enc=sae.b_enc.detach().numpy(), x=x.numpy(), f_x=f_x.numpy(),
        labels=labels, edit_latent=np.array([e[0] for e in edits], dtype=np.int32), edit_op=np.array([e[1] for e in edits], dtype=np.int32),
        edit_value=np.array([e[2] for e in edits], dtype=np.float32), edit_group=np.array([e[3] for e in edits], dtype=np.int32),
        out_ref=ref_out.numpy(), bound_ref=bound, K=K).items()}


def main():
    ref = G._refshim.install()
    arrays = {"n_groups": C}
    for kind in ("topk", "relu"):
        arrays.update(fixture(ref, kind))
    G.npz("g30_interventions", **arrays)


if __name__ == "__main__":
    main()
