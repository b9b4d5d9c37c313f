"""How well does a row's norm predict its TopK bound?  (profiles/rho_predictor_probe.txt is this tool's output.)

For a row b of a batch, T_b is the exact k-th largest pre-activation and rho_b = T_b / ||x_b - mu|| with mu the centring vector of
the streamed preparation (the previous batch's column mean).  A predictor "bound_b = c * rho_lo * ||x_b - mu||" with rho_lo a low
order statistic of the PREVIOUS step's ratios is only worth building if rho clusters tightly within a step and drifts slowly from
step to step.  This tool runs the benchmark's loop (configs[1], draw from a pool + train step) on the three data regimes of
bench.py and, around steps 25, 700 and 1 500, recomputes every row's pre-activations densely (fp32 matmul on the parameters as they
stand in front of the step) and prints

  * the spread of rho within the step (quantiles relative to the median);
  * the drift of min rho and of its 0.1 % quantile against the step before;
  * for c = 0.98, 0.95, 0.9 and rho_lo = the previous step's minimum / 0.1 % quantile: candidates per row the bound would leave
    (number of pre-activations >= bound_b - 2 E_b, mean and longest list over ALL rows of the batch) and the number of rows whose
    prediction would have failed (bound_b > T_b);
  * for comparison, the longest list of the step's guaranteed-bound encoder (StepStats.cand_max).

2 E_b is the f16r margin of select.hip with the a-priori rounding terms scaled by the 0.38 measured on this data; it
moves the counts by a few per cent only.

    python tools/experiments/rho_predictor_probe.py [--kinds mean,isotropic,lowrank] [--at 25,700,1500]
"""

import argparse
import math
import pathlib
import sys

import torch

ROOT = pathlib.Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

import bench  # noqa: E402  (shapes and pools of the benchmark)
from saev_amd.engine import EngineConfig, SaeEngine  # noqa: E402

QS = (0.0, 1e-4, 1e-3, 1e-2, 0.5, 0.99, 1.0)


def quantiles(v):
    s = v.sort().values
    n = s.numel()
    return [s[min(n - 1, int(q * (n - 1) + 0.5))].item() for q in QS]


def probe(eng, xb, mu, k):
    """rho, T, norms and dense pre-activations of the batch xb on the engine's current parameters."""
    h = torch.addmm(eng.view("b_enc"), xb, eng.view("W_enc"))
    T = h.topk(k, dim=1).values[:, -1]
    nrm = (xb - mu).norm(dim=1)
    dxn = (xb - mu - (xb - mu).half().float()).norm(dim=1)  # what the fp16 image of the row loses (up to its power-of-two scale)
    wn = eng.view("W_enc").norm(dim=0).max()
    D = xb.shape[1]
    e_b = 1.02 * (dxn * wn + 0.38 * 2.0**-11 * nrm * wn) + (1.05 * D * 2.0**-22 + 2.0**-17) * nrm * wn
    return h, T, nrm, 2.0 * e_b


def run(kind, at, dev):
    B, D, S, K = bench.BATCH, bench.D_MODEL, bench.D_SAE, bench.TOP_K
    pool_batches = bench.POOL_BATCHES if kind == "mean" else 16
    cfg = (EngineConfig(d_model=D, d_sae=S, top_k=K, max_batch=B, dead_threshold_tokens=10_000_000) if kind == "mean"
           else EngineConfig(d_model=D, d_sae=S, top_k=K, max_batch=B, aux_dead_cap=4096))
    eng = SaeEngine(cfg, dev)
    g = torch.Generator(device=dev).manual_seed(42)
    W = (torch.rand(S, D, device=dev, generator=g) * 2 - 1) * math.sqrt(6.0 / D)
    W /= W.norm(dim=1, keepdim=True)
    eng.view("W_dec").copy_(W)
    eng.view("W_enc").copy_(W.t())
    del W
    pool = bench.synthetic_pool(dev, kind, pool_batches * B, D)
    perm = torch.randperm(pool.shape[0], device=dev, generator=g)
    x = torch.empty(B, D, device=dev)
    rows_of = lambda i: perm[(i % pool_batches) * B:(i % pool_batches + 1) * B]  # noqa: E731
    want = sorted({s + o for s in at for o in (-1, 0, 1)})
    prev = None  # (step, min rho, 0.1 % quantile of rho)
    print(f"== {kind}: d_model {D}, d_sae {S}, k {K}, batch {B}, pool of {pool_batches} batches ==", flush=True)
    for i in range(max(want) + 1):
        if i in want and i > 0:
            xb = pool[rows_of(i)]
            mu = pool[rows_of(i - 1)].mean(dim=0)
            h, T, nrm, m2 = probe(eng, xb, mu, K)
            rho = T / nrm
            q = quantiles(rho)
            med = q[4]
            print(f"step {i}: ||x - mu|| min/median/max {nrm.min().item():.4g} / {nrm.median().item():.4g} / {nrm.max().item():.4g}; "
                  f"T min/median/max {T.min().item():.4g} / {T.median().item():.4g} / {T.max().item():.4g}; "
                  f"margin 2E median {m2.median().item():.3g}")
            print("  rho quantiles (min, 1e-4, 1e-3, 1e-2, median, 0.99, max): " + " ".join(f"{v:.5g}" for v in q))
            print("  relative to the median:                                   " + " ".join(f"{v / med:.4f}" for v in q))
            print(f"  survivors of the exact cut itself (h >= T - 2E): mean {(h >= (T - m2)[:, None]).sum(1).float().mean().item():.1f}")
            if prev is not None and prev[0] == i - 1:
                print(f"  drift against step {i - 1}: min rho {q[0] / prev[1] - 1:+.4%}, 1e-3 quantile {q[2] / prev[2] - 1:+.4%}")
                for name, lo in (("previous min", prev[1]), ("previous 1e-3 quantile", prev[2])):
                    for c in (0.98, 0.95, 0.9):
                        bound = c * lo * nrm
                        cnt = (h >= (bound - m2)[:, None]).sum(1)
                        fails = int((bound > T).sum().item())
                        print(f"  rho_lo = {name}, c = {c}: candidates per row mean {cnt.float().mean().item():.1f} longest {int(cnt.max().item())}; "
                              f"rows with bound > T: {fails} of {B}")
            prev = (i, q[0], q[2])
            del h
        eng.train_step_gather(pool, rows_of(i), 4e-4 * min(1.0, i / 500), 1.0, out=x)
        if i in want:
            st = eng.read_stats()
            print(f"  the step's own encoder (guaranteed bounds): longest list {st.cand_max}, dense route {st.dense_route}, "
                  f"overflowing rows {st.n_overflow_rows}, mse {st.mse:.5f}, dead {st.n_dead}", flush=True)
    eng.close()
    del eng, pool
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kinds", default="mean,isotropic,lowrank")
    ap.add_argument("--at", default="25,700,1500")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    for kind in args.kinds.split(","):
        run(kind, [int(s) for s in args.at.split(",")], dev)


if __name__ == "__main__":
    main()
