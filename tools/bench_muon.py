"""Muon at bench.py's workload (configs[1]: d_model 1024, d_sae 32768, k 32, batch 16384) on one device -> one JSON line:

  adam_step_ms     SaeEngine.train_step (the fused Adam step), ms per step
  muon_step_ms     SaeEngine.train_step_muon (phases + saev_muon_tail), ms per step, same process, same batches
  ns_ms            the Newton-Schulz iteration alone (5 steps, both matrices: the HIP kernels of the tail), its TFLOP/s and
                   fraction of the 2.5 PF dense bf16 peak
  torch_ns_ms      torch.optim._muon._zeropower_via_newtonschulz on the same two matrices, same card (the vendor BLAS)

All timings are HIP events around back-to-back launches after a warm-up.

    python tools/bench_muon.py [--steps N] [--warmup W]
"""
import argparse
import json
import pathlib
import sys

import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1]))

from saev_amd.engine import EngineConfig, MuonConfig, SaeEngine, newton_schulz  # noqa: E402

D, S, K, B = 1024, 32768, 32, 16384
PEAK_TFLOPS = 2500.0


def timed(fn, n: int) -> float:
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(n):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    pool = torch.randn(8, B, D, device=dev, generator=g) + 0.5
    engines = {}
    for name in ("adam", "muon"):
        e = SaeEngine(EngineConfig(d_model=D, d_sae=S, top_k=K, max_batch=B, aux_dead_cap=4096), dev)
        W = torch.randn(S, D, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
        W /= W.norm(dim=1, keepdim=True)
        e.view("W_dec").copy_(W)
        e.view("W_enc").copy_(W.t())
        e.params_touched()
        engines[name] = e
    steps = {"adam": lambda i: engines["adam"].train_step(pool[i % 8], 1e-4, 1.0),
             "muon": lambda i: engines["muon"].train_step_muon(pool[i % 8], 1e-4, 1.0)}
    out = {"config": {"d_model": D, "d_sae": S, "top_k": K, "batch": B}, "steps": args.steps}
    for name, fn in steps.items():
        timed(fn, args.warmup)
        out[f"{name}_step_ms"] = round(timed(fn, args.steps), 4)
    mats = [(torch.randn(S, D, device=dev, generator=g) * 1e-3), (torch.randn(D, S, device=dev, generator=g) * 1e-3)]
    flop = 5 * 2 * (2 * D * D * S + 2 * D ** 3 + 2 * D * D * S)
    cfg = MuonConfig()

    def ours(i):
        for m in mats:
            newton_schulz(m, cfg)

    def theirs(i):
        from torch.optim._muon import _zeropower_via_newtonschulz

        for m in mats:
            _zeropower_via_newtonschulz(m, cfg.ns_coefficients, cfg.ns_steps, cfg.eps)

    for name, fn in (("ns", ours), ("torch_ns", theirs)):
        timed(fn, args.warmup)
        ms = timed(fn, args.steps)
        out[f"{name}_ms"] = round(ms, 4)
        out[f"{name}_tflops"] = round(flop / ms / 1e9, 1)
        out[f"{name}_peak_fraction"] = round(flop / ms / 1e9 / PEAK_TFLOPS, 3)
    out["muon_minus_adam_ms"] = round(out["muon_step_ms"] - out["adam_step_ms"], 4)
    out["muon_scratch_bytes"] = engines["muon"].scratch_bytes(3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
