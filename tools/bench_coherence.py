"""Dictionary coherence (the log block's metrics/dictionary_coherence) on one device -> one JSON line:

  <shape>.<rows>.hip_ms         saev_dictionary_coherence (engine.dictionary_coherence, one read-back included), its TFLOP/s
                                and fraction of the 2.5 PF dense fp16 peak, counting S (S - 1) D flops (the upper triangle)
  <shape>.<rows>.torch_ms       the torch expression the train loop used before (4 096-row blocks, vendor BLAS), same card
  <shape>.<rows>.candidates     candidate pairs the filter kept, the list capacity, the route taken, workspace bytes
  train_e2e                     train() at configs[1] on a resident synthetic feed: steps/s with log_every=25 against
                                log_every=10**9, and the ms a log step adds

shapes: configs[1] (S 32 768, D 1 024) and configs[3] (S 81 920, D 1 280).  rows: "random" (Gaussian rows) and "trained"
(datapoint initialisation from low-rank data: rows are samples x = z U + noise with rank-64 U, as the reference's
data-initialised decoder starts).  Timings are HIP events around back-to-back calls after a warm-up.

    python tools/bench_coherence.py [--reps N] [--no-train]
"""
import argparse
import json
import os
import pathlib
import sys
import tempfile
import time

import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1]))

from saev_amd import _lib  # noqa: E402
from saev_amd.engine import dictionary_coherence  # noqa: E402

SHAPES = {"configs1": (32768, 1024), "configs3": (81920, 1280)}
PEAK_TFLOPS = 2500.0


def torch_coherence(W: torch.Tensor, block: int = 4096) -> float:
    """The train loop's former _coherence: a torch matmul in row blocks."""
    Wn = W / W.norm(dim=1, keepdim=True)
    best = 0.0
    for lo in range(0, Wn.shape[0], block):
        g = torch.triu((Wn[lo : lo + block] @ Wn[lo:].T).abs(), diagonal=1)
        best = max(best, g.max().item())
    return best


def rows(kind: str, S: int, D: int, dev) -> torch.Tensor:
    g = torch.Generator(device=dev).manual_seed(S + D)
    if kind == "random":
        return torch.randn(S, D, device=dev, generator=g)
    U = torch.randn(64, D, device=dev, generator=g)
    z = torch.randn(S, 64, device=dev, generator=g)
    return z @ U + 0.3 * torch.randn(S, D, device=dev, generator=g)


def timed(fn, n: int) -> float:
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def train_rate(log_every: int, steps: int, shards: str, root: str) -> float:
    """train() at configs[1] (d_model 1 024, d_sae 32 768, k 32, batch 16 384) on the resident synthetic cache `shards`; steps/s
    over the train loop after make_saes."""
    from saev_amd import data, nn
    from saev_amd.framework import train as T
    from saev_amd.nn import modeling, objectives

    D, B = 1024, 16384
    os.environ["SAEV_AMD_RESIDENT_GB"] = "1000"
    dcfg = data.ShuffledConfig(shards=shards, layer=23, batch_size=B, n_threads=4)
    cfg = T.Config(train_data=dcfg, val_data=dcfg, n_train=steps * B, n_val=B,
                   sae=nn.SparseAutoencoderConfig(d_model=D, d_sae=32 * D, reinit_blend=0.0, activation=modeling.TopK(top_k=32)),
                   objective=objectives.Matryoshka(n_prefixes=1), log_every=log_every, track=False,
                   runs_root=os.path.join(root, "runs"), device="cuda")
    import saev_amd.utils.scheduling as sched

    t = {}
    orig = sched.BatchLimiter.__iter__

    def timed_iter(self, _orig=orig):
        torch.cuda.synchronize()
        t["t0"] = time.perf_counter()
        yield from _orig(self)

    sched.BatchLimiter.__iter__ = timed_iter
    try:
        _, _, _, n = T.train([cfg])
    finally:
        sched.BatchLimiter.__iter__ = orig
    torch.cuda.synchronize()
    return n / (time.perf_counter() - t["t0"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--train-steps", type=int, default=400)
    ap.add_argument("--no-train", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _lib.load()
    out = {"peak_tflops": PEAK_TFLOPS}
    for name, (S, D) in SHAPES.items():
        flop = S * (S - 1) * D
        for kind in ("trained", "random"):
            W = rows(kind, S, D, dev)
            r = dictionary_coherence(W)
            rec = {"value": r.value, "pair": [r.i, r.j], "route": r.route, "overflow": r.overflow, "candidates": r.candidates,
                   "capacity": r.capacity, "tiles_refiltered": r.tiles_refiltered, "tiles": (S + 127) // 128 * ((S + 127) // 128 + 1) // 2,
                   "workspace_bytes": int(lib.saev_coherence_workspace_bytes(S, D))}
            ms = timed(lambda: dictionary_coherence(W), args.reps)
            rec.update(hip_ms=round(ms, 4), hip_tflops=round(flop / ms / 1e9, 1), hip_peak_fraction=round(flop / ms / 1e9 / PEAK_TFLOPS, 3))
            tv = torch_coherence(W)
            tms = timed(lambda: torch_coherence(W), max(2, args.reps // 3))
            rec.update(torch_value=tv, torch_ms=round(tms, 3), speedup=round(tms / ms, 1))
            ems = timed(lambda: dictionary_coherence(W, route="exact"), 2)
            rec["exact_route_ms"] = round(ems, 3)
            out[f"{name}.{kind}"] = rec
            del W
            torch.cuda.empty_cache()
    if not args.no_train:
        import numpy as np

        from saev_amd import data

        with tempfile.TemporaryDirectory(prefix="coh_") as root:
            Tk = 64
            acts = np.random.default_rng(0).standard_normal((1024, 1, Tk + 1, 1024), dtype=np.float32)
            shards = data.write_shards(root, acts, layers=(23,), cls_token=True, max_tokens_per_shard=(Tk + 1) * 1024)
            n = args.train_steps
            fast = train_rate(10**9, n, shards, root)
            logged = train_rate(25, n, shards, root)
            out["train_e2e"] = {"config": "configs[1]", "steps": n, "steps_per_s_log_every_1e9": round(fast, 2),
                                "steps_per_s_log_every_25": round(logged, 2),
                                "ms_per_log_step": round((1 / logged - 1 / fast) * 25 * 1e3, 2)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
