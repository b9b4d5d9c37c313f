"""The dense ReLU train step beside the TopK and the BatchTopK step, at configs[1] (d_model 1 024, 32 x, k 32,
batch 16 384), on one device in one process.

    python tools/bench_relu_train.py [--iters 20] [--warmup 5] [--out profiles/relu_train_bench_line.json]

Measured twice -- at random init (b_enc = 0, W_enc = W_dec^T: about half of the latents fire in every row) and with b_enc shifted down
so that ~64 latents fire per row: a dense step should cost the same in both, and the line shows whether it does.  Per regime:
  * the whole step (``train_step``) of a ReLU, a TopK and a BatchTopK engine on the same parameters and batches, ALTERNATING step by
    step after a warm-up (host clock around work that ends in a device synchronise): median, interquartile range, min, max of --iters;
  * the ReLU phases one by one -- forward, dead-latent update, backward, tail -- the same way;
  * the ReLU step split by kernel, from a torch.profiler trace of --iters steps (device durations, no host time): the dense encode,
    the four contractions (x_hat = f W_dec, dA = g W_dec^T, dW_dec = f^T g, dW_enc = x^T dH: the step's launches of the split-fp16
    kernel in that order), the three element-wise kernels, the operand-image writes (split_both_kernel), the tail, everything else.
One JSON line.  A run without a HIP device fails: nothing here falls back."""
import argparse
import json
import pathlib
import statistics
import sys
import time

import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1]))

from saev_amd.engine import EngineConfig, SaeEngine  # noqa: E402

CONTRACTIONS = ("x_hat", "dA", "dW_dec", "dW_enc")


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def summary(ms):
    q = statistics.quantiles(ms, n=4)
    return {"median_ms": statistics.median(ms), "iqr_ms": q[2] - q[0], "min_ms": min(ms), "max_ms": max(ms), "n": len(ms)}


def kernel_split(eng, batches, lr, clip, iters, encoder):
    """Device time per step and kernel group, from a profiler trace of `iters` ReLU steps (phases: the kernels are the fused step's)."""
    from torch.profiler import ProfilerActivity, profile

    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for i in range(iters):
            eng.train_step(batches[i % len(batches)], lr, clip)
        torch.cuda.synchronize()
    evs = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    evs.sort(key=lambda e: e.time_range.start)
    groups = {}
    n_f16 = 0
    per_step_f16 = 4 + (1 if encoder == "f16x3" else 0)  # (the f16x3 encoder's dense h runs on the same kernel, first in the step)
    for e in evs:
        name, us = e.name, e.device_time if hasattr(e, "device_time") else e.cuda_time
        if "encode_f16x3_kernel" in name or "encode_m16_kernel" in name:
            pos = n_f16 % per_step_f16
            n_f16 += 1
            key = "encode" if per_step_f16 == 5 and pos == 0 else "contraction_" + CONTRACTIONS[pos - (per_step_f16 - 4)]
        elif "encode_gemm_kernel" in name:
            key = "encode"
        elif "relu_act_kernel" in name or "relu_mse_kernel" in name or "relu_dact_kernel" in name:
            key = name[name.index("relu_"):].split("(")[0].split("<")[0]
        elif "split_both_kernel" in name:
            key = "image_writes"
        elif "split_rows" in name or "split_wT" in name:
            key = "encode_images"
        elif "adam" in name or "rpg" in name or "sumsq" in name:
            key = "tail"
        elif "sum_parts" in name:
            key = "split_k_sums"
        else:
            key = "other"
        groups[key] = groups.get(key, 0.0) + us
    out = {k: v / iters / 1e3 for k, v in sorted(groups.items())}
    out["sum_ms"] = sum(out.values())
    return out


def regime(tag, params, batches, a, D, S, K, B):
    common = dict(d_model=D, d_sae=S, max_batch=B)
    relu = SaeEngine(EngineConfig(activation="relu_train", k_aux=0, l1_coeff=a.l1_coeff, **common))
    topk = SaeEngine(EngineConfig(top_k=K, k_aux=512, **common))
    btk = SaeEngine(EngineConfig(activation="batch_topk", top_k=K, k_aux=512, **common))
    engines = {"relu": relu, "topk": topk, "batch_topk": btk}
    for e in engines.values():
        e.load_params(params)
    lr, clip = 1e-4, 1.0
    for i in range(a.warmup):
        for e in engines.values():
            e.train_step(batches[i % len(batches)], lr, clip)
    step = {k: [] for k in engines}
    for i in range(a.iters):
        x = batches[i % len(batches)]
        for k, e in engines.items():
            step[k].append(timed(lambda e=e: e.train_step(x, lr, clip)))
    phases = {k: [] for k in ("forward", "dead", "backward", "tail")}
    for i in range(a.iters):
        x = batches[i % len(batches)]
        phases["forward"].append(timed(lambda: relu.step_forward(x, training=True)))
        phases["dead"].append(timed(lambda: relu.step_dead(B)))
        phases["backward"].append(timed(relu.step_backward))
        phases["tail"].append(timed(lambda: relu.step_tail(lr, clip)))
    relu.step_forward(batches[0], training=False)
    st = relu.read_stats()
    print(json.dumps({"regime": tag, "step": {k: summary(v) for k, v in step.items()}, "phases_relu": {k: summary(v) for k, v in phases.items()}}),
          flush=True)  # (the host-clock figures, in the log before the trace is taken)
    split = kernel_split(relu, batches, lr, clip, a.iters, relu.cfg.encoder)
    med = statistics.median(step["relu"])
    out = {
        "regime": tag, "l0_per_row": st.l0, "mse": st.mse,
        "step": {k: summary(v) for k, v in step.items()},
        "phases_relu": {k: summary(v) for k, v in phases.items()},
        "kernel_split_relu_ms_per_step": split,
        "relu_dense_tflops_executed": 5 * 2.0 * B * D * S / (med * 1e-3) / 1e12,  # (five fp32-accurate n x D x S products per step)
        "relu_scratch_gb": relu.scratch_bytes() / 1e9,
    }
    for e in engines.values():
        e.close()
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d-model", type=int, default=1024)
    ap.add_argument("--expansion", type=int, default=32)
    ap.add_argument("--top-k", type=int, default=32)
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--l1-coeff", type=float, default=4e-4)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="profiles/relu_train_bench_line.json")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_relu_train needs a HIP device")
    D, S, K, B = a.d_model, a.d_model * a.expansion, a.top_k, a.batch
    gen = torch.Generator().manual_seed(0)
    W_dec = torch.nn.init.kaiming_uniform_(torch.empty(S, D), generator=gen)
    W_dec /= W_dec.norm(dim=1, keepdim=True)
    params = {"W_dec": W_dec, "b_dec": torch.zeros(D), "W_enc": W_dec.T.contiguous(), "b_enc": torch.zeros(S)}
    # low-rank-plus-noise activations, a few batches cycled
    atoms = torch.randn(4 * D, D, generator=gen)
    atoms /= atoms.norm(dim=1, keepdim=True)
    batches = []
    for _ in range(4):
        codes = torch.zeros(B, 4 * D)
        pick = torch.randint(0, 4 * D, (B, 16), generator=gen)
        codes.scatter_(1, pick, torch.empty(B, 16).exponential_(1.0, generator=gen))
        batches.append((codes @ atoms + 0.1 * torch.randn(B, D, generator=gen)).cuda())
    # the shift that leaves ~64 latents per row: the (1 - 64 / S) quantile of the pre-activations of one batch's first rows
    h = batches[0][:512].cpu() @ params["W_enc"]
    shift = float(h.flatten().kthvalue(int(h.numel() * (1 - 64.0 / S))).values)
    sparse = dict(params, b_enc=torch.full((S,), -shift))
    line = {
        "bench": "relu_train", "device": torch.cuda.get_device_name(0), "d_model": D, "d_sae": S, "top_k": K, "batch": B,
        "l1_coeff": a.l1_coeff, "encoder": EngineConfig(d_model=D, d_sae=S).encoder,
        "regimes": [regime("random_init", params, batches, a, D, S, K, B), regime("b_enc_shifted", sparse, batches, a, D, S, K, B)],
        "timing_note": "step / phases: host-synchronised wall times, each one launch sequence; kernel split: device durations of a profiler trace",
    }
    out = pathlib.Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(line) + "\n")
    print(json.dumps(line))


if __name__ == "__main__":
    main()
