"""The BatchTopK train step beside the TopK step, at configs[1] (d_model 1 024, 32 x, k 32, batch 16 384), on
one device in one process.

    python tools/bench_batch_topk.py [--iters 20] [--warmup 5] [--out profiles/batch_topk_bench_line.json]

Measured, all from the host clock around work that ends in a device synchronise (the BatchTopK forward synchronises by itself: it
reads its overflow word back):
  * the whole step (``train_step``) of a BatchTopK engine and of a TopK engine on the same parameters and batches, ALTERNATING
    step by step after a warm-up that covers every shape and lets the BatchTopK rows grow to their size: median, interquartile
    spread, min, max;
  * the BatchTopK phases one by one -- forward (dense encode + select + compaction + decode), dead-latent update, backward, tail;
  * inside the forward: the dense encode (``encode_dense``) and select + compaction (``batch_topk_dense`` on that h) on their own,
    with the bytes they must move (h written once by the encoder; read twice by the select -- histogram pass and list pass -- and
    once by the compaction) over their time as a share of the 6.29 TB/s of a float4 copy.
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

HBM_COPY = 6.29e12


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def summary(ms):
    q = statistics.quantiles(ms, n=4)
    return {"median_ms": statistics.median(ms), "iqr_ms": q[2] - q[0], "min_ms": min(ms), "max_ms": max(ms), "n": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d-model", type=int, default=1024)
    ap.add_argument("--expansion", type=int, default=32)
    ap.add_argument("--top-k", type=int, default=32)
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="profiles/batch_topk_bench_line.json")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_batch_topk needs a HIP device")
    D, S, K, B = a.d_model, a.d_model * a.expansion, a.top_k, a.batch
    gen = torch.Generator().manual_seed(0)
    W_dec = torch.nn.init.kaiming_uniform_(torch.empty(S, D), generator=gen)
    W_dec /= W_dec.norm(dim=1, keepdim=True)
    params = {"W_dec": W_dec, "b_dec": torch.zeros(D), "W_enc": W_dec.T.contiguous(), "b_enc": torch.zeros(S)}
    common = dict(d_model=D, d_sae=S, top_k=K, k_aux=512, max_batch=B)
    btk = SaeEngine(EngineConfig(activation="batch_topk", **common))
    topk = SaeEngine(EngineConfig(**common))
    for e in (btk, topk):
        e.load_params(params)
    # low-rank-plus-noise activations, a few batches cycled (the selection changes from batch to batch)
    atoms = torch.randn(4 * D, D, generator=gen)
    atoms /= atoms.norm(dim=1, keepdim=True)
    batches = []
    for _ in range(4):
        codes = torch.zeros(B, 4 * D)
        pick = torch.randint(0, 4 * D, (B, 16), generator=gen)
        codes.scatter_(1, pick, torch.empty(B, 16).exponential_(1.0, generator=gen))
        batches.append((codes @ atoms + 0.1 * torch.randn(B, D, generator=gen)).cuda())
    lr, clip = 1e-4, 1.0
    for i in range(a.warmup):
        x = batches[i % len(batches)]
        btk.train_step(x, lr, clip)
        topk.train_step(x, lr, clip)
    regrows_warm = btk.row_regrows
    step = {"batch_topk": [], "topk": []}
    for i in range(a.iters):
        x = batches[i % len(batches)]
        step["batch_topk"].append(timed(lambda: btk.train_step(x, lr, clip)))
        step["topk"].append(timed(lambda: topk.train_step(x, lr, clip)))
    phases = {k: [] for k in ("forward", "dead", "backward", "tail")}
    parts = {k: [] for k in ("encode_dense", "select_compact_train", "select_compact_eval")}
    for i in range(a.iters):
        x = batches[i % len(batches)]
        phases["forward"].append(timed(lambda: btk.step_forward(x, training=True)))
        phases["dead"].append(timed(lambda: btk.step_dead(B)))
        phases["backward"].append(timed(btk.step_backward))
        phases["tail"].append(timed(lambda: btk.step_tail(lr, clip)))
    h = btk.encode_dense(batches[0])
    for i in range(a.iters):
        parts["encode_dense"].append(timed(lambda: btk.encode_dense(batches[i % len(batches)])))
        parts["select_compact_train"].append(timed(lambda: btk.batch_topk_dense(h, training=True)))
        parts["select_compact_eval"].append(timed(lambda: btk.batch_topk_dense(h, training=False)))
    st = btk.batch_topk_state()
    h_bytes = 4.0 * B * S
    med = {k: statistics.median(v) for k, v in parts.items()}
    line = {
        "bench": "batch_topk", "device": torch.cuda.get_device_name(0), "d_model": D, "d_sae": S, "top_k": K, "batch": B,
        "row_cap": btk.row_cap, "row_regrows_in_warmup": regrows_warm, "row_regrows_timed": btk.row_regrows - regrows_warm,
        "step": {k: summary(v) for k, v in step.items()},
        "step_ratio_batch_topk_over_topk": statistics.median(step["batch_topk"]) / statistics.median(step["topk"]),
        "phases_batch_topk": {k: summary(v) for k, v in phases.items()},
        "forward_parts": {k: summary(v) for k, v in parts.items()},
        "encode_dense_tflops_fp32": 2.0 * B * D * S / (med["encode_dense"] * 1e-3) / 1e12,
        "select_compact_train_share_of_copy_rate": (3 * h_bytes / HBM_COPY) / (med["select_compact_train"] * 1e-3),
        "select_compact_eval_share_of_copy_rate": (h_bytes / HBM_COPY) / (med["select_compact_eval"] * 1e-3),
        "timing_note": "host-synchronised times: each includes one launch sequence and one 4-byte read-back",
        "last_select": st,
    }
    out = pathlib.Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(line) + "\n")
    print(json.dumps(line))


if __name__ == "__main__":
    main()
