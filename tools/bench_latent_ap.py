"""Latent AP (engine.latent_ap) at the audit's shape: N = 2^20 rows, S = 16 384 latents, 32 codes per row
(nnz = 2^25), C = 150 classes.

  whole call   events around ``engine.latent_ap`` (workspace allocation included, as a caller pays it), median of ``--iters`` calls
  stages       the device time of one call split by kernel, from torch's profiler: ``sort`` (the entry pass, and per radix pass the
               digit count, the table scan and the stable scatter, then the latents' starts), ``labels`` (class counts), ``terms``
               (the walk: tie groups, terms and sums; the library has no separate group or regroup pass -- DESIGN.md 3.19 says
               why) and ``best``; null if the profiler reports no kernels of the library
  baseline     the method this replaces, in plain torch on the same device: a dense (N, 64) batch of latents, per latent a
               descending ``sort``, the one-hot labels gathered in that order, ``cumsum``, precision x delta-recall -- the
               reference's compute_ap_batched -- timed for 64 latents and scaled to S

    python tools/bench_latent_ap.py [--iters 5] [--out profiles/latent_ap_bench_line.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_latent_ap.py --calls-only --iters 2     (the kernels' own times)

Writes one JSON line.  No test asserts a time."""
import argparse
import json
import pathlib
import statistics
import sys

import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1]))

from saev_amd import engine  # noqa: E402

N, CAP, S, C, BATCH = 1 << 20, 32, 16384, 150, 64
STAGES = {"la_init": "sort", "la_hist": "sort", "la_scan": "sort", "la_scatter": "sort", "la_starts": "sort", "la_labels": "labels",
          "la_terms": "terms", "la_best": "best"}


def make_codes(gen, dev):
    """Codes as a TopK encoder leaves them: CAP distinct latents per row in ascending order, positive values quantised to 1/64 (so
    that a latent has tie groups, as fp16-trained codes do)."""
    start = torch.randint(0, S, (N, 1), device=dev, generator=gen)
    stride = torch.randint(1, S // CAP, (N, 1), device=dev, generator=gen)
    idx = ((start + torch.arange(CAP, device=dev)[None, :] * stride) % S).sort(dim=1).values.to(torch.int32)
    val = torch.ceil(torch.randn(N, CAP, device=dev, generator=gen).abs() * 64) / 64 + 1 / 64
    indptr = torch.arange(N + 1, device=dev, dtype=torch.int64) * CAP
    return indptr, idx.reshape(-1).contiguous(), val.reshape(-1).contiguous()


def event_ms(fn, iters):
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "n": len(ts)}


def stage_ms(fn):
    from torch.profiler import ProfilerActivity, profile

    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    out = {}
    for ev in prof.events():
        for prefix, stage in STAGES.items():
            if prefix in ev.name:
                out[stage] = out.get(stage, 0.0) + (ev.device_time if hasattr(ev, "device_time") else ev.cuda_time) / 1e3
    return out or None


def torch_dense_ap(acts_nb, one_hot, n_pos):
    """compute_ap_batched of the reference in torch: per latent sort, gather, cumsum."""
    n = acts_nb.shape[0]
    ranks = torch.arange(1, n + 1, device=acts_nb.device, dtype=torch.float32)[:, None]
    out = torch.empty(acts_nb.shape[1], one_hot.shape[1], device=acts_nb.device)
    for b in range(acts_nb.shape[1]):
        order = torch.sort(acts_nb[:, b], descending=True).indices
        tp = one_hot[order].cumsum(dim=0)
        recall = tp / n_pos
        delta = recall - torch.cat([torch.zeros_like(recall[:1]), recall[:-1]])
        out[b] = ((tp / ranks) * delta).sum(dim=0)
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", type=pathlib.Path, default=pathlib.Path("profiles/latent_ap_bench_line.json"))
    ap.add_argument("--calls-only", action="store_true", help="only the calls (for a kernel trace by rocprofv3 --kernel-trace --stats): nothing written")
    a = ap.parse_args()
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(0)
    indptr, indices, data = make_codes(gen, dev)
    labels = torch.randint(0, C, (N,), device=dev, generator=gen, dtype=torch.int32)

    def call():
        return engine.latent_ap(indptr, indices, data, N, S, C, labels=labels)

    res = call()
    best = float(res.best_ap.max().item())  # (reads the error word: the inputs are good)
    whole = event_ms(call, a.iters)
    if a.calls_only:
        print(json.dumps({"whole_call": whole}))
        return 0
    stages = stage_ms(call)

    dense = torch.zeros(N, BATCH, device=dev)
    rows = torch.arange(N, device=dev).repeat_interleave(CAP)
    keep = indices < BATCH
    dense[rows[keep], indices[keep].long()] = data[keep]
    one_hot = torch.nn.functional.one_hot(labels.long(), C).float()
    n_pos = one_hot.sum(dim=0).clamp(min=1)
    torch_dense_ap(dense[:, :2], one_hot, n_pos)
    base = event_ms(lambda: torch_dense_ap(dense, one_hot, n_pos), max(1, a.iters // 2))
    line = {"bench": "latent_ap", "n_rows": N, "n_latents": S, "n_classes": C, "nnz": int(indices.numel()), "device": torch.cuda.get_device_name(0),
            "whole_call": whole, "stages_ms": stages, "workspace_bytes": int(res.layout.total_bytes), "largest_best_ap": best,
            "torch_dense_baseline": {"batch": BATCH, "batch_ms": base, "scaled_to_all_latents_ms": base["median_ms"] * S / BATCH},
            "speedup_vs_baseline": base["median_ms"] * S / BATCH / whole["median_ms"]}
    a.out.parent.mkdir(parents=True, exist_ok=True)
    a.out.write_text(json.dumps(line) + "\n")
    print(json.dumps(line))
    return 0


if __name__ == "__main__":
    sys.exit(main())
