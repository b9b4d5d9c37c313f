"""Probe AP (engine.probe_ap) at the shape of tools/bench_latent_ap.py, on the same inputs: N = 2^20 rows,
S = 16 384 latents, 32 codes per row (nnz = 2^25), C = 150 classes; weights of mixed sign (every wave walks both directions).

  whole call   events around ``engine.probe_ap`` with ``top_k = 256`` (workspace allocation included), median of ``--iters`` calls,
               for float32 and for float64 weights
  stages       the device time of one call split by kernel, from torch's profiler: ``sort`` (as in bench_latent_ap), ``labels``,
               ``values`` (the finiteness check), ``walk`` (pa_terms: both directions, per-lane group closing) and ``top_rows``
               (the gather); null if the profiler reports no kernels of the library
  latent_ap    ``engine.latent_ap`` on the same inputs in the same process, whole call and stages: the yardstick.  ``walk_ratio``
               is this entry's walk over that one's ``terms``.

    python tools/bench_probe_ap.py [--iters 5] [--out profiles/probe_ap_bench_line.json]

Writes one JSON line.  No test asserts a time."""
import argparse
import json
import pathlib
import sys

import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1]))
sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))

import bench_latent_ap as base  # noqa: E402
from saev_amd import engine  # noqa: E402

N, S, C, TOP_K = base.N, base.S, base.C, 256
STAGES = {**base.STAGES, "pa_values": "values", "pa_terms": "walk", "pa_top_rows": "top_rows"}


def stage_ms(fn):
    saved, base.STAGES = base.STAGES, STAGES
    try:
        return base.stage_ms(fn)
    finally:
        base.STAGES = saved


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", type=pathlib.Path, default=pathlib.Path("profiles/probe_ap_bench_line.json"))
    a = ap.parse_args()
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(0)
    indptr, indices, data = base.make_codes(gen, dev)
    labels = torch.randint(0, C, (N,), device=dev, generator=gen, dtype=torch.int32)
    w64 = (torch.rand(S, C, device=dev, generator=gen, dtype=torch.float64) * 2.75 + 0.25) * (torch.randint(0, 2, (S, C), device=dev, generator=gen) * 2 - 1)
    b64 = torch.rand(S, C, device=dev, generator=gen, dtype=torch.float64) * 3 - 2

    line = {"bench": "probe_ap", "n_rows": N, "n_latents": S, "n_classes": C, "nnz": int(indices.numel()), "top_k": TOP_K,
            "device": torch.cuda.get_device_name(0), "negative_weights": float((w64 < 0).double().mean().item())}
    for name, dtype in (("fp32", torch.float32), ("fp64", torch.float64)):
        w, b = w64.to(dtype), b64.to(dtype)

        def call():
            return engine.probe_ap(indptr, indices, data, N, S, C, labels=labels, weights=w, biases=b, top_k=TOP_K)

        res = call()
        mean_ap = float(res.ap.mean().item())  # (reads the error word: the inputs are good)
        line[name] = {"whole_call": base.event_ms(call, a.iters), "stages_ms": stage_ms(call), "mean_ap": mean_ap}
        line["workspace_bytes"] = int(res.layout.total_bytes)
        del res

    def latent():
        return engine.latent_ap(indptr, indices, data, N, S, C, labels=labels)

    latent().ap
    line["latent_ap"] = {"whole_call": base.event_ms(latent, a.iters), "stages_ms": stage_ms(latent)}
    terms = (line["latent_ap"]["stages_ms"] or {}).get("terms")
    line["walk_ratio"] = {k: (line[k]["stages_ms"] or {}).get("walk") / terms if terms and line[k]["stages_ms"] else None for k in ("fp32", "fp64")}
    a.out.parent.mkdir(parents=True, exist_ok=True)
    a.out.write_text(json.dumps(line) + "\n")
    print(json.dumps(line))
    return 0


if __name__ == "__main__":
    sys.exit(main())
