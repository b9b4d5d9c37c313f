"""Latent spatial (engine.latent_spatial).

The inputs of tools/bench_latent_ap.py (N = 2^20 rows, S = 16 384 latents, 32 codes a row) read as 4 096 images of a 16 x 16 grid, at
G = 2 and G = 16 groups, and once more with one extra latent that fires on every row (the serial walk of DESIGN.md 7).  For each:

  whole_call     by device events (workspace and output allocation included), median of ``--iters`` calls
  stages_ms      the device time of one call by kernel from torch's profiler: ``prepare`` (group counts, count, parts, scan, place;
                 each of them under ``prepare_by_kernel``), ``walk``, ``overlap``; the memsets of the maps are in the whole call only
  bytes_bound    one read of the events (8 bytes each) plus one write of the maps (12 bytes a cell) at the 6.29 TB/s of a float4
                 copy, and the whole call over it
  dense_torch    the dense formulation on the same card: densify a 256-latent chunk to (images, gh, gw, 256), shifted ANDs for the
                 pairs, ``index_add_`` by group for the sums and the maps; measured on the chunk and scaled to S.  The integers of the
                 two are ASSERTED equal on that chunk.

    python tools/bench_latent_spatial.py [--iters 5] [--out profiles/latent_spatial_bench_line.json]

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

N, S, CAP = base.N, base.S, base.CAP
GH = GW = 16
T = GH * GW
N_IMAGES = N // T
CHUNK = 256
HBM_COPY = 6.29e12
PREPARE = ("groups", "count", "parts", "scan", "place")
STAGES = {**{f"lm_{k}_kernel": k for k in PREPARE}, "sp_walk": "walk", "sp_overlap": "overlap"}  # (prefixes: template arguments follow)


def stage_ms(fn):
    saved, base.STAGES = base.STAGES, STAGES
    try:
        by_kernel = base.stage_ms(fn)
    finally:
        base.STAGES = saved
    if by_kernel is None:
        return None
    return {"prepare": sum(by_kernel.get(k, 0.0) for k in PREPARE), "walk": by_kernel.get("walk"), "overlap": by_kernel.get("overlap"),
            "prepare_by_kernel": {k: by_kernel.get(k) for k in PREPARE}}


def with_every_row_latent(indices, data):
    """One more latent, id S, stored last in every row."""
    idx = torch.cat([indices.view(N, CAP), torch.full((N, 1), S, device=indices.device, dtype=torch.int32)], dim=1)
    val = torch.cat([data.view(N, CAP), torch.ones(N, 1, device=data.device)], dim=1)
    return torch.arange(N + 1, device=indices.device, dtype=torch.int64) * (CAP + 1), idx.reshape(-1).contiguous(), val.reshape(-1).contiguous()


def dense_chunk(indptr, indices, data, groups, n_groups, lo):
    """The integers of latents [lo, lo + CHUNK) the dense way."""
    rows = torch.repeat_interleave(torch.arange(N, device=indices.device), indptr[1:] - indptr[:-1])
    at = (indices >= lo) & (indices < lo + CHUNK)
    dense = torch.zeros(N, CHUNK, device=indices.device)
    dense[rows[at], (indices[at] - lo).long()] = data[at]
    fire = (dense > 0).view(N_IMAGES, GH, GW, CHUNK)
    m = fire.sum(dim=(1, 2))
    per_image = dict(n_events=m, n_images_fire=(m > 0).long(), sum_m2=m * m, pairs_h=(fire[:, :, :-1] & fire[:, :, 1:]).sum(dim=(1, 2)),
                     pairs_v=(fire[:, :-1] & fire[:, 1:]).sum(dim=(1, 2)))
    out = {k: torch.zeros(n_groups, CHUNK, device=indices.device, dtype=torch.int64).index_add_(0, groups.long(), v).T for k, v in per_image.items()}
    count = torch.zeros(n_groups, T, CHUNK, device=indices.device, dtype=torch.int32).index_add_(0, groups.long(), fire.view(N_IMAGES, T, CHUNK).int())
    out["count_map"] = count.permute(2, 0, 1)
    out["overlap"] = (out["count_map"].long() ** 2).sum(dim=2)
    out["sum_map"] = torch.zeros(n_groups, T, CHUNK, device=indices.device, dtype=torch.float64).index_add_(
        0, groups.long(), torch.where(fire, dense.view(N_IMAGES, GH, GW, CHUNK), 0.0).view(N_IMAGES, T, CHUNK).double()).permute(2, 0, 1)
    return out


def measure(csr, n_latents, n_groups, gen, iters, baseline):
    indptr, indices, data = csr
    dev = indices.device
    groups = torch.randint(0, n_groups, (N_IMAGES,), device=dev, generator=gen, dtype=torch.int32)

    def call():
        return engine.latent_spatial(indptr, indices, data, n_images=N_IMAGES, grid=(GH, GW), n_latents=n_latents, groups=groups, n_groups=n_groups)

    res = call()
    n_events = int(res.n_events.sum().item())  # (reads the error word: the inputs are good)
    cells = n_latents * n_groups * T
    bound_ms = (8 * n_events + 12 * cells) / HBM_COPY * 1e3
    out = {"n_images": N_IMAGES, "grid": [GH, GW], "n_latents": n_latents, "n_groups": n_groups, "nnz": int(indices.numel()), "n_events": n_events,
           "longest_list": int(res.n_events.sum(dim=1).max().item()), "workspace_bytes": int(res._ws.numel()), "map_bytes": 12 * cells,
           "whole_call": base.event_ms(call, iters), "stages_ms": stage_ms(call), "bytes_bound_ms": bound_ms}
    out["whole_call_over_bytes_bound"] = out["whole_call"]["median_ms"] / bound_ms
    if baseline:
        lo = 1024
        want = dense_chunk(indptr, indices, data, groups, n_groups, lo)
        for k, v in want.items():
            got = getattr(res, k)[lo:lo + CHUNK].reshape(v.shape)
            if k == "sum_map":  # the dense sum adds in another order
                assert torch.allclose(got, v, rtol=1e-12, atol=0), k
            else:
                assert torch.equal(got.long(), v.long()), k
        chunk = base.event_ms(lambda: dense_chunk(indptr, indices, data, groups, n_groups, lo), iters)
        out["dense_torch"] = {"chunk_latents": CHUNK, "chunk": chunk, "scaled_to_all_latents_ms": chunk["median_ms"] * n_latents / CHUNK,
                              "over_whole_call": chunk["median_ms"] * n_latents / CHUNK / out["whole_call"]["median_ms"],
                              "agrees_on_chunk": True}
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", type=pathlib.Path, default=pathlib.Path("profiles/latent_spatial_bench_line.json"))
    ap.add_argument("--skip-baseline", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(0)
    line = {"bench": "latent_spatial", "device": torch.cuda.get_device_name(0)}
    csr = base.make_codes(gen, dev)
    line["g2"] = measure(csr, S, 2, gen, a.iters, not a.skip_baseline)
    line["g16"] = measure(csr, S, 16, gen, a.iters, not a.skip_baseline)
    line["g2_every_row_latent"] = measure(with_every_row_latent(csr[1], csr[2]), S + 1, 2, gen, a.iters, False)
    a.out.parent.mkdir(parents=True, exist_ok=True)
    a.out.write_text(json.dumps(line) + "\n")
    print(json.dumps(line))
    return 0


if __name__ == "__main__":
    sys.exit(main())
