"""Latent exemplars (engine.latent_exemplars and engine.latent_patch_rows).

The inputs of tools/bench_latent_spatial.py (N = 2^20 rows, S = 16 384 latents, 32 codes a row, read as 4 096 images of 256 tokens)
at G = 2 and G = 16 groups and k = 8, and once more with one extra latent that fires on every row (the serial walk of DESIGN.md 7).
For each, after ``--warmup`` calls:

  whole_call     by device events (workspace and output allocation included): median, quartiles and range of ``--iters`` calls
  stages_ms      the device time by kernel from torch's profiler over ``--iters`` calls of a run of its own: ``prepare`` (group counts
                 and member lists, count, parts, scan, place), ``walk``; median and quartiles per call
  spatial        engine.latent_spatial with ``sum_map=False`` in the same process on the same inputs, its calls ALTERNATING with
                 those of latent_exemplars: the same prepare, a walk that does more per event.  ``walk_over_spatial_walk`` and
                 ``whole_call_over_spatial`` are the ratios of the medians
  bytes_bound    one read of the events (8 bytes each) plus one write of the outputs at the 6.29 TB/s of a float4 copy, and the whole
                 call over it
  dense_torch    the dense formulation on the same card: densify a 256-latent chunk, ``amax`` over the patches, a masked ``topk`` of
                 both signs per group; measured on the chunk and scaled to S.  n_fire and both lists' values are ASSERTED equal on
                 that chunk (the images of equal values may differ: torch's topk does not say which it keeps)
  patch_rows     engine.latent_patch_rows for the top lists of 256 latents (256 x G x k queries of 256 tokens)

    python tools/bench_latent_exemplars.py [--iters 20] [--warmup 3] [--out profiles/latent_exemplars_bench_line.json]

Writes one JSON line.  No test asserts a time."""
import argparse
import json
import pathlib
import statistics
import sys

import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1]))
sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))

import bench_latent_ap as base  # noqa: E402
from saev_amd import engine  # noqa: E402

N, S, CAP = base.N, base.S, base.CAP
T = 256
N_IMAGES = N // T
K = 8
CHUNK = 256
HBM_COPY = 6.29e12
REGROUP = ("groups", "count", "parts", "scan", "place")  # latent_major.h; the names are prefixes: template arguments follow
STAGES = {**{f"lm_{k}_kernel": "prepare" for k in REGROUP}, "ex_members_kernel": "prepare", "ex_walk_kernel": "walk"}
SPATIAL_STAGES = {**{f"lm_{k}_kernel": "prepare" for k in REGROUP}, "sp_walk_kernel": "walk", "sp_overlap_kernel": "overlap"}


def spread(ts):
    q = statistics.quantiles(ts, n=4) if len(ts) > 1 else [ts[0]] * 3
    return {"median_ms": statistics.median(ts), "q1_ms": q[0], "q3_ms": q[2], "iqr_ms": q[2] - q[0], "min_ms": min(ts), "max_ms": max(ts), "n": len(ts)}


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def stage_ms(fn, stages, iters):
    """Per stage the device time of each of ``iters`` calls: every kernel runs once a call, so its n-th record belongs to call n."""
    from torch.profiler import ProfilerActivity, profile

    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
    by_kernel = {}
    for ev in sorted(prof.events(), key=lambda ev: ev.time_range.start):
        for name in stages:
            if name in ev.name:
                by_kernel.setdefault(name, []).append((ev.device_time if hasattr(ev, "device_time") else ev.cuda_time) / 1e3)
    per_call = {}
    for name, ts in by_kernel.items():
        if len(ts) != iters:
            return None
        acc = per_call.setdefault(stages[name], [0.0] * iters)
        for n, t in enumerate(ts):
            acc[n] += t
    return {stage: spread(ts) for stage, ts in per_call.items()} or None


def with_every_row_latent(indices, data):
    """One more latent, id S, stored last in every row."""
    idx = torch.cat([indices.view(N, CAP), torch.full((N, 1), S, device=indices.device, dtype=torch.int32)], dim=1)
    val = torch.cat([data.view(N, CAP), torch.ones(N, 1, device=data.device)], dim=1)
    return torch.arange(N + 1, device=indices.device, dtype=torch.int64) * (CAP + 1), idx.reshape(-1).contiguous(), val.reshape(-1).contiguous()


def dense_chunk(indptr, indices, data, groups, n_groups, lo):
    """n_fire (CHUNK, G) and the values of both lists (CHUNK, G, K) of latents [lo, lo + CHUNK) the dense way."""
    rows = torch.repeat_interleave(torch.arange(N, device=indices.device), indptr[1:] - indptr[:-1])
    at = (indices >= lo) & (indices < lo + CHUNK)
    dense = torch.zeros(N, CHUNK, device=indices.device)
    dense[rows[at], (indices[at] - lo).long()] = data[at]
    pooled = dense.view(N_IMAGES, T, CHUNK).amax(dim=1)
    n_fire, top, bot = [], [], []
    for g in range(n_groups):
        fires = (pooled > 0) & (groups == g)[:, None]
        n_fire.append(fires.sum(dim=0))
        t = torch.where(fires, pooled, -torch.inf).topk(K, dim=0).values
        b = -torch.where(fires, -pooled, -torch.inf).topk(K, dim=0).values
        top.append(torch.where(torch.isinf(t), 0.0, t).T)
        bot.append(torch.where(torch.isinf(b), 0.0, b).T)
    return torch.stack(n_fire, dim=1), torch.stack(top, dim=1), torch.stack(bot, dim=1)


def measure(csr, n_latents, n_groups, gen, iters, warmup, baseline):
    indptr, indices, data = csr
    dev = indices.device
    groups = torch.randint(0, n_groups, (N_IMAGES,), device=dev, generator=gen, dtype=torch.int32)

    def call():
        return engine.latent_exemplars(indptr, indices, data, n_images=N_IMAGES, tokens_per_image=T, n_latents=n_latents, groups=groups, n_groups=n_groups,
                                       k=K)

    def spatial():
        return engine.latent_spatial(indptr, indices, data, n_images=N_IMAGES, grid=(16, 16), n_latents=n_latents, groups=groups, n_groups=n_groups,
                                     sum_map=False)

    res = call()
    n_fire = res.n_fire  # (reads the error word: the inputs are good)
    n_events = int(spatial().n_events.sum().item())
    out_bytes = 8 * n_groups + n_latents * n_groups * (4 + 28 * K)
    bound_ms = (8 * n_events + out_bytes) / HBM_COPY * 1e3
    for _ in range(warmup):
        call(), spatial()
    ours, theirs = [], []
    for _ in range(iters):  # alternating: what else runs on the host meets both alike
        ours.append(event_ms(call))
        theirs.append(event_ms(spatial))
    out = {"n_images": N_IMAGES, "tokens_per_image": T, "n_latents": n_latents, "n_groups": n_groups, "k": K, "nnz": int(indices.numel()),
           "n_events": n_events, "firing_images": int(n_fire.sum().item()), "most_firing_images": int(n_fire.sum(dim=1).max().item()),
           "workspace_bytes": int(res._ws.numel()), "output_bytes": out_bytes, "whole_call": spread(ours), "stages_ms": stage_ms(call, STAGES, iters),
           "bytes_bound_ms": bound_ms,
           "spatial": {"whole_call": spread(theirs), "stages_ms": stage_ms(spatial, SPATIAL_STAGES, iters)}}
    out["whole_call_over_bytes_bound"] = out["whole_call"]["median_ms"] / bound_ms
    out["whole_call_over_spatial"] = out["whole_call"]["median_ms"] / out["spatial"]["whole_call"]["median_ms"]
    if out["stages_ms"] and out["spatial"]["stages_ms"]:
        out["walk_over_spatial_walk"] = out["stages_ms"]["walk"]["median_ms"] / out["spatial"]["stages_ms"]["walk"]["median_ms"]
    if baseline:
        lo = 1024
        want_fire, want_top, want_bot = dense_chunk(indptr, indices, data, groups, n_groups, lo)
        assert torch.equal(n_fire[lo:lo + CHUNK].long(), want_fire.long()), "n_fire"
        assert torch.equal(res.top_val[lo:lo + CHUNK], want_top), "top_val"
        assert torch.equal(res.bot_val[lo:lo + CHUNK], want_bot), "bot_val"
        for _ in range(warmup):
            dense_chunk(indptr, indices, data, groups, n_groups, lo)
        chunk = spread([event_ms(lambda: dense_chunk(indptr, indices, data, groups, n_groups, lo)) for _ in range(iters)])
        out["dense_torch"] = {"chunk_latents": CHUNK, "chunk": chunk, "scaled_to_all_latents_ms": chunk["median_ms"] * n_latents / CHUNK,
                              "over_whole_call": chunk["median_ms"] * n_latents / CHUNK / out["whole_call"]["median_ms"], "agrees_on_chunk": True}
        lat = torch.arange(lo, lo + CHUNK, device=dev, dtype=torch.int32)[:, None, None].expand(CHUNK, n_groups, K).contiguous()
        img = res.top_img[lo:lo + CHUNK].contiguous()

        def rows():
            return engine.latent_patch_rows(indptr, indices, data, lat, img, n_images=N_IMAGES, tokens_per_image=T, n_latents=n_latents)

        got = rows()
        held = img >= 0
        at_max = torch.gather(got, 3, res.top_patch[lo:lo + CHUNK].clamp_min(0).long()[..., None])[..., 0]
        assert torch.equal(at_max[held], res.top_val[lo:lo + CHUNK][held]), "the patch vector has the maximum where top_patch says"
        for _ in range(warmup):
            rows()
        out["patch_rows"] = {"queries": int(img.numel()), "values": int(got.numel()), "whole_call": spread([event_ms(rows) for _ in range(iters)])}
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", type=pathlib.Path, default=pathlib.Path("profiles/latent_exemplars_bench_line.json"))
    ap.add_argument("--skip-baseline", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(0)
    line = {"bench": "latent_exemplars", "device": torch.cuda.get_device_name(0)}
    csr = base.make_codes(gen, dev)
    line["g2"] = measure(csr, S, 2, gen, a.iters, a.warmup, not a.skip_baseline)
    line["g16"] = measure(csr, S, 16, gen, a.iters, a.warmup, not a.skip_baseline)
    line["g2_every_row_latent"] = measure(with_every_row_latent(csr[1], csr[2]), S + 1, 2, gen, a.iters, a.warmup, False)
    a.out.parent.mkdir(parents=True, exist_ok=True)
    a.out.write_text(json.dumps(line) + "\n")
    print(json.dumps(line))
    return 0


if __name__ == "__main__":
    sys.exit(main())
