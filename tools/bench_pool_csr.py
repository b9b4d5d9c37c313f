"""Sparse pooling (engine.pool_csr) beside the path it replaces, in one process on one card.

Shapes:
  mimics        the mimic shape of tools/bench_latent_auroc.py: 16 384 images x 16 tokens, S = 16 384
  exemplars     the shape of tools/bench_latent_exemplars.py: 4 096 images x 256 tokens x 32 codes, S = 16 384
  every_latent  the adverse case: ONE image whose 16 tokens each store all 16 384 latents (the output row is as long as S, and the
                work is four workgroups'); reported, not compared

For each, after ``--warmup`` calls, medians, quartiles and range of ``--iters`` calls by device events:

  count, fill    the two C entries alone, on a workspace and outputs allocated before
  whole_call     engine.pool_csr: both passes, the allocations and the 8-byte read-back between them
  parent         engine.pool_images("max"), the clamp at 0 and torch's conversion of the non-zero entries to CSR (!=, sum, cumsum,
                 nonzero, masked gather): what the image-level workers did before.  Its triple is ASSERTED equal to pool_csr's
  peak_bytes     torch.cuda.max_memory_allocated over one call of either, above what was allocated before it
  bytes_bound    two reads of the image spans (indices and data, and the row positions) plus one write of the outputs at the 6.29 TB/s
                 of a float4 copy, and the whole call over it
  faster         whole_call's third quartile below the parent's first: the interquartile ranges do not overlap

    python tools/bench_pool_csr.py [--iters 20] [--warmup 3] [--out profiles/pool_csr_bench_line.json]

Writes one JSON line.  No test asserts a time."""
import argparse
import ctypes as C
import json
import pathlib
import statistics
import sys

import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1]))
sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))

import bench_latent_ap as base  # noqa: E402
import bench_latent_auroc as au  # noqa: E402
from saev_amd import _lib, engine  # noqa: E402

S = base.S
HBM_COPY = 6.29e12


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


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    del out
    return int(peak)


def every_latent(dev):
    t = 16
    indptr = torch.arange(t + 1, device=dev, dtype=torch.int64) * S
    indices = torch.arange(S, device=dev, dtype=torch.int32).repeat(t)
    data = (torch.arange(t * S, device=dev) % 97 + 1).to(torch.float32) / 64
    return (indptr, indices.contiguous(), data.contiguous()), 1, t


def measure(csr, n_images, tpi, iters, warmup, compare):
    indptr, indices, data = csr
    dev = indices.device
    nnz_in = int(indices.numel())
    lib = _lib.load()
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def ours():
        return engine.pool_csr(indptr, indices, data, n_images, tpi, S)

    def parent():
        pooled = torch.clamp_min(engine.pool_images(indptr, indices, data, n_images, tpi, S, "max").pooled, 0.0)
        at = pooled != 0
        p = torch.zeros(n_images + 1, device=dev, dtype=torch.int64)
        p[1:] = torch.cumsum(at.sum(dim=1), dim=0)
        return p, at.nonzero()[:, 1].to(torch.int32), pooled[at]

    res = ours()
    got = res.triple()  # (reads the error word: the inputs are good)
    want = parent()
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and torch.equal(a, b), "pool_csr and the dense detour disagree"
    nnz_out = res.nnz
    need = int(lib.saev_pool_csr_workspace_bytes(n_images, tpi, S, nnz_in))
    ws = torch.empty(need, device=dev, dtype=torch.uint8)
    err = torch.empty(1, device=dev, dtype=torch.int32)
    o_indptr = torch.empty(n_images + 1, device=dev, dtype=torch.int64)
    o_indices, o_data = torch.empty(nnz_out, device=dev, dtype=torch.int32), torch.empty(nnz_out, device=dev)
    head = (ptr(indptr), ptr(indices), ptr(data), nnz_in, n_images, tpi, S, 0.0, None)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def count():
        assert lib.saev_pool_csr_count(*head, ptr(o_indptr), ptr(ws), need, ptr(err), stream) == 0

    def fill():
        assert lib.saev_pool_csr_fill(*head, ptr(o_indptr), ptr(o_indices), ptr(o_data), None, None, ptr(ws), need, ptr(err), stream) == 0

    del res, got, want
    for _ in range(warmup):
        ours(), count(), fill()
        if compare:
            parent()
    t_ours, t_parent, t_count, t_fill = [], [], [], []
    for _ in range(iters):  # alternating: what else runs on the host meets all alike
        t_ours.append(event_ms(ours))
        if compare:
            t_parent.append(event_ms(parent))
        t_count.append(event_ms(count))
        t_fill.append(event_ms(fill))
    bound_ms = (2 * (8 * nnz_in + 8 * (n_images * tpi + 1)) + 8 * (n_images + 1) + 8 * nnz_out) / HBM_COPY * 1e3
    out = {"n_images": n_images, "tokens_per_image": tpi, "n_latents": S, "token_nnz": nnz_in, "pooled_nnz": nnz_out, "workspace_bytes": need,
           "count": spread(t_count), "fill": spread(t_fill), "whole_call": spread(t_ours), "peak_bytes": peak_bytes(ours), "bytes_bound_ms": bound_ms}
    out["whole_call_over_bytes_bound"] = out["whole_call"]["median_ms"] / bound_ms
    if compare:
        out["parent"] = {"whole_call": spread(t_parent), "peak_bytes": peak_bytes(parent), "agrees": True}
        out["parent_over_whole_call"] = out["parent"]["whole_call"]["median_ms"] / out["whole_call"]["median_ms"]
        out["parent_peak_over_peak"] = out["parent"]["peak_bytes"] / max(out["peak_bytes"], 1)
        out["faster"] = out["whole_call"]["q3_ms"] < out["parent"]["whole_call"]["q1_ms"]
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", type=pathlib.Path, default=pathlib.Path("profiles/pool_csr_bench_line.json"))
    a = ap.parse_args()
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(0)
    line = {"bench": "pool_csr", "device": torch.cuda.get_device_name(0), "range": int(_lib.load().saev_pool_csr_range())}
    line["mimics"] = measure(au.mimic_tokens(gen, dev), au.M_IMAGES, au.M_TPI, a.iters, a.warmup, True)
    line["exemplars"] = measure(base.make_codes(gen, dev), base.N // 256, 256, a.iters, a.warmup, True)
    csr, n_images, tpi = every_latent(dev)
    line["every_latent"] = measure(csr, n_images, tpi, a.iters, a.warmup, True)
    line["every_latent"].pop("faster")  # the adverse case is reported, not compared
    a.out.parent.mkdir(parents=True, exist_ok=True)
    a.out.write_text(json.dumps(line) + "\n")
    print(json.dumps(line))
    return 0


if __name__ == "__main__":
    sys.exit(main())
