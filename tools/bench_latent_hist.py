"""Per-latent histograms and exact quantiles (engine.LatentHist, engine.LatentQuantiles) on the latent-AP bench's
inputs: N = 2^20 rows, S = 16 384 latents, 32 codes per row (nnz = 2^25), Q = 4 quantiles (8 target ranks a latent).

  level0_chunk     one level-0 update of the whole CSR chunk (2^20 rows)
  level0_batch     one level-0 update of a 16 384-row inference batch as padded rows, calls enqueued back to back
  refine_chunk     one level-1 update of the chunk (the prefix filter and the per-target counters)
  locate0          the level-0 locate (one launch)
  three_pass       engine.latent_quantiles over the chunk already on the device: three updates, three locates, three read-backs of
                   the row counter, the tables' allocation and zeroing
  crowded          the same updates with latent 0 on every row at one value: every increment of it lands on one counter
  torch_bincount   the obvious torch form of the histogram: torch.bincount(latent * 4096 + bin), the key arithmetic included
  sort_and_gather  the in-memory route to the quantiles: the latent AP's radix sort (engine.latent_ap with one class; the call also
                   walks the sorted events once, so this is an upper bound of the sort by that walk) and a gather at the ranks
  inference        wall seconds of framework.inference.worker_fn over a synthetic cache, with and without activation_hist

Medians and interquartile ranges over ``--iters`` timed calls after a warm-up call, by device events.

    python tools/bench_latent_hist.py [--iters 20] [--out profiles/latent_hist_bench_line.json]

Writes one JSON line.  No test asserts a time."""
import argparse
import ctypes as C
import json
import pathlib
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1]))

from saev_amd import engine  # noqa: E402

N, CAP, S, BATCH_ROWS, D = 1 << 20, 32, 16384, 16384, 1024
Q = (0.5, 0.9, 0.95, 0.99)


def make_codes(gen, dev):
    """tools/bench_latent_ap.py's codes: CAP distinct latents per row in ascending order, positive values quantised to 1/64."""
    start = torch.randint(0, S, (N, 1), device=dev, generator=gen)
    stride = torch.randint(1, S // CAP, (N, 1), device=dev, generator=gen)
    idx = ((start + torch.arange(CAP, device=dev)[None, :] * stride) % S).sort(dim=1).values.to(torch.int32)
    val = torch.ceil(torch.randn(N, CAP, device=dev, generator=gen).abs() * 64) / 64 + 1 / 64
    return torch.arange(N + 1, device=dev, dtype=torch.int64) * CAP, idx, val


def summary(ts):
    q = statistics.quantiles(ts, n=4)
    return {"median_ms": statistics.median(ts), "iqr_ms": q[2] - q[0], "min_ms": min(ts), "max_ms": max(ts), "n": len(ts)}


def device_ms(fn, iters, burst=1):
    fn()  # warm-up
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(burst):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / burst)
    return summary(ts)


def torch_bincount(indices, data):
    u = data.view(torch.int32)
    key_hi = torch.where(u < 0, (~u >> 20) & 0xFFF, ((u >> 20) & 0xFFF) | 0x800)
    return torch.bincount(indices.to(torch.int64) * 4096 + key_hi, minlength=S * 4096)


def updates(indptr, indices, data, idx, val, iters):
    """The update and locate timings of one set of codes."""
    hist = engine.LatentHist(S, indices.device)
    out = {"level0_chunk": device_ms(lambda: hist.add_csr(indptr, indices, data), iters)}
    hist.zero_()
    bi, bv = idx[:BATCH_ROWS].contiguous(), val[:BATCH_ROWS].contiguous()
    out["level0_batch"] = device_ms(lambda: hist.add(bi, bv), iters, burst=10)
    del hist
    acc = engine.LatentQuantiles(S, Q, indices.device, "rows")
    acc.add_csr(indptr, indices, data)
    locate = lambda: acc.lib.saev_latent_hist_locate(C.byref(acc._state), C.byref(acc._targets), S, engine._stream())  # noqa: E731
    out["locate0"] = device_ms(locate, iters)
    acc.next_pass()

    def refine():
        acc._offered = 0
        acc.add_csr(indptr, indices, data)

    out["refine_chunk"] = device_ms(refine, iters)
    del acc
    out["three_pass"] = device_ms(lambda: engine.latent_quantiles(indptr, indices, data, N, S, Q, over="rows"), max(3, iters // 4))
    return out


def sort_and_gather(indptr, indices, data):
    """Quantiles over the entries by the latent AP's sort: element floor((m - 1) q) of every latent's ascending values."""
    res = engine.latent_ap(indptr, indices, data, N, S, 1, labels=torch.zeros(N, device=indices.device, dtype=torch.int32))
    starts, key, _, _ = res.sorted_events()  # (latent, value descending)
    m = starts[1:] - starts[:-1]
    qs = torch.tensor(Q, device=indices.device, dtype=torch.float64)
    lo = torch.floor((m - 1).clamp(min=0).to(torch.float64)[:, None] * qs[None, :]).to(torch.int64)
    at = (starts[1:, None] - 1 - lo).clamp(0, max(key.numel() - 1, 0))
    return key[at], m


def inference_pass(dev, n_batches, reps):
    """worker_fn (save=True) over a synthetic cache of n_batches x 16 384 tokens of width D, TopK(32) SAE with S latents."""
    from saev_amd import disk, nn
    from saev_amd.data import OrderedConfig
    from saev_amd.data.shards import write_shards
    from saev_amd.framework import inference

    T = 256
    with tempfile.TemporaryDirectory(prefix="latent_hist_bench_") as tmp:
        tmp = pathlib.Path(tmp)
        acts = np.random.default_rng(0).standard_normal((n_batches * BATCH_ROWS // T, 1, T, D), dtype=np.float32)
        d = write_shards(tmp, acts, layers=(0,), max_tokens_per_shard=BATCH_ROWS * 4)
        runs_root = tmp / "saev" / "runs"
        runs_root.mkdir(parents=True)
        run = disk.Run.new("bench0lh", train_shards_dir=d, val_shards_dir=d, runs_root=runs_root)
        torch.manual_seed(0)
        nn.dump(run.ckpt, nn.SparseAutoencoder(nn.SparseAutoencoderConfig(d_model=D, d_sae=S, activation=nn.modeling.TopK(
            top_k=CAP, aux=nn.modeling.AuxK(k_aux=512)))))
        cfg = inference.Config(run=run.run_dir, data=OrderedConfig(shards=d, layer=0, batch_size=BATCH_ROWS), force_recompute=True, device=str(dev))
        inference.worker_fn(cfg, activation_hist=True)  # warm-up
        ts = {False: [], True: []}
        for _ in range(reps):
            for on in (False, True):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                inference.worker_fn(cfg, activation_hist=on)
                torch.cuda.synchronize()
                ts[on].append(time.perf_counter() - t0)
        return {"tokens": n_batches * BATCH_ROWS, "reps": reps, "without_s": ts[False], "with_s": ts[True],
                "median_without_s": statistics.median(ts[False]), "median_with_s": statistics.median(ts[True])}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--pass-batches", type=int, default=4)
    ap.add_argument("--pass-reps", type=int, default=3)
    ap.add_argument("--out", type=pathlib.Path, default=pathlib.Path("profiles/latent_hist_bench_line.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    indptr, idx, val = make_codes(gen, dev)
    indices, data = idx.reshape(-1), val.reshape(-1)
    line = {"bench": "latent_hist", "n_rows": N, "n_latents": S, "nnz": int(indices.numel()), "q": list(Q), "device": torch.cuda.get_device_name(0)}
    line["typical"] = updates(indptr, indices, data, idx, val, a.iters)

    line["torch_bincount"] = device_ms(lambda: torch_bincount(indices, data), a.iters)
    hist = engine.LatentHist(S, dev)
    hist.add_csr(indptr, indices, data)
    line["histogram_equals_torch_bincount"] = bool(torch.equal(hist.counts0.reshape(-1).to(torch.int64), torch_bincount(indices, data)))
    del hist
    line["sort_and_gather"] = device_ms(lambda: sort_and_gather(indptr, indices, data), max(3, a.iters // 4))
    key, m = sort_and_gather(indptr, indices, data)
    ours = engine.latent_quantiles(indptr, indices, data, N, S, Q, over="entries")
    line["quantiles_equal_sort_and_gather"] = bool(torch.equal(
        ours.lower.to(dev).view(torch.int32)[m > 0], torch.where(~key < 0, ~key & 0x7FFFFFFF, key)[m > 0]))  # the sort's key is ~f2ukey

    cidx, cval = idx.clone(), val.clone()
    cidx[:, 0], cval[:, 0] = 0, 2.5  # latent 0 on every row at one value (0 is every row's lowest latent or below it)
    line["crowded"] = updates(indptr, cidx.reshape(-1), cval.reshape(-1), cidx, cval, a.iters)
    del cidx, cval
    line["inference"] = inference_pass(dev, a.pass_batches, a.pass_reps)
    a.out.parent.mkdir(parents=True, exist_ok=True)
    a.out.write_text(json.dumps(line) + "\n")
    print(json.dumps(line))
    return 0


if __name__ == "__main__":
    sys.exit(main())
