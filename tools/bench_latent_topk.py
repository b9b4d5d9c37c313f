"""Per-latent top-k activating tokens (engine.LatentTopK) at configs[1]'s inference shape (n 16 384 rows, 32 codes
per row, S 32 768, k 20):

  (a) the first update of an empty state, where every entry is a candidate;
  (b) a warmed-up update, after ``--warm`` other batches have filled the lists;
  (c) a whole inference pass (framework/inference.worker_fn over a synthetic cache) with and without ``top_k_tokens``,

against two baselines it also runs: the torch formulation on the same GPU (scatter the batch to a dense (n, S) matrix, ``torch.topk``
over the state's values stacked on it), and the reference's algorithm restated on the host -- dense blocks of 1 024 rows walked row
by row, every nonzero column replacing its list's minimum -- on a slice of rows small enough to finish, scaled to the batch.  The
BatchStats call the pass already makes per batch is timed beside (b): the expectation was that (b) costs less.

    python tools/bench_latent_topk.py [--iters 30] [--out profiles/latent_topk_bench_line.json]

Two device figures per call, both from events.  ``burst``: ``--burst`` calls on distinct batches enqueued back to back between one
pair of events, divided by their number -- the queue stays full, so this is what a call costs on the device inside a pass (or the
host's enqueue rate where that is slower; the host's own time per enqueue is reported beside it).  ``single``: one call on an idle,
synchronised device -- launch latency and the Python / ctypes path included, not the kernels.  Every timed update takes a batch no
earlier update has seen (a re-fed batch would come back as ties of itself); the pool, --iters x --burst batches of 4.2 MB, is larger
than the 256 MB Infinity Cache.  (c) is host wall clock around the pass, the two variants alternating."""
import argparse
import json
import pathlib
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1]))

from saev_amd.engine import BatchStats, LatentTopK  # noqa: E402

N, CAP, S, K, D = 16384, 32, 32768, 20, 1024


def summary(ts):
    q = statistics.quantiles(ts, n=4)
    return {"median_ms": statistics.median(ts), "spread_ms": q[2] - q[0], "min_ms": min(ts), "max_ms": max(ts), "n": len(ts)}


def device_ms(fn, iters, setup=None):
    ts = []
    for i in range(iters):
        if setup is not None:
            setup(i)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn(i)
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return summary(ts)


def burst_ms(fn, iters, burst, setup=None):
    """Per-call device time of ``burst`` calls enqueued back to back (fn(j) with j counting over all calls), and the host's time
    to enqueue one."""
    ts, host = [], []
    for i in range(iters):
        if setup is not None:
            setup(i)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        for j in range(burst):
            fn(i * burst + j)
        e1.record()
        host.append((time.perf_counter() - t0) * 1e3 / burst)
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / burst)
    return {**summary(ts), "burst": burst, "host_enqueue_median_ms": statistics.median(host)}


def make_batch(gen, dev):
    """Codes as a TopK encoder leaves them: CAP distinct latents per row (a random start and stride through the latents) in
    ascending order, positive values."""
    start = torch.randint(0, S, (N, 1), device=dev, generator=gen)
    stride = torch.randint(1, S // CAP, (N, 1), device=dev, generator=gen)
    idx = ((start + torch.arange(CAP, device=dev)[None, :] * stride) % S).sort(dim=1).values.to(torch.int32)
    val = torch.randn(N, CAP, device=dev, generator=gen).abs() + 1e-3
    return idx, val


def torch_update(state_val, state_row, idx, val, row_base):
    """The torch formulation: dense scatter, then topk over [state | batch] along the rows."""
    dense = torch.zeros(N, S, device=idx.device)
    dense.scatter_(1, idx.long(), val)
    both = torch.cat([state_val, dense])
    top = torch.topk(both, K, dim=0)
    rows = torch.cat([state_row, (torch.arange(N, device=idx.device) + row_base)[:, None].expand(N, S)])
    return top.values, torch.gather(rows, 0, top.indices)


def host_reference_algorithm(idx, val, n_rows, block=1024):
    """Seconds for ``n_rows`` rows of the batch by the reference's algorithm, restated: densify ``block`` rows at a time; for every
    row, every nonzero column either fills its list or replaces the list's minimum."""
    import scipy.sparse

    idx, val = idx[:n_rows].cpu().numpy(), val[:n_rows].cpu().numpy()
    arr = scipy.sparse.csr_array((val.reshape(-1), idx.reshape(-1), np.arange(n_rows + 1) * CAP), shape=(n_rows, S))
    t0 = time.perf_counter()
    top_v = np.full((K, S), -np.inf, dtype=np.float32)
    top_i = np.zeros((K, S), dtype=np.int64)
    low = np.full(S, -np.inf, dtype=np.float32)
    cnt = np.zeros(S, dtype=np.int32)
    for r0 in range(0, n_rows, block):
        dense = arr[r0:r0 + block].toarray()
        for b in range(dense.shape[0]):
            row = dense[b]
            for c in np.flatnonzero((row != 0) & ((cnt < K) | (row > low))):
                at = cnt[c] if cnt[c] < K else int(top_v[:, c].argmin())
                top_v[at, c], top_i[at, c] = row[c], r0 + b
                cnt[c] = min(K, cnt[c] + 1)
                low[c] = top_v[:cnt[c], c].min() if cnt[c] == K else -np.inf
    return time.perf_counter() - t0


def inference_pass(dev, n_batches, reps):
    """worker_fn over a synthetic cache of n_batches x N tokens of width D, TopK(32) SAE with S latents: wall seconds of the pass
    with and without top_k_tokens = K, alternating."""
    from saev_amd import disk, nn
    from saev_amd.data import OrderedConfig
    from saev_amd.data.shards import write_shards
    from saev_amd.framework import inference

    T = 256
    with tempfile.TemporaryDirectory(prefix="latent_topk_bench_") as tmp:
        tmp = pathlib.Path(tmp)
        rng = np.random.default_rng(0)
        acts = rng.standard_normal((n_batches * N // T, 1, T, D), dtype=np.float32)
        d = write_shards(tmp, acts, layers=(0,), max_tokens_per_shard=N * 4)
        runs_root = tmp / "saev" / "runs"
        runs_root.mkdir(parents=True)
        run = disk.Run.new("bench0lt", train_shards_dir=d, val_shards_dir=d, runs_root=runs_root)
        torch.manual_seed(0)
        sae = nn.SparseAutoencoder(nn.SparseAutoencoderConfig(d_model=D, d_sae=S, activation=nn.modeling.TopK(top_k=CAP, aux=nn.modeling.AuxK(k_aux=512))))
        nn.dump(run.ckpt, sae)
        out = {}
        for save in (False, True):
            cfg = inference.Config(run=run.run_dir, data=OrderedConfig(shards=d, layer=0, batch_size=N), force_recompute=True, save=save,
                                   device=str(dev))
            inference.worker_fn(cfg, top_k_tokens=K)  # warm-up: code objects, the loader, the allocator
            ts = {0: [], K: []}
            for _ in range(reps):
                for k in (0, K):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    inference.worker_fn(cfg, top_k_tokens=k)
                    torch.cuda.synchronize()
                    ts[k].append(time.perf_counter() - t0)
            without, with_ = statistics.median(ts[0]), statistics.median(ts[K])
            out["save" if save else "metrics_only"] = {
                "tokens": n_batches * N, "batches": n_batches, "reps": reps, "without_s": ts[0], "with_s": ts[K],
                "median_without_s": without, "median_with_s": with_, "added_ms_per_pass": (with_ - without) * 1e3}
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warm", type=int, default=24, help="batches fed before the warmed-up update is timed")
    ap.add_argument("--burst", type=int, default=10, help="calls enqueued back to back per event pair")
    ap.add_argument("--host-rows", type=int, default=512)
    ap.add_argument("--pass-batches", type=int, default=8)
    ap.add_argument("--pass-reps", type=int, default=3)
    ap.add_argument("--out", default=str(pathlib.Path(__file__).resolve().parent.parent / "profiles" / "latent_topk_bench_line.json"))
    a = ap.parse_args()
    a.pool = a.iters * a.burst
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    code_bytes = N * CAP * 8
    out = {"tool": "tools/bench_latent_topk.py", "device": torch.cuda.get_device_name(0), "iters": a.iters,
           "shape": {"n": N, "codes_per_row": CAP, "d_sae": S, "k": K}, "algorithmic_bytes": code_bytes,
           "burst": a.burst, "timing": "device events; burst = calls enqueued back to back per event pair, single = one call on an idle device"}
    warm = [make_batch(gen, dev) for _ in range(a.warm)]
    pool = [make_batch(gen, dev) for _ in range(a.pool)]
    acc = LatentTopK(S, K, dev)

    # (a) every entry a candidate: each call of a burst updates an empty state of its own
    fresh = [LatentTopK(S, K, dev) for _ in range(a.burst)]
    for f in fresh:
        f.add(*pool[0], row_base=0)  # code objects, the workspaces
    out["first_update"] = burst_ms(lambda j: fresh[j % a.burst].add(*pool[j], row_base=0), a.iters, a.burst,
                                   setup=lambda i: [f.zero_() for f in fresh])
    out["first_update_single"] = device_ms(lambda i: fresh[0].add(*pool[i], row_base=0), a.iters, setup=lambda i: fresh[0].zero_())
    del fresh
    # (b) warmed up: every timed update takes a batch the lists have not seen
    for j, (idx, val) in enumerate(warm):
        acc.add(idx, val, row_base=j * N)
    torch.cuda.synchronize()
    base = a.warm * N
    out["lists_full_after_warm"] = float((acc.top_cnt == K).float().mean())
    out["warm_update"] = burst_ms(lambda j: acc.add(*pool[j], row_base=base + j * N), a.iters, a.burst)
    base += a.pool * N
    more = [make_batch(gen, dev) for _ in range(a.iters)]
    out["warm_update_single"] = device_ms(lambda i: acc.add(*more[i], row_base=base + i * N), a.iters)
    base += a.iters * N
    # what a pass pays once, whatever its length: the state, its read-back and the file (host wall clock)
    fixed = []
    with tempfile.TemporaryDirectory(prefix="latent_topk_bench_") as tmp:
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fresh = LatentTopK(S, K, dev)
            got = fresh.read()
            torch.save({"values": got.values, "indices": got.indices, "counts": got.counts}, pathlib.Path(tmp) / "top_tokens.pt")
            fixed.append((time.perf_counter() - t0) * 1e3)
    out["once_per_pass_state_read_save"] = summary(fixed)
    # the BatchStats call of the pass (unmasked TopK batch: column sums of x and the per-latent sums over the codes)
    x = torch.randn(N, D, device=dev, generator=gen)
    stats = BatchStats(D, S, dev, want=("scalars", "col_sum", "n_pos", "value_sum"))
    stats.add(x, None, *pool[0], scalars=False)
    out["batch_stats_call_of_the_pass"] = burst_ms(lambda j: stats.add(x, None, *pool[j], scalars=False), a.iters, a.burst)
    out["batch_stats_call_of_the_pass_single"] = device_ms(lambda i: stats.add(x, None, *pool[i], scalars=False), a.iters)
    # the torch formulation, on the same state
    sv, sr = acc.top_val.t().contiguous(), acc.top_row.t().contiguous()
    sv = torch.where(torch.arange(K, device=dev)[:, None] < acc.top_cnt[None, :], sv, torch.full_like(sv, -torch.inf))
    torch_update(sv, sr, *pool[0], 0)
    out["torch_dense_topk_update"] = device_ms(lambda i: torch_update(sv, sr, *pool[i], base + i * N), max(3, a.iters // 5))
    got_v, got_r = torch_update(sv, sr, *pool[0], base + 10**9)
    acc2 = LatentTopK(S, K, dev)
    for t_, s_ in ((acc2.top_val, acc.top_val), (acc2.top_row, acc.top_row), (acc2.top_cnt, acc.top_cnt)):
        t_.copy_(s_)
    acc2.add(*pool[0], row_base=base + 10**9)
    out["torch_values_equal"] = bool(torch.equal(torch.where(got_v == -torch.inf, torch.zeros_like(got_v), got_v), acc2.top_val.t()))
    assert out["torch_values_equal"], "the torch baseline and the HIP update disagree on the values: neither timing may be quoted"
    del got_v, got_r, sv, sr
    torch.cuda.empty_cache()
    # the reference's algorithm on the host, on a slice
    secs = host_reference_algorithm(*pool[0], a.host_rows)
    out["host_reference_algorithm"] = {"rows": a.host_rows, "seconds": secs, "scaled_to_batch_ms": secs / a.host_rows * N * 1e3,
                                       "note": "empty lists: every entry updates one, as in (a)"}
    for key in ("first_update", "first_update_single", "warm_update", "warm_update_single", "batch_stats_call_of_the_pass",
                "batch_stats_call_of_the_pass_single", "torch_dense_topk_update", "once_per_pass_state_read_save"):
        host = f", host {out[key]['host_enqueue_median_ms'] * 1e3:.1f} us per enqueue" if "burst" in out[key] else ""
        print(f"{key}: {out[key]['median_ms'] * 1e3:.1f} us (spread {out[key]['spread_ms'] * 1e3:.1f}){host}", flush=True)
    print(f"host reference algorithm: {out['host_reference_algorithm']['scaled_to_batch_ms']:.0f} ms per batch (scaled)", flush=True)
    # (c) the whole pass
    out["inference_pass"] = inference_pass(dev, a.pass_batches, a.pass_reps)
    for mode, r in out["inference_pass"].items():
        print(f"inference pass ({mode}): {r['median_without_s']:.3f} s -> {r['median_with_s']:.3f} s with top_k_tokens={K}, "
              f"{r['added_ms_per_pass']:+.1f} ms per pass of {r['batches']} batches", flush=True)
    pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps({"written": a.out}))


if __name__ == "__main__":
    main()
