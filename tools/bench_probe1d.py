"""Per-latent logistic probes (engine.Probe1D) on a synthetic split shaped like a TopK SAE's ``token_acts.npz``:
``--rows`` tokens x ``--latents`` latents with ``--k`` codes per row, ``--classes`` classes (default 1 M x 16 384 x 32 x 151).

Per size it reports, from device events around calls that end in a synchronise (median of ``--iters`` after a warm-up call):

  prepare_ms            the latent-major sort, qx, label bits
  stats_ms              the event sums of all pairs at the current (b, w): the hot kernel and the chunk reduction -- one iteration's
                        share of a fit; beside it the sigmoid evaluations per second (events x classes / time)
  update_ms             one solver iteration of all pairs from those sums
  fit_ms                a whole fit at max_iter = 30, polling the done counter every iteration (host wall clock, one run)
  evaluate_ms           loss and confusion counts at the fitted coefficients
  torch_slab_iter_ms    ONE slab (``--slab`` classes) of ONE iteration in plain torch on the same GPU, written for this tool: gather
                        (b, w) per event, the elementwise terms, seven ``index_add_`` into (latents, slab) float32 sums -- the
                        formulation the HIP path replaces; ``torch_iter_ms_scaled`` = that x the number of slabs

    python tools/bench_probe1d.py [--rows 1048576 [4194304 ...]] [--out profiles/probe1d_bench_line.json]
"""
import argparse
import json
import pathlib
import statistics
import sys
import time

import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1]))

from saev_amd.engine import Probe1D, Probe1DHyper  # noqa: E402


def summary(ts):
    q = statistics.quantiles(ts, n=4) if len(ts) > 1 else [ts[0]] * 3
    return {"median_ms": statistics.median(ts), "spread_ms": q[2] - q[0], "min_ms": min(ts), "n": len(ts)}


def device_ms(fn, iters):
    fn()  # warm-up: code objects, allocator
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return summary(ts)


def make_split(n, s, k, c, dev, seed):
    """k distinct latents per row (a random start and stride through the latents, ascending), positive values that lean on the row's
    class for a tenth of the latents, class ids uniform over c."""
    gen = torch.Generator(device=dev).manual_seed(seed)
    labels = torch.randint(0, c, (n,), device=dev, generator=gen)
    start = torch.randint(0, s, (n, 1), device=dev, generator=gen)
    stride = torch.randint(1, s // k, (n, 1), device=dev, generator=gen)
    idx = ((start + torch.arange(k, device=dev)[None, :] * stride) % s).sort(dim=1).values
    val = torch.randn(n, k, device=dev, generator=gen).abs() + 1e-3
    val = val + ((idx % (10 * c)) == labels[:, None]).float()
    indptr = torch.arange(n + 1, device=dev, dtype=torch.int64) * k
    return indptr, idx.reshape(-1).to(torch.int32), val.reshape(-1), labels.to(torch.uint8 if c <= 256 else torch.int32)


def torch_slab_iteration(cols, rows, vals, y_slab, b, w, s):
    """One slab of one iteration, plain torch, float32 (the reference's default dtype): returns the seven (latents, slab) sums."""
    v = vals[:, None]
    logits = b[cols] + w[cols] * v
    mu = torch.sigmoid(logits)
    sv = mu * (1 - mu)
    yy = y_slab[rows]
    out = []
    for term in (mu, (mu - yy) * v, sv, sv * v, sv * v * v, torch.nn.functional.binary_cross_entropy_with_logits(logits, yy, reduction="none"), yy):
        out.append(torch.zeros(s, y_slab.shape[1], device=vals.device).index_add_(0, cols, term))
    return out


def run_size(n, a, dev):
    s, k, c = a.latents, a.k, a.classes
    indptr, indices, data, labels = make_split(n, s, k, c, dev, seed=n % 9973)
    nnz = indices.numel()
    p = Probe1D(n, s, c, nnz, dev)
    out = {"rows": n, "latents": s, "k": k, "classes": c, "nnz": nnz, "workspace_gib": p.layout.total_bytes / 2**30, "chunk": p.layout.chunk,
           "chunks": None}
    out["prepare_ms"] = device_ms(lambda: p.prepare(indptr, indices, data, labels=labels), max(3, a.iters // 3))
    out["chunks"] = int(p.chunk_starts[-1].item())
    timing = Probe1DHyper(max_iter=30, class_slab_size=a.slab, tol=0.0)  # tol 0: no slab stops while update is being timed
    p.init(timing)
    for _ in range(3):  # a few real iterations, so that (b, w) are not the all-equal start
        p.update(timing, p.stats(p.state("b"), p.state("w")))
    sums = p.stats(p.state("b"), p.state("w"))
    out["stats_ms"] = device_ms(lambda: p.stats(p.state("b"), p.state("w")), a.iters)
    out["stats_evaluations_per_s"] = nnz * c / (out["stats_ms"]["median_ms"] * 1e-3)
    out["update_ms"] = device_ms(lambda: p.update(timing, sums), a.iters)
    hp = Probe1DHyper(max_iter=30, class_slab_size=a.slab)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    coef, icpt, n_iter = p.fit(hp, dtype=torch.float32, poll_every=1)
    torch.cuda.synchronize()
    out["fit_ms"] = (time.perf_counter() - t0) * 1e3
    out["fit_n_iter_max"] = int(n_iter.max().item())
    b64, w64 = icpt.double(), coef.double()
    out["evaluate_ms"] = device_ms(lambda: p.evaluate(b64, w64, 0.5), a.iters)
    # the torch formulation of one slab iteration (float32)
    rows = torch.repeat_interleave(torch.arange(n, device=dev), k)
    cols = indices.long()
    y_slab = torch.nn.functional.one_hot(labels.long(), c)[:, :a.slab].float()
    b32, w32 = icpt[:, :a.slab].float().contiguous(), coef[:, :a.slab].float().contiguous()
    out["torch_slab_iter_ms"] = device_ms(lambda: torch_slab_iteration(cols, rows, data, y_slab, b32, w32, s), max(3, a.iters // 3))
    n_slabs = -(-c // a.slab)
    out["torch_iter_ms_scaled"] = out["torch_slab_iter_ms"]["median_ms"] * n_slabs
    out["iter_ms"] = out["stats_ms"]["median_ms"] + out["update_ms"]["median_ms"]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, nargs="+", default=[1 << 20])
    ap.add_argument("--latents", type=int, default=16384)
    ap.add_argument("--k", type=int, default=32)
    ap.add_argument("--classes", type=int, default=151)
    ap.add_argument("--slab", type=int, default=8)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=str(pathlib.Path(__file__).resolve().parent.parent / "profiles" / "probe1d_bench_line.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_probe1d needs a HIP device: there is nothing to measure without one")
    dev = torch.device("cuda", 0)
    out = {"tool": "tools/bench_probe1d.py", "device": torch.cuda.get_device_name(0), "iters": a.iters, "slab": a.slab,
           "sizes": [run_size(n, a, dev) for n in a.rows]}
    line = json.dumps(out)
    print(line)
    if a.out:
        pathlib.Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
