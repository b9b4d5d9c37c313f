"""Pooling and the L1 solver (engine.pool_images, engine.l1_logistic) at the audit's training shape: 16 384 images x
256 patches x 32 codes, S = 16 384 latents (nnz = 2^27), K = 10 classes; the pooled X is 1.07 GB.

  pooling      events around ``engine.pool_images`` for max and mean (output allocation included), median of ``--iters`` calls
  iteration    one solver iteration: the difference of two fits stopped by ``max_iter`` at ``--iter-a`` and ``--iter-b`` iterations,
               divided by their distance (init, result and the first iterations' rejected steps cancel); beside it the bytes bound --
               two passes over X at the 6.3 TB/s copy rate -- and the ratio to it
  fit          a whole fit to kkt_tol = 1e-4 with its iteration count, rejected steps and restarts
  baselines    plain torch on the same device: the same iteration as ``X @ W.T``, a softmax and ``R.T @ X`` on a float64 copy of X
               (made outside the timed region), and the dense max-pool of a block of ``--block`` images (densified outside the timed
               region), scaled to all images

    python tools/bench_sparse_linear.py [--iters 5] [--out profiles/sparse_linear_bench_line.json]

Writes one JSON line.  No test asserts a time."""
import argparse
import json
import pathlib
import statistics
import sys
import warnings

import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1]))

from saev_amd import engine  # noqa: E402

N_IMAGES, TPI, CAP, S, K = 16384, 256, 32, 16384, 10
COPY_RATE = 6.3e12  # bytes / s


def make_codes(gen, dev):
    """Codes as a TopK encoder leaves them: CAP distinct latents per patch in ascending order, positive values."""
    n = N_IMAGES * TPI
    start = torch.randint(0, S, (n, 1), device=dev, generator=gen)
    stride = torch.randint(1, S // CAP, (n, 1), device=dev, generator=gen)
    idx = ((start + torch.arange(CAP, device=dev)[None, :] * stride) % S).sort(dim=1).values.to(torch.int32)
    val = torch.randn(n, CAP, device=dev, generator=gen).abs() + 1 / 64
    indptr = torch.arange(n + 1, device=dev, dtype=torch.int64) * CAP
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


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--iter-a", type=int, default=20)
    ap.add_argument("--iter-b", type=int, default=60)
    ap.add_argument("--block", type=int, default=64)
    ap.add_argument("--C", type=float, default=0.01)
    ap.add_argument("--out", type=pathlib.Path, default=pathlib.Path("profiles/sparse_linear_bench_line.json"))
    a = ap.parse_args()
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(0)
    indptr, indices, data = make_codes(gen, dev)

    pool = {}
    for agg in ("max", "mean"):
        engine.pool_images(indptr, indices, data, N_IMAGES, TPI, S, agg).pooled  # (reads the error word: the inputs are good)
        pool[agg] = event_ms(lambda: engine.pool_images(indptr, indices, data, N_IMAGES, TPI, S, agg), a.iters)
    X = engine.pool_images(indptr, indices, data, N_IMAGES, TPI, S, "max").pooled

    # torch's dense max-pool of one block of images
    rows = a.block * TPI
    dense = torch.zeros(rows, S, device=dev)
    dense[torch.arange(rows, device=dev).repeat_interleave(CAP), indices[:rows * CAP].long()] = data[:rows * CAP]
    dense = dense.reshape(a.block, TPI, S)
    assert torch.equal(dense.amax(dim=1), X[:a.block])
    base_pool = event_ms(lambda: dense.amax(dim=1), a.iters)
    del dense, indptr, indices, data

    # three class-informative latents per class on top of the pooled codes
    y = torch.randint(0, K, (N_IMAGES,), device=dev, generator=gen)
    for j in range(3):
        X[torch.arange(N_IMAGES, device=dev), 3 * y + j] += 2.0 * torch.rand(N_IMAGES, device=dev, generator=gen)

    def fit(max_iter):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return engine.l1_logistic(X, y, a.C, max_iter=max_iter, check_every=max_iter)

    fit(2)
    t_a, t_b = event_ms(lambda: fit(a.iter_a), a.iters), event_ms(lambda: fit(a.iter_b), a.iters)
    iteration_ms = (t_b["median_ms"] - t_a["median_ms"]) / (a.iter_b - a.iter_a)
    bound_ms = 2 * X.numel() * 4 / COPY_RATE * 1e3
    whole = {}
    res = None

    def whole_fit():
        nonlocal res
        res = engine.l1_logistic(X, y, a.C)

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        whole = event_ms(whole_fit, 1)

    Xd = X.double()
    W = torch.zeros(K, S, device=dev, dtype=torch.float64)
    onehot = torch.nn.functional.one_hot(y, K).double()

    def torch_iteration():
        Z = Xd @ W.T
        R = torch.softmax(Z, dim=1) - onehot
        return R.T @ Xd

    torch_iteration()
    base_iter = event_ms(torch_iteration, a.iters)
    line = {"bench": "sparse_linear", "n_images": N_IMAGES, "tokens_per_image": TPI, "codes_per_token": CAP, "n_latents": S, "n_classes": K, "C": a.C,
            "device": torch.cuda.get_device_name(0), "x_bytes": X.numel() * 4, "pool_ms": pool,
            "torch_dense_max_pool": {"block_images": a.block, "block_ms": base_pool, "scaled_to_all_images_ms": base_pool["median_ms"] * N_IMAGES / a.block},
            "iteration_ms": iteration_ms, "iteration_from_fits_of": [a.iter_a, a.iter_b], "fits_ms": [t_a, t_b],
            "bytes_bound_ms": bound_ms, "iteration_over_bytes_bound": iteration_ms / bound_ms,
            "fit": {"ms": whole["median_ms"], "n_iter": res.n_iter_, "converged": res.converged_, "kkt_residual": res.kkt_residual_, "objective": res.objective_,
                    "lipschitz": res.lipschitz_, "rejected": res.n_rejected_, "restarts": res.n_restarts_, "features_kept": int((res.coef_ != 0).any(dim=0).sum().item())},
            "workspace_bytes": int(res.layout.total_bytes), "torch_fp64_iteration_ms": base_iter, "torch_iteration_over_ours": base_iter["median_ms"] / iteration_ms}
    a.out.parent.mkdir(parents=True, exist_ok=True)
    a.out.write_text(json.dumps(line) + "\n")
    print(json.dumps(line))
    return 0


if __name__ == "__main__":
    sys.exit(main())
