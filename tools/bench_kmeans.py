"""The k-means stages (engine.kmeans_*; baselines.MiniBatchKMeans) on one device -> one JSON line, also written to
profiles/kmeans_bench_line.json.  n = k = 16 384, D = 1 024 (the reference's default k at its default batch), rows "trained" (batch and
centres drawn from low-rank data-like rows, as tools/bench_dictionary_match.py) and "random" (Gaussian rows):

  assign.<rows>        hip_ms: engine.kmeans_assign, nearest (its read-back of `info` included); torch_ms: torch.cdist + argmin on the
                       same card; candidates per row, capacity, route, second-pass tiles of all tiles; exact_route_ms
  collapsed.<rows>     hip_ms: engine.kmeans_collapsed on the centres (tol 0.5); torch_ms: cdist + triu + nonzero
  group_update.<rows>  hip_ms: kmeans_group + kmeans_update; torch_ms: bincount + index_add_ + the blend
  partial_fit.<rows>   hip_ms: one MiniBatchKMeans.partial_fit on a warmed model; torch_ms: the same step written with cdist

Each stage runs in a child process of its own under its own time limit, after warm-up runs; medians with interquartile ranges from
HIP events.  The first stage that fails or runs out of time ends the run: nothing more is started on the device.

    python tools/bench_kmeans.py [--reps N] [--stages a,b] [--rows trained,random] [--n N --k K --d D]
"""
import argparse
import json
import pathlib
import statistics
import subprocess
import sys

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

STAGES = ("assign", "collapsed", "group_update", "partial_fit")
KINDS = ("trained", "random")
STAGE_LIMIT_S = 240


def rows(kind, S, D, dev, seed):
    import torch

    g = torch.Generator(device=dev).manual_seed(S + D + seed)
    if kind == "random":
        return torch.randn(S, D, device=dev, generator=g)
    U = torch.randn(64, D, device=dev, generator=g)
    z = torch.randn(S, 64, device=dev, generator=g)
    return z @ U + 0.3 * torch.randn(S, D, device=dev, generator=g)


def timed(fn, n, warmup=2):
    import torch

    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    q = statistics.quantiles(ms, n=4) if len(ms) >= 2 else [ms[0]] * 3
    return {"median": round(statistics.median(ms), 4), "iqr": round(q[2] - q[0], 4), "n": n}


def torch_step(x, centers, counts, tol):
    """What a user writes today: the reference's partial_fit on the device (no empty clusters or re-seeding on this path)."""
    import torch

    d = torch.cdist(x, centers)
    a = d.argmin(dim=1)
    cb = torch.bincount(a, minlength=centers.shape[0]).to(x.dtype)
    sums = torch.zeros_like(centers).index_add_(0, a, x)
    prev = counts.clone()
    counts += cb
    m = cb > 0
    centers[m] = (centers[m] * prev[m].unsqueeze(1) + sums[m]) / counts[m].unsqueeze(1)
    inertia = d[torch.arange(x.shape[0], device=x.device), a].pow(2).mean().item()
    close = torch.triu(torch.cdist(centers, centers) < tol, diagonal=1)
    return inertia, bool(close.any())


def stage(name, kind, n, k, D, reps):
    import torch

    from saev_amd import _lib, baselines, engine

    dev = torch.device("cuda:0")
    X, C = rows(kind, n, D, dev, 0), rows(kind, k, D, dev, 1)
    counts = torch.randint(1, 100, (k,), device=dev).float()
    rec = {}
    if name == "assign":
        r = engine.kmeans_assign(X, C)
        rec.update(route=r.route, overflow=r.overflow, candidates_per_row=round(r.candidates / n, 3), capacity=r.capacity,
                   tiles_refiltered=r.tiles_refiltered, tiles=-(-n // 128) * -(-k // 128),
                   workspace_bytes=int(_lib.load().saev_kmeans_workspace_bytes(n, k, D)))
        rec["hip_ms"] = timed(lambda: engine.kmeans_assign(X, C), reps)
        rec["torch_ms"] = timed(lambda: torch.cdist(X, C).argmin(dim=1), reps)
        rec["exact_route_ms"] = timed(lambda: engine.kmeans_assign(X, C, route="exact"), 2, warmup=1)["median"]
    elif name == "collapsed":
        r = engine.kmeans_collapsed(C, counts, 0.5)
        rec.update(route=r.route, overflow=r.overflow, candidates=r.candidates, capacity=r.capacity, losers=int(r.losers.sum()))
        rec["hip_ms"] = timed(lambda: engine.kmeans_collapsed(C, counts, 0.5), reps)
        rec["torch_ms"] = timed(lambda: torch.triu(torch.cdist(C, C) < 0.5, diagonal=1).nonzero(), reps)
    elif name == "group_update":
        idx = engine.kmeans_assign(X, C).indices

        def hip():
            c, cn = C.clone(), counts.clone()
            _, starts, rws = engine.kmeans_group(idx, k)
            engine.kmeans_update(X, starts, rws, c, cn)

        def ref():
            c, cn = C.clone(), counts.clone()
            cb = torch.bincount(idx.long(), minlength=k).float()
            sums = torch.zeros_like(c).index_add_(0, idx.long(), X)
            m = cb > 0
            c[m] = (c[m] * cn[m].unsqueeze(1) + sums[m]) / (cn[m] + cb[m]).unsqueeze(1)

        rec["hip_ms"], rec["torch_ms"] = timed(hip, reps), timed(ref, reps)
    elif name == "partial_fit":
        model = baselines.MiniBatchKMeans(k, device="cuda:0")
        model.cluster_centers_, model.cluster_counts_, model.n_features_in_, model._zero_counts = C.clone(), counts.clone(), D, False
        rec["hip_ms"] = timed(lambda: model.partial_fit(X), reps)
        rec["last_assign"] = model.last_assign_
        c, cn = C.clone(), counts.clone()
        rec["torch_ms"] = timed(lambda: torch_step(X, c, cn, 0.5), reps)
    else:
        raise SystemExit(f"unknown stage {name!r}")
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--stages", default=",".join(STAGES))
    ap.add_argument("--rows", default=",".join(KINDS))
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--k", type=int, default=16384)
    ap.add_argument("--d", type=int, default=1024)
    ap.add_argument("--child", help="STAGE.ROWS: run that stage in this process (what the parent starts)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "kmeans_bench_line.json"))
    args = ap.parse_args()
    if args.child:
        name, kind = args.child.split(".")
        return stage(name, kind, args.n, args.k, args.d, args.reps)
    out = {"n": args.n, "k": args.k, "D": args.d}
    for name in args.stages.split(","):
        for kind in args.rows.split(","):
            cmd = [sys.executable, __file__, "--child", f"{name}.{kind}", "--reps", str(args.reps), "--n", str(args.n), "--k", str(args.k),
                   "--d", str(args.d)]
            try:
                done = subprocess.run(cmd, capture_output=True, text=True, timeout=STAGE_LIMIT_S)
            except subprocess.TimeoutExpired:
                out[f"{name}.{kind}"] = {"error": f"no result within {STAGE_LIMIT_S} s"}
                print(json.dumps(out))
                return 1
            if done.returncode != 0:
                out[f"{name}.{kind}"] = {"error": f"exit status {done.returncode}", "stderr": done.stderr[-400:]}
                print(json.dumps(out))
                return 1
            out[f"{name}.{kind}"] = json.loads(done.stdout.strip().splitlines()[-1])
    line = json.dumps(out)
    print(line)
    pathlib.Path(args.out).write_text(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
