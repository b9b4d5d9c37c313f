"""Batch statistics (engine.BatchStats / row_norm_mean) against the torch glue they replaced, restated here as it
stood in framework/train.py and framework/inference.py before: the log block's statistics, one evaluate() batch, one masked
inference batch and the decoder row-norm mean, at configs[1] (n 16 384, D 1 024, S 32 768, k 32) and at configs[3]'s shape
(D 1 280, S 81 920, k 64).

    python tools/bench_batch_stats.py [--iters 30] [--out profiles/batch_stats_bench_line.json]

Both sides run in one process, alternating call by call after a warm-up; every call is timed from the host with the device
synchronised before and after (the glue's own read-backs are part of what it costs).  Reported per pair: median, interquartile
spread, min and max of each side in ms, and whether the gap between the medians exceeds the larger spread.  The kernels' own
device time (events around the enqueue, no read-back) gives bytes per second over the algorithmic bytes -- x, x_hat and the codes
once; W once for the row norms -- as a share of the HBM rates (8.0 TB/s datasheet, 6.29 TB/s measured float4 copy)."""
import argparse
import json
import pathlib
import statistics
import sys
import time

import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1]))

from saev_amd.engine import BatchStats, row_norm_mean

SHAPES = {"configs1": (16384, 1024, 32768, 32), "configs3": (16384, 1280, 81920, 64)}
HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12


# ---- the glue as it stood ------------------------------------------------------------------------------------------------------

def glue_copy_last(src):
    """eng.last_codes(n): device-to-device copies of the context's idx, val and x_hat."""
    return src["idx"].clone(), src["val"].clone(), src["x_hat"].clone()


def glue_log(x, src, S):
    n, D = x.shape
    idx, val, x_hat = glue_copy_last(src)
    x64 = x.to(torch.float64)
    residual = x - x_hat
    r64 = residual.to(torch.float64)
    sums = torch.cat([x64.sum(dim=0), torch.stack([x64.sum(), r64.sum(), (r64 * r64).sum()]),
                      torch.tensor([1.0, 2.0, 3.0, 4.0, 5.0, 6.0, float(n)], dtype=torch.float64, device=x.device)])
    live = torch.zeros(S, device=x.device, dtype=torch.int32)
    live[idx[val.abs() > 1e-12].long()] = 1
    sum_vec, rest = sums[:D], sums[D:].tolist()
    base = rest[4] - torch.dot(sum_vec, sum_vec).item() / n
    explained = (1 - residual.var() / x.var()).item()
    return explained, (live == 0).float().mean().item(), base


def new_log(acc, x, src):
    acc.zero_()
    acc.add(x, src["x_hat"], src["idx"], src["val"])
    h = acc.read()
    n, D = x.shape
    m = n * D
    explained = 1 - ((h.sum_rr - h.sum_r ** 2 / m) / (m - 1)) / ((h.sum_xx - h.sum_x ** 2 / m) / (m - 1))
    base = h.sum_xx - torch.dot(h.col_sum, h.col_sum).item() / n
    return explained, (h.live == 0).float().mean().item(), base


def glue_eval(x, src, st):
    st["sum_vec"] += x.to(torch.float64).sum(dim=0)
    idx, val, _ = glue_copy_last(src)
    pos = val > 0
    st["n_fired"].index_add_(0, idx[pos].long(), torch.ones_like(val[pos]))
    st["values"].index_add_(0, idx.reshape(-1).long().clamp_min(0), val.reshape(-1))


def new_eval(acc, x, src):
    acc.add(x, None, src["idx"], src["val"])


def glue_infer_masked(x, src, keep, st):
    idx, val, x_hat = glue_copy_last(src)
    x64 = x[keep].to(torch.float64)
    diff = x64 - x_hat[keep].to(torch.float64)
    st["sse"] += (diff * diff).sum()
    st["sum_sq"] += (x64 * x64).sum()
    st["sum_vec"] += x64.sum(dim=0)
    live = (val != 0) & keep[:, None]
    cols, vals = idx[live].long(), val[live]
    st["values"].index_add_(0, cols, vals)
    st["n_fired"].index_add_(0, cols, (vals > 0).to(torch.float32))


def new_infer_masked(acc, x, src, keep):
    acc.add(x, src["x_hat"], src["idx"], src["val"], keep=keep)


# ---- timing ----------------------------------------------------------------------------------------------------------------------

def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def summary(ts):
    q = statistics.quantiles(ts, n=4)
    return {"median_ms": statistics.median(ts), "spread_ms": q[2] - q[0], "min_ms": min(ts), "max_ms": max(ts), "n": len(ts)}


def pair(old, new, warmup, iters):
    for _ in range(warmup):
        old(); new()
    a, b = [], []
    for _ in range(iters):
        a.append(timed(old))
        b.append(timed(new))
    so, sn = summary(a), summary(b)
    gap = so["median_ms"] - sn["median_ms"]
    return {"glue": so, "new": sn, "gap_ms": gap, "speedup": so["median_ms"] / sn["median_ms"],
            "gap_exceeds_larger_spread": gap > max(so["spread_ms"], sn["spread_ms"])}


def device_ms(fn, iters):
    """Median device time of the enqueued work alone (events, no read-back)."""
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


def bytes_line(ms, nbytes):
    rate = nbytes / (ms["median_ms"] * 1e-3)
    return {**ms, "algorithmic_bytes": nbytes, "bytes_per_s": rate, "share_of_8.0TBps": rate / HBM_SPEC, "share_of_6.29TBps_copy": rate / HBM_COPY}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES))
    ap.add_argument("--out", default=str(pathlib.Path(__file__).resolve().parent.parent / "profiles" / "batch_stats_bench_line.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    out = {"tool": "tools/bench_batch_stats.py", "device": torch.cuda.get_device_name(0), "iters": a.iters, "warmup": a.warmup,
           "timing": "host wall clock, device synchronised before and after each call, glue and new alternating", "shapes": {}}
    for name in a.shapes:
        n, D, S, k = SHAPES[name]
        gen = torch.Generator(device=dev).manual_seed(0)
        x = torch.randn(n, D, device=dev, generator=gen)
        src = {"x_hat": x + 0.3 * torch.randn(n, D, device=dev, generator=gen),
               "idx": torch.randint(0, S, (n, k), device=dev, generator=gen, dtype=torch.int32),
               "val": torch.randn(n, k, device=dev, generator=gen).abs()}
        W = torch.randn(S, D, device=dev, generator=gen)
        keep = torch.zeros(n, dtype=torch.bool, device=dev)
        keep[::3] = True
        z = lambda *s, dt=torch.float32: torch.zeros(*s, device=dev, dtype=dt)  # noqa: E731
        st = {"sum_vec": z(D, dt=torch.float64), "n_fired": z(S), "values": z(S), "sse": z((), dt=torch.float64), "sum_sq": z((), dt=torch.float64)}
        acc_log = BatchStats(D, S, dev, want=("scalars", "col_sum", "live"))
        acc_eval = BatchStats(D, S, dev, want=("col_sum", "n_pos", "value_sum"))
        acc_inf = BatchStats(D, S, dev, want=("scalars", "col_sum", "n_pos", "value_sum"))
        res = {"n": n, "d_model": D, "d_sae": S, "k": k}
        g, w = glue_log(x, src, S), new_log(acc_log, x, src)
        res["log_block_values"] = {"glue": g, "new": w}
        res["log_block"] = pair(lambda: glue_log(x, src, S), lambda: new_log(acc_log, x, src), a.warmup, a.iters)
        res["evaluate_batch"] = pair(lambda: glue_eval(x, src, st), lambda: new_eval(acc_eval, x, src), a.warmup, a.iters)
        res["inference_masked_batch"] = pair(lambda: glue_infer_masked(x, src, keep, st), lambda: new_infer_masked(acc_inf, x, src, keep),
                                             a.warmup, a.iters)
        res["row_norm_mean"] = pair(lambda: W.norm(dim=1).mean().item(), lambda: row_norm_mean(W), a.warmup, a.iters)
        dense_bytes, code_bytes = 2 * n * D * 4, n * k * 8
        res["device_time"] = {
            "log_block_kernels": bytes_line(device_ms(lambda: acc_log.add(x, src["x_hat"], src["idx"], src["val"]), a.iters), dense_bytes + code_bytes),
            "evaluate_kernels": bytes_line(device_ms(lambda: acc_eval.add(x, None, src["idx"], src["val"]), a.iters), n * D * 4 + code_bytes),
            "inference_masked_kernels": bytes_line(device_ms(lambda: acc_inf.add(x, src["x_hat"], src["idx"], src["val"], keep=keep), a.iters),
                                                   dense_bytes + code_bytes),
        }
        out["shapes"][name] = res
        for key in ("log_block", "evaluate_batch", "inference_masked_batch", "row_norm_mean"):
            r = res[key]
            print(f"{name} {key}: glue {r['glue']['median_ms']:.3f} ms (spread {r['glue']['spread_ms']:.3f}) -> new {r['new']['median_ms']:.3f} ms "
                  f"(spread {r['new']['spread_ms']:.3f}), x{r['speedup']:.1f}, gap > spread: {r['gap_exceeds_larger_spread']}", flush=True)
        for key, r in res["device_time"].items():
            print(f"{name} {key}: {r['median_ms'] * 1e3:.1f} us on the device, {r['bytes_per_s'] / 1e12:.2f} TB/s = {r['share_of_6.29TBps_copy']:.0%} of the "
                  f"measured copy rate, {r['share_of_8.0TBps']:.0%} of the datasheet rate", flush=True)
        del x, src, W, st, acc_log, acc_eval, acc_inf
        torch.cuda.empty_cache()
    pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps({"written": a.out}))


if __name__ == "__main__":
    main()
