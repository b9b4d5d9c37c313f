"""Interventions on latents (saev_amd/interventions.py) at configs[1]'s shape (n 16 384 rows, D 1 024, S 32 768,
k 32), in one process:

  (a) the edit kernel (engine.intervene_rows) with 1 global edit, with 64 global edits, and with a 150-class lookup (one SET per
      class, every row in one class);
  (b) a device ``copy_`` of the same n x D floats: the bytes floor (one read and one write of x);
  (c) the whole ``intervene`` call (encode_sparse + the kernel) beside ``sae(x)``;
  (d) the dense torch formulation ``(x - x_hat) + decode(f_mod)`` on as many rows as fit (an n x S matrix and two dense products);
  (e) ``ClassFireCounts.add`` and ``f1`` at C = 151, T = 4.

    python tools/bench_interventions.py [--iters 30] [--out profiles/interventions_bench_line.json]

Device events around one call on a synchronised device; the kernel figures alternate x buffers out of a pool larger than the
Infinity Cache, so that x streams from HBM as it does inside a model's forward pass.  There is no pass/fail threshold on a time."""
import argparse
import json
import pathlib
import statistics
import sys

import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1]))

from saev_amd import engine, interventions, nn  # noqa: E402

N, D, S, K = 16384, 1024, 32768, 32


def summary(ts):
    q = statistics.quantiles(ts, n=4)
    return {"median_ms": statistics.median(ts), "spread_ms": q[2] - q[0], "min_ms": min(ts), "max_ms": max(ts), "n": len(ts)}


def device_ms(fn, iters, warmup=3):
    ts = []
    for i in range(-warmup, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn(i % 1000003)
        e1.record()
        torch.cuda.synchronize()
        if i >= 0:
            ts.append(e0.elapsed_time(e1))
    return summary(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--pool", type=int, default=6, help="x buffers alternated (6 x 64 MiB: past the 256 MiB Infinity Cache)")
    ap.add_argument("--dense-rows", type=int, default=4096)
    ap.add_argument("--out", default=str(pathlib.Path(__file__).resolve().parent.parent / "profiles" / "interventions_bench_line.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    torch.manual_seed(0)
    sae = nn.SparseAutoencoder(nn.SparseAutoencoderConfig(d_model=D, d_sae=S, activation=nn.modeling.TopK(top_k=K, aux=nn.modeling.AuxK(k_aux=512)))).to(dev).eval()
    xs = [torch.randn(N, D, device=dev, generator=gen) for _ in range(a.pool)]
    outs = [torch.empty_like(xs[0]) for _ in range(2)]
    with torch.no_grad():
        idx, val = sae.encode_sparse(xs[0])
    fired = torch.bincount(idx.reshape(-1).long(), minlength=S)
    busy = torch.argsort(fired, descending=True)[:256].tolist()
    labels = torch.randint(0, 151, (N,), device=dev, generator=gen).to(torch.int32)
    plans = {
        "1_global_edit": interventions.EditSet([interventions.Edit(busy[0], "set", 3.0)], S),
        "64_global_edits": interventions.EditSet([interventions.Edit(l, "set", 3.0) for l in busy[:64]], S),
        "150_class_lookup": interventions.EditSet([interventions.Edit(busy[c % 256], "set", 3.0, group=c) for c in range(1, 151)], S, n_groups=151),
    }
    out = {"tool": "tools/bench_interventions.py", "device": torch.cuda.get_device_name(0), "iters": a.iters,
           "shape": {"n": N, "d_model": D, "d_sae": S, "k": K}, "floor_bytes": 2 * N * D * 4 + N * K * 8,
           "timing": "device events around one call on a synchronised device; x alternates over a pool past the Infinity Cache"}
    W = sae.W_dec.detach()
    for name, es in plans.items():
        plan = es.plan(dev)
        rg = labels if es.n_groups else None
        counts = torch.zeros(len(es), device=dev, dtype=torch.int64)
        out[f"kernel_{name}"] = device_ms(lambda i: engine.intervene_rows(xs[i % a.pool], W, idx, val, None, plan, len(es), es.n_groups, row_group=rg,
                                                                          out=outs[i % 2]), a.iters)
        out[f"kernel_{name}_with_counts"] = device_ms(lambda i: engine.intervene_rows(xs[i % a.pool], W, idx, val, None, plan, len(es), es.n_groups,
                                                                                      row_group=rg, out=outs[i % 2], rows_changed=counts), a.iters)
    out["copy_n_by_d"] = device_ms(lambda i: outs[i % 2].copy_(xs[i % a.pool]), a.iters)
    floor = out["copy_n_by_d"]["median_ms"]
    for name in plans:
        out[f"kernel_{name}"]["ratio_to_copy"] = out[f"kernel_{name}"]["median_ms"] / floor
    with torch.no_grad():
        es = plans["1_global_edit"]
        out["intervene_call_1_global_edit"] = device_ms(lambda i: interventions.intervene(sae, xs[i % a.pool], es), a.iters)
        out["intervene_call_150_class_lookup"] = device_ms(lambda i: interventions.intervene(sae, xs[i % a.pool], plans["150_class_lookup"], row_group=labels),
                                                           a.iters)
        out["encode_sparse"] = device_ms(lambda i: sae.encode_sparse(xs[i % a.pool]), a.iters)
        out["sae_forward"] = device_ms(lambda i: sae(xs[i % a.pool]), a.iters)
        # the dense torch formulation on a slice (the reference's modify): n x S latents, two dense decodes
        r = a.dense_rows
        lat = busy[0]

        def dense(i):
            x = xs[i % a.pool][:r]
            f = torch.zeros(r, S, device=dev)
            f.scatter_(1, idx[:r].long(), val[:r])
            x_hat = f @ W + sae.b_dec
            f[:, lat] = 3.0
            return (x - x_hat) + (f @ W + sae.b_dec)

        out["dense_torch_formulation"] = {**device_ms(dense, max(3, a.iters // 5)), "rows": r}
        out["dense_torch_formulation"]["scaled_to_batch_ms"] = out["dense_torch_formulation"]["median_ms"] * N / r
        # same answer, within the dense path's own rounding
        plan = es.plan(dev)
        got = engine.intervene_rows(xs[0][:r].contiguous(), W, idx[:r].contiguous(), val[:r].contiguous(), None, plan, 1, 0)
        out["max_abs_difference_from_dense"] = float((got - dense(0)).abs().max())
        cfc = engine.ClassFireCounts(S, 151, dev)
        out["class_fire_counts_add"] = device_ms(lambda i: cfc.add(idx, val, None, labels), a.iters)
        out["class_fire_counts_f1"] = device_ms(lambda i: cfc.f1(), a.iters)
    for key, v in out.items():
        if isinstance(v, dict) and "median_ms" in v:
            extra = f", {v['ratio_to_copy']:.2f} x the copy" if "ratio_to_copy" in v else ""
            print(f"{key}: {v['median_ms'] * 1e3:.1f} us (spread {v['spread_ms'] * 1e3:.1f}){extra}", flush=True)
    print(f"max |kernel - dense| on {a.dense_rows} rows: {out['max_abs_difference_from_dense']:.3g}", flush=True)
    pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps({"written": a.out}))


if __name__ == "__main__":
    main()
