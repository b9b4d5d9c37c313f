"""End-to-end rate of `framework.train.train()` on a synthetic protocol-2.1 cache (BASELINE.json config 5 shape):
shards -> feed (streaming reservoir or resident pool) -> train step, one epoch each.

    python tools/bench_train_e2e.py --gb 12 --root /dev/shm
    python tools/bench_train_e2e.py --gb 12 --root /dev/shm --modes resident --log-every 25   # with the log block (coherence on)

The cache is page-cache hot, so the streaming number is the framework's ceiling, not a disk measurement.  make_saes
(reference train.py:108-189) consumes the first batches; the rate is over the train loop only."""
import argparse
import dataclasses
import os
import shutil
import tempfile
import time

import numpy as np
import torch

from saev_amd import data, nn
from saev_amd.framework import train as T
from saev_amd.nn import modeling, objectives


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gb", type=float, default=12.0)
    ap.add_argument("--d-model", type=int, default=1024)
    ap.add_argument("--exp", type=int, default=32)
    ap.add_argument("--top-k", type=int, default=32)
    ap.add_argument("--tokens", type=int, default=256)
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--threads", type=int, default=4)
    ap.add_argument("--root", default=None)
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--dead-threshold", type=int, default=10_000_000)
    ap.add_argument("--modes", nargs="+", default=["streaming", "resident"])
    ap.add_argument("--log-every", type=int, default=10**9, help="log block every this many steps (default: never, the bare loop)")
    a = ap.parse_args()
    D, Tk = a.d_model, a.tokens
    n_ex = int(a.gb * 1e9 / (4 * D * (Tk + 1)))
    root = tempfile.mkdtemp(prefix="e2e_", dir=a.root)
    try:
        rng = np.random.default_rng(0)
        acts = rng.standard_normal((n_ex, 1, Tk + 1, D), dtype=np.float32)
        d = data.write_shards(root, acts, layers=(23,), cls_token=True, max_tokens_per_shard=(Tk + 1) * 1024)
        del acts
        n_rows = n_ex * Tk
        for mode in a.modes:
            gb = "0" if mode == "streaming" else "1000"
            os.environ["SAEV_AMD_RESIDENT_GB"] = gb
            dcfg = data.ShuffledConfig(shards=d, layer=23, batch_size=a.batch, n_threads=a.threads)
            cfg = T.Config(
                train_data=dcfg, val_data=dcfg, n_train=n_rows * a.epochs, n_val=a.batch,
                sae=nn.SparseAutoencoderConfig(d_model=D, d_sae=D * a.exp, reinit_blend=0.0,
                                               activation=modeling.TopK(top_k=a.top_k)),
                objective=objectives.Matryoshka(n_prefixes=1, dead_threshold_tokens=a.dead_threshold), log_every=a.log_every, track=False,
                runs_root=os.path.join(root, "runs"), device="cuda")
            import saev_amd.utils.scheduling as sched
            t_loop = {}
            orig_iter = sched.BatchLimiter.__iter__

            def timed_iter(self, _orig=orig_iter, _t=t_loop):
                torch.cuda.synchronize()
                _t["t0"] = time.perf_counter()
                yield from _orig(self)

            sched.BatchLimiter.__iter__ = timed_iter
            loaders = []
            orig_make = T._make_loader
            T._make_loader = lambda *aa, **kw: (loaders.append(orig_make(*aa, **kw)), loaders[-1])[1]
            try:
                saes, objs, run, steps = T.train([cfg])
            finally:
                sched.BatchLimiter.__iter__ = orig_iter
                T._make_loader = orig_make
            torch.cuda.synchronize()
            dt = time.perf_counter() - t_loop["t0"]
            print(f"{mode}: {steps} steps in {dt:.2f} s = {steps * a.batch / dt / 1e6:.2f} M activations/s "
                  f"({dt / steps * 1e3:.2f} ms/step)", flush=True)
            st = objs[0].__dict__["_eng_ref"].read_stats()
            print(f"    last step: mse {st.mse:.4f} aux {st.aux:.5f} n_dead {st.n_dead} dense_route {st.dense_route} "
                  f"cand_max {st.cand_max}", flush=True)
            if loaders and loaders[0].reservoir is not None:
                print("    feed phases [s, summed over threads]: "
                      + ", ".join(f"{k} {v:.2f}" for k, v in loaders[0].reservoir.phase_s.items()), flush=True)
            del saes, objs
            torch.cuda.empty_cache()
    finally:
        shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    main()
