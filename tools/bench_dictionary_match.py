"""Dictionary match (engine.dictionary_match) on one device -> one JSON line, also written to profiles/dictionary_match_bench_line.json:

  <case>.<rows>.hip_ms          median of engine.dictionary_match (its read-back of `info` included), the interquartile range,
                                TFLOP/s counting 2 Sa Sb D flops
  <case>.<rows>.torch_ms        the torch form on the same card: fp32 A_n @ B_n.T in 4 096-row blocks (vendor BLAS) with
                                max(dim=1), the diagonal masked in self mode; median and interquartile range
  <case>.<rows>.candidates      candidates the filter kept, per row, the list capacity, the route, second-pass tiles of all tiles
  <case>.<rows>.coherence_ms    self-mode cases: engine.dictionary_coherence on the same matrix, same card
  <case>.<rows>.kernels_us      per-kernel device time per call, from a kernel trace of `--trace CASE.ROWS` (see below)

cases: configs1.pair (32 768 x 1 024 against a second dictionary of that shape), configs1.self, width.pair (8 192 against 32 768,
D 1 024) and configs3.self (81 920 x 1 280).  rows: "random" (Gaussian rows) and "trained" (datapoint initialisation from low-rank
data, as tools/bench_coherence.py).  Each call is timed on its own with HIP events after a warm-up.

    python tools/bench_dictionary_match.py [--reps N] [--cases a,b] [--kernel-db CASE.ROWS=run_results.db ...]
    rocprofv3 --kernel-trace -d DIR -o run -- python tools/bench_dictionary_match.py --trace configs1.self.random
"""
import argparse
import json
import pathlib
import re
import sqlite3
import statistics
import sys

import torch

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from saev_amd import _lib  # noqa: E402
from saev_amd.engine import dictionary_coherence, dictionary_match  # noqa: E402

CASES = {"configs1.pair": (32768, 32768, 1024), "configs1.self": (32768, None, 1024), "width.pair": (8192, 32768, 1024),
         "configs3.self": (81920, None, 1280)}
KINDS = ("trained", "random")


def rows(kind: str, S: int, D: int, dev, seed: int) -> torch.Tensor:
    g = torch.Generator(device=dev).manual_seed(S + D + seed)
    if kind == "random":
        return torch.randn(S, D, device=dev, generator=g)
    U = torch.randn(64, D, device=dev, generator=g)
    z = torch.randn(S, 64, device=dev, generator=g)
    return z @ U + 0.3 * torch.randn(S, D, device=dev, generator=g)


def torch_match(A: torch.Tensor, B: torch.Tensor | None, block: int = 4096):
    """What a user writes today: a torch matmul in row blocks."""
    An = A / A.norm(dim=1, keepdim=True)
    Bn = An if B is None else B / B.norm(dim=1, keepdim=True)
    vals, idx = [], []
    for lo in range(0, An.shape[0], block):
        g = An[lo : lo + block] @ Bn.T
        if B is None:
            g.diagonal(lo).fill_(float("-inf"))
        m = g.max(dim=1)
        vals.append(m.values)
        idx.append(m.indices)
    return torch.cat(vals), torch.cat(idx)


def timed(fn, n: int) -> dict:
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


def kernel_table(db_path: str, calls: int) -> dict:
    """Microseconds per call of every dm_* / coh_* kernel in a rocprofv3 kernel-trace database of `--trace` (its last `calls` calls)."""
    db = sqlite3.connect(db_path)
    tables = [r[0] for r in db.execute("select name from sqlite_master where type='table'")]
    suffix = next(t for t in tables if t.startswith("rocpd_kernel_dispatch"))[len("rocpd_kernel_dispatch"):]
    kd, ks = "rocpd_kernel_dispatch" + suffix, "rocpd_info_kernel_symbol" + suffix
    scols = [r[1] for r in db.execute(f"pragma table_info({ks})")]
    name_col = "kernel_name" if "kernel_name" in scols else "display_name"
    per = {}
    for name, dur in db.execute(f"select s.{name_col}, d.end - d.start from {kd} d join {ks} s on d.kernel_id = s.id order by d.start"):
        m = re.search(r"((?:dm|coh)_\w+?_kernel)(?:ILi(\d)E)?", name)
        if m:
            per.setdefault(m.group(1) + (f"<{m.group(2)}>" if m.group(2) else ""), []).append(dur)
    out = {}
    for name, durs in per.items():
        per_call = max(1, round(len(durs) / (calls + 1)))  # (--trace makes calls + 1 calls)
        tail = durs[-calls * per_call:]
        out[name] = round(sum(tail) / calls / 1e3, 1)
    return out


def inputs(case: str, kind: str, dev):
    Sa, Sb, D = CASES[case]
    return rows(kind, Sa, D, dev, 0), (None if Sb is None else rows(kind, Sb, D, dev, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--trace", help="CASE.ROWS: run that call reps + 1 times and nothing else (for a kernel trace)")
    ap.add_argument("--kernel-db", action="append", default=[], help="CASE.ROWS=path of the rocpd database of such a trace")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "dictionary_match_bench_line.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    if args.trace:
        case, kind = args.trace.rsplit(".", 1)
        A, B = inputs(case, kind, dev)
        for _ in range(args.reps + 1):
            dictionary_match(A, B)
        torch.cuda.synchronize()
        return
    lib = _lib.load()
    dbs = dict(s.split("=", 1) for s in args.kernel_db)
    out = {"reps": args.reps}
    for case in args.cases.split(","):
        Sa, Sb, D = CASES[case]
        for kind in KINDS:
            A, B = inputs(case, kind, dev)
            sb = Sa if Sb is None else Sb
            r = dictionary_match(A, B)
            rec = {"shape": [Sa, sb, D], "self": Sb is None, "mmcs": r.mmcs, "route": r.route, "overflow": r.overflow,
                   "candidates": r.candidates, "candidates_per_row": round(r.candidates / Sa, 3), "capacity": r.capacity,
                   "tiles_refiltered": r.tiles_refiltered, "tiles": ((Sa + 127) // 128) * ((sb + 127) // 128),
                   "workspace_bytes": int(lib.saev_dictionary_match_workspace_bytes(Sa, sb, D))}
            t = timed(lambda: dictionary_match(A, B), args.reps)
            flop = 2 * Sa * sb * D
            rec.update(hip_ms=t["median"], hip_iqr_ms=t["iqr"], hip_tflops=round(flop / t["median"] / 1e9, 1))
            tv, ti = torch_match(A, B)
            rec["torch_max_abs_diff"] = (tv - r.values).abs().max().item()
            rec["torch_index_agreement"] = (ti.int() == r.indices).double().mean().item()
            del tv, ti
            tt = timed(lambda: torch_match(A, B), max(3, args.reps // 3))
            rec.update(torch_ms=tt["median"], torch_iqr_ms=tt["iqr"], speedup=round(tt["median"] / t["median"], 2))
            if Sb is None:
                tc = timed(lambda: dictionary_coherence(A), args.reps)
                rec.update(coherence_ms=tc["median"], coherence_iqr_ms=tc["iqr"], ratio_to_coherence=round(t["median"] / tc["median"], 2))
            rec["exact_route_ms"] = timed(lambda: dictionary_match(A, B, route="exact"), 2)["median"]
            key = f"{case}.{kind}"
            if key in dbs:
                rec["kernels_us"] = kernel_table(dbs[key], args.reps)
            out[key] = rec
            del A, B
            torch.cuda.empty_cache()
    line = json.dumps(out)
    pathlib.Path(args.out).write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
