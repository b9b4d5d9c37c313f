"""Coactivation matching (engine.coactivation_match) at the shapes the alignment runs, beside plain torch.

  token      N = 2^20 rows, Sa = Sb = 16 384, 32 codes per row (the latent-AP bench's codes, two draws)
  image      16 384 images x 16 tokens of such codes, max-pooled (engine.pool_images): ~500 latents per pooled row
  top20      the token case with every latent's set cut to its 20 highest rows (engine.LatentTopK)
  every_row  the token case with latent 0 of A and of B firing on EVERY row (the heavy route: 128 chunks of 8192 rows)

  kernel     events around ``engine.coactivation_match`` (workspace allocation included, as a caller pays it), top_m = 1, Jaccard;
             ``--reps`` calls per timed window, median of ``--iters`` windows, per call
  torch      the alternative without the kernel, on the same card: the 0/1 dense columns of ``--chunk`` latents of A against the 0/1
             dense B on the vendor GEMM (int8 x int8 -> int32 where torch offers it, else fp32: both exact for counts below 2^24),
             Jaccard in float64 from the counts and ``argmax``; timed for one chunk and scaled to Sa.  Its partners and
             intersections on the chunk must EQUAL the kernel's, or the tool fails.

    python tools/bench_coactivation.py [--iters 5] [--reps 3] [--chunk 256] [--cases token,image,top20,every_row]
                                       [--out profiles/coactivation_bench_line.json]

Writes one JSON line.  No test asserts a time."""
import argparse
import json
import pathlib
import statistics
import sys

import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1]))
sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))

import bench_latent_ap as codes  # noqa: E402
from saev_amd import engine  # noqa: E402

N, CAP, S = codes.N, codes.CAP, codes.S
N_IMG, TPI = 16384, 16


def event_ms(fn, iters, reps):
    fn()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / reps)
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "n": len(ts), "calls_per_window": reps}


def dense_to_csr(dense):
    at = dense != 0
    indptr = torch.zeros(dense.shape[0] + 1, device=dense.device, dtype=torch.int64)
    indptr[1:] = torch.cumsum(at.sum(dim=1), dim=0)
    return indptr, at.nonzero()[:, 1].to(torch.int32), dense[at]


def pooled_csr(csr):
    n_tok = N_IMG * TPI
    indptr, indices, data = csr[0][:n_tok + 1].contiguous(), csr[1][:n_tok * CAP].contiguous(), csr[2][:n_tok * CAP].contiguous()
    return dense_to_csr(torch.clamp_min(engine.pool_images(indptr, indices, data, N_IMG, TPI, S, "max").pooled, 0.0))


def top_sets_csr(csr, k, dev):
    """Every latent's k highest rows, back as a row-major CSR triple on the device."""
    acc = engine.LatentTopK(S, k, dev)
    acc.add_csr(*csr, row_base=0)
    real = torch.arange(k, device=dev)[None, :] < acc.top_cnt[:, None]
    rows, cols = acc.top_row[real].to(torch.int64), torch.arange(S, device=dev)[:, None].expand(S, k)[real]
    order = torch.argsort(rows * S + cols)
    indptr = torch.zeros(N + 1, device=dev, dtype=torch.int64)
    indptr[1:] = torch.cumsum(torch.bincount(rows, minlength=N), dim=0)
    return indptr, cols[order].to(torch.int32), acc.top_val[real][order].contiguous()


def every_row(csr):
    """Latent 0 in every row: the rows' columns ascend and are distinct, so the first may become 0."""
    indices = csr[1].clone()
    indices[::CAP] = 0
    return csr[0], indices, csr[2]


def int8_gemm_works(dev):
    try:
        a, b = torch.ones(256, 4096, device=dev, dtype=torch.int8), torch.ones(4096, 512, device=dev, dtype=torch.int8)
        return bool((torch._int_mm(a, b) == 4096).all().item())
    except Exception:  # noqa: BLE001  (whatever torch raises where the vendor library lacks the routine)
        return False


def dense01(csr, n_rows, lo, hi, dtype):
    """The 0/1 matrix (n_rows, hi - lo) of the entries > 0 in the columns [lo, hi)."""
    indptr, indices, data = csr
    rows = torch.repeat_interleave(torch.arange(n_rows, device=indices.device), indptr[1:] - indptr[:-1])
    keep = (indices >= lo) & (indices < hi) & (data > 0)
    out = torch.zeros(n_rows, hi - lo, device=indices.device, dtype=dtype)
    out[rows[keep], (indices[keep] - lo).long()] = 1
    return out


def torch_match(a01_t, b01, n_a, n_b, use_int8):
    inter = torch._int_mm(a01_t, b01) if use_int8 else (a01_t @ b01)
    inter = inter.to(torch.int64)
    union = n_a[:, None] + n_b[None, :] - inter
    jac = inter.double() / union.clamp_min(1).double()
    best = jac.argmax(dim=1)
    return best, inter.gather(1, best[:, None])[:, 0]


def run_case(name, A, B, n_rows, a, use_int8):
    def call():
        return engine.coactivation_match(A, B, n_rows=n_rows, n_latents_a=S, n_latents_b=S)

    res = call()
    res.check()
    kernel = event_ms(call, a.iters, a.reps)
    dtype = torch.int8 if use_int8 else torch.float32
    b01 = dense01(B, n_rows, 0, S, dtype)
    a01_t = dense01(A, n_rows, 0, a.chunk, dtype).t().contiguous()
    n_a, n_b = res.support_a[:a.chunk].to(torch.int64), res.support_b.to(torch.int64)
    best, inter = torch_match(a01_t, b01, n_a, n_b, use_int8)
    want_index = torch.where(inter > 0, best, -1).to(torch.int32)
    if not (torch.equal(res.index[:a.chunk, 0], want_index) and torch.equal(res.intersection[:a.chunk, 0], inter.to(torch.int32))):
        raise SystemExit(f"{name}: the kernel and the torch alternative disagree on the chunk")
    alt = event_ms(lambda: torch_match(a01_t, b01, n_a, n_b, use_int8), a.iters, 1)
    scaled = alt["median_ms"] * S / a.chunk
    jac = res.jaccard[:, 0]
    return {"n_rows": n_rows, "nnz_a": int(A[1].numel()), "nnz_b": int(B[1].numel()), "largest_support_a": int(res.support_a.max().item()),
            "mutual_fraction": float(res.mutual.double().mean().item()), "mean_best_jaccard": float(jac[~jac.isnan()].mean().item()),
            "workspace_bytes": int(res._ws.numel()), "kernel": kernel, "torch_chunk": alt, "torch_scaled_to_all_latents_ms": scaled,
            "torch_over_kernel": scaled / kernel["median_ms"], "checked_equal_on_chunk": True}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=256)
    ap.add_argument("--cases", default="token,image,top20,every_row")
    ap.add_argument("--out", type=pathlib.Path, default=pathlib.Path("profiles/coactivation_bench_line.json"))
    a = ap.parse_args()
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(0)
    A, B = codes.make_codes(gen, dev), codes.make_codes(gen, dev)
    use_int8 = int8_gemm_works(dev)
    build = {"token": lambda: (A, B, N), "image": lambda: (pooled_csr(A), pooled_csr(B), N_IMG),
             "top20": lambda: (top_sets_csr(A, 20, dev), top_sets_csr(B, 20, dev), N), "every_row": lambda: (every_row(A), every_row(B), N)}
    line = {"bench": "coactivation", "n_latents_a": S, "n_latents_b": S, "measure": "jaccard", "top_m": 1, "device": torch.cuda.get_device_name(0),
            "torch_gemm": "int8 x int8 -> int32" if use_int8 else "fp32", "torch_chunk_latents": a.chunk, "cases": {}}
    for name in a.cases.split(","):
        Ac, Bc, n_rows = build[name]()
        line["cases"][name] = run_case(name, Ac, Bc, n_rows, a, use_int8)
        print(name, json.dumps(line["cases"][name]), flush=True)
        del Ac, Bc
        torch.cuda.empty_cache()
    a.out.parent.mkdir(parents=True, exist_ok=True)
    a.out.write_text(json.dumps(line) + "\n")
    print(json.dumps(line))
    return 0


if __name__ == "__main__":
    sys.exit(main())
