"""Latent AUROC (engine.latent_auroc).

  (a) audit     the inputs of tools/bench_latent_ap.py (N = 2^20 rows, S = 16 384 latents, nnz = 2^25, C = 150) with T = 150
                one-vs-rest tasks: the whole call by device events (workspace allocation included), median of ``--iters`` calls, and the
                device time of one call by kernel from torch's profiler -- ``sort``, ``labels``, ``roles`` (the class-major table and
                the task counts) and ``walk``.  ``engine.latent_ap`` runs on the same inputs in the same process as the yardstick;
                ``walk_ratio`` is this entry's walk over that one's ``terms``.
  (b) mimics    16 384 images of 16 tokens pooled to images, S = 16 384, 16 tasks over 32 classes, as ``mimics.score_run`` makes the
                call: ``pool`` (engine.pool_images and the clamp), ``to_csr`` (the pooled matrix's non-zero entries as CSR, in torch)
                and the call with its stages; ``pooled_density`` is the share of non-zero pooled entries.
  baseline      the reference's formulation on the host: ``scipy.stats.rankdata`` over a dense (images x 1 024 latents) chunk and the
                positives' rank sum, for ONE task, measured on that slice and scaled to S latents and 16 tasks.

    python tools/bench_latent_auroc.py [--iters 5] [--out profiles/latent_auroc_bench_line.json]

Writes one JSON line.  No test asserts a time."""
import argparse
import json
import pathlib
import sys
import time

import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1]))
sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))

import bench_latent_ap as base  # noqa: E402
from saev_amd import engine  # noqa: E402

N, S, C = base.N, base.S, base.C
STAGES = {**base.STAGES, "au_roles": "roles", "au_counts": "roles", "au_walk": "walk"}
M_IMAGES, M_TPI, M_CODES, M_CLASSES, M_TASKS, CHUNK = 16384, 16, 32, 32, 16, 1024


def stage_ms(fn):
    saved, base.STAGES = base.STAGES, STAGES
    try:
        return base.stage_ms(fn)
    finally:
        base.STAGES = saved


def mimic_tokens(gen, dev):
    """Token codes of M_IMAGES x M_TPI rows, M_CODES a row, drawn from a skewed latent distribution (an image's tokens share latents)."""
    n = M_IMAGES * M_TPI
    u = torch.rand(n, M_CODES, device=dev, generator=gen)
    idx = (u * u * u * S).long().clamp(max=S - 1).sort(dim=1).values
    dup = torch.zeros_like(idx, dtype=torch.bool)
    dup[:, 1:] = idx[:, 1:] == idx[:, :-1]
    val = torch.ceil(torch.randn(n, M_CODES, device=dev, generator=gen).abs() * 64) / 64 + 1 / 64
    keep = ~dup  # canonical rows: no column twice
    indptr = torch.zeros(n + 1, device=dev, dtype=torch.int64)
    indptr[1:] = keep.sum(dim=1).cumsum(dim=0)
    return indptr, idx[keep].to(torch.int32).contiguous(), val[keep].contiguous()


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", type=pathlib.Path, default=pathlib.Path("profiles/latent_auroc_bench_line.json"))
    ap.add_argument("--skip-baseline", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(0)
    line = {"bench": "latent_auroc", "device": torch.cuda.get_device_name(0)}

    # (a) the audit's shape, one-vs-rest
    indptr, indices, data = base.make_codes(gen, dev)
    labels = torch.randint(0, C, (N,), device=dev, generator=gen, dtype=torch.int32)
    roles = torch.ones(C, C, device=dev, dtype=torch.uint8) + torch.eye(C, device=dev, dtype=torch.uint8)

    def call():
        return engine.latent_auroc(indptr, indices, data, N, S, C, labels=labels, roles=roles)

    def latent():
        return engine.latent_ap(indptr, indices, data, N, S, C, labels=labels)

    res = call()
    mean_auroc = float(res.auroc.mean().item())  # (reads the error word: the inputs are good)
    audit = {"n_rows": N, "n_latents": S, "n_classes": C, "n_tasks": C, "nnz": int(indices.numel()), "whole_call": base.event_ms(call, a.iters),
             "stages_ms": stage_ms(call), "mean_auroc": mean_auroc, "workspace_bytes": int(res._ws.numel())}
    del res
    latent().ap
    audit["latent_ap"] = {"whole_call": base.event_ms(latent, a.iters), "stages_ms": stage_ms(latent)}
    terms = (audit["latent_ap"]["stages_ms"] or {}).get("terms")
    audit["walk_ratio"] = (audit["stages_ms"] or {}).get("walk") / terms if terms and audit["stages_ms"] else None
    line["audit"] = audit
    del indptr, indices, data, labels, roles

    # (b) the mimic shape
    t_indptr, t_indices, t_data = mimic_tokens(gen, dev)
    m_labels = torch.randint(-1, M_CLASSES, (M_IMAGES,), device=dev, generator=gen, dtype=torch.int32)
    m_roles = torch.zeros(M_TASKS, M_CLASSES, device=dev, dtype=torch.uint8)
    for t in range(M_TASKS):
        m_roles[t, 2 * t], m_roles[t, 2 * t + 1] = 1, 2

    def pool():
        return torch.clamp_min(engine.pool_images(t_indptr, t_indices, t_data, M_IMAGES, M_TPI, S, "max").pooled, 0.0)

    def to_csr(pooled):
        at = pooled != 0
        p = torch.zeros(M_IMAGES + 1, device=dev, dtype=torch.int64)
        p[1:] = torch.cumsum(at.sum(dim=1), dim=0)
        return p, at.nonzero()[:, 1].to(torch.int32), pooled[at]

    pooled = pool()
    p_indptr, p_indices, p_data = to_csr(pooled)

    def m_call():
        return engine.latent_auroc(p_indptr, p_indices, p_data, M_IMAGES, S, M_CLASSES, labels=m_labels, roles=m_roles)

    m_res = m_call()
    m_mean = float(m_res.auroc.nanmean().item())
    line["mimics"] = {"n_images": M_IMAGES, "tokens_per_image": M_TPI, "n_latents": S, "n_classes": M_CLASSES, "n_tasks": M_TASKS,
                      "token_nnz": int(t_indices.numel()), "pooled_nnz": int(p_indices.numel()), "pooled_density": p_indices.numel() / (M_IMAGES * S),
                      "pool": base.event_ms(pool, a.iters), "to_csr": base.event_ms(lambda: to_csr(pooled), a.iters),
                      "whole_call": base.event_ms(m_call, a.iters), "stages_ms": stage_ms(m_call), "mean_auroc": m_mean}

    if not a.skip_baseline:
        from scipy.stats import rankdata

        inc = (m_labels.cpu().numpy() >= 0) & (m_labels.cpu().numpy() < 2)  # the images of one task
        chunk = pooled[:, :CHUNK].cpu().numpy()[inc]
        binary = m_labels.cpu().numpy()[inc] == 1
        t0 = time.perf_counter()
        r = rankdata(chunk, axis=0)
        ps = r[binary].sum(axis=0)
        u = (ps - binary.sum() * (binary.sum() + 1) / 2) / (binary.sum() * (~binary).sum())
        chunk_s = time.perf_counter() - t0
        line["host_rankdata_baseline"] = {"images_in_task": int(inc.sum()), "chunk_latents": CHUNK, "chunk_ms": chunk_s * 1e3, "mean_auroc_of_chunk": float(u.mean()),
                                          "scaled_to_all_latents_and_tasks_ms": chunk_s * 1e3 * (S / CHUNK) * M_TASKS,
                                          "note": "measured on one chunk of one task and scaled; the reference's per-image pooling loop is not included"}
    a.out.parent.mkdir(parents=True, exist_ok=True)
    a.out.write_text(json.dumps(line) + "\n")
    print(json.dumps(line))
    return 0


if __name__ == "__main__":
    sys.exit(main())
