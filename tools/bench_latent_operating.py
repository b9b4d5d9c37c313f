"""Latent operating points (engine.latent_operating), on the inputs of tools/bench_latent_auroc.py.

  (a) audit     N = 2^20 rows, S = 16 384 latents, nnz = 2^25, C = 150, T = 150 one-vs-rest tasks.
  (b) mimics    16 384 images of 16 tokens pooled to images, S = 16 384, 16 tasks over 32 classes.

At either shape: the whole call by device events (workspace allocation included), median of ``--iters`` calls, FRESH and with
``reuse=`` of a ``latent_auroc`` result; the device time of one call by kernel from torch's profiler (``sort``, ``labels``, ``roles``,
``walk``); ``engine.latent_auroc`` in the same process on the same inputs as the yardstick, and ``walk_ratio`` = this entry's walk
over that one's.  Then two baselines:

  dense torch   the dense formulation on the device: a chunk of latents densified, per latent ``sort`` descending, the row roles
                gathered, ``cumsum`` to TP and FP at every rank, the candidates (the last rank of every run of equal values) scored
                -- F1 in float64, which orders ratios of integers below 2^22 exactly, J2 in int64 -- and ``argmax`` (the first index
                that attains the maximum: the tie rule).  ASSERTED EQUAL to the entry on the chunk, timed on it and scaled to S
                latents.  256 latents at the mimic shape, ``--dense-chunk`` (32) at the audit's.
  roc_curve     ``sklearn.metrics.roc_curve(drop_intermediate=False)`` on the host for a few pairs of the mimic shape, per pair.

    python tools/bench_latent_operating.py [--iters 5] [--out profiles/latent_operating_bench_line.json]

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
import bench_latent_auroc as au  # noqa: E402
from saev_amd import engine  # noqa: E402

N, S, C = base.N, base.S, base.C
STAGES = {**au.STAGES, "op_walk": "walk"}
DENSE_KEYS = ("f1_tp", "f1_fp", "f1_thr", "j2", "j_tp", "j_fp", "j_thr")


def stage_ms(fn):
    saved, base.STAGES = base.STAGES, STAGES
    try:
        return base.stage_ms(fn)
    finally:
        base.STAGES = saved


def dense_points(indptr, indices, data, n_rows, lo, hi, labels, roles):
    """The dense formulation for the latents [lo, hi): (f1_tp, f1_fp, f1_thr, j2, j_tp, j_fp, j_thr), each (hi - lo, T)."""
    dev = data.device
    n_tasks = roles.shape[0]
    rows = torch.repeat_interleave(torch.arange(n_rows, device=dev), indptr[1:] - indptr[:-1])
    keep = (indices >= lo) & (indices < hi)
    dense = torch.zeros(n_rows, hi - lo, device=dev)
    dense[rows[keep], (indices[keep] - lo).long()] = data[keep]
    table = torch.cat([torch.zeros(n_tasks, 1, device=dev, dtype=torch.uint8), roles], dim=1)  # column 0: class -1
    row_role = table[:, (labels + 1).long()].T.contiguous()  # (N, T)
    is_pos, is_neg = row_role == 2, row_role == 1
    n_pos, n_neg = is_pos.sum(dim=0), is_neg.sum(dim=0)
    inf = torch.tensor(float("inf"), device=dev)
    outs = {k: [] for k in DENSE_KEYS}
    for b in range(hi - lo):
        v, order = torch.sort(dense[:, b] + 0.0, descending=True, stable=True)
        tp, fp = is_pos[order].cumsum(dim=0), is_neg[order].cumsum(dim=0)  # (N, T) int64
        last = torch.ones(n_rows, device=dev, dtype=torch.bool)
        last[:-1] = v[1:] != v[:-1]
        f1 = torch.where(last[:, None], 2.0 * tp.double() / (tp + fp + n_pos[None, :]).clamp_min(1).double(), -1.0)
        j2 = torch.where(last[:, None], tp * n_neg[None, :] - fp * n_pos[None, :], -1)
        for name, score in (("f1", f1), ("j", j2)):
            at = score.argmax(dim=0)[None, :]
            won = score.gather(0, at)[0] > 0  # (else "predict nothing", which scores 0 and comes first)
            outs[f"{name}_tp"].append(torch.where(won, tp.gather(0, at)[0], 0))
            outs[f"{name}_fp"].append(torch.where(won, fp.gather(0, at)[0], 0))
            outs[f"{name}_thr"].append(torch.where(won, v[at[0]], inf))
        outs["j2"].append(outs["j_tp"][-1] * n_neg - outs["j_fp"][-1] * n_pos)
    return {k: torch.stack(v) for k, v in outs.items()}


def against_dense(res, indptr, indices, data, n_rows, chunk, labels, roles, iters):
    def run():
        return dense_points(indptr, indices, data, n_rows, 0, chunk, labels, roles)

    got = run()
    differ = [key for key in DENSE_KEYS if not torch.equal(got[key].to(getattr(res, key).dtype), getattr(res, key)[:chunk])]
    if differ:  # (the line is still written: main() ends with a non-zero status)
        return {"chunk_latents": chunk, "equal_on_the_chunk": False, "differs_in": differ}
    t = base.event_ms(run, max(1, min(iters, 3)))
    return {"chunk_latents": chunk, "chunk": t, "scaled_to_all_latents_ms": t["median_ms"] * S / chunk, "equal_on_the_chunk": True}


def measure(indptr, indices, data, n_rows, n_classes, labels, roles, iters):
    kw = dict(labels=labels, roles=roles)

    def ranked():
        return engine.latent_auroc(indptr, indices, data, n_rows, S, n_classes, **kw)

    def fresh():
        return engine.latent_operating(indptr, indices, data, n_rows, S, n_classes, **kw)

    prior = ranked()
    prior.check()

    def reused():
        return engine.latent_operating(indptr, indices, data, n_rows, S, n_classes, **kw, reuse=prior)

    res = fresh()
    res.check()
    again = reused()
    assert all(torch.equal(getattr(res, k).view(torch.int64 if getattr(res, k).element_size() == 8 else torch.int32),
                           getattr(again, k).view(torch.int64 if getattr(res, k).element_size() == 8 else torch.int32)) for k in res.PAIRS)
    nothing = ((res.f1_tp + res.f1_fp) == 0).double().mean().item()
    out = {"fresh": {"whole_call": base.event_ms(fresh, iters), "stages_ms": stage_ms(fresh)},
           "reuse": {"whole_call": base.event_ms(reused, iters), "stages_ms": stage_ms(reused)},
           "latent_auroc": {"whole_call": base.event_ms(ranked, iters), "stages_ms": stage_ms(ranked)},
           "mean_best_f1": float(res.f1.nanmean().item()), "mean_best_j": float(res.youden.nanmean().item()), "predict_nothing_share_f1": nothing,
           "workspace_bytes": int(res._ws.numel())}
    walk, yard = (out["fresh"]["stages_ms"] or {}).get("walk"), (out["latent_auroc"]["stages_ms"] or {}).get("walk")
    out["walk_ratio"] = walk / yard if walk and yard else None
    return out, res


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--dense-chunk", type=int, default=32)
    ap.add_argument("--out", type=pathlib.Path, default=pathlib.Path("profiles/latent_operating_bench_line.json"))
    ap.add_argument("--skip-baselines", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(0)
    line = {"bench": "latent_operating", "device": torch.cuda.get_device_name(0)}

    # (a) the audit's shape, one-vs-rest
    indptr, indices, data = base.make_codes(gen, dev)
    labels = torch.randint(0, C, (N,), device=dev, generator=gen, dtype=torch.int32)
    roles = torch.ones(C, C, device=dev, dtype=torch.uint8) + torch.eye(C, device=dev, dtype=torch.uint8)
    audit, res = measure(indptr, indices, data, N, C, labels, roles, a.iters)
    audit.update(n_rows=N, n_latents=S, n_classes=C, n_tasks=C, nnz=int(indices.numel()))
    if not a.skip_baselines:
        audit["dense_torch"] = against_dense(res, indptr, indices, data, N, a.dense_chunk, labels, roles, a.iters)
    line["audit"] = audit
    del indptr, indices, data, labels, roles, res

    # (b) the mimic shape
    t_indptr, t_indices, t_data = au.mimic_tokens(gen, dev)
    m_labels = torch.randint(-1, au.M_CLASSES, (au.M_IMAGES,), device=dev, generator=gen, dtype=torch.int32)
    m_roles = torch.zeros(au.M_TASKS, au.M_CLASSES, device=dev, dtype=torch.uint8)
    for t in range(au.M_TASKS):
        m_roles[t, 2 * t], m_roles[t, 2 * t + 1] = 1, 2
    pooled = torch.clamp_min(engine.pool_images(t_indptr, t_indices, t_data, au.M_IMAGES, au.M_TPI, S, "max").pooled, 0.0)
    at = pooled != 0
    p_indptr = torch.zeros(au.M_IMAGES + 1, device=dev, dtype=torch.int64)
    p_indptr[1:] = torch.cumsum(at.sum(dim=1), dim=0)
    p_indices, p_data = at.nonzero()[:, 1].to(torch.int32), pooled[at]
    mimic, m_res = measure(p_indptr, p_indices, p_data, au.M_IMAGES, au.M_CLASSES, m_labels, m_roles, a.iters)
    mimic.update(n_images=au.M_IMAGES, n_latents=S, n_classes=au.M_CLASSES, n_tasks=au.M_TASKS, pooled_nnz=int(p_indices.numel()))
    if not a.skip_baselines:
        mimic["dense_torch"] = against_dense(m_res, p_indptr, p_indices, p_data, au.M_IMAGES, 256, m_labels, m_roles, a.iters)
        from sklearn.metrics import roc_curve

        lab = m_labels.cpu().numpy()
        times, agree = [], 0
        for j, t in ((0, 0), (1, 3), (17, 7), (255, 15)):
            inc = (lab == 2 * t) | (lab == 2 * t + 1)
            y, col = lab[inc] == 2 * t + 1, pooled[:, j].cpu().numpy()[inc]
            t0 = time.perf_counter()
            fpr, tpr, thr = roc_curve(y, col, drop_intermediate=False)
            tp, fp = tpr * y.sum(), fpr * (~y).sum()
            best = int((2 * tp / (tp + fp + y.sum())).argmax())
            times.append((time.perf_counter() - t0) * 1e3)
            agree += int(float(thr[best]) == float(m_res.f1_thr[j, t].item()) or (tp[best] == 0 and int(m_res.f1_tp[j, t].item()) == 0))
        mimic["host_roc_curve"] = {"pairs": len(times), "per_pair_ms": sum(times) / len(times), "rows_per_pair": int(inc.sum()),
                                   "scaled_to_all_pairs_ms": sum(times) / len(times) * S * au.M_TASKS, "thresholds_equal_to_the_entrys": agree,
                                   "note": "float F1 on the host; scaled from a few pairs"}
    line["mimics"] = mimic
    a.out.parent.mkdir(parents=True, exist_ok=True)
    a.out.write_text(json.dumps(line) + "\n")
    print(json.dumps(line))
    assert all(line[k].get("dense_torch", {}).get("equal_on_the_chunk", True) for k in ("audit", "mimics")), "the dense formulation differs from the entry"
    return 0


if __name__ == "__main__":
    sys.exit(main())
