"""Per-latent thresholds chosen per task: the best operating point of every latent of a run (saev_amd.operating).

Reads ``<run root>/<run id>/inference/<shards>/token_acts.npz`` (written by the inference pass) and the labels of the shards --
``image_labels.csv`` for ``--level image`` (mimic-pair tasks on max-pooled codes), ``labels.bin`` for ``--level token`` (one
segmentation class against the rest) --, writes ``latent_operating.npz`` beside ``token_acts.npz`` unless it is there already, and
prints per task the quantiles of the best F1 and of Youden's J over the latents, the ten best latents by each with their threshold,
precision and recall (true and false positive rate for J), and the share of latents whose best point is "predict nothing".  With
``--latent`` it prints that latent's row in every task instead.

    python tools/latent_thresholds.py --run RUN --shards DIR [--level token|image] [--task NAME] [--latent J] [--force]
                                      [--pairs erato:melpomene ...] [--views dorsal ventral] [--min-samples 10] [--ignore-label-ids 0]
"""
import argparse
import pathlib
import sys

import numpy as np

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1]))

from saev_amd import operating  # noqa: E402

QUANTILES = (0.0, 0.1, 0.25, 0.5, 0.75, 0.9, 1.0)


def _row(card, at):
    return {k: (v[at].item() if hasattr(v[at], "item") else v[at]) for k, v in card.items()}


def main(argv=None) -> dict:
    d = operating.Config()
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--run", type=pathlib.Path, required=True, help="<run root>/<run id>")
    ap.add_argument("--shards", type=pathlib.Path, required=True)
    ap.add_argument("--level", choices=operating.LEVELS, default="token")
    ap.add_argument("--task", default=None)
    ap.add_argument("--latent", type=int, default=None)
    ap.add_argument("--force", action="store_true")
    ap.add_argument("--pairs", nargs="+", default=[f"{e}:{m}" for e, m in d.pair_specs])
    ap.add_argument("--views", nargs="+", default=list(d.views))
    ap.add_argument("--min-samples", type=int, default=d.min_samples)
    ap.add_argument("--ignore-label-ids", type=int, nargs="*", default=list(d.ignore_label_ids))
    a = ap.parse_args(argv)
    run = a.run.resolve()
    cfg = operating.Config(run_root_dpath=run.parent, shards_dpath=a.shards, run_ids=[run.name], level=a.level,
                           pair_specs=[operating.mimics.parse_pair_spec(p) for p in a.pairs], views=a.views, min_samples=a.min_samples,
                           ignore_label_ids=tuple(a.ignore_label_ids), force_recompute=a.force)
    z = operating.score_run(run.name, cfg)
    if z is None:
        raise SystemExit(f"no token_acts.npz under '{run / 'inference' / a.shards.name}'")
    card = operating.scorecard(z)
    names = z["task"].tolist()
    tasks = names if a.task is None else [a.task]
    if a.task is not None and a.task not in names:
        raise SystemExit(f"task '{a.task}' is not scored (the file has {names})")
    s = z["f1"].shape[1]
    out = {"level": str(z["level"]), "n_latents": s, "tasks": {}}
    if a.latent is not None:
        if not 0 <= a.latent < s:
            raise SystemExit(f"--latent must lie in [0, {s})")
        out["latent"] = a.latent
        print(f"latent {a.latent} ({out['level']} level)")
        print(f"{'task':<40} {'auroc':>7} {'f1':>7} {'theta':>11} {'prec':>6} {'rec':>6} {'J':>7} {'theta':>11} {'tpr':>6} {'fpr':>6}")
        for name in tasks:
            r = _row(card, names.index(name) * s + a.latent)
            out["tasks"][name] = r
            print(f"{name:<40} {r['auroc']:7.4f} {r['f1']:7.4f} {r['f1_thr']:11.5g} {r['precision']:6.3f} {r['recall']:6.3f} {r['youden']:7.4f} "
                  f"{r['j_thr']:11.5g} {r['tpr']:6.3f} {r['fpr']:6.3f}")
        return out
    for name in tasks:
        t = names.index(name)
        at = slice(t * s, (t + 1) * s)
        f1, j = card["f1"][at], card["youden"][at]
        nothing_f1 = float(((z["f1_tp"][t] + z["f1_fp"][t]) == 0).mean())
        nothing_j = float(((z["j_tp"][t] + z["j_fp"][t]) == 0).mean())
        rec = {"n_pos": int(z["n_pos"][t]), "n_neg": int(z["n_neg"][t]), "predict_nothing_f1": nothing_f1, "predict_nothing_j": nothing_j,
               "f1_quantiles": [], "j_quantiles": [], "best_by_f1": [], "best_by_j": []}
        print(f"task {name}: {rec['n_pos']} positives, {rec['n_neg']} negatives; best point is 'predict nothing' for {100 * nothing_f1:.1f} % of the latents "
              f"by F1, {100 * nothing_j:.1f} % by J")
        for key, v in (("f1", f1), ("j", j)):
            if not np.isnan(v).all():
                rec[f"{key}_quantiles"] = np.nanquantile(v, QUANTILES).tolist()
            print(f"  best {key.upper():<2} quantiles {QUANTILES}: " + " ".join(f"{q:.4f}" for q in rec[f"{key}_quantiles"]))
        for key, v, a_name, b_name in (("f1", f1, "precision", "recall"), ("j", j, "tpr", "fpr")):
            order = np.argsort(-np.nan_to_num(v, nan=-np.inf), kind="stable")[:10]
            thr = card[f"{key}_thr"][at]
            print(f"  ten best by {key.upper()}: latent, score, theta, {a_name}, {b_name}")
            for i in order.tolist():
                rec[f"best_by_{key}"].append([i, float(v[i]), float(thr[i]), float(card[a_name][at][i]), float(card[b_name][at][i])])
                print(f"    {i:>7} {v[i]:7.4f} {thr[i]:11.5g} {card[a_name][at][i]:6.3f} {card[b_name][at][i]:6.3f}")
        out["tasks"][name] = rec
    return out


if __name__ == "__main__":
    main()
