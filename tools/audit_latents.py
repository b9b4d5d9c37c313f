"""Audit the latents a classifier leans on against the segmentation classes of a run (saev_amd.classification.eval_worker_fn;
DESIGN.md 3.19).

Reads ``<run>/inference/<shards>/token_acts.npz`` (written by the inference pass), ``<shards>/labels.bin`` and the classifier
checkpoints (a JSON header line, then a pickle with key "classifier"), scores EVERY latent against every class on the device (exact
tie-aware average precision) and writes next to ``token_acts.npz``: ``audit_ap_s.npy`` and ``audit_best_class_s.npy`` (filled for the
union of the classifiers' top ``--max-budget`` features, NaN / -1 elsewhere), ``audit_results.json`` (Yield@B and AUC_B per
classifier) and ``audit_ap_sc.npy`` (d_sae x classes float32, every latent).

    python tools/audit_latents.py --run RUN --test-shards DIR --cls-checkpoints A.pkl B.pkl [--tau 0.3] [--max-budget 1000]
                                  [--budgets 3 10 30 100 300 1000] [--ignore-label-ids 0]
"""
import argparse
import pathlib
import sys

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1]))

from saev_amd import classification  # noqa: E402


def main() -> int:
    d = classification.EvalConfig()
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--run", type=pathlib.Path, required=True)
    ap.add_argument("--test-shards", type=pathlib.Path, required=True)
    ap.add_argument("--cls-checkpoints", type=pathlib.Path, nargs="+", required=True)
    ap.add_argument("--tau", type=float, default=d.tau)
    ap.add_argument("--max-budget", type=int, default=d.max_budget)
    ap.add_argument("--budgets", type=int, nargs="+", default=list(d.budgets))
    ap.add_argument("--ignore-label-ids", type=int, nargs="*", default=list(d.ignore_label_ids))
    ap.add_argument("--debug", action="store_true")
    a = ap.parse_args()
    return classification.eval_worker_fn(classification.EvalConfig(
        run=a.run, test_shards=a.test_shards, cls_checkpoints=tuple(a.cls_checkpoints), tau=a.tau, max_budget=a.max_budget,
        budgets=tuple(a.budgets), ignore_label_ids=tuple(a.ignore_label_ids), debug=a.debug))


if __name__ == "__main__":
    sys.exit(main())
