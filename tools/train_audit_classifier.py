"""Train the sparse linear classifier of the concept audit on a run's pooled SAE codes (saev_amd.classification.train_worker_fn;
DESIGN.md 3.20).

Reads ``<run>/inference/<train shards>/token_acts.npz`` and ``<run>/inference/<test shards>/token_acts.npz`` (written by the inference
pass) and ``image_labels.csv`` of both shards directories (a header ``stem,<col>,...``, one row per example), pools the patches of
every image on the device (max or mean), fits the L1-penalised logistic regression there to a KKT residual of ``--kkt-tol`` and writes
``<run>/inference/<test shards>/cls_{task}_{agg}_C{C}.pkl``, the checkpoint ``tools/audit_latents.py --cls-checkpoints`` reads.

    python tools/train_audit_classifier.py --run RUN --train-shards DIR --test-shards DIR --task-name habitat --source-col habitat
                                           [--groups '{"low": ["reef-associated"], "high": ["pelagic"]}'] [--patch-agg max|mean]
                                           [--C 0.01] [--kkt-tol 1e-4]
"""
import argparse
import json
import pathlib
import sys

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1]))

from saev_amd import classification  # noqa: E402


def main() -> int:
    d = classification.SparseLinear()
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--run", type=pathlib.Path, required=True)
    ap.add_argument("--train-shards", type=pathlib.Path, required=True)
    ap.add_argument("--test-shards", type=pathlib.Path, required=True)
    ap.add_argument("--task-name", required=True)
    ap.add_argument("--source-col", required=True)
    ap.add_argument("--groups", type=json.loads, default={}, help="JSON: group name -> list of original labels")
    ap.add_argument("--patch-agg", choices=[a.value for a in classification.PatchAgg], default=classification.PatchAgg.MAX.value)
    ap.add_argument("--C", type=float, default=d.C)
    ap.add_argument("--kkt-tol", type=float, default=d.kkt_tol)
    ap.add_argument("--debug", action="store_true")
    a = ap.parse_args()
    return classification.train_worker_fn(classification.TrainConfig(
        run=a.run, train_shards=a.train_shards, test_shards=a.test_shards,
        task=classification.LabelGrouping(name=a.task_name, source_col=a.source_col, groups=a.groups),
        patch_agg=classification.PatchAgg(a.patch_agg), cls=classification.SparseLinear(C=a.C, kkt_tol=a.kkt_tol), debug=a.debug))


if __name__ == "__main__":
    sys.exit(main())
