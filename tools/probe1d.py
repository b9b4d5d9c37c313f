"""Fit a logistic probe for every (SAE latent, class) pair of a run and score it on a train and a test split
(saev_amd.probe1d.worker_fn).

Reads ``<run>/inference/<shards>/token_acts.npz`` (written by the inference pass) and ``<shards>/labels.bin`` of both splits, and
writes ``<run>/inference/<shards>/probe1d_metrics.npz`` with loss, weights, biases, tp, fp, tn, fn, each (d_sae, n_classes) float32.

    python tools/probe1d.py --run RUN --train-shards DIR --test-shards DIR [--ridge 1e-8] [--max-iter 30] [--class-slab-size 8]
"""
import argparse
import pathlib
import sys

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1]))

from saev_amd import probe1d  # noqa: E402


def main() -> int:
    d = probe1d.Config()
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--run", type=pathlib.Path, required=True)
    ap.add_argument("--train-shards", type=pathlib.Path, required=True)
    ap.add_argument("--test-shards", type=pathlib.Path, required=True)
    ap.add_argument("--ridge", type=float, default=d.ridge)
    ap.add_argument("--class-slab-size", type=int, default=d.class_slab_size)
    ap.add_argument("--row-batch-size", type=int, default=d.row_batch_size, help="accepted and ignored")
    ap.add_argument("--max-iter", type=int, default=d.max_iter)
    ap.add_argument("--device", default=d.device)
    ap.add_argument("--debug", action="store_true")
    a = ap.parse_args()
    return probe1d.worker_fn(probe1d.Config(run=a.run, train_shards=a.train_shards, test_shards=a.test_shards, ridge=a.ridge,
                                            class_slab_size=a.class_slab_size, row_batch_size=a.row_batch_size, max_iter=a.max_iter,
                                            device=a.device, debug=a.debug))


if __name__ == "__main__":
    sys.exit(main())
