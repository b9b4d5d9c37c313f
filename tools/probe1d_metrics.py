"""Score the fitted per-latent probes of a run on its test split (saev_amd.probe_metrics.worker_fn).

Reads ``<run>/inference/<train shards>/probe1d_metrics.npz`` (written by tools/probe1d.py), ``<run>/inference/<test shards>/token_acts.npz``
and ``<test shards>/labels.bin``; writes ``<run>/inference/<test shards>/probe1d_metrics__train-<train shards>.npz`` with ap, precision,
recall, f1 (n_classes float32) and top_labels (d_sae, max_k uint8), and ``probe1d_ap_lc__train-<train shards>.npy`` beside it.

    python tools/probe1d_metrics.py --run RUN --train-shards DIR --test-shards DIR [--max-k 256]
"""
import argparse
import pathlib
import sys

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1]))

from saev_amd import probe_metrics  # noqa: E402


def main() -> int:
    d = probe_metrics.Config()
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--run", type=pathlib.Path, required=True)
    ap.add_argument("--train-shards", type=pathlib.Path, required=True)
    ap.add_argument("--test-shards", type=pathlib.Path, required=True)
    ap.add_argument("--max-k", type=int, default=d.max_k)
    ap.add_argument("--debug", action="store_true")
    a = ap.parse_args()
    probe_metrics.worker_fn(probe_metrics.Config(run=a.run, train_shards=a.train_shards, test_shards=a.test_shards, max_k=a.max_k, debug=a.debug))
    return 0


if __name__ == "__main__":
    sys.exit(main())
