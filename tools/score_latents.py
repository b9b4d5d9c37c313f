"""Score every latent of one or more runs on the mimic-pair tasks (saev_amd.mimics.worker_fn).

Reads ``<shards>/image_labels.csv`` (column ``subspecies_view``) and ``<run root>/<run id>/inference/<shards name>/token_acts.npz``;
writes ``cambridge-mimics.npz`` beside the latter -- per (task, latent) ``run_id``, ``task``, ``feature_id``, ``auroc``,
``support_erato``, ``support_melpomene``, ``mean_act_erato``, ``mean_act_melpomene`` -- and ``cambridge-mimics.parquet`` when pyarrow
is installed.

    python tools/score_latents.py --run-root DIR --shards DIR --run-ids ID [ID ...] [--pairs erato:melp ...] [--views dorsal ventral]
                                  [--min-samples 10] [--force-recompute]
"""
import argparse
import pathlib
import sys

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1]))

from saev_amd import mimics  # noqa: E402


def main() -> int:
    d = mimics.Config()
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--run-root", type=pathlib.Path, required=True)
    ap.add_argument("--shards", type=pathlib.Path, required=True)
    ap.add_argument("--run-ids", nargs="+", required=True)
    ap.add_argument("--pairs", nargs="+", default=[f"{e}:{m}" for e, m in d.pair_specs], help="erato_ssp:melp_ssp")
    ap.add_argument("--views", nargs="+", default=d.views)
    ap.add_argument("--min-samples", type=int, default=d.min_samples)
    ap.add_argument("--force-recompute", action="store_true")
    a = ap.parse_args()
    mimics.worker_fn(mimics.Config(run_root_dpath=a.run_root, shards_dpath=a.shards, run_ids=a.run_ids, pair_specs=[mimics.parse_pair_spec(p) for p in a.pairs],
                                   views=a.views, min_samples=a.min_samples, force_recompute=a.force_recompute))
    return 0


if __name__ == "__main__":
    sys.exit(main())
