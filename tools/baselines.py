"""Train the k-means baseline on a shard cache, or run it over one (saev_amd.baselines).

``train`` fits ``k`` centres on ``--n-train`` shuffled rows, evaluates on the validation cache and writes
``<runs-root>/<run id>/checkpoint/{baseline.pt,config.json}``; ``inference`` writes ``<run>/inference/<shards>/`` with
``token_acts.npz`` (one entry per token: column = nearest centre, value = 1 / (1 + distance)), ``mean_values.pt``, ``sparsity.pt``,
``distributions.pt`` and ``metrics.json``.

    python tools/baselines.py train --train-shards DIR --val-shards DIR --layer L --runs-root .../saev/runs [--k 16384] [--n-train N]
    python tools/baselines.py inference --run RUN --shards DIR --layer L [--no-save] [--force]
"""
import argparse
import logging
import pathlib
import sys

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1]))

from saev_amd import baselines, data  # noqa: E402


def main() -> int:
    t, i = baselines.TrainConfig(), baselines.InferenceConfig()
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    tr = sub.add_parser("train")
    tr.add_argument("--method", default=t.method, help="'kmeans'; 'pca' and 'semi-nmf' are not built")
    tr.add_argument("--train-shards", type=pathlib.Path, required=True)
    tr.add_argument("--val-shards", type=pathlib.Path, required=True)
    tr.add_argument("--layer", type=int, required=True)
    tr.add_argument("--batch-size", type=int, default=t.train_data.batch_size)
    tr.add_argument("--runs-root", type=pathlib.Path, required=True)
    tr.add_argument("--k", type=int, default=t.k)
    tr.add_argument("--collapse-tol", type=float, default=t.collapse_tol)
    tr.add_argument("--n-train", type=int, default=t.n_train)
    tr.add_argument("--n-val", type=int, default=t.n_val)
    tr.add_argument("--seed", type=int, default=t.seed)
    tr.add_argument("--log-every", type=int, default=t.log_every)
    tr.add_argument("--device", default=t.device)
    inf = sub.add_parser("inference")
    inf.add_argument("--run", type=pathlib.Path, required=True)
    inf.add_argument("--shards", type=pathlib.Path, required=True)
    inf.add_argument("--layer", type=int, required=True)
    inf.add_argument("--batch-size", type=int, default=i.data.batch_size)
    inf.add_argument("--n-dists", type=int, default=i.n_dists)
    inf.add_argument("--no-save", action="store_true")
    inf.add_argument("--force", action="store_true")
    inf.add_argument("--device", default=i.device)
    a = ap.parse_args()
    logging.basicConfig(level=logging.INFO, format="[%(asctime)s] [%(levelname)s] [%(name)s] %(message)s")
    if a.cmd == "train":
        mk = lambda shards: data.ShuffledConfig(shards=shards, layer=a.layer, batch_size=a.batch_size)  # noqa: E731
        run = baselines.train_worker_fn(baselines.TrainConfig(
            method=a.method, train_data=mk(a.train_shards), val_data=mk(a.val_shards), n_train=a.n_train, n_val=a.n_val, k=a.k,
            collapse_tol=a.collapse_tol, device=a.device, seed=a.seed, runs_root=a.runs_root, log_every=a.log_every))
        print(run.run_dir)
    else:
        baselines.inference_worker_fn(baselines.InferenceConfig(
            run=a.run, data=data.OrderedConfig(shards=a.shards, layer=a.layer, batch_size=a.batch_size), device=a.device,
            n_dists=a.n_dists, save=not a.no_save, force=a.force))
    return 0


if __name__ == "__main__":
    sys.exit(main())
