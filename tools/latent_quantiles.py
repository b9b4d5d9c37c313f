"""Where every latent's activations lie (saev_amd.activation_stats): computes (or reuses) ``activation_stats.npz``
beside a run's ``token_acts.npz`` and prints, per quantile, the share of latents whose quantile is 0 -- a threshold there
separates nothing -- and the spread of the thresholds over the latents.

    python tools/latent_quantiles.py --run RUN --shards DIR [--q 0.5 0.9 0.95 0.99] [--over rows|entries] [--level token|image]
"""

import argparse
import pathlib
import sys

import numpy as np

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))

from saev_amd import activation_stats  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--run", required=True, type=pathlib.Path)
    ap.add_argument("--shards", required=True, type=pathlib.Path)
    ap.add_argument("--q", type=float, nargs="+", default=[0.5, 0.9, 0.95, 0.99])
    ap.add_argument("--over", choices=("rows", "entries"), default="rows")
    ap.add_argument("--level", choices=("token", "image"), default="token")
    ap.add_argument("--device", default="cuda")
    a = ap.parse_args()
    path = activation_stats.worker_fn(activation_stats.Config(run=a.run, shards=a.shards, q=tuple(a.q), over=a.over, level=a.level, device=a.device))
    with np.load(path) as z:
        count, linear = z["count"], z["linear"]
    S = count.size
    print(f"{path}: {S} latents, level={a.level}, over={a.over}, {int((count == 0).sum())} with an empty multiset")
    for i, q in enumerate(a.q):
        thr = linear[:, i]
        live = thr[~np.isnan(thr)]
        pos = live[live > 0]
        spread = "no positive threshold" if pos.size == 0 else "positive thresholds min {:.4g} / median {:.4g} / max {:.4g}".format(
            pos.min(), np.median(pos), pos.max())
        print(f"q={q:g}: share of latents whose quantile is 0: {(live == 0).sum() / max(S, 1):.4f}; {spread}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
