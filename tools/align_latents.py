"""Align the latents of two runs (or of one run with itself) by the tokens or images they fire on -> one JSON line.

For every latent of run A its best partners in run B by Jaccard similarity (or containment) of the firing sets
(saev_amd.alignment on engine.coactivation_match: HIP kernels, exact integers, no Sa x Sb matrix), and the same from B to A.
Writes latent_alignment__<run B's id>.npz (latent_alignment__self.npz) into run A's inference directory and prints:

  mutual_fraction      share of A's latents whose best partner has them as its own best partner
  matched_fraction     share of A's latents with any partner at all
  jaccard_quantiles    min, 5 %, 25 %, 50 %, 75 %, 95 %, max of the best partner's Jaccard over the matched latents
  closest, isolated    the ten best- and worst-matched latents of A: [a, b, jaccard, intersection] (b = -1: fires with nothing)

Unlike tools/match_saes.py (cosine of decoder rows) this needs no common activation space: other layers, backbones and widths align.

    python tools/align_latents.py RUN_A [RUN_B] --shards DIR [--level token|image] [--tokens-per-image T] [--top-k K]
                                  [--threshold X] [--measure jaccard|containment] [--top-m M] [--device cuda:0]
"""
import argparse
import json
import pathlib
import sys

import numpy as np

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1]))

from saev_amd import alignment  # noqa: E402


def summary(z: dict, n: int = 10) -> dict:
    """The printed figures from the arrays of an alignment file."""
    partner, jac, inter = z["partner"][:, 0], z["jaccard"][:, 0], z["intersection"][:, 0]
    matched = partner >= 0
    score = np.where(matched, jac, -1.0)  # a latent without a partner is the most isolated
    order = np.argsort(-score, kind="stable")
    rows = lambda sel: [[int(a), int(partner[a]), float(jac[a]) if matched[a] else None, int(inter[a])] for a in sel]  # noqa: E731
    q = [0.0, 0.05, 0.25, 0.5, 0.75, 0.95, 1.0]
    return dict(n_latents_a=int(len(partner)), n_latents_b=int(len(z["support_b"])), mutual_fraction=float(np.mean(z["mutual"])),
                matched_fraction=float(np.mean(matched)),
                jaccard_quantiles=[float(v) for v in np.quantile(jac[matched], q)] if matched.any() else None,
                closest=rows(order[:n]), isolated=rows(order[::-1][:n]))


def main(argv=None) -> dict:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("run_a", type=pathlib.Path)
    ap.add_argument("run_b", type=pathlib.Path, nargs="?")
    ap.add_argument("--shards", required=True)
    ap.add_argument("--level", choices=("token", "image"), default="token")
    ap.add_argument("--tokens-per-image", type=int, default=1)
    ap.add_argument("--top-k", type=int)
    ap.add_argument("--threshold", type=float, default=0.0)
    ap.add_argument("--measure", choices=("jaccard", "containment"), default="jaccard")
    ap.add_argument("--top-m", type=int, default=1)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    cfg = alignment.Config(run_a=args.run_a, run_b=args.run_b, shards=args.shards, level=args.level, tokens_per_image=args.tokens_per_image,
                           top_k=args.top_k, threshold=args.threshold, measure=args.measure, top_m=args.top_m, device=args.device)
    fpath = alignment.worker_fn(cfg)
    with np.load(fpath) as z:
        out = dict(mode="self" if args.run_b is None else "pair", level=args.level, top_k=args.top_k, measure=args.measure, out=str(fpath),
                   **summary({k: z[k] for k in alignment.KEYS}))
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
