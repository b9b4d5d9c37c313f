"""Where the latents of a run fire on the patch grid -> a short report and one JSON line.

Scores every latent per group of images (saev_amd.spatial on engine.latent_spatial: HIP kernels, exact integers, fixed-order float64
sums), writes latent_spatial.npz beside the run's token_acts.npz and prints:

  clustered_fraction              share of the latents with clustering > 2 in some group (twice the firing 4-neighbour pairs that
                                  patches thrown at random would make)
  position_consistency_quantiles  min, 5 %, 25 %, 50 %, 75 %, 95 %, max of each latent's best position consistency
  most_coherent, most_scattered   the ten latents at either end: [latent, group, position_consistency, clustering, firing images]

With --latent J: J's rate map per group as a text grid (tenths of the group's images firing there; '.' = none) and, with --pair A B,
the difference of its mean maps on groups A and B.

    python tools/latent_spatial.py --run RUN --shards DIR [--group-col COL] [--grid H W] [--threshold X] [--min-images N]
                                   [--latent J [--pair A B]]
"""
import argparse
import json
import pathlib
import sys

import numpy as np

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1]))

from saev_amd import spatial  # noqa: E402


def summary(z: dict, min_images: int, n: int = 10) -> dict:
    """The printed figures from the arrays of a latent_spatial.npz."""
    enough = z["n_images_fire"] >= min_images
    pc = np.where(enough, z["position_consistency"], np.nan)
    cl = np.where(enough, z["clustering"], np.nan)
    scored = ~np.isnan(pc).all(axis=1)
    best_g = np.zeros(len(pc), dtype=np.int64)
    best_g[scored] = np.nanargmax(pc[scored], axis=1)
    best = np.where(scored, pc[np.arange(len(pc)), best_g], np.nan)
    with np.errstate(invalid="ignore"):
        clustered = (cl > 2).any(axis=1)
    ids = np.flatnonzero(scored)
    order = ids[np.argsort(-best[ids], kind="stable")]
    none = lambda v: None if np.isnan(v) else float(v)  # noqa: E731
    rows = lambda sel: [[int(j), int(best_g[j]), float(best[j]), none(cl[j, best_g[j]]), int(z["n_images_fire"][j, best_g[j]])] for j in sel]  # noqa: E731
    q = [0.0, 0.05, 0.25, 0.5, 0.75, 0.95, 1.0]
    return dict(n_latents=int(len(pc)), n_scored=int(scored.sum()), groups=[str(g) for g in z["group_names"]],
                clustered_fraction=float(clustered.mean()),
                position_consistency_quantiles=[float(v) for v in np.quantile(best[ids], q)] if len(ids) else None,
                most_coherent=rows(order[:n]), most_scattered=rows(order[::-1][:n]))


def text_grid(rate: np.ndarray) -> str:
    """A rate map in [0, 1] as one character per cell: '.' for 0, else the tenths (9 for 0.9 and above, 0 for below 0.1)."""
    return "\n".join(" ".join("." if v == 0 or np.isnan(v) else str(min(int(v * 10), 9)) for v in row) for row in rate)


def main(argv=None) -> dict:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--run", type=pathlib.Path, required=True)
    ap.add_argument("--shards", type=pathlib.Path, required=True)
    ap.add_argument("--group-col")
    ap.add_argument("--grid", type=int, nargs=2, metavar=("H", "W"))
    ap.add_argument("--threshold", type=float, default=0.0)
    ap.add_argument("--min-images", type=int, default=8)
    ap.add_argument("--latent", type=int)
    ap.add_argument("--pair", nargs=2, metavar=("A", "B"))
    args = ap.parse_args(argv)
    if args.pair and args.latent is None:
        ap.error("--pair goes with --latent")
    cfg = spatial.Config(run=args.run, shards=args.shards, grid=tuple(args.grid) if args.grid else None, group_col=args.group_col,
                         threshold=args.threshold, min_images=args.min_images, map_latents=256 if args.latent is None else (args.latent,))
    fpath = spatial.worker_fn(cfg)
    with np.load(fpath) as z:
        z = {k: z[k] for k in spatial.KEYS}
    out = dict(out=str(fpath), grid=[int(g) for g in z["grid"]], **summary(z, args.min_images))
    print(f"{out['n_latents']} latents, {len(out['groups'])} groups, grid {out['grid'][0]} x {out['grid'][1]}")
    print(f"clustering > 2 in some group: {100.0 * out['clustered_fraction']:.1f}% of the latents")
    print(f"position consistency (min, 5%, 25%, 50%, 75%, 95%, max): {out['position_consistency_quantiles']}")
    print(f"most coherent  [latent, group, consistency, clustering, images]: {out['most_coherent']}")
    print(f"most scattered [latent, group, consistency, clustering, images]: {out['most_scattered']}")
    if args.latent is not None:
        names = out["groups"]
        rate = spatial.rate_map(z["count_map"], z["n_group_images"])[0]
        for g, name in enumerate(names):
            print(f"latent {args.latent}, rate map on '{name}' ({int(z['n_group_images'][g])} images, tenths):\n{text_grid(rate[g])}")
        out.update(latent=args.latent, rate_map=rate.tolist())
        if args.pair:
            for name in args.pair:
                if name not in names:
                    ap.error(f"group '{name}' is not among {names}")
            a, b = (names.index(name) for name in args.pair)
            diff = spatial.difference_map(z, 0, a, b)
            print(f"latent {args.latent}, mean map on '{args.pair[0]}' minus '{args.pair[1]}':")
            print("\n".join(" ".join(f"{v:+8.3f}" for v in row) for row in diff))
            out.update(pair=list(args.pair), difference_map=diff.tolist())
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
