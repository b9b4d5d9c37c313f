"""Which images to look at for the latents of a run -> a short report and one JSON line.

Lists, per latent and group of images, the k strongest firing images, the k weakest firing images and the first k silent ones
(saev_amd.exemplars on engine.latent_exemplars: HIP kernels, pooled on the fly, exact and deterministic), writes
latent_exemplars.npz beside the run's token_acts.npz and prints:

  short_fraction   share of the (latent, group) pairs with fewer than k firing images (their lists are not full)

With --latent J: J's strips per group as image:value@patch (strongest first, then weakest first), its first silent images, and its
top image's patch vector as a text grid (tenths of the image's maximum; '.' = nothing stored).  With --pos A --neg B also J's
counter-examples as a detector of A against B: B's images that fire hardest, A's images that stay silent.

    python tools/latent_exemplars.py --run RUN --shards DIR [--group-col COL] [-k 8] [--threshold X] [--min-images N]
                                     [--latent J [--pos A --neg B]]
"""
import argparse
import json
import math
import pathlib
import sys

import numpy as np

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1]))

from saev_amd import exemplars  # noqa: E402


def strip_text(records: list[dict]) -> str:
    return " ".join(f"{r['image']}:{r['value']:.4g}@{r['patch']}" for r in records) or "-"


def text_grid(vec: np.ndarray) -> str:
    """A patch vector as one character per patch, rows of the square grid's width (one row when the patches are no square): '.' for a
    patch that stores nothing, else the tenths of the vector's maximum (9 for 0.9 and above)."""
    finite = vec[np.isfinite(vec)]
    top = float(finite.max()) if len(finite) else 0.0
    side = math.isqrt(len(vec))
    width = side if side * side == len(vec) else len(vec)
    cell = lambda v: "." if v == 0 or np.isnan(v) else "9" if v == np.inf else str(min(max(int(10 * v / top), 0), 9)) if top > 0 else "-"  # noqa: E731
    return "\n".join(" ".join(cell(v) for v in vec[at:at + width]) for at in range(0, len(vec), width))


def main(argv=None) -> dict:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--run", type=pathlib.Path, required=True)
    ap.add_argument("--shards", type=pathlib.Path, required=True)
    ap.add_argument("--group-col")
    ap.add_argument("-k", type=int, default=8)
    ap.add_argument("--threshold", type=float, default=0.0)
    ap.add_argument("--min-images", type=int, default=8)
    ap.add_argument("--latent", type=int)
    ap.add_argument("--pos")
    ap.add_argument("--neg")
    args = ap.parse_args(argv)
    if (args.pos is None) != (args.neg is None) or (args.pos is not None and args.latent is None):
        ap.error("--pos and --neg go together, with --latent")
    cfg = exemplars.Config(run=args.run, shards=args.shards, group_col=args.group_col, k=args.k, threshold=args.threshold, min_images=args.min_images,
                           patch_latents=256 if args.latent is None else (args.latent,))
    fpath = exemplars.worker_fn(cfg)
    with np.load(fpath) as z:
        z = {key: z[key] for key in exemplars.KEYS}
    names = [str(g) for g in z["group_names"]]
    live = z["n_group_images"] > 0
    out = dict(out=str(fpath), n_latents=int(z["n_fire"].shape[0]), groups=names, k=args.k,
               short_fraction=float((z["n_fire"][:, live] < args.k).mean()) if live.any() else None)
    print(f"{out['n_latents']} latents, {len(names)} groups, k = {args.k}")
    print(f"fewer than k firing images: {100.0 * (out['short_fraction'] or 0.0):.1f}% of the (latent, group) pairs")
    if args.latent is not None:
        j = args.latent
        per_group = {}
        for g, name in enumerate(names):
            s = exemplars.strips(z, j, g)
            silent = [int(i) for i in z["silent_img"][j, g] if i >= 0]
            per_group[name] = dict(n_images=int(z["n_group_images"][g]), n_fire=int(z["n_fire"][j, g]), silent=silent, **s)
            print(f"latent {j} on '{name}' ({per_group[name]['n_fire']} of {per_group[name]['n_images']} images fire):")
            print(f"  top    {strip_text(s['top'])}\n  bottom {strip_text(s['bottom'])}\n  silent {' '.join(map(str, silent)) or '-'}")
        out.update(latent=j, strips=per_group)
        best = max(range(len(names)), key=lambda g: (z["top_img"][j, g, 0] >= 0, z["top_val"][j, g, 0], -g))
        if z["top_img"][j, best, 0] >= 0:
            vec = z["patch_top"][0, best, 0]
            print(f"latent {j}, patch vector of its top image {int(z['top_img'][j, best, 0])} ('{names[best]}', tenths of its maximum):\n{text_grid(vec)}")
            out.update(top_image=int(z["top_img"][j, best, 0]), top_image_group=names[best], top_image_patches=vec.tolist())
        if args.pos is not None:
            for name in (args.pos, args.neg):
                if name not in names:
                    ap.error(f"group '{name}' is not among {names}")
            ce = exemplars.counter_examples(z, j, names.index(args.pos), names.index(args.neg))
            print(f"latent {j} as a detector of '{args.pos}' against '{args.neg}':")
            print(f"  false positives ({ce['n_false_positives']} images of '{args.neg}' fire): {strip_text(ce['false_positives'])}")
            print(f"  false negatives ({ce['n_false_negatives']} images of '{args.pos}' are silent): {' '.join(map(str, ce['false_negatives'])) or '-'}")
            out.update(pos=args.pos, neg=args.neg, counter_examples=ce)
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
