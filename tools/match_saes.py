"""Match the latents of two SAE checkpoints (or the latents of one against each other) by cosine similarity -> one JSON line.

For every latent of A its nearest neighbour in B and the similarity (engine.dictionary_match: HIP kernels, no Sa x Sb matrix),
and the same from B to A:

  mmcs_a_to_b, mmcs_b_to_a   mean max cosine similarity in each direction
  mutual_fraction            share of A's latents i whose match j has i as its own match
  closest, farthest          the ten best- and worst-matched latents of A: [i, j, similarity]

With one checkpoint the latents of A are matched among themselves (pair j == i excluded): mmcs, mutual_fraction, closest and
farthest describe A's nearest neighbours -- how duplicate or split features are found.

--which W_dec (default) compares decoder rows; W_enc compares encoder columns (the transpose).  --absolute scores |cos|.
--out FILE.pt saves the values and indices of every direction computed.

    python tools/match_saes.py CKPT_A [CKPT_B] [--which W_dec|W_enc] [--absolute] [--out FILE.pt]
"""
import argparse
import json
import pathlib
import sys

import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1]))

from saev_amd import nn  # noqa: E402
from saev_amd.engine import dictionary_match  # noqa: E402


def latents(path: str, which: str, dev) -> torch.Tensor:
    """(d_sae, d_model) float32 on `dev`: the decoder's rows or the encoder's columns."""
    sae = nn.load(path)
    W = sae.W_dec.detach() if which == "W_dec" else sae.W_enc.detach().T
    return W.to(dev, torch.float32).contiguous()


def extremes(values: torch.Tensor, indices: torch.Tensor, n: int = 10) -> tuple[list, list]:
    n = min(n, values.numel())
    order = torch.argsort(values, descending=True, stable=True)
    rows = lambda sel: [[int(i), int(indices[i]), float(values[i])] for i in sel.tolist()]  # noqa: E731
    return rows(order[:n]), rows(order.flip(0)[:n])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("ckpt_a")
    ap.add_argument("ckpt_b", nargs="?")
    ap.add_argument("--which", choices=("W_dec", "W_enc"), default="W_dec")
    ap.add_argument("--absolute", action="store_true")
    ap.add_argument("--out")
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    dev = torch.device(args.device)
    A = latents(args.ckpt_a, args.which, dev)
    out = {"which": args.which, "absolute": args.absolute, "a": {"path": args.ckpt_a, "shape": list(A.shape)}}
    saved = {}
    if args.ckpt_b is None:
        r = dictionary_match(A, absolute=args.absolute)
        v, j = r.values.cpu(), r.indices.cpu().long()
        mutual = (j[j.clamp_min(0)] == torch.arange(len(j))) & (j >= 0)
        closest, farthest = extremes(v, j)
        out.update(mode="self", mmcs=r.mmcs, mutual_fraction=mutual.double().mean().item(), closest=closest, farthest=farthest,
                   route=r.route, candidates=r.candidates)
        saved = {"values": v, "indices": r.indices.cpu()}
    else:
        B = latents(args.ckpt_b, args.which, dev)
        if B.shape[1] != A.shape[1]:
            raise SystemExit(f"the checkpoints disagree on d_model: {A.shape[1]} and {B.shape[1]}")
        ab, ba = dictionary_match(A, B, absolute=args.absolute), dictionary_match(B, A, absolute=args.absolute)
        v, j, back = ab.values.cpu(), ab.indices.cpu().long(), ba.indices.cpu().long()
        mutual = back[j] == torch.arange(len(j))
        closest, farthest = extremes(v, j)
        out.update(mode="pair", b={"path": args.ckpt_b, "shape": list(B.shape)}, mmcs_a_to_b=ab.mmcs, mmcs_b_to_a=ba.mmcs,
                   mutual_fraction=mutual.double().mean().item(), closest=closest, farthest=farthest,
                   route=[ab.route, ba.route], candidates=[ab.candidates, ba.candidates])
        saved = {"values_a_to_b": v, "indices_a_to_b": ab.indices.cpu(), "values_b_to_a": ba.values.cpu(),
                 "indices_b_to_a": ba.indices.cpu()}
    if args.out:
        torch.save(saved, args.out)
        out["out"] = args.out
    print(json.dumps(out))


if __name__ == "__main__":
    main()
