"""Run an intervention experiment (saev_amd.interventions.evaluate_edits) with the SAE of a run on disk: the model
runs clean and with one block's output edited through the SAE, a head classifies the patch tokens of both, and the changes are
counted per class and written as the reference's summary CSV.

    python tools/intervene.py --run <...>/saev/runs/<id> --bundle bundle.pt --layer 11 --edits 123:set:5.0 77:scale:0:-1:active \\
                              [--auto VALUE] [--random-vector SCALE] [--scale -2.0] [--batch 16] [--out results.csv]

``--bundle`` is a ``torch.save`` dict: ``vit`` (the keyword arguments of saev_amd.data.vit.VisionTransformer), ``vit_state`` and
``head_state`` (state dicts; the head is a Linear from d_model to the classes, channel 0 the null class), ``image`` (N, 3, H, W)
and, for ``--auto``, ``patch_labels`` (N, patches).  ``--edits`` are latent:op:value[:group[:active]]; ``--auto VALUE`` picks for every
class the latent whose firing predicts it best (get_latent_lookup on the block's own activations) and sets it to VALUE on the
patches of that class; ``--random-vector SCALE`` is the baseline.  ``--sae`` names a checkpoint directly instead of ``--run``."""
import argparse
import pathlib
import sys

import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1]))

from saev_amd import disk, interventions as IV, nn  # noqa: E402
from saev_amd.data import vit  # noqa: E402


def parse_edit(text: str) -> IV.Edit:
    parts = text.split(":")
    if not 3 <= len(parts) <= 5:
        raise SystemExit(f"--edits takes latent:op:value[:group[:active]], got {text!r}")
    return IV.Edit(int(parts[0]), parts[1], float(parts[2]), int(parts[3]) if len(parts) > 3 else -1, len(parts) > 4 and parts[4] == "active")


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--run", type=pathlib.Path)
    ap.add_argument("--sae", type=pathlib.Path)
    ap.add_argument("--bundle", type=pathlib.Path, required=True)
    ap.add_argument("--layer", type=int, required=True, help="index of the block whose output is edited")
    ap.add_argument("--edits", nargs="*", default=[])
    ap.add_argument("--auto", type=float, default=None)
    ap.add_argument("--random-vector", type=float, default=None)
    ap.add_argument("--scale", type=float, default=-2.0, help="recorded in the report")
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--out", type=pathlib.Path, default=pathlib.Path("results.csv"))
    a = ap.parse_args()
    if (a.run is None) == (a.sae is None):
        raise SystemExit("give --run or --sae, one of the two")
    sae = nn.load(disk.Run(a.run).ckpt if a.run is not None else a.sae, device=a.device).eval()
    bundle = torch.load(a.bundle, map_location="cpu", weights_only=True)
    model = vit.VisionTransformer(**bundle["vit"])
    model.load_state_dict(bundle["vit_state"])
    n_out, d = bundle["head_state"]["weight"].shape
    head = torch.nn.Linear(d, n_out)
    head.load_state_dict(bundle["head_state"])
    model, head = model.to(a.device).eval(), head.to(a.device).eval()
    block = model.blocks[a.layer]
    images, labels = bundle["image"], bundle.get("patch_labels")
    batches = [{"image": images[i:i + a.batch].to(a.device), **({} if labels is None else {"patch_labels": labels[i:i + a.batch]})}
               for i in range(0, len(images), a.batch)]
    classes = range(1, n_out)
    reports = []
    if a.random_vector is not None:
        reports.append(IV.evaluate_edits(model, block, head, sae, [], batches, method="random-vector", scale=a.random_vector, classes=classes,
                                         hook=IV.random_vector_hook(a.random_vector, a.seed)))
    if a.edits:
        edits = [parse_edit(t) for t in a.edits]
        grouped = any(e.group >= 0 for e in edits)
        if grouped and labels is None:
            raise SystemExit("edits with a group need patch_labels in the bundle")
        reports.append(IV.evaluate_edits(model, block, head, sae, edits, batches, method="manual-feature", scale=a.scale, classes=classes,
                                         row_group_key="patch_labels" if grouped else None))
    if a.auto is not None:
        if labels is None:
            raise SystemExit("--auto needs patch_labels in the bundle")
        seen = {}
        acts = []
        with torch.no_grad():
            handle = block.register_forward_hook(lambda m, args, out: seen.__setitem__("x", out[:, 1:, :].clone()))
            try:
                for b in batches:
                    model(b["image"])
                    acts.append((seen["x"], b["patch_labels"]))
            finally:
                handle.remove()
        lookup = IV.get_latent_lookup(sae, acts, n_classes=n_out)
        for c in classes:
            print(f"class {c}: latent {int(lookup.lookup[c])} (F1 {float(lookup.scores[c, 0]):.3f} above {float(lookup.thresholds[c, 0]):g})")
        edits = IV.EditSet([IV.Edit(int(lookup.lookup[c]), "set", a.auto, group=c) for c in classes], sae.cfg.d_sae, n_groups=n_out)
        reports.append(IV.evaluate_edits(model, block, head, sae, edits, batches, method="automatic-feature", scale=a.scale, classes=classes,
                                         row_group_key="patch_labels"))
    if not reports:
        raise SystemExit("nothing to do: give --edits, --auto or --random-vector")
    IV.save(reports, str(a.out))
    for r in reports:
        print(f"{r.method}: target change {r.mean_target_change:.4f} (std {r.target_change_std:.4f}), other change {r.mean_other_change:.4f} "
              f"(std {r.other_change_std:.4f})")
    return 0


if __name__ == "__main__":
    sys.exit(main())
