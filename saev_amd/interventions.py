"""Interventions on SAE latents inside a model's forward pass (the reference's contrib/interactive_interp/semseg:
``interactive.py::modify`` and ``quantitative.py``): set, scale or shift a few latents of every token, put the edited activations
back into the transformer and count which predictions change.

The reference decodes twice and keeps an n x d_sae matrix: ``x' = (x - x_hat) + decode(f_mod)``.  Here the edit is k-sparse,

    x' = x + sum_e (t_e(f_l) - f_l) W_dec[l_e, :]

-- ``b_dec`` and every unedited latent cancel --, one HIP kernel over x (include/saev_amd.h: LATENT EDITS).  Rows
that no edit touches come back bit for bit, which the reference's ``(x - x_hat) + x_hat`` does not give.  The codes come from
``sae.encode_sparse``; there is no CPU path.
"""

from __future__ import annotations

import collections.abc
import csv
import dataclasses
import os
import typing as tp

import numpy as np
import torch

from . import _lib, engine

_OPS = {"set": _lib.EDIT_SET, "scale": _lib.EDIT_SCALE, "add": _lib.EDIT_ADD}


@dataclasses.dataclass(frozen=True)
class Edit:
    """One edit of one latent: ``op`` "set" (f -> value), "scale" (f -> value * f) or "add" (f -> f + value).  ``group`` -1
    applies it to every row, g >= 0 to the rows whose ``row_group`` is g; ``if_active`` only where the latent fires (f != 0)."""

    latent: int
    op: str = "set"
    value: float = 0.0
    group: int = -1
    if_active: bool = False

    def record(self) -> tuple[int, int, float, int]:
        if self.op not in _OPS:
            raise ValueError(f"Edit.op must be one of {sorted(_OPS)}, got {self.op!r}")
        return (int(self.latent), _OPS[self.op] | (_lib.EDIT_IF_ACTIVE if self.if_active else 0), float(self.value), int(self.group))


class EditSet:
    """A validated list of edits for SAEs of ``d_sae`` latents and ``n_groups`` row groups.  The library validates at construction
    (on the host: no device is needed) and raises ValueError with its message; the device plan is built once per device, on
    first use.  Edits do not compose: a latent appears once in a list, and not in both the global list and a group's."""

    def __init__(self, edits: tp.Iterable[Edit], d_sae: int, n_groups: int = 0):
        self.edits = tuple(edits)
        self.d_sae, self.n_groups = int(d_sae), int(n_groups)
        self.records = [e.record() for e in self.edits]
        lib = _lib.load()
        rc = lib.saev_edit_plan_build(engine.edit_records(self.records), len(self.records), self.n_groups, self.d_sae, None, 0, None)
        if rc != 0:
            raise ValueError((lib.saev_last_error(None) or b"saev_edit_plan_build refused the edits").decode())
        self._plans: dict[torch.device, torch.Tensor] = {}

    def __len__(self) -> int:
        return len(self.edits)

    @property
    def lists(self) -> list[list[int]]:
        """The caller's indices of the edits as the plan groups them: ``lists[0]`` the global list, ``lists[g + 1]`` group g's,
        each in the caller's order."""
        out: list[list[int]] = [[] for _ in range(self.n_groups + 1)]
        for i, e in enumerate(self.edits):
            out[e.group + 1].append(i)
        return out

    def plan(self, device) -> torch.Tensor:
        device = engine._hip_device("EditSet.plan", device)
        if device not in self._plans:
            self._plans[device] = engine.build_edit_plan(self.records, self.d_sae, self.n_groups, device)
        return self._plans[device]


def _as_edit_set(sae, edits) -> EditSet:
    if isinstance(edits, EditSet):
        if edits.d_sae != sae.cfg.d_sae:
            raise ValueError(f"the EditSet was built for d_sae {edits.d_sae}, the SAE has {sae.cfg.d_sae}")
        return edits
    if isinstance(edits, Edit):
        edits = [edits]
    edits = list(edits)
    return EditSet(edits, sae.cfg.d_sae, max((e.group for e in edits), default=-1) + 1)


def intervene(sae, x: torch.Tensor, edits, *, row_group: torch.Tensor | None = None, row_keep: torch.Tensor | None = None,
              out: torch.Tensor | None = None, return_counts: bool = False):
    """``x`` (..., d_model) with the edits applied through ``sae``: x + sum_e (t_e(f_l) - f_l) W_dec[l_e, :], f the SAE's own codes
    of x (``sae.encode_sparse``: TopK, ReLU or BatchTopK rows).  ``edits`` is an ``EditSet`` (or Edits, planned on the spot);
    ``row_group`` (...) integer groups select the group lists, ``row_keep`` (...) bool rows to edit at all.  ``out=x`` edits in
    place.  With ``return_counts`` also the number of rows each edit changed, (n_edits) int64 on the device."""
    from .nn import modeling

    if isinstance(sae.cfg.activation, modeling.BatchTopK) and sae.training:
        raise RuntimeError("intervene on a BatchTopK SAE in training mode: its encode selects over the batch and moves the threshold; "
                           "call sae.eval() first")
    es = _as_edit_set(sae, edits)
    D = sae.cfg.d_model
    if x.shape[-1] != D:
        raise ValueError(f"x must be (..., {D}), got {tuple(x.shape)}")
    lead = x.shape[:-1]
    if out is not None and (out.shape != x.shape or not out.is_contiguous() or not x.is_contiguous()):
        raise ValueError("out must be contiguous and of x's shape (and x contiguous)")
    rows = x.reshape(-1, D)
    n = rows.shape[0]
    with torch.no_grad():
        rows = rows.detach().contiguous()
        codes = sae.encode_sparse(rows)
        idx, val = codes[0], codes[1]
        row_nnz = codes[2] if len(codes) > 2 else None
        if row_group is not None:
            row_group = row_group.reshape(-1).to(device=rows.device, dtype=torch.int32)
        if row_keep is not None:
            row_keep = row_keep.reshape(-1).to(device=rows.device, dtype=torch.bool)
        counts = torch.zeros(len(es), device=rows.device, dtype=torch.int64) if return_counts else None
        res = engine.intervene_rows(rows, sae.W_dec, idx, val, row_nnz, es.plan(rows.device), len(es), es.n_groups, row_group=row_group,
                                    row_keep=row_keep, out=None if out is None else out.detach().view(n, D), rows_changed=counts)
    res = out if out is not None else res.view(*lead, D)
    return (res, counts) if return_counts else res


# ---- choosing a latent per class ---------------------------------------------------------------------------------------------------


@dataclasses.dataclass(frozen=True)
class LatentLookup:
    """``latents`` / ``scores`` / ``thresholds`` (n_classes, top_k), best first; ``lookup`` (n_classes) int64 = latents[:, 0], 0 for a
    skipped class (as the reference leaves it)."""

    lookup: torch.Tensor
    latents: torch.Tensor
    scores: torch.Tensor
    thresholds: torch.Tensor


def get_latent_lookup(sae, batches, *, n_classes: int, thresholds=(0.0, 0.1, 0.3, 1.0), sparsity: torch.Tensor | None = None,
                      max_freq: float = 3e-2, skip_classes=(0,), top_k: int = 3) -> LatentLookup:
    """For every class the latents whose firing predicts it best: F1 of ``f > threshold`` against ``label == class`` over all rows,
    the best of a few thresholds (the reference's ``get_latent_lookup``).  ``batches`` yields ``(x, labels)`` or ``(x, labels, keep)``:
    x (..., d_model), labels (...) integers (a label outside [0, n_classes) drops the row), keep (...) bool.  ``sparsity`` (d_sae)
    firing frequencies: latents at or above ``max_freq`` are masked out.  Classes in ``skip_classes`` are scored but get latent 0.

    One difference from the reference: a batch without a row of class c still adds its firing rows to c's false positives; the
    reference's loop over the batch's unique classes skips such batches, so its counts depend on how the data was batched."""
    counts = None
    for batch in batches:
        x, labels = batch[0], batch[1]
        keep = batch[2] if len(batch) > 2 else None
        rows = x.reshape(-1, sae.cfg.d_model)
        with torch.no_grad():
            codes = sae.encode_sparse(rows.contiguous())
        if counts is None:
            counts = engine.ClassFireCounts(sae.cfg.d_sae, n_classes, rows.device, thresholds)
        counts.add(codes[0], codes[1], codes[2] if len(codes) > 2 else None, labels.reshape(-1).to(rows.device),
                   None if keep is None else keep.reshape(-1).to(rows.device))
    if counts is None:
        raise ValueError("get_latent_lookup: no batches")
    mask = None if sparsity is None else (sparsity.to(counts.device) < max_freq)
    latents, scores, thr = counts.lookup(top_k, mask)
    lookup = latents[:, 0].to(torch.int64).clone()
    for c in skip_classes:
        if 0 <= c < n_classes:
            lookup[c] = 0
    return LatentLookup(lookup=lookup, latents=latents, scores=scores, thresholds=thr)


# ---- hooks -------------------------------------------------------------------------------------------------------------------------


def make_hook(sae, edits, *, tokens=slice(1, None), row_group=None):
    """A ``register_forward_hook`` function for a module whose output is (B, T, D): the tokens ``output[:, tokens, :]`` are edited
    through ``intervene`` and written back into the output tensor, the others (the CLS token, by default) are not touched.  The
    selected tokens are copied out once -- the encoder needs contiguous rows --, edited in place, and one ``copy_`` puts them back;
    a selection that is already contiguous is edited where it lies.  ``row_group``: a (B, n_tokens) integer tensor, or a callable
    that returns the current batch's."""

    def hook(module, args, output):
        sel = output[:, tokens, :]
        b, t, d = sel.shape
        rg = row_group() if callable(row_group) else row_group
        if rg is not None:
            rg = rg.reshape(b * t)
        with torch.no_grad():
            if sel.is_contiguous():
                intervene(sae, sel.view(b * t, d), edits, row_group=rg, out=sel.view(b * t, d))
            else:
                rows = sel.reshape(b * t, d)
                sel.copy_(intervene(sae, rows, edits, row_group=rg, out=rows).view(b, t, d))
        return output

    return hook


def random_vector_hook(scale: float, seed: int, *, tokens=slice(1, None)):
    """The reference's baseline (``eval_rand_vec``): a forward hook that adds ``scale`` times a random unit vector to every selected
    token.  The generator is seeded once, when the hook first runs, on the output's device."""
    state: dict = {}

    def hook(module, args, output):
        sel = output[:, tokens, :]
        if "gen" not in state:
            state["gen"] = torch.Generator(device=sel.device).manual_seed(seed)
        with torch.no_grad():
            v = torch.randn(sel.shape, device=sel.device, dtype=sel.dtype, generator=state["gen"])
            sel.add_(v / torch.norm(v, dim=-1, keepdim=True) * scale)
        return output

    return hook


def map_range(x: float, domain: tuple[float, float], range: tuple[float, float]) -> float:
    a, b = domain
    c, d = range
    if not (a <= x <= b):
        raise ValueError(f"x={x:.3f} must be in {[a, b]}.")
    return c + (x - a) * (d - c) / (b - a)


def unscaled(x: float, max_obs: float) -> float:
    """Scale from [-10, 10] to [10 * -max_obs, 10 * max_obs]."""
    return map_range(x, (-10.0, 10.0), (-10.0 * max_obs, 10.0 * max_obs))


def argmax_logits(logits_bpc: torch.Tensor) -> torch.Tensor:
    """(batch, patches) class ids from logits whose channel 0 is the null class."""
    return logits_bpc[:, :, 1:].argmax(dim=-1) + 1


# ---- the report --------------------------------------------------------------------------------------------------------------------


@dataclasses.dataclass(frozen=True)
class ClassResults:
    """Results for a single class (the reference's fields)."""

    class_id: int
    class_name: str
    n_orig_patches: int
    n_changed_patches: int
    n_other_patches: int
    n_other_changed: int
    change_distribution: dict[int, int]


@dataclasses.dataclass(frozen=True)
class Report:
    """Complete results of an intervention experiment (the reference's fields and properties)."""

    method: str
    class_results: list[ClassResults]
    intervention_scale: float

    @property
    def mean_target_change(self) -> float:
        total_target = sum(r.n_orig_patches for r in self.class_results)
        total_changed = sum(r.n_changed_patches for r in self.class_results)
        return total_changed / total_target if total_target > 0 else 0.0

    @property
    def mean_other_change(self) -> float:
        total_other = sum(r.n_other_patches for r in self.class_results)
        total_changed = sum(r.n_other_changed for r in self.class_results)
        return total_changed / total_other if total_other > 0 else 0.0

    @property
    def target_change_std(self) -> float:
        return float(np.std(np.array([r.n_changed_patches / r.n_orig_patches if r.n_orig_patches > 0 else 0.0 for r in self.class_results])))

    @property
    def other_change_std(self) -> float:
        return float(np.std(np.array([r.n_other_changed / r.n_other_patches if r.n_other_patches > 0 else 0.0 for r in self.class_results])))

    def to_csv_row(self) -> dict[str, float | str]:
        return {"method": self.method, "target_change": self.mean_target_change, "other_change": self.mean_other_change,
                "target_std": self.target_change_std, "other_std": self.other_change_std}


def save(results: list[Report], fpath: str) -> None:
    """The summary CSV of the reference: one row per report."""
    os.makedirs(os.path.dirname(os.path.abspath(fpath)), exist_ok=True)
    columns = ["method", "target_change", "target_std", "other_change", "other_std"]
    with open(fpath, "w", newline="") as fd:
        writer = csv.DictWriter(fd, fieldnames=columns)
        writer.writeheader()
        for result in results:
            writer.writerow(result.to_csv_row())


def compute_class_results(orig_preds: torch.Tensor, mod_preds: torch.Tensor, classes=range(1, 151)) -> list[ClassResults]:
    """Per class: how many of its patches changed prediction, how many of the others did, and where its patches went -- from ONE
    confusion matrix (one device-to-host copy), not a read-back per pair of classes."""
    if orig_preds.shape != mod_preds.shape:
        raise ValueError(f"orig_preds and mod_preds differ in shape: {tuple(orig_preds.shape)} and {tuple(mod_preds.shape)}")
    classes = [int(c) for c in classes]
    o, m = orig_preds.reshape(-1).long(), mod_preds.reshape(-1).to(orig_preds.device).reshape(-1).long()
    n = o.numel()
    if n and (int(torch.minimum(o.min(), m.min())) < 0):
        raise ValueError("predictions must be non-negative class ids")
    k = max([int(torch.maximum(o.max(), m.max())) if n else 0] + classes) + 1
    conf = torch.bincount(o * k + m, minlength=k * k).reshape(k, k).cpu().numpy()
    n_changed_all = int(n - np.trace(conf))
    row_sum = conf.sum(axis=1)
    out = []
    for c in classes:
        n_orig = int(row_sum[c])
        n_changed = n_orig - int(conf[c, c])
        changes = {new: int(conf[c, new]) for new in classes if new != c and conf[c, new] > 0}
        out.append(ClassResults(class_id=c, class_name="TODO", n_orig_patches=n_orig, n_changed_patches=n_changed,
                                n_other_patches=n - n_orig, n_other_changed=n_changed_all - n_changed, change_distribution=changes))
    return out


def evaluate_edits(model, block, head, sae, edits, batches, *, method: str, scale: float, row_group_key: str | None = None,
                   tokens=slice(1, None), classes=range(1, 151), hook=None) -> Report:
    """Run ``model`` clean and with ``block``'s output edited, classify the selected tokens of both with ``head`` and count the
    changes (the reference's ``eval_rand_feat`` / ``eval_auto_feat``).  ``batches`` yields image tensors, or mappings with the
    images under "image" and, for ``row_group_key``, the (B, n_tokens) row groups under that key.  ``hook`` replaces the edit hook
    (``random_vector_hook`` for the baseline).  The hook is removed after every hooked forward, also when it raises."""
    current: dict = {}
    if hook is None:
        hook = make_hook(sae, edits, tokens=tokens, row_group=(lambda: current["row_group"]) if row_group_key is not None else None)
    orig_preds, mod_preds = [], []
    with torch.no_grad():
        for batch in batches:
            if isinstance(batch, collections.abc.Mapping):
                images = batch["image"]
                if row_group_key is not None:
                    current["row_group"] = batch[row_group_key]
            else:
                images = batch
            orig_preds.append(argmax_logits(head(model(images)[:, tokens, :])))
            handle = block.register_forward_hook(hook)
            try:
                mod_preds.append(argmax_logits(head(model(images)[:, tokens, :])))
            finally:
                handle.remove()
    if not orig_preds:
        raise ValueError("evaluate_edits: no batches")
    class_results = compute_class_results(torch.cat(orig_preds, dim=0), torch.cat(mod_preds, dim=0), classes)
    return Report(method=method, class_results=class_results, intervention_scale=scale)
