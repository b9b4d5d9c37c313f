"""Which images to look at: per latent and per class of images the strongest firing images, the weakest firing images and the silent
ones (ideas 1 and 5 of the reference's contrib/mimics/README.md: per-class activation grids with labels, and the counter-example
explorer -- the wrong class's images that fire strongly, the right class's images that stay silent), on ``engine.latent_exemplars``
and ``engine.latent_patch_rows`` (include/saev_amd.h: LATENT EXEMPLARS).

Row ``i * T + p`` of ``token_acts.npz`` is patch ``p`` of image ``i``.  An image FIRES for a latent when one of its patches is above
the threshold; its value is the maximum over its patches (what ``pool_images("max")`` gives) and its patch the lowest one that attains
it.  The lists hold DISTINCT images -- the reference's ``csr_topk(token_acts, k, axis=0).indices // tokens_per_image`` holds the top
TOKENS, so an image with several strong patches takes several slots there -- and ties go to the lower image.

``worker_fn`` reads a run's ``token_acts.npz``, groups the images by a column of ``image_labels.csv`` and writes
``latent_exemplars.npz`` beside it.  Everything that touches activations runs on the HIP device; there is no CPU path."""

from __future__ import annotations

import dataclasses
import logging
import pathlib

import numpy as np
import scipy.sparse
import torch

from . import classification, engine, mimics, spatial
from . import data as saev_data
from .classification import LabelGrouping

logger = logging.getLogger("exemplars")

LISTS = ("top_val", "top_img", "top_patch", "bot_val", "bot_img", "bot_patch", "silent_img")
KEYS = ("group_names", "n_group_images", "n_fire") + LISTS + ("patch_latents", "patch_top", "patch_bot")
MAX_GROUPS, MAX_K = 64, 32


def _np(x) -> np.ndarray:
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _get(result, name: str) -> np.ndarray:
    """An array of a ``LatentExemplarsResult``, of ``compute``'s dict or of a loaded ``latent_exemplars.npz``."""
    return _np(getattr(result, name) if isinstance(result, engine.LatentExemplarsResult) else result[name])


@dataclasses.dataclass(frozen=True)
class Config:
    run: pathlib.Path = pathlib.Path("./runs/abcdefg")
    """Run directory: ``<run>/inference/<shards name>/token_acts.npz`` is read and ``latent_exemplars.npz`` written beside it."""
    shards: pathlib.Path = pathlib.Path("./shards/01234567")
    """Shards directory: its metadata gives the tokens of an image, its ``image_labels.csv`` the groups."""
    group_col: str | None = None
    """Column of ``image_labels.csv`` whose labels group the images; None puts all images in one group."""
    grouping: LabelGrouping | None = None
    """A grouping of labels (its ``source_col`` is the column) instead of ``group_col``'s own labels."""
    k: int = 8
    """Images per list."""
    threshold: float = 0.0
    """An activation fires when it is > threshold."""
    patch_latents: int | tuple[int, ...] = 256
    """The latents whose listed images keep their patch vectors: a list of ids, or the K with the largest spread of firing rate."""
    min_images: int = 8
    """With an integer ``patch_latents``, only pairs that fire in at least this many images compete."""


def exemplars_fpath(cfg: Config) -> pathlib.Path:
    return pathlib.Path(cfg.run) / "inference" / pathlib.Path(cfg.shards).name / "latent_exemplars.npz"


def choose_patch_latents(n_fire_sg, n_group_images, k: int, min_images: int) -> np.ndarray:
    """The ``k`` latents with the largest spread of firing rate, max_g n_fire / n_g - min_g n_fire / n_g, over the (latent, group)
    pairs that fire in at least ``min_images`` images (another pair counts as rate 0; an empty group does not count); with one group
    the ``k`` latents that fire in the largest share of its images.  Ties go to the lower index, and a latent without such a pair is never chosen.
    Ascending latent ids."""
    nf, ng = _np(n_fire_sg).astype(np.float64), _np(n_group_images).astype(np.float64)
    live = ng > 0
    if not live.any():
        return np.zeros(0, dtype=np.int64)
    enough = nf[:, live] >= min_images
    rate = np.where(enough, nf[:, live] / ng[live][None, :], 0.0)
    score = rate.max(axis=1) - (rate.min(axis=1) if rate.shape[1] > 1 else 0.0)
    valid = enough.any(axis=1)
    order = np.argsort(-np.where(valid, score, -np.inf), kind="stable")
    order = order[valid[order]][:max(int(k), 0)]
    return np.sort(order).astype(np.int64)


def _latents_per_call(n_groups: int, k: int) -> int:
    """Latents a call may take: S * G * k below 2^31, and lists of at most 1 GiB (seven arrays of 4 bytes a slot)."""
    return max(1, min((2**31 - 1) // (n_groups * k), 2**30 // (28 * n_groups * k)))


def compute(ta: scipy.sparse.csr_matrix, groups: np.ndarray, n_groups: int, T: int, *, k: int = 8, threshold: float = 0.0, patch_latents=256,
            min_images: int = 8, device=None) -> dict[str, np.ndarray]:
    """The arrays of ``latent_exemplars.npz`` but the group names, from the token activations of ``len(groups)`` images."""
    n_images, S = len(groups), ta.shape[1]
    if ta.shape[0] != n_images * T:
        raise ValueError(f"token_acts has {ta.shape[0]} rows, {n_images} images of {T} tokens are {n_images * T}")
    dev = classification._device(device)
    g_dev = torch.from_numpy(np.ascontiguousarray(groups, dtype=np.int32)).to(dev)
    ta = scipy.sparse.csr_matrix(ta)
    out = dict(n_fire=np.zeros((S, n_groups), dtype=np.int32))
    for name in LISTS:
        out[name] = np.zeros((S, n_groups, k), dtype=np.float32 if name.endswith("val") else np.int32)
    step = _latents_per_call(n_groups, k)
    for lo in range(0, S, step):  # a latent scored alone has the bits it has among others
        hi = min(lo + step, S)
        part = ta if (lo, hi) == (0, S) else ta[:, lo:hi]
        res = engine.latent_exemplars(*classification._csr_on(part, dev), n_images=n_images, tokens_per_image=T, n_latents=hi - lo, groups=g_dev,
                                      n_groups=n_groups, k=k, threshold=threshold)
        for name in ("n_fire",) + LISTS:
            out[name][lo:hi] = _np(getattr(res, name))
        out["n_group_images"] = _np(res.n_group_images)
    if isinstance(patch_latents, (int, np.integer)):
        chosen = choose_patch_latents(out["n_fire"], out["n_group_images"], int(patch_latents), min_images)
    else:
        chosen = np.asarray(list(patch_latents), dtype=np.int64)
        if chosen.size and (chosen.min() < 0 or chosen.max() >= S):
            raise ValueError(f"patch_latents must lie in [0, {S})")
    csr = classification._csr_on(ta, dev)
    lat = torch.from_numpy(np.broadcast_to(chosen[:, None, None], (len(chosen), n_groups, k)).astype(np.int32)).to(dev)
    step = max(1, 2**28 // (n_groups * k * T))  # at most 1 GiB of patch vectors a call
    for end in ("top", "bot"):
        img = torch.from_numpy(out[end + "_img"][chosen]).to(dev)
        rows = np.zeros((len(chosen), n_groups, k, T), dtype=np.float32)
        for lo in range(0, len(chosen), step):
            rows[lo:lo + step] = _np(engine.latent_patch_rows(*csr, lat[lo:lo + step], img[lo:lo + step], n_images=n_images, tokens_per_image=T,
                                                              n_latents=S))
        out["patch_" + end] = rows
    out["patch_latents"] = chosen
    return out


def worker_fn(cfg: Config) -> pathlib.Path:
    """List the exemplars of every latent of a run and write ``latent_exemplars.npz`` (keys ``KEYS``) beside its ``token_acts.npz``;
    returns its path."""
    fpath = exemplars_fpath(cfg)
    ta = scipy.sparse.load_npz(str(fpath.parent / "token_acts.npz")).tocsr()
    T = saev_data.Metadata.load(pathlib.Path(cfg.shards)).content_tokens_per_example
    if ta.shape[0] % T:
        raise ValueError(f"token_acts.npz has {ta.shape[0]} rows, no whole number of images of {T} tokens")
    if not 1 <= cfg.k <= MAX_K:
        raise ValueError(f"k = {cfg.k} must lie in [1, {MAX_K}]")
    groups, names = spatial.image_groups(spatial.Config(shards=cfg.shards, group_col=cfg.group_col, grouping=cfg.grouping), ta.shape[0] // T)
    out = compute(ta, groups, len(names), T, k=cfg.k, threshold=cfg.threshold, patch_latents=cfg.patch_latents, min_images=cfg.min_images)
    out["group_names"] = np.asarray(names, dtype=str)
    np.savez(fpath, **{key: out[key] for key in KEYS})
    logger.info("Wrote the exemplars of %d latents in %d groups (patch vectors of %d) to '%s'.", ta.shape[1], len(names), len(out["patch_latents"]), fpath)
    return fpath


def _records(result, end: str, latent: int, group: int) -> list[dict]:
    img = _get(result, end + "_img")[latent, group]
    val, patch = _get(result, end + "_val")[latent, group], _get(result, end + "_patch")[latent, group]
    return [dict(image=int(i), value=float(v), patch=int(p)) for i, v, p in zip(img, val, patch) if i >= 0]


def strips(result, latent: int, group: int) -> dict[str, list[dict]]:
    """The two lists of (latent, group) as records ``{image, value, patch}``: ``top`` strongest first, ``bottom`` weakest first."""
    return dict(top=_records(result, "top", latent, group), bottom=_records(result, "bot", latent, group))


def counter_examples(result, latent: int, pos_group: int, neg_group: int) -> dict:
    """The counter-examples of a latent read as a detector of ``pos_group`` against ``neg_group``: ``false_positives`` are the
    ``neg_group``'s strongest firing images (records), ``false_negatives`` the first silent images of ``pos_group``, of which there
    are ``n_false_negatives`` = n_g - n_fire in all (``n_false_positives``: the firing images of ``neg_group``)."""
    silent = _get(result, "silent_img")[latent, pos_group]
    n_fire, n_g = _get(result, "n_fire"), _get(result, "n_group_images")
    return dict(false_positives=_records(result, "top", latent, neg_group), n_false_positives=int(n_fire[latent, neg_group]),
                false_negatives=[int(i) for i in silent if i >= 0], n_false_negatives=int(n_g[pos_group] - n_fire[latent, pos_group]))


def top_images(ta: scipy.sparse.csr_matrix, T: int, k: int, *, threshold: float = 0.0, device=None) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(image, value, patch), each (S, k): the ``k`` strongest DISTINCT images of every latent over all images, -1 / 0.0 / -1 where
    fewer fire -- the replacement of ``csr_topk(token_acts, k, axis=0).indices // T`` of the reference's ``visuals.py``, which lists
    tokens and so repeats an image with several strong patches."""
    if ta.shape[0] % T:
        raise ValueError(f"token_acts has {ta.shape[0]} rows, no whole number of images of {T} tokens")
    n_images, S = ta.shape[0] // T, ta.shape[1]
    dev = classification._device(device)
    g_dev = torch.zeros(n_images, device=dev, dtype=torch.int32)
    ta = scipy.sparse.csr_matrix(ta)
    img, val, patch = np.zeros((S, k), dtype=np.int32), np.zeros((S, k), dtype=np.float32), np.zeros((S, k), dtype=np.int32)
    step = _latents_per_call(1, k)
    for lo in range(0, S, step):
        hi = min(lo + step, S)
        part = ta if (lo, hi) == (0, S) else ta[:, lo:hi]
        res = engine.latent_exemplars(*classification._csr_on(part, dev), n_images=n_images, tokens_per_image=T, n_latents=hi - lo, groups=g_dev,
                                      n_groups=1, k=k, threshold=threshold)
        img[lo:hi], val[lo:hi], patch[lo:hi] = _np(res.top_img)[:, 0], _np(res.top_val)[:, 0], _np(res.top_patch)[:, 0]
    return img, val, patch


def for_tasks(task_specs: list, n_images: int) -> tuple[np.ndarray, int, dict[str, tuple[list[int], list[int]]]]:
    """The groups behind the tasks ``mimics.worker_fn`` scores: (group id per image int32, the number of groups, per task name the
    groups of its erato images -- the negatives -- and of its melpomene images -- the positives).  The groups are the classes of
    ``mimics.task_classes``: the images with the same role in every task, -1 for an image that no task includes."""
    groups, roles = mimics.task_classes(task_specs, n_images)
    n_groups = roles.shape[1] if (groups >= 0).any() else 0
    if n_groups > MAX_GROUPS:
        raise ValueError(f"the tasks make {n_groups} groups of images; at most {MAX_GROUPS} are listed in one call")
    sides = {spec.name: ([int(c) for c in np.flatnonzero(roles[t, :n_groups] == 1)], [int(c) for c in np.flatnonzero(roles[t, :n_groups] == 2)])
             for t, spec in enumerate(task_specs)}
    return groups, n_groups, sides
