"""Spatial coherence of latents: where on the patch grid a latent fires (the third property of a good latent in the reference's
contrib/mimics/logbook.md, and idea 4, "spatial activation heatmaps", of its README: a latent's activation map averaged over the
specimens of a class, and the difference map of two classes), on ``engine.latent_spatial`` (include/saev_amd.h: LATENT SPATIAL;
DESIGN.md 3.27).  The specimens are pose-normalised, so position carries meaning: row ``i * T + p`` of ``token_acts.npz`` is
position ``p`` of image ``i`` on a ``gh x gw`` grid.

The kernels leave exact integers per (latent, group of images); every score here is ONE float64 expression on them, NaN where it is
undefined:

  adjacency             2 (pairs_h + pairs_v) / n_events: the mean number of firing 4-neighbours of a firing patch
  clustering            (pairs_h + pairs_v) / expected, expected = E (sum_m2 - n_events) / (T (T - 1)) with E = gh (gw - 1) +
                        gw (gh - 1) grid edges: the pairs there would be if every image's m patches lay uniformly at random, so
                        1 means no spatial structure
  position_consistency  (overlap - n_events) / (n_events (n_images_fire - 1)): the mean, over firing patches, of the share of the
                        OTHER firing images that fire at the same position; in [0, 1]
  centroid, spread      the activation-weighted mean (row, column) and the root of the two weighted variances added

``worker_fn`` reads a run's ``token_acts.npz``, groups the images by a column of ``image_labels.csv`` and writes
``latent_spatial.npz`` beside it.  Everything that touches activations runs on the HIP device; there is no CPU path."""

from __future__ import annotations

import dataclasses
import logging
import math
import pathlib

import numpy as np
import scipy.sparse
import torch

from . import classification, engine
from . import data as saev_data
from .classification import LabelGrouping, apply_grouping, load_image_labels

logger = logging.getLogger("spatial")

INTEGERS = ("n_events", "n_images_fire", "pairs_h", "pairs_v", "sum_m2", "overlap")
SCORES = ("adjacency", "clustering", "position_consistency", "centroid", "spread")
KEYS = INTEGERS + ("moments",) + SCORES + ("group_names", "n_group_images", "grid", "map_latents", "count_map", "mean_map")
MAX_GROUPS = 64


def _np(x) -> np.ndarray:
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _f(x) -> np.ndarray:
    return _np(x).astype(np.float64)


def n_grid_edges(grid) -> int:
    gh, gw = grid
    return gh * (gw - 1) + gw * (gh - 1)


def adjacency(pairs_h, pairs_v, n_events) -> np.ndarray:
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(_np(n_events) > 0, 2.0 * (_f(pairs_h) + _f(pairs_v)) / _f(n_events), np.nan)


def clustering(pairs_h, pairs_v, sum_m2, n_events, grid) -> np.ndarray:
    T = grid[0] * grid[1]
    with np.errstate(divide="ignore", invalid="ignore"):
        expected = float(n_grid_edges(grid)) * (_f(sum_m2) - _f(n_events)) / float(T * (T - 1)) if T > 1 else np.zeros(_np(n_events).shape)
        return np.where(expected > 0, (_f(pairs_h) + _f(pairs_v)) / expected, np.nan)


def position_consistency(overlap, n_events, n_images_fire) -> np.ndarray:
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(_np(n_images_fire) > 1, (_f(overlap) - _f(n_events)) / (_f(n_events) * (_f(n_images_fire) - 1.0)), np.nan)


def centroid(moments) -> np.ndarray:
    """(..., 2): the activation-weighted mean grid row and column; NaN for a pair without events."""
    m = _f(moments)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.stack([m[..., 1] / m[..., 0], m[..., 2] / m[..., 0]], axis=-1)


def spread(moments) -> np.ndarray:
    """The root of the weighted variance of the row plus that of the column (a variance that rounds below 0 counts as 0)."""
    m = _f(moments)
    with np.errstate(divide="ignore", invalid="ignore"):
        var = (m[..., 3] / m[..., 0] - (m[..., 1] / m[..., 0]) ** 2) + (m[..., 4] / m[..., 0] - (m[..., 2] / m[..., 0]) ** 2)
        return np.sqrt(np.where(var < 0, 0.0, var))


def rate_map(count_map, n_group_images) -> np.ndarray:
    """count_map (S, G, gh, gw) over the images of each group: the share of the group's images in which the latent fires there."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return _f(count_map) / _f(n_group_images)[None, :, None, None]


def mean_map(sum_map, n_group_images) -> np.ndarray:
    """sum_map (S, G, gh, gw) over the images of each group: the mean activation there, a silent image counting as 0."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return _f(sum_map) / _f(n_group_images)[None, :, None, None]


def difference_map(result, j: int, a: int, b: int) -> np.ndarray:
    """(gh, gw): latent j's mean map on group a minus that on group b.  ``result`` is a ``LatentSpatialResult`` or a loaded
    ``latent_spatial.npz`` (j is then a position in its ``map_latents``)."""
    if isinstance(result, engine.LatentSpatialResult):
        if result.sum_map is None:
            raise ValueError("difference_map needs a result computed with sum_map=True")
        n = _f(result.n_group_images)
        with np.errstate(divide="ignore", invalid="ignore"):
            return _f(result.sum_map[j, a]) / n[a] - _f(result.sum_map[j, b]) / n[b]
    return _f(result["mean_map"][j, a]) - _f(result["mean_map"][j, b])


def scores_of(ints: dict, moments, grid) -> dict[str, np.ndarray]:
    """Every derived score from the integer outputs (a dict with the keys ``INTEGERS``) and the moments."""
    return dict(adjacency=adjacency(ints["pairs_h"], ints["pairs_v"], ints["n_events"]),
                clustering=clustering(ints["pairs_h"], ints["pairs_v"], ints["sum_m2"], ints["n_events"], grid),
                position_consistency=position_consistency(ints["overlap"], ints["n_events"], ints["n_images_fire"]),
                centroid=centroid(moments), spread=spread(moments))


def infer_grid(tokens_per_image: int, grid=None) -> tuple[int, int]:
    """``grid`` checked against the tokens of an image, or the square grid of that many tokens; ValueError when there is none."""
    if grid is not None:
        gh, gw = (int(g) for g in grid)
        if gh < 1 or gw < 1 or gh * gw != tokens_per_image:
            raise ValueError(f"a {gh} x {gw} grid does not hold the {tokens_per_image} tokens of an image")
        return gh, gw
    side = math.isqrt(tokens_per_image)
    if side * side != tokens_per_image:
        raise ValueError(f"{tokens_per_image} tokens per image are not a square grid: give grid=(gh, gw)")
    return side, side


def choose_map_latents(position_consistency_sg, n_images_fire_sg, k: int, min_images: int) -> np.ndarray:
    """The ``k`` latents with the largest position consistency in any group, among the (latent, group) pairs that fire in at least
    ``min_images`` images; ties go to the lower index, and a latent without such a pair is never chosen.  Ascending latent ids."""
    pc = np.where(_np(n_images_fire_sg) >= min_images, _f(position_consistency_sg), np.nan)
    valid = ~np.isnan(pc).all(axis=1)
    best = np.full(pc.shape[0], -np.inf)
    best[valid] = np.nanmax(pc[valid], axis=1)
    order = np.argsort(-best, kind="stable")
    order = order[valid[order]][:max(int(k), 0)]
    return np.sort(order).astype(np.int64)


@dataclasses.dataclass(frozen=True)
class Config:
    run: pathlib.Path = pathlib.Path("./runs/abcdefg")
    """Run directory: ``<run>/inference/<shards name>/token_acts.npz`` is read and ``latent_spatial.npz`` written beside it."""
    shards: pathlib.Path = pathlib.Path("./shards/01234567")
    """Shards directory: its metadata gives the tokens of an image, its ``image_labels.csv`` the groups."""
    grid: tuple[int, int] | None = None
    """(gh, gw); None takes the square grid of the image's tokens."""
    group_col: str | None = None
    """Column of ``image_labels.csv`` whose labels group the images; None puts all images in one group."""
    grouping: LabelGrouping | None = None
    """A grouping of labels (its ``source_col`` is the column) instead of ``group_col``'s own labels."""
    threshold: float = 0.0
    """An activation fires when it is > threshold."""
    map_latents: int | tuple[int, ...] = 256
    """The latents whose maps are kept: a list of ids, or the K most position-consistent ones."""
    min_images: int = 8
    """With an integer ``map_latents``, only pairs that fire in at least this many images compete."""


def spatial_fpath(cfg: Config) -> pathlib.Path:
    return pathlib.Path(cfg.run) / "inference" / pathlib.Path(cfg.shards).name / "latent_spatial.npz"


def image_groups(cfg: Config, n_images: int) -> tuple[np.ndarray, list[str]]:
    """(group id per image int32 with -1 for an image left out, the group names)."""
    if cfg.group_col is None and cfg.grouping is None:
        return np.zeros(n_images, dtype=np.int32), ["all"]
    task = cfg.grouping if cfg.grouping is not None else LabelGrouping(name=cfg.group_col, source_col=cfg.group_col)
    _, labels_by_col = load_image_labels(pathlib.Path(cfg.shards))
    if task.source_col not in labels_by_col:
        raise ValueError(f"column '{task.source_col}' is not in image_labels.csv (it has {sorted(labels_by_col)})")
    targets, names, _ = apply_grouping(labels_by_col[task.source_col], task)
    if len(targets) != n_images:
        raise ValueError(f"image_labels.csv names {len(targets)} images, token_acts.npz holds {n_images}")
    if len(names) > MAX_GROUPS:
        raise ValueError(f"'{task.source_col}' makes {len(names)} groups; at most {MAX_GROUPS} are scored in one call (give a grouping)")
    return targets.astype(np.int32), list(names)


def _latents_per_call(n_groups: int, T: int) -> int:
    """Latents a call may take: S * G * T below 2^31, and a count map of at most 1 GiB."""
    return max(1, min((2**31 - 1) // (n_groups * T), 2**28 // (n_groups * T)))


def compute(ta: scipy.sparse.csr_matrix, groups: np.ndarray, n_groups: int, grid, *, threshold: float = 0.0, map_latents=256, min_images: int = 8,
            device=None) -> dict[str, np.ndarray]:
    """The arrays of ``latent_spatial.npz`` but the group names, from the token activations of ``len(groups)`` images."""
    gh, gw = grid
    T, n_images, S = gh * gw, len(groups), ta.shape[1]
    if ta.shape[0] != n_images * T:
        raise ValueError(f"token_acts has {ta.shape[0]} rows, {n_images} images of {gh} x {gw} tokens are {n_images * T}")
    dev = classification._device(device)
    g_dev = torch.from_numpy(np.ascontiguousarray(groups, dtype=np.int32)).to(dev)
    ta = scipy.sparse.csr_matrix(ta)
    step = _latents_per_call(n_groups, T)
    ints = {k: np.zeros((S, n_groups), dtype=np.int64) for k in INTEGERS}
    moments = np.zeros((S, n_groups, 5), dtype=np.float64)
    n_group_images = None
    for lo in range(0, S, step):
        hi = min(lo + step, S)
        part = ta if (lo, hi) == (0, S) else ta[:, lo:hi]
        res = engine.latent_spatial(*classification._csr_on(part, dev), n_images=n_images, grid=grid, n_latents=hi - lo, groups=g_dev, n_groups=n_groups,
                                    threshold=threshold, sum_map=False)
        for k in INTEGERS:
            ints[k][lo:hi] = _np(getattr(res, k))
        moments[lo:hi] = _np(res.moments)
        n_group_images = _np(res.n_group_images)
    out = dict(ints, moments=moments, **scores_of(ints, moments, grid))
    if isinstance(map_latents, (int, np.integer)):
        chosen = choose_map_latents(out["position_consistency"], ints["n_images_fire"], int(map_latents), min_images)
    else:
        chosen = np.asarray(list(map_latents), dtype=np.int64)
        if chosen.size and (chosen.min() < 0 or chosen.max() >= S):
            raise ValueError(f"map_latents must lie in [0, {S})")
    count = np.zeros((len(chosen), n_groups, gh, gw), dtype=np.int32)
    mean = np.zeros((len(chosen), n_groups, gh, gw), dtype=np.float64)
    step = max(1, _latents_per_call(n_groups, T) // 3)  # the float64 map is twice the count map
    for lo in range(0, len(chosen), step):  # a latent scored alone has the bits it has among others
        sel = chosen[lo:lo + step]
        res = engine.latent_spatial(*classification._csr_on(ta[:, sel], dev), n_images=n_images, grid=grid, n_latents=len(sel), groups=g_dev,
                                    n_groups=n_groups, threshold=threshold, sum_map=True)
        count[lo:lo + len(sel)] = _np(res.count_map)
        mean[lo:lo + len(sel)] = mean_map(res.sum_map, res.n_group_images)
    out.update(n_group_images=n_group_images, grid=np.asarray(grid, dtype=np.int64), map_latents=chosen, count_map=count, mean_map=mean)
    return out


def worker_fn(cfg: Config) -> pathlib.Path:
    """Score every latent of a run and write ``latent_spatial.npz`` (keys ``KEYS``) beside its ``token_acts.npz``; returns its path."""
    fpath = spatial_fpath(cfg)
    ta = scipy.sparse.load_npz(str(fpath.parent / "token_acts.npz")).tocsr()
    T = saev_data.Metadata.load(pathlib.Path(cfg.shards)).content_tokens_per_example
    grid = infer_grid(T, cfg.grid)
    if ta.shape[0] % T:
        raise ValueError(f"token_acts.npz has {ta.shape[0]} rows, no whole number of images of {T} tokens")
    groups, names = image_groups(cfg, ta.shape[0] // T)
    out = compute(ta, groups, len(names), grid, threshold=cfg.threshold, map_latents=cfg.map_latents, min_images=cfg.min_images)
    out["group_names"] = np.asarray(names, dtype=str)
    np.savez(fpath, **{k: out[k] for k in KEYS})
    logger.info("Wrote the spatial scores of %d latents in %d groups (maps of %d) to '%s'.", ta.shape[1], len(names), len(out["map_latents"]), fpath)
    return fpath
