"""Per-latent thresholds chosen per task: the best operating point of every latent on every binary task, over
``engine.latent_auroc`` and ``engine.latent_operating`` (include/saev_amd.h: LATENT OPERATING POINTS).

The reference's ``contrib/mimics`` logbook asks three things of a good latent: it discriminates a mimic pair (``latent_auroc``), it
has "high precision and recall ... for some threshold" (this module), and it is spatially coherent (``saev_amd.spatial``).  For every
(task, latent) the rule "activation >= theta => positive" is scored at EVERY distinct activation value and the best F1 and the best
Youden J are kept with their thresholds and confusion counts -- exactly, on integers.

  level="image"   the mimic-pair tasks of ``mimics.build_task_specs`` on the max-pooled image codes (``mimics.max_pool_csr``'s values)
  level="token"   every segmentation class of ``labels.bin`` against the rest, on the token codes (``classification``'s columns)

``worker_fn`` writes ``latent_operating.npz`` (keys ``KEYS``, per-pair arrays (n_tasks, d_sae)) beside ``token_acts.npz``;
``thresholds`` hands a task's thresholds to the consumers that compare strictly (``a > thr``); ``scorecard`` joins AUROC, the operating
points and, when given, the spatial scores into one table with a pass flag per criterion.  There is no CPU path: without a HIP device
everything that computes raises."""

from __future__ import annotations

import dataclasses
import logging
import pathlib

import numpy as np
import scipy.sparse
import torch

from . import classification, engine, mimics
from . import data as saev_data
from .classification import load_image_labels

logger = logging.getLogger(__name__)

NPZ_FNAME = "latent_operating.npz"
PAIRS = engine.LatentOperatingResult.PAIRS
KEYS = ("level", "task", "n_pos", "n_neg") + PAIRS + ("auroc", "fire_pos", "fire_neg")
LEVELS = ("image", "token")


@dataclasses.dataclass(frozen=True)
class Config:
    run_root_dpath: pathlib.Path = pathlib.Path("./runs")
    """Root directory containing SAE run folders."""
    shards_dpath: pathlib.Path = pathlib.Path("./shards/01234567")
    """Shards directory: ``image_labels.csv`` for level "image", ``labels.bin`` for level "token"."""
    run_ids: list[str] = dataclasses.field(default_factory=list)
    """Run IDs to score. Required."""
    level: str = "image"
    """"image": mimic-pair tasks on max-pooled codes; "token": one segmentation class against the rest on token codes."""
    pair_specs: list[tuple[str, str]] = dataclasses.field(default_factory=lambda: mimics.SCORING_PAIR_SPECS.copy())
    views: list[str] = dataclasses.field(default_factory=lambda: mimics.DEFAULT_VIEWS.copy())
    min_samples: int = 10
    """Level "image": minimum images per class to include a task."""
    ignore_label_ids: tuple[int, ...] = (0,)
    """Level "token": labels that are no class of their own; their rows are left out of every task."""
    ignored_as_negative: bool = False
    """Level "token": the rows with an ignored label are negatives of every task instead."""
    force_recompute: bool = False


def operating_fpath(run_root_dpath: pathlib.Path, *, run_id: str, shard_id: str) -> pathlib.Path:
    return pathlib.Path(run_root_dpath) / run_id / "inference" / shard_id / NPZ_FNAME


def compute(x_csr, cls: np.ndarray, roles: np.ndarray, *, device=None) -> dict[str, np.ndarray]:
    """The per-pair arrays of ``latent_operating.npz`` with ``n_pos`` and ``n_neg``, each (n_tasks, d_sae) or (n_tasks): x (rows, d_sae)
    scipy CSR, ``cls`` one class per row (-1: none), ``roles`` (n_tasks, n_classes) uint8.  One ``latent_auroc`` call sorts the
    events; ``latent_operating`` walks them again out of the same workspace."""
    dev = classification._device(device)
    n, s = x_csr.shape
    roles = np.ascontiguousarray(roles, dtype=np.uint8)
    args = (*classification._csr_on(x_csr, dev), n, s, roles.shape[1])
    kw = dict(labels=torch.from_numpy(np.ascontiguousarray(cls, dtype=np.int32)).to(dev), roles=torch.from_numpy(roles).to(dev))
    ranked = engine.latent_auroc(*args, **kw)
    res = engine.latent_operating(*args, **kw, reuse=ranked)
    per_task = lambda x: np.ascontiguousarray(x.cpu().numpy().T)  # noqa: E731  (n_tasks, d_sae)
    out = {k: per_task(getattr(res, k)) for k in PAIRS}
    out.update(auroc=per_task(ranked.auroc), fire_pos=per_task(ranked.fire_pos), fire_neg=per_task(ranked.fire_neg),
               n_pos=res.n_pos.cpu().numpy(), n_neg=res.n_neg.cpu().numpy())
    return out


def _image_tasks(cfg: Config, shards_dpath: pathlib.Path):
    _, labels_by_col = load_image_labels(shards_dpath)
    assert mimics.SOURCE_COL in labels_by_col, f"'{mimics.SOURCE_COL}' missing in labels loaded from '{shards_dpath}'."
    sv = labels_by_col[mimics.SOURCE_COL]
    specs = mimics.build_task_specs(sv, pair_specs=list(cfg.pair_specs), views=list(cfg.views), min_samples=cfg.min_samples)
    assert specs, "No task to score."
    cls, roles = mimics.task_classes(specs, len(sv))
    return len(sv), [s.name for s in specs], cls, roles


def _token_tasks(cfg: Config, shards_dpath: pathlib.Path, ta):
    md = saev_data.Metadata.load(shards_dpath)
    n_rows = ta.shape[0]
    assert n_rows == md.n_examples * md.content_tokens_per_example, f"token_acts.npz has {n_rows} rows, the shards {md.n_examples} x {md.content_tokens_per_example}"
    labels = np.fromfile(shards_dpath / "labels.bin", dtype=np.uint8)
    assert labels.shape == (n_rows,), f"labels.bin holds {labels.shape[0]} labels, token_acts.npz {n_rows} rows"
    _, _, classes, remap, roles = classification._one_vs_rest(ta, labels, cfg.ignore_label_ids, cfg.ignored_as_negative)
    return [f"label_{c}" for c in classes.tolist()], remap[labels].astype(np.int32), roles


def score_run(run_id: str, cfg: Config) -> dict[str, np.ndarray] | None:
    """The arrays of ``latent_operating.npz`` of one run, computed and written unless the file is there already (and holds
    ``cfg.level``) and ``force_recompute`` is off; None when ``token_acts.npz`` is missing."""
    assert cfg.level in LEVELS, f"level must be one of {LEVELS}, got '{cfg.level}'"
    shards_dpath = pathlib.Path(cfg.shards_dpath).expanduser()
    fpath = operating_fpath(pathlib.Path(cfg.run_root_dpath), run_id=run_id, shard_id=shards_dpath.name)
    if fpath.exists() and not cfg.force_recompute:
        with np.load(fpath) as z:
            if str(z["level"]) == cfg.level:
                logger.info("Cached: '%s'.", fpath)
                return {k: z[k] for k in KEYS}
    ta_fpath = fpath.parent / "token_acts.npz"
    if not ta_fpath.exists():
        logger.warning("Missing token_acts: '%s'.", ta_fpath)
        return None
    ta = scipy.sparse.load_npz(str(ta_fpath)).tocsr()
    if cfg.level == "image":
        n_images, names, cls, roles = _image_tasks(cfg, shards_dpath)
        tpi = ta.shape[0] // n_images
        x = mimics.max_pool_sparse(ta, n_images, tpi)
    else:
        names, cls, roles = _token_tasks(cfg, shards_dpath, ta)
        x = ta
    assert roles.shape[1] <= 4096 and len(names) <= 4096, f"{roles.shape[1]} classes, {len(names)} tasks; at most 4096 of either are supported"
    out = dict(compute(x, cls, roles), level=np.asarray(cfg.level), task=np.asarray(names, dtype=str))
    np.savez(fpath, **{k: out[k] for k in KEYS})
    logger.info("Wrote the operating points of %d latents on %d tasks to '%s'.", x.shape[1], len(names), fpath)
    return {k: out[k] for k in KEYS}


def worker_fn(cfg: Config) -> None:
    """Score all latents on all tasks across several runs; one ``latent_operating.npz`` per run."""
    logging.basicConfig(level=logging.INFO, format="[%(asctime)s] [%(levelname)s] [%(name)s] %(message)s", force=True)
    assert cfg.run_ids, "Provide at least one run id."
    assert pathlib.Path(cfg.shards_dpath).expanduser().is_dir(), f"Shards missing: '{cfg.shards_dpath}'."
    for i, run_id in enumerate(cfg.run_ids, start=1):
        logger.info("[%d/%d] Operating points of run '%s'.", i, len(cfg.run_ids), run_id)
        score_run(run_id, cfg)


# ---------------------------------------------------------------- readers -----------------------------------------------------------------

def _load(source) -> dict[str, np.ndarray]:
    if isinstance(source, dict):
        return source
    with np.load(source) as z:
        return {k: z[k] for k in z.files}


def _task_index(z: dict, task) -> int:
    if isinstance(task, (int, np.integer)):
        return int(task)
    names = z["task"].tolist()
    if task not in names:
        raise ValueError(f"task '{task}' is not in the file (it has {names})")
    return names.index(task)


def strict(theta: np.ndarray) -> np.ndarray:
    """The thresholds of "a >= theta" in the strict form "a > thr": the next float32 below theta; +Inf (predict nothing) stays +Inf.
    An infinite event value that wins has no strict form: theta = -Inf stays -Inf, and ``a > thr`` then misses the rows AT -Inf;
    theta = +Inf with predicted rows stays +Inf and predicts none."""
    theta = np.asarray(theta, dtype=np.float32)
    return np.where(np.isposinf(theta), theta, np.nextafter(theta, np.float32(-np.inf))).astype(np.float32)


def thresholds(path, task, which: str = "f1") -> np.ndarray:
    """(d_sae) float32: the chosen threshold of every latent for ``task`` (a name of the file's ``task``, or its index), in the
    STRICT form the library's consumers compare with (``a > thr``): ready for ``coactivation_match(thr_a=...)``,
    ``ClassFireCounts(thresholds=...)`` and their like.  ``which``: "f1" or "j"."""
    if which not in ("f1", "j"):
        raise ValueError(f"which must be 'f1' or 'j', got '{which}'")
    z = _load(path)
    return strict(z[f"{which}_thr"][_task_index(z, task)])


def _ratio(num, den):
    num, den = np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64)
    return np.divide(num, den, out=np.full(np.broadcast(num, den).shape, np.nan), where=den > 0)


def scorecard(operating_file, auroc=None, spatial_file=None, *, min_auroc: float = 0.8, min_f1: float = 0.8, min_consistency: float = 0.5) -> dict[str, np.ndarray]:
    """One row per (task, latent), task-major, as a dict of columns: ``task``, ``feature_id``, ``auroc``, ``f1``, ``f1_thr``,
    ``precision``, ``recall`` (at ``f1_thr``), ``youden``, ``j_thr``, ``tpr``, ``fpr`` (at ``j_thr``), ``fire_rate_pos`` and
    ``fire_rate_neg`` (the share of the task's positives / negatives with activation > 0); with a ``latent_spatial.npz``
    ``position_consistency`` and ``clustering`` (the latent's largest over the file's groups).  ``auroc``: None takes the operating
    file's own, else a (n_tasks, d_sae) array or a ``cambridge-mimics.npz`` with the same tasks.  The logbook's three criteria as
    flags: ``pass_discriminative`` (auroc >= min_auroc), ``pass_operating`` (f1 >= min_f1), ``pass_spatial`` (position consistency >=
    min_consistency; absent without a spatial file) and ``pass_all``.  A plain table: nothing is rendered."""
    z = _load(operating_file)
    n_tasks, s = z["f1"].shape
    if auroc is None:
        au = z["auroc"]
    elif isinstance(auroc, np.ndarray):
        au = auroc
    else:
        m = _load(auroc)
        names = m["task"].reshape(n_tasks, s)[:, 0].tolist()
        if names != z["task"].tolist():
            raise ValueError(f"the AUROC file scores the tasks {names}, the operating file {z['task'].tolist()}")
        au = m["auroc"].reshape(n_tasks, s)
    if au.shape != (n_tasks, s):
        raise ValueError(f"auroc must be (n_tasks, d_sae) = {(n_tasks, s)}, got {au.shape}")
    flat = lambda x: np.ascontiguousarray(x).reshape(-1)  # noqa: E731
    n_pos, n_neg = z["n_pos"][:, None], z["n_neg"][:, None]
    cols = {
        "task": np.repeat(z["task"], s), "feature_id": np.tile(np.arange(s, dtype=np.int32), n_tasks), "auroc": flat(au.astype(np.float64)),
        "f1": flat(z["f1"]), "f1_thr": flat(z["f1_thr"]), "precision": flat(_ratio(z["f1_tp"], z["f1_tp"] + z["f1_fp"])),
        "recall": flat(_ratio(z["f1_tp"], n_pos)), "youden": flat(z["youden"]), "j_thr": flat(z["j_thr"]), "tpr": flat(_ratio(z["j_tp"], n_pos)),
        "fpr": flat(_ratio(z["j_fp"], n_neg)), "fire_rate_pos": flat(_ratio(z["fire_pos"], n_pos)), "fire_rate_neg": flat(_ratio(z["fire_neg"], n_neg)),
    }
    with np.errstate(invalid="ignore"):
        cols["pass_discriminative"] = cols["auroc"] >= min_auroc
        cols["pass_operating"] = cols["f1"] >= min_f1
        cols["pass_all"] = cols["pass_discriminative"] & cols["pass_operating"]
        if spatial_file is not None:
            sp = _load(spatial_file)
            for key in ("position_consistency", "clustering"):
                v = np.asarray(sp[key], dtype=np.float64)
                if v.shape[0] != s:
                    raise ValueError(f"the spatial file scores {v.shape[0]} latents, the operating file {s}")
                best = np.where(np.isnan(v).all(axis=1), np.nan, np.nanmax(np.where(np.isnan(v), -np.inf, v), axis=1))
                cols[key] = np.tile(best, n_tasks)
            cols["pass_spatial"] = cols["position_consistency"] >= min_consistency
            cols["pass_all"] = cols["pass_all"] & cols["pass_spatial"]
    return cols
