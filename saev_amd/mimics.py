"""Latent-level scoring for mimic-pair feature triage: the reference's ``contrib/mimics`` ``mimics.tasks`` and ``mimics.scoring`` over
``engine.pool_csr`` and ``engine.latent_auroc`` (include/saev_amd.h: POOL CSR, LATENT AUROC), without polars.

Every SAE latent is scored on every mimic-pair task -- one subspecies of H. erato against its co-mimic of H. melpomene, in one view
-- by AUROC, the share of each class's images on which it fires, and its mean activation per class.  The token codes of
``token_acts.npz`` are max-pooled to images on the device, the pooled matrix's non-zero entries become a CSR there, the labels any
task uses become class ids, and ONE ``latent_auroc`` call scores all tasks: exact and tie-aware (what ``scipy.stats.rankdata``'s
average ranks give the reference), with no dense rank matrix.  The positives are "melpomene", as in the reference.

The frames of the reference are dicts of numpy columns (``score_run``) and lists of row dicts (``decide_task_specs``).  ``score_run``
always writes ``cambridge-mimics.npz`` beside ``token_acts.npz``; the reference's ``cambridge-mimics.parquet`` is written as well
when ``pyarrow`` imports.  There is no CPU path: without a HIP device everything that computes raises."""

from __future__ import annotations

import dataclasses
import logging
import pathlib
import re

import numpy as np
import scipy.sparse
import torch

from . import classification, engine
from .classification import LabelGrouping, apply_grouping, load_image_labels

logger = logging.getLogger(__name__)

# ---------------------------------------------------------------- mimics.tasks ------------------------------------------------------------

DEFAULT_PAIR_SPECS = ["lativitta:malleti", "cyrbia:cythera", "notabilis:plesseni", "hydara:melpomene", "venus:vulcanus", "demophoon:rosina",
                      "phyllis:nanna", "erato:thelxiopeia"]
DEFAULT_VIEWS = ["dorsal", "ventral"]
TASK_NAME_RE = re.compile(r"^(?P<erato>[a-zA-Z0-9]+)_(?P<view_a>[a-zA-Z0-9]+)_vs_(?P<melp>[a-zA-Z0-9]+)_(?P<view_b>[a-zA-Z0-9]+)$")
SOURCE_COL = "subspecies_view"


@dataclasses.dataclass(frozen=True)
class DecidedTaskSpec:
    """A candidate task of ``decide_task_specs`` (the reference's ``mimics.tasks.TaskSpec``)."""

    task_name: str
    source_col: str
    groups: dict[str, list[str]]
    n_erato: int
    n_melpomene: int
    n_total: int
    keep: bool


@dataclasses.dataclass(frozen=True)
class DecideTaskSpecsConfig:
    shards_dpath: pathlib.Path = pathlib.Path("/fs/scratch/PAS2136/samuelstevens/saev/shards/79239bdd")
    pair_specs: list[str] = dataclasses.field(default_factory=lambda: DEFAULT_PAIR_SPECS.copy())
    views: list[str] = dataclasses.field(default_factory=lambda: DEFAULT_VIEWS.copy())
    task_names: list[str] = dataclasses.field(default_factory=list)
    min_samples_per_class: int = 50
    include_filtered: bool = False


def parse_pair_spec(pair_spec: str) -> tuple[str, str]:
    erato_ssp, sep, melp_ssp = pair_spec.partition(":")
    assert sep == ":", f"Pair spec must look like 'erato_ssp:melp_ssp', got '{pair_spec}'."
    erato_ssp, melp_ssp = erato_ssp.strip(), melp_ssp.strip()
    assert erato_ssp and melp_ssp, f"Pair spec has empty side: '{pair_spec}'."
    return erato_ssp, melp_ssp


def get_task_name(erato_ssp: str, melp_ssp: str, view: str) -> str:
    return f"{erato_ssp}_{view}_vs_{melp_ssp}_{view}"


def parse_task_name(task_name: str) -> tuple[str, str, str]:
    match = TASK_NAME_RE.fullmatch(task_name)
    assert match is not None, f"Task must match '{{erato_ssp}}_{{view}}_vs_{{melp_ssp}}_{{view}}', got '{task_name}'."
    view_a, view_b = match.group("view_a"), match.group("view_b")
    assert view_a == view_b, f"Task has mismatched views: '{view_a}' vs '{view_b}'."
    return match.group("erato"), match.group("melp"), view_a


def make_label_grouping(task_name: str) -> LabelGrouping:
    erato_ssp, melp_ssp, view = parse_task_name(task_name)
    return LabelGrouping(name=task_name, source_col=SOURCE_COL, groups={"erato": [f"{erato_ssp}_{view}"], "melpomene": [f"{melp_ssp}_{view}"]})


def _candidate_task_names(cfg: DecideTaskSpecsConfig) -> list[str]:
    names = list(cfg.task_names)
    if not names:
        for pair_spec in cfg.pair_specs:
            erato_ssp, melp_ssp = parse_pair_spec(pair_spec)
            names += [get_task_name(erato_ssp, melp_ssp, view) for view in cfg.views]
    return list(dict.fromkeys(names))


def decide_task_specs(cfg: DecideTaskSpecsConfig) -> tuple[list[DecidedTaskSpec], list[dict]]:
    """(the tasks to keep -- or all with ``include_filtered`` --, the summary): one row dict per candidate with the reference's
    columns, sorted as the reference sorts its frame: kept first, then by ``n_total`` descending, then by ``task_name``."""
    shards_dpath = pathlib.Path(cfg.shards_dpath).expanduser()
    assert shards_dpath.is_dir(), f"Shards directory missing: '{shards_dpath}'."
    _, labels_by_col = load_image_labels(shards_dpath)
    assert SOURCE_COL in labels_by_col, f"'{SOURCE_COL}' missing in labels loaded from '{shards_dpath}'."
    sv = labels_by_col[SOURCE_COL]
    task_names = _candidate_task_names(cfg)
    assert task_names, "No task candidates. Set task_names or pair_specs."
    specs, rows = [], []
    for task_name in task_names:
        grouping = make_label_grouping(task_name)
        targets, class_names, include = apply_grouping(sv, grouping)
        c2i = {name: i for i, name in enumerate(class_names)}
        n_erato = int((targets[include] == c2i["erato"]).sum())
        n_melpomene = int((targets[include] == c2i["melpomene"]).sum())
        spec = DecidedTaskSpec(task_name=task_name, source_col=grouping.source_col, groups=grouping.groups, n_erato=n_erato, n_melpomene=n_melpomene,
                               n_total=n_erato + n_melpomene, keep=min(n_erato, n_melpomene) >= cfg.min_samples_per_class)
        rows.append({"task_name": spec.task_name, "n_erato": spec.n_erato, "n_melpomene": spec.n_melpomene, "n_total": spec.n_total, "keep": spec.keep,
                     "source_col": spec.source_col, "erato_label": spec.groups["erato"][0], "melpomene_label": spec.groups["melpomene"][0]})
        if spec.keep or cfg.include_filtered:
            specs.append(spec)
    rows.sort(key=lambda r: (not r["keep"], -r["n_total"], r["task_name"]))
    return specs, rows


# ---------------------------------------------------------------- mimics.scoring ----------------------------------------------------------

SCORING_PAIR_SPECS: list[tuple[str, str]] = [("lativitta", "malleti"), ("cyrbia", "cythera"), ("notabilis", "plesseni"), ("hydara", "melpomene"),
                                             ("venus", "vulcanus")]
COLUMNS = ("run_id", "task", "feature_id", "auroc", "support_erato", "support_melpomene", "mean_act_erato", "mean_act_melpomene")
NPZ_FNAME, PARQUET_FNAME = "cambridge-mimics.npz", "cambridge-mimics.parquet"


@dataclasses.dataclass(frozen=True)
class Config:
    """Score all SAE latents for mimic pair discrimination: the reference's fields and defaults (the Slurm fields are accepted and
    unused; ``feature_chunk`` bounded the reference's dense rank matrix and is unused as well)."""

    run_root_dpath: pathlib.Path = pathlib.Path("/fs/ess/PAS2136/samuelstevens/saev/runs")
    """Root directory containing SAE run folders."""
    shards_dpath: pathlib.Path = pathlib.Path("/fs/scratch/PAS2136/samuelstevens/saev/shards/a6be28a1")
    """Shards directory used for labels."""
    run_ids: list[str] = dataclasses.field(default_factory=list)
    """Run IDs to score. Required."""
    pair_specs: list[tuple[str, str]] = dataclasses.field(default_factory=lambda: SCORING_PAIR_SPECS.copy())
    """(erato_ssp, melp_ssp) pairs."""
    views: list[str] = dataclasses.field(default_factory=lambda: DEFAULT_VIEWS.copy())
    """Views to score."""
    min_samples: int = 10
    """Minimum images per class to include a task."""
    feature_chunk: int = 1024
    force_recompute: bool = False
    """If True, recompute even when the scores already exist."""
    slurm_acct: str = ""
    slurm_partition: str = ""
    n_hours: float = 4.0
    mem_gb: int = 80
    log_to: str = "logs"


@dataclasses.dataclass(frozen=True)
class TaskSpec:
    """A scoring task, the reference's fields: ``include`` over all images, the masks and ``binary`` over the included ones."""

    name: str
    include: np.ndarray
    erato_mask: np.ndarray
    melp_mask: np.ndarray
    binary: np.ndarray
    n_pos: int
    n_neg: int


def build_task_specs(sv: list[str], *, pair_specs: list[tuple[str, str]], views: list[str], min_samples: int) -> list[TaskSpec]:
    specs = []
    for e, m in pair_specs:
        for v in views:
            task_name = get_task_name(e, m, v)
            targets, names, include = apply_grouping(sv, make_label_grouping(task_name))
            c2i = {name: i for i, name in enumerate(names)}
            inc_tgt = targets[include]
            em, mm = inc_tgt == c2i["erato"], inc_tgt == c2i["melpomene"]
            if em.sum() < min_samples or mm.sum() < min_samples:
                continue
            specs.append(TaskSpec(name=task_name, include=include, erato_mask=em, melp_mask=mm, binary=mm.astype(np.int8), n_pos=int(mm.sum()),
                                  n_neg=int(em.sum())))
    return specs


def _pool_on_device(ta_csr, n_images: int, tpi: int, dev) -> torch.Tensor:
    """The reference's ``max_pool_csr`` on the device: the pooled maximum CLAMPED AT 0, for the reference starts from zeros (a latent
    stored in every patch of an image with negative values only pools to 0 there, not to its negative maximum)."""
    pooled = engine.pool_images(*classification._csr_on(ta_csr, dev), n_images, tpi, ta_csr.shape[1], "max").pooled
    return torch.clamp_min(pooled, 0.0)


def max_pool_csr(ta_csr, n_images: int, tpi: int, device=None) -> np.ndarray:
    """Max-pool token-level sparse activations to image-level: (n_images, d_sae) float32, the reference's values."""
    assert ta_csr.shape[0] == n_images * tpi, f"{ta_csr.shape[0]} != {n_images} * {tpi}"
    return _pool_on_device(ta_csr, n_images, tpi, classification._device(device)).cpu().numpy()


def _pool_sparse_on_device(ta_csr, n_images: int, tpi: int, dev):
    """The image-level CSR triple of ``max_pool_csr``'s non-zero entries on the device, pooled in sparse form (``engine.pool_csr`` at
    threshold 0: the positive maxima, for the reference's pooling starts from zeros); never an (n_images, d_sae) matrix."""
    return engine.pool_csr(*classification._csr_on(ta_csr, dev), n_images, tpi, ta_csr.shape[1]).triple()


def max_pool_sparse(ta_csr, n_images: int, tpi: int, device=None) -> scipy.sparse.csr_matrix:
    """``scipy.sparse.csr_matrix(max_pool_csr(...))`` without the dense matrix: (n_images, d_sae) float32 CSR with sorted columns."""
    assert ta_csr.shape[0] == n_images * tpi, f"{ta_csr.shape[0]} != {n_images} * {tpi}"
    indptr, indices, data = _pool_sparse_on_device(ta_csr, n_images, tpi, classification._device(device))
    return scipy.sparse.csr_matrix((data.cpu().numpy(), indices.cpu().numpy(), indptr.cpu().numpy()), shape=(n_images, ta_csr.shape[1]))


def get_scores_fpath(run_root_dpath: pathlib.Path, *, run_id: str, shard_id: str) -> pathlib.Path:
    return pathlib.Path(run_root_dpath) / run_id / "inference" / shard_id / PARQUET_FNAME


def task_classes(task_specs: list[TaskSpec], n_images: int) -> tuple[np.ndarray, np.ndarray]:
    """(class id per image int32, roles (n_tasks, n_classes) uint8) of a list of tasks: the images with the same role in every task
    (0 = left out, 1 = erato, the negatives, 2 = melpomene, the positives) form a class -- for mimic-pair tasks one class per label that
    any task uses --, and an image that no task includes has class -1."""
    pattern = np.zeros((n_images, len(task_specs)), dtype=np.uint8)
    for t, spec in enumerate(task_specs):
        at = np.flatnonzero(spec.include)
        pattern[at[spec.erato_mask], t] = 1
        pattern[at[spec.melp_mask], t] = 2
    used = pattern.any(axis=1)
    cls = np.full(n_images, -1, dtype=np.int32)
    if not used.any():
        return cls, np.zeros((len(task_specs), 1), dtype=np.uint8)
    patterns, inverse = np.unique(pattern[used], axis=0, return_inverse=True)
    cls[used] = inverse.reshape(-1).astype(np.int32)
    return cls, np.ascontiguousarray(patterns.T)


def _write_parquet(columns: dict, fpath: pathlib.Path) -> bool:
    try:
        import pyarrow
        import pyarrow.parquet
    except ImportError:
        logger.info("pyarrow is not installed: '%s' is not written (the scores are in '%s').", fpath, NPZ_FNAME)
        return False
    pyarrow.parquet.write_table(pyarrow.table({k: pyarrow.array(v.tolist() if v.dtype.kind == "U" else v) for k, v in columns.items()}), fpath)
    return True


def score_run(run_id: str, *, run_root_dpath: pathlib.Path, shard_id: str, task_specs: list[TaskSpec], n_images: int, feature_chunk: int = 1024,
              force_recompute: bool = False, device=None) -> dict[str, np.ndarray] | None:
    """The reference's columns for every (task, latent), as numpy arrays with the reference's dtypes: ``run_id`` and ``task``
    (strings), ``feature_id`` int32, and float32 ``auroc``, ``support_erato``, ``support_melpomene``, ``mean_act_erato``,
    ``mean_act_melpomene``, task-major as the reference concatenates them.  Cached in ``cambridge-mimics.npz`` beside ``token_acts.npz`` unless ``force_recompute``;
    None when ``token_acts.npz`` is missing.  support = fire / n; mean = sum / n in float64, then cast to float32."""
    inference_dpath = pathlib.Path(run_root_dpath) / run_id / "inference" / shard_id
    npz_fpath = inference_dpath / NPZ_FNAME
    if npz_fpath.exists() and not force_recompute:
        logger.info("Cached: '%s'.", npz_fpath)
        with np.load(npz_fpath) as z:
            return {k: z[k] for k in COLUMNS}
    ta_fpath = inference_dpath / "token_acts.npz"
    if not ta_fpath.exists():
        logger.warning("Missing token_acts: '%s'.", ta_fpath)
        return None
    assert task_specs, "No task to score."
    ta = scipy.sparse.load_npz(str(ta_fpath)).tocsr()
    d_sae = ta.shape[1]
    tpi = ta.shape[0] // n_images
    assert ta.shape[0] == n_images * tpi, f"{ta.shape[0]} != {n_images} * {tpi}"
    dev = classification._device(device)

    logger.info("Max-pooling %s (shape %s, tpi=%d).", run_id, ta.shape, tpi)
    # the non-zero pooled entries as CSR, on the device (ascending columns inside ascending rows)
    indptr, indices, data = _pool_sparse_on_device(ta, n_images, tpi, dev)
    del ta

    cls, roles = task_classes(task_specs, n_images)
    assert roles.shape[1] <= 4096, f"{roles.shape[1]} classes of images; at most 4096 are supported"
    res = engine.latent_auroc(indptr, indices, data, n_images, d_sae, roles.shape[1], labels=torch.from_numpy(cls).to(dev),
                              roles=torch.from_numpy(roles).to(dev))
    n_pos, n_neg = res.n_pos.cpu().numpy(), res.n_neg.cpu().numpy()
    for t, spec in enumerate(task_specs):
        assert (n_pos[t], n_neg[t]) == (spec.n_pos, spec.n_neg), f"task {spec.name}: {n_pos[t]} / {n_neg[t]} images, the spec has {spec.n_pos} / {spec.n_neg}"
    per_task = lambda x: x.cpu().numpy().T  # noqa: E731  (n_tasks, d_sae)
    n_tasks = len(task_specs)
    f32 = lambda x: np.ascontiguousarray(x, dtype=np.float32).reshape(-1)  # noqa: E731
    with np.errstate(divide="ignore", invalid="ignore"):
        columns = {
            "run_id": np.full(n_tasks * d_sae, run_id),
            "task": np.repeat(np.asarray([spec.name for spec in task_specs]), d_sae),
            "feature_id": np.tile(np.arange(d_sae, dtype=np.int32), n_tasks),
            "auroc": f32(per_task(res.auroc)),
            "support_erato": f32(per_task(res.fire_neg) / n_neg[:, None].astype(np.float64)),
            "support_melpomene": f32(per_task(res.fire_pos) / n_pos[:, None].astype(np.float64)),
            "mean_act_erato": f32(per_task(res.sum_neg) / n_neg[:, None].astype(np.float64)),
            "mean_act_melpomene": f32(per_task(res.sum_pos) / n_pos[:, None].astype(np.float64)),
        }
    np.savez(npz_fpath, **columns)
    pq_fpath = get_scores_fpath(pathlib.Path(run_root_dpath), run_id=run_id, shard_id=shard_id)
    if _write_parquet(columns, pq_fpath):
        logger.info("Wrote '%s'.", pq_fpath)
    logger.info("Wrote %d rows to '%s'.", n_tasks * d_sae, npz_fpath)
    return columns


def worker_fn(cfg: Config) -> None:
    """Score all latents for all tasks across several runs, as the reference's function of this name."""
    log_format = "[%(asctime)s] [%(levelname)s] [%(name)s] %(message)s"
    logging.basicConfig(level=logging.INFO, format=log_format, force=True)
    assert cfg.run_ids, "Provide at least one run id."
    shards_dpath = pathlib.Path(cfg.shards_dpath).expanduser()
    assert shards_dpath.is_dir(), f"Shards missing: '{shards_dpath}'."
    _, labels_by_col = load_image_labels(shards_dpath)
    assert SOURCE_COL in labels_by_col, f"'{SOURCE_COL}' missing in labels loaded from '{shards_dpath}'."
    sv = labels_by_col[SOURCE_COL]
    n_images, shard_id = len(sv), shards_dpath.name
    task_specs = build_task_specs(sv, pair_specs=list(cfg.pair_specs), views=list(cfg.views), min_samples=cfg.min_samples)
    logger.info("Built %d task specs from %d pairs x %d views.", len(task_specs), len(cfg.pair_specs), len(cfg.views))
    for i, run_id in enumerate(cfg.run_ids, start=1):
        logger.info("[%d/%d] Scoring run '%s'.", i, len(cfg.run_ids), run_id)
        score_run(run_id, run_root_dpath=pathlib.Path(cfg.run_root_dpath), shard_id=shard_id, task_specs=task_specs, n_images=n_images,
                  feature_chunk=cfg.feature_chunk, force_recompute=cfg.force_recompute)
    logger.info("Done scoring %d runs.", len(cfg.run_ids))
