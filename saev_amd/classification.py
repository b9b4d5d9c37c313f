"""The concept audit on sparse codes: the evaluation half of the reference's ``tdiscovery.classification`` (``compute_ap_for_latent``,
``compute_ap_batched``, ``extract_feature_ranking``, ``load_classifier_checkpoint``, ``EvalConfig``, ``eval_worker_fn``) over the HIP
kernels behind ``engine.latent_ap`` (include/saev_amd.h: LATENT AP).

The average precision of a latent's activation as a detector of each segmentation class is the exact tie-aware value of McSherry and
Najork (2008) -- the expectation over all orders of tied scores -- for every latent and every class, in one call on the device: the
stored entries are sorted once and each latent's zero rows enter as one tie group in closed form.  All sums are fp64 in a fixed
order (two runs give the same bits).  There is no CPU path: without a HIP device everything that computes raises.

The training half (``train_worker_fn``: ``PatchAgg``, ``LabelGrouping``, ``SparseLinear``, ``DecisionTree``, ``TrainConfig``,
``apply_grouping``, ``aggregate_to_images``, ``load_image_labels``) pools the token codes to one row per image with
``engine.pool_images`` and fits the L1-penalised logistic regression with ``engine.l1_logistic``: the reference's
problem solved to a certified optimum on the device, and written as the checkpoint ``eval_worker_fn`` reads."""

from __future__ import annotations

import csv
import dataclasses
import enum
import json
import logging
import pathlib
import pickle
import typing as tp

import numpy as np
import scipy.sparse
import torch

from . import data as saev_data
from . import disk
from . import engine


def _device(device=None) -> torch.device:
    if not torch.cuda.is_available():
        raise RuntimeError("saev_amd.classification runs on a HIP device only (there is no CPU path)")
    return torch.device(device if device is not None else "cuda")


def _csr_on(csr, dev):
    """(indptr int64, indices int32, data float32) of a scipy CSR matrix on the device, duplicates summed (more than one entry per
    (row, latent) is outside the kernels' contract)."""
    csr = scipy.sparse.csr_matrix(csr)
    if csr.dtype != np.float32:
        csr = csr.astype(np.float32)
    if not csr.has_canonical_format:
        csr = csr.copy()
        csr.sum_duplicates()
    parts = (csr.indptr.astype(np.int64), csr.indices.astype(np.int32), np.ascontiguousarray(csr.data))
    return tuple(torch.from_numpy(p).to(dev) for p in parts)


def _score(csr, cls_n: np.ndarray, n_classes: int, device=None) -> "engine.LatentAPResult":
    dev = _device(device)
    n, s = csr.shape
    return engine.latent_ap(*_csr_on(csr, dev), n, s, n_classes, labels=torch.from_numpy(np.ascontiguousarray(cls_n)).to(dev))


def _class_ids(labels_one_hot_nc: np.ndarray) -> np.ndarray:
    """One class per row (-1: none) from a 0/1 matrix with at most one 1 per row."""
    y = np.asarray(labels_one_hot_nc)
    if y.ndim != 2 or not np.isin(y, (0, 1)).all() or (y.sum(axis=1) > 1).any():
        raise ValueError("labels_one_hot_nc must be an (n_patches, n_seg_classes) 0/1 matrix with at most one 1 in each row.")
    return np.where(y.any(axis=1), y.argmax(axis=1), -1).astype(np.int32)


def compute_ap_batched(acts_nb: np.ndarray, labels_one_hot_nc: np.ndarray, n_pos_c: np.ndarray) -> np.ndarray:
    """AP (batch, n_seg_classes) float32 of a batch of dense latents against all segmentation classes.

    UNLIKE the reference's function of this name this is the TIE-AWARE value, the same as ``compute_ap_for_latent``.  The reference
    ranks tied scores in whatever order an unstable ``np.argsort`` leaves them; on sparse codes 95-99.9 % of a latent's rows are tied
    at zero, so its value depends on the numpy build (it differs from the tie-aware value by up to 0.02 AP on a latent that fires on a
    few per cent of the rows).  On a latent without ties the two agree to float32 rounding.  Each row of ``labels_one_hot_nc`` may
    hold at most one 1 (ValueError otherwise); ``n_pos_c`` must be its column sums."""
    acts_nb = np.asarray(acts_nb, dtype=np.float32)
    if acts_nb.ndim != 2 or acts_nb.shape[0] != np.asarray(labels_one_hot_nc).shape[0]:
        raise ValueError(f"acts_nb must be (n_patches, batch) with the labels' n_patches, got {acts_nb.shape}.")
    cls_n = _class_ids(labels_one_hot_nc)
    n_classes = np.asarray(labels_one_hot_nc).shape[1]
    res = _score(scipy.sparse.csr_matrix(acts_nb), cls_n, n_classes)
    if not (res.n_pos.cpu().numpy() == np.asarray(n_pos_c).astype(np.int64)).all():
        raise ValueError("n_pos_c does not hold the column sums of labels_one_hot_nc.")
    return res.ap.cpu().numpy().astype(np.float32)


def compute_ap_for_latent(acts_n: np.ndarray, labels_one_hot_nc: np.ndarray, n_pos_c: np.ndarray) -> np.ndarray:
    """Tie-aware AP (n_seg_classes) float32 of one dense latent against all segmentation classes (McSherry and Najork 2008), as the
    reference's function of this name; each row of ``labels_one_hot_nc`` may hold at most one 1 (ValueError otherwise)."""
    acts_n = np.asarray(acts_n, dtype=np.float32)
    if acts_n.ndim != 1:
        raise ValueError(f"acts_n must be a vector, got {acts_n.shape}.")
    return compute_ap_batched(acts_n[:, None], labels_one_hot_nc, n_pos_c)[0]


def _columns(labels_flat: np.ndarray, ignore_label_ids) -> tuple[np.ndarray, np.ndarray]:
    """(classes: the unique labels minus the ignored ones, ascending; remap: 256 int32, byte -> column or -1)."""
    unique = np.unique(labels_flat)
    classes = np.asarray([c for c in unique if c not in ignore_label_ids], dtype=np.int64)
    remap = np.full(256, -1, dtype=np.int32)
    remap[classes] = np.arange(len(classes), dtype=np.int32)
    return classes, remap


def _matrix_on_device(token_acts_csr, labels_flat, ignore_label_ids, device=None):
    labels_flat = np.ascontiguousarray(labels_flat)
    if labels_flat.dtype != np.uint8 or labels_flat.ndim != 1:
        raise ValueError(f"labels_flat must be a uint8 vector, got {labels_flat.dtype} {labels_flat.shape}.")
    csr = scipy.sparse.csr_matrix(token_acts_csr)
    if csr.shape[0] != labels_flat.shape[0]:
        raise ValueError(f"token_acts_csr has {csr.shape[0]} rows, labels_flat {labels_flat.shape[0]}.")
    classes, remap = _columns(labels_flat, tuple(ignore_label_ids))
    if len(classes) == 0:
        raise ValueError("every label is ignored: there is no class to score.")
    dev = _device(device)
    n, s = csr.shape
    res = engine.latent_ap(*_csr_on(csr, dev), n, s, len(classes), labels=torch.from_numpy(labels_flat).to(dev), remap=torch.from_numpy(remap).to(dev))
    return res, classes


def latent_ap_matrix(token_acts_csr, labels_flat: np.ndarray, *, ignore_label_ids=(0,)):
    """(ap_sc (d_sae, n_seg_classes) float64, classes (n_seg_classes) int64, n_pos_c (n_seg_classes) int64) of EVERY latent of a scipy
    CSR matrix (n_patches, d_sae) against the uint8 labels of its rows.  The unique labels minus ``ignore_label_ids`` become the
    columns in ascending order, as in the reference; a row with an ignored label belongs to no class and is still ranked."""
    res, classes = _matrix_on_device(token_acts_csr, labels_flat, ignore_label_ids)
    return res.ap.cpu().numpy(), classes, res.n_pos.cpu().numpy()


def _one_vs_rest(token_acts_csr, labels_flat, ignore_label_ids, ignored_as_negative):
    """(csr, labels_flat, classes, remap, roles) of the one-vs-rest tasks ``latent_auroc_matrix`` describes."""
    labels_flat = np.ascontiguousarray(labels_flat)
    if labels_flat.dtype != np.uint8 or labels_flat.ndim != 1:
        raise ValueError(f"labels_flat must be a uint8 vector, got {labels_flat.dtype} {labels_flat.shape}.")
    csr = scipy.sparse.csr_matrix(token_acts_csr)
    if csr.shape[0] != labels_flat.shape[0]:
        raise ValueError(f"token_acts_csr has {csr.shape[0]} rows, labels_flat {labels_flat.shape[0]}.")
    classes, remap = _columns(labels_flat, tuple(ignore_label_ids))
    n_tasks = len(classes)
    if n_tasks == 0:
        raise ValueError("every label is ignored: there is no class to score.")
    n_classes = n_tasks
    if ignored_as_negative and n_tasks < len(np.unique(labels_flat)):
        remap[np.setdiff1d(np.unique(labels_flat), classes)] = n_tasks
        n_classes = n_tasks + 1
    roles = np.ones((n_tasks, n_classes), dtype=np.uint8)
    roles[np.arange(n_tasks), np.arange(n_tasks)] = 2
    return csr, labels_flat, classes, remap, roles


def latent_auroc_matrix(token_acts_csr, labels_flat: np.ndarray, *, ignore_label_ids=(0,), ignored_as_negative: bool = False, device=None):
    """(auroc_sc (d_sae, n_seg_classes) float64, classes (n_seg_classes) int64, n_pos_c (n_seg_classes) int64): the exact tie-aware
    AUROC of EVERY latent against every segmentation class, one-vs-rest, over the columns of ``latent_ap_matrix`` -- threshold-free
    and, unlike AP, independent of the class's prevalence (``engine.latent_auroc``).  A row with an ignored label is
    left out of every task; with ``ignored_as_negative`` those rows form a class of their own that is negative in every task."""
    csr, labels_flat, classes, remap, roles = _one_vs_rest(token_acts_csr, labels_flat, ignore_label_ids, ignored_as_negative)
    n_classes = roles.shape[1]
    dev = _device(device)
    n, s = csr.shape
    res = engine.latent_auroc(*_csr_on(csr, dev), n, s, n_classes, labels=torch.from_numpy(labels_flat).to(dev), remap=torch.from_numpy(remap).to(dev),
                              roles=torch.from_numpy(roles).to(dev))
    return res.auroc.cpu().numpy(), classes, res.n_pos.cpu().numpy()


def latent_operating_matrix(token_acts_csr, labels_flat: np.ndarray, *, ignore_label_ids=(0,), ignored_as_negative: bool = False, device=None):
    """(points, classes (n_seg_classes) int64, n_pos_c, n_neg_c (n_seg_classes) int64): the best operating point of EVERY latent
    against every segmentation class, one-vs-rest, over the tasks of ``latent_auroc_matrix`` (``engine.latent_operating``; DESIGN.md
    3.29).  ``points`` is a dict of (d_sae, n_seg_classes) arrays: ``f1`` and ``youden`` float64, ``f1_thr`` and ``j_thr`` float32 (the
    rule is "activation >= threshold"; +Inf with no predicted row is "predict nothing"), ``f1_tp``, ``f1_fp``, ``j2``, ``j_tp``
    and ``j_fp`` int64, and ``precision_f1``, ``recall_f1``, ``tpr_j``, ``fpr_j`` float64."""
    csr, labels_flat, classes, remap, roles = _one_vs_rest(token_acts_csr, labels_flat, ignore_label_ids, ignored_as_negative)
    dev = _device(device)
    n, s = csr.shape
    res = engine.latent_operating(*_csr_on(csr, dev), n, s, roles.shape[1], labels=torch.from_numpy(labels_flat).to(dev), remap=torch.from_numpy(remap).to(dev),
                                  roles=torch.from_numpy(roles).to(dev))
    points = {k: getattr(res, k).cpu().numpy() for k in res.PAIRS + ("precision_f1", "recall_f1", "tpr_j", "fpr_j")}
    return points, classes, res.n_pos.cpu().numpy(), res.n_neg.cpu().numpy()


def extract_feature_ranking(classifier: object, cls_type: str) -> tuple[np.ndarray, np.ndarray]:
    """(ranked_indices by descending importance with a stable sort, importance_scores) of a trained classifier: the sum of |coef_|
    over classes for "sparse-linear", feature_importances_ for "decision-tree" (duck-typed)."""
    if cls_type == "sparse-linear":
        importance = np.abs(np.asarray(classifier.coef_)).sum(axis=0)
    elif cls_type == "decision-tree":
        importance = np.asarray(classifier.feature_importances_)
    else:
        raise ValueError(f"Unknown classifier type: {cls_type}")
    return np.argsort(-importance, kind="stable"), importance


def load_classifier_checkpoint(fpath: pathlib.Path, logger: logging.Logger) -> tuple[object, str, np.ndarray, np.ndarray]:
    """Load a classifier checkpoint (a JSON header line, then a pickle with key "classifier") and extract its feature ranking.  The
    payload is read with the standard library's pickle; a pickled sklearn estimator imports sklearn itself."""
    with open(fpath, "rb") as fd:
        header = json.loads(fd.readline())
        payload = pickle.load(fd)
    classifier = payload["classifier"]
    cls_type = header["cfg"]["cls"]["key"]
    ranked_i, importance = extract_feature_ranking(classifier, cls_type)
    logger.debug("Loaded %s from %s", cls_type, pathlib.Path(fpath).name)
    return classifier, cls_type, ranked_i, importance


@dataclasses.dataclass(frozen=True)
class EvalConfig:
    """Configuration of the audit stage, the reference's fields and defaults (the Slurm fields are accepted and unused)."""

    run: pathlib.Path = pathlib.Path("./runs/abcdefg")
    """SAE run directory for loading SAE activations."""
    test_shards: pathlib.Path = pathlib.Path("./shards/abcdef01")
    """Test shards directory with labels.bin for segmentation labels."""
    cls_checkpoints: tuple[pathlib.Path, ...] = ()
    """Paths to trained classifier checkpoints."""
    max_budget: int = 1000
    """Maximum budget for feature selection. Union of top-max_budget from each classifier."""
    tau: float = 0.3
    """Grounding threshold: feature is grounded if best-class AP >= tau."""
    budgets: tuple[int, ...] = (3, 10, 30, 100, 300, 1000)
    """Browsing budgets for Yield@B computation."""
    ignore_label_ids: tuple[int, ...] = (0,)
    """Segmentation label IDs to ignore (e.g., background=0, void=255)."""
    seed: int = 42
    debug: bool = False
    mem_gb: int = 80
    slurm_acct: str = ""
    slurm_partition: str = ""
    n_hours: float = 4.0
    log_to: pathlib.Path = pathlib.Path("./logs")


def yield_at_budgets(ranked_i: np.ndarray, best_ap_s: np.ndarray, budgets, tau: float) -> tuple[dict[int, float], float]:
    """(Yield@B for each budget, AUC_B): the share of a classifier's top-B features whose best-class AP is >= tau (NaN, a feature
    outside the evaluated union, is not grounded), and the mean over the budgets -- the reference's arithmetic."""
    yield_at_b = {}
    for b in budgets:
        top_b_ap = best_ap_s[ranked_i[:b]]
        with np.errstate(invalid="ignore"):
            yield_at_b[b] = float(int(np.nansum(top_b_ap >= tau)) / b)
    return yield_at_b, sum(yield_at_b.values()) / len(yield_at_b)


def eval_worker_fn(cfg: EvalConfig) -> int:
    """Evaluate several classifiers on the same SAE run, as the reference's function of this name.  Every latent is scored against
    every class on the device in one call; next to ``token_acts.npz`` it writes the reference's ``audit_ap_s.npy`` (float32) and
    ``audit_best_class_s.npy`` (int32, original label ids) -- filled for the union of the classifiers' top-``max_budget`` features,
    NaN / -1 elsewhere --, ``audit_results.json`` with the reference's keys, and ``audit_ap_sc.npy`` (float32, d_sae x classes) for
    every latent."""
    log_format = "[%(asctime)s] [%(levelname)s] [%(name)s] %(message)s"
    logging.basicConfig(level=logging.DEBUG if cfg.debug else logging.INFO, format=log_format, force=True)
    logger = logging.getLogger("cls::eval")
    logger.info("Started eval_worker_fn().")

    assert cfg.cls_checkpoints, "No classifier checkpoints provided."
    for ckpt in cfg.cls_checkpoints:
        assert pathlib.Path(ckpt).exists(), f"Classifier checkpoint {ckpt} does not exist."
    test_shards_dpath = pathlib.Path(cfg.test_shards)
    assert test_shards_dpath.exists(), f"Test shards directory {test_shards_dpath} does not exist."
    run = disk.Run(cfg.run)
    test_inference_dpath = run.inference / test_shards_dpath.name
    assert test_inference_dpath.exists(), f"Test inference directory {test_inference_dpath} doesn't exist. Run inference.py."
    test_token_acts_fpath = test_inference_dpath / "token_acts.npz"
    assert test_token_acts_fpath.exists(), f"Test SAE acts missing: '{test_token_acts_fpath}'. Run inference.py."
    test_labels_fpath = test_shards_dpath / "labels.bin"
    assert test_labels_fpath.exists(), f"Test labels missing: '{test_labels_fpath}'."

    logger.info("Loading %d classifier checkpoints...", len(cfg.cls_checkpoints))
    classifiers = []
    for ckpt in cfg.cls_checkpoints:
        _, cls_type, ranked_i, importance = load_classifier_checkpoint(pathlib.Path(ckpt), logger)
        classifiers.append((pathlib.Path(ckpt), cls_type, ranked_i, importance))
    d_sae = len(classifiers[0][2])
    for ckpt, _, ranked_i, _ in classifiers:
        assert len(ranked_i) == d_sae, f"Classifier {ckpt} has different d_sae: {len(ranked_i)} != {d_sae}"

    feature_union: set[int] = set()
    for _, _, ranked_i, _ in classifiers:
        feature_union.update(ranked_i[: cfg.max_budget].tolist())
    features_to_eval = sorted(feature_union)
    n_features = len(features_to_eval)
    logger.info("Union of top-%d features: %d unique (%.1f%% of d_sae=%d)", cfg.max_budget, n_features, 100.0 * n_features / d_sae, d_sae)
    for b in cfg.budgets:
        assert b <= cfg.max_budget, f"Budget {b} exceeds max_budget={cfg.max_budget}."

    test_md = saev_data.Metadata.load(test_shards_dpath)
    n_images, patches_per_image = test_md.n_examples, test_md.content_tokens_per_example
    n_patches = n_images * patches_per_image
    logger.info("Test set: %d images, %d patches/image, %d total patches.", n_images, patches_per_image, n_patches)

    logger.info("Loading segmentation labels from %s...", test_labels_fpath)
    labels_flat = np.memmap(test_labels_fpath, mode="r", dtype=np.uint8, shape=(n_images, patches_per_image)).copy().reshape(-1)
    assert labels_flat.shape[0] == n_patches, f"Labels shape {labels_flat.shape[0]} != expected {n_patches}."

    logger.info("Loading SAE activations from %s...", test_token_acts_fpath)
    token_acts_csr = scipy.sparse.load_npz(test_token_acts_fpath).tocsr()
    assert token_acts_csr.shape == (n_patches, d_sae), f"SAE acts shape {token_acts_csr.shape} != expected ({n_patches}, {d_sae})."
    logger.info("SAE acts: shape=%s, nnz=%d", token_acts_csr.shape, token_acts_csr.nnz)

    # every latent against every class, on the device; the class ids go there as bytes with a 256-entry remap
    res, all_seg_classes = _matrix_on_device(token_acts_csr, labels_flat, cfg.ignore_label_ids)
    n_seg_classes = len(all_seg_classes)
    logger.info("Segmentation: %d unique labels, %d after ignoring %s.", len(np.unique(labels_flat)), n_seg_classes, cfg.ignore_label_ids)
    n_pos_c = res.n_pos.cpu().numpy()
    for idx, c in enumerate(all_seg_classes):
        assert n_pos_c[idx] > 0, f"Segmentation class {c} has no positive samples."
    logger.info("Positives per class: min=%d, max=%d, mean=%.1f", n_pos_c.min(), n_pos_c.max(), n_pos_c.mean())
    ap_sc = res.ap.cpu().numpy().astype(np.float32)
    best_all_ap = res.best_ap.cpu().numpy().astype(np.float32)
    best_all_class = res.best_class.cpu().numpy()

    best_ap_s = np.full(d_sae, np.nan, dtype=np.float32)
    best_class_s = np.full(d_sae, -1, dtype=np.int32)
    idx = np.asarray(features_to_eval, dtype=np.int64)
    best_ap_s[idx] = best_all_ap[idx]
    best_class_s[idx] = all_seg_classes[best_all_class[idx]].astype(np.int32)
    computed_aps = best_ap_s[~np.isnan(best_ap_s)]
    logger.info("AP stats (n=%d): mean=%.4f, min=%.4f, max=%.4f", len(computed_aps), computed_aps.mean(), computed_aps.min(), computed_aps.max())

    np.save(test_inference_dpath / "audit_ap_s.npy", best_ap_s)
    np.save(test_inference_dpath / "audit_best_class_s.npy", best_class_s)
    np.save(test_inference_dpath / "audit_ap_sc.npy", ap_sc)
    logger.info("Saved AP results to %s", test_inference_dpath)

    all_results = []
    for ckpt, cls_type, ranked_i, importance in classifiers:
        yield_at_b, auc_b = yield_at_budgets(ranked_i, best_ap_s, cfg.budgets, cfg.tau)
        all_results.append({
            "cls_checkpoint": str(ckpt),
            "cls_type": cls_type,
            "n_nonzero_importance": int((importance > 0).sum()),
            "tau": cfg.tau,
            "budgets": list(cfg.budgets),
            "yield_at_b": {str(k): v for k, v in yield_at_b.items()},
            "auc_b": auc_b,
        })
        logger.info("%s: AUC_B=%.4f", ckpt.name, auc_b)

    results_fpath = test_inference_dpath / "audit_results.json"
    with open(results_fpath, "w") as fd:
        json.dump({
            "run": str(cfg.run),
            "test_shards": str(cfg.test_shards),
            "max_budget": cfg.max_budget,
            "n_features_evaluated": n_features,
            "n_seg_classes": n_seg_classes,
            "ignore_label_ids": list(cfg.ignore_label_ids),
            "d_sae": d_sae,
            "classifiers": all_results,
        }, fd)
    logger.info("Saved %d classifier results to %s", len(all_results), results_fpath)
    return 0


# ---------------------------------------------------------------- the training half ------------------------------------------------------

class PatchAgg(enum.Enum):
    """How to aggregate patch-level features to image-level."""

    MEAN = "mean"
    MAX = "max"


@dataclasses.dataclass(frozen=True)
class LabelGrouping:
    """A classification task as a grouping of labels, the reference's fields: with ``groups`` empty the original labels of
    ``source_col`` are the classes; otherwise each group name is a class, and an image whose label is in no group is left out."""

    name: str
    """Task name for output files."""
    source_col: str
    """Label column to read. Use 'class' for ImgFolder class names."""
    groups: dict[str, list[str]] = dataclasses.field(default_factory=dict)
    """Mapping from group name to list of original labels. Empty = no grouping."""


@dataclasses.dataclass(frozen=True)
class DecisionTree:
    """The reference's decision-tree choice.  Accepted as a configuration and NOT trained here: a CPU tree has nothing for a kernel to
    win (the policy of PCA in ``baselines.py``); ``train_worker_fn`` raises NotImplementedError naming it."""

    key: tp.Literal["decision-tree"] = "decision-tree"
    max_depth: int = -1
    """Maximum depth of the tree. Negative numbers mean unlimited."""


@dataclasses.dataclass(frozen=True)
class SparseLinear:
    """Sparse linear classifier: logistic regression with an L1 penalty, ``engine.l1_logistic``.  ``C`` is scikit-learn's inverse
    regularisation strength.  ``max_iter`` is the reference's field, the epoch cap of its saga solver; it does not translate to this
    solver and is accepted and recorded in the checkpoint header like the Slurm fields.  What bounds this solver is ``kkt_tol`` (the
    KKT residual at which it stops) and ``solver_iters`` (its iteration cap)."""

    key: tp.Literal["sparse-linear"] = "sparse-linear"
    C: float = 0.01
    """Inverse regularization strength. Lower C = more sparsity."""
    max_iter: int = 90
    """The reference's saga epoch cap: recorded, unused."""
    kkt_tol: float = 1e-4
    solver_iters: int = 5000


@dataclasses.dataclass(frozen=True)
class TrainConfig:
    """Configuration of the training stage, the reference's fields and defaults (the Slurm fields are accepted and unused)."""

    run: pathlib.Path = pathlib.Path("./runs/abcdefg")
    """Run directory."""
    train_shards: pathlib.Path = pathlib.Path("./shards/01234567")
    """Training shards directory."""
    test_shards: pathlib.Path = pathlib.Path("./shards/abcdef01")
    """Test shards directory."""
    task: LabelGrouping = dataclasses.field(default_factory=lambda: LabelGrouping(name="habitat", source_col="habitat"))
    """Classification task definition."""
    patch_agg: PatchAgg = PatchAgg.MAX
    """How to aggregate patch features to image features."""
    cls: DecisionTree | SparseLinear = SparseLinear()
    """Classifier architecture."""
    debug: bool = False
    mem_gb: int = 80
    slurm_acct: str = ""
    slurm_partition: str = ""
    n_hours: float = 4.0
    log_to: pathlib.Path = pathlib.Path("./logs")


IMAGE_LABELS_FNAME = "image_labels.csv"


def load_image_labels(shards_dpath: pathlib.Path) -> tuple[list[str], dict[str, list[str]]]:
    """(label_columns, {column: one string label per image}) of a shards directory.  The reference rebuilds the image dataset from
    the shard metadata; here the labels are read from ``image_labels.csv`` in the shards directory: a header ``stem,<col>,...`` (the
    columns of the reference's ``labels.csv``) and one row per example in example order (INTEGRATION.md has the lines that write it
    from the reference's function).  The row count is checked against ``Metadata.n_examples``."""
    shards_dpath = pathlib.Path(shards_dpath)
    fpath = shards_dpath / IMAGE_LABELS_FNAME
    if not fpath.exists():
        raise FileNotFoundError(f"Image labels missing: '{fpath}' (a header 'stem,<col>,...' and one row per example in example order).")
    with open(fpath, newline="") as fd:
        rows = list(csv.reader(fd))
    if not rows or len(rows[0]) < 2 or rows[0][0] != "stem":
        raise ValueError(f"'{fpath}' must start with the header 'stem,<col>,...'.")
    label_cols = rows[0][1:]
    body = rows[1:]
    n_examples = saev_data.Metadata.load(shards_dpath).n_examples
    if len(body) != n_examples:
        raise ValueError(f"'{fpath}' has {len(body)} rows, the shards hold {n_examples} examples.")
    if not body:
        raise ValueError("Dataset has no samples")
    for i, row in enumerate(body):
        if len(row) != len(rows[0]):
            raise ValueError(f"'{fpath}' row {i + 1} has {len(row)} fields, the header {len(rows[0])}.")
    return label_cols, {col: [row[j + 1] for row in body] for j, col in enumerate(label_cols)}


def apply_grouping(labels: list[str], task: LabelGrouping) -> tuple[np.ndarray, list[str], np.ndarray]:
    """(targets int32 (-1 if excluded), class_names in order, mask of the images to include) of a list of string labels, the
    reference's arithmetic: without groups the sorted unique labels are the classes; with groups the sorted group names are, and a
    label in no group is masked out."""
    n = len(labels)
    if not task.groups:
        unique_labels = sorted(set(labels))
        label_to_idx = {lbl: i for i, lbl in enumerate(unique_labels)}
        return np.array([label_to_idx[lbl] for lbl in labels], dtype=np.int32), unique_labels, np.ones(n, dtype=bool)
    label_to_group: dict[str, str] = {}
    for group_name, group_labels in task.groups.items():
        for lbl in group_labels:
            assert lbl not in label_to_group, f"Label '{lbl}' in multiple groups"
            label_to_group[lbl] = group_name
    group_names = sorted(task.groups.keys())
    group_to_idx = {g: i for i, g in enumerate(group_names)}
    targets = np.full(n, -1, dtype=np.int32)
    mask = np.zeros(n, dtype=bool)
    for i, lbl in enumerate(labels):
        if lbl in label_to_group:
            targets[i] = group_to_idx[label_to_group[lbl]]
            mask[i] = True
    return targets, group_names, mask


def aggregate_to_images(patch_acts, n_images: int, n_patches_per_image: int, patch_agg: PatchAgg, device=None) -> np.ndarray:
    """Dense (n_images, d_sae) float32 of a scipy CSR matrix (n_patches, d_sae), the reference's values as numbers: per image the
    column maximum or mean of its ``n_patches_per_image`` dense rows, computed by ``engine.pool_images`` on the device without the
    dense rows."""
    n_patches, d_sae = patch_acts.shape
    assert n_patches == n_images * n_patches_per_image
    if not isinstance(patch_agg, PatchAgg):
        raise ValueError(f"Unknown aggregation: {patch_agg}")
    dev = _device(device)
    return engine.pool_images(*_csr_on(patch_acts, dev), n_images, n_patches_per_image, d_sae, patch_agg.value).pooled.cpu().numpy()


class SparseLinearClassifier:
    """A trained sparse linear classifier: a plain class (it pickles with the standard library; it is not a scikit-learn object)
    with scikit-learn's attributes -- ``coef_`` (1, d) for two classes and (K, d) otherwise, ``intercept_``, ``classes_`` -- and the
    solver's certificate ``n_iter_``, ``kkt_residual_``, ``objective_``, ``converged_``."""

    def __init__(self, coef_, intercept_, classes_, *, C: float = 0.01, n_iter_: int = 0, kkt_residual_: float = float("nan"),
                 objective_: float = float("nan"), converged_: bool = True):
        self.coef_ = np.asarray(coef_, dtype=np.float64)
        self.intercept_ = np.asarray(intercept_, dtype=np.float64)
        self.classes_ = np.asarray(classes_)
        self.C, self.n_iter_, self.kkt_residual_, self.objective_, self.converged_ = C, n_iter_, kkt_residual_, objective_, converged_

    @classmethod
    def fit(cls, X: np.ndarray, y: np.ndarray, *, C: float = 0.01, kkt_tol: float = 1e-4, solver_iters: int = 5000, device=None) -> "SparseLinearClassifier":
        """Fit on dense float32 rows X (n, d) and integer targets y (n) with ``engine.l1_logistic``."""
        dev = _device(device)
        res = engine.l1_logistic(torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)).to(dev),
                                 torch.from_numpy(np.ascontiguousarray(y).astype(np.int64)).to(dev), C, kkt_tol=kkt_tol, max_iter=solver_iters)
        return cls(res.coef_.cpu().numpy(), res.intercept_.cpu().numpy(), res.classes_.cpu().numpy().astype(np.asarray(y).dtype), C=C,
                   n_iter_=res.n_iter_, kkt_residual_=res.kkt_residual_, objective_=res.objective_, converged_=res.converged_)

    def decision_function(self, X: np.ndarray) -> np.ndarray:
        """X @ coef_.T + intercept_ in float64: (n,) for two classes, (n, K) otherwise, as scikit-learn's."""
        scores = np.asarray(X, dtype=np.float64) @ self.coef_.T + self.intercept_
        return scores[:, 0] if self.coef_.shape[0] == 1 else scores

    def predict(self, X: np.ndarray) -> np.ndarray:
        scores = self.decision_function(X)
        return self.classes_[(scores > 0).astype(np.int64)] if scores.ndim == 1 else self.classes_[scores.argmax(axis=1)]


def _jsonable(obj):
    if isinstance(obj, dict):
        return {k: _jsonable(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return [_jsonable(v) for v in obj]
    if isinstance(obj, pathlib.PurePath):
        return str(obj)
    if isinstance(obj, enum.Enum):
        return obj.value
    return obj


def train_worker_fn(cfg: TrainConfig) -> int:
    """Train a classifier on pooled SAE codes, as the reference's function of this name: the same checks and messages, both splits
    pooled on the device, the images masked by ``apply_grouping``, the fit, ``test_pred`` and ``test_acc``, and the checkpoint
    ``<run>/inference/<test shards>/cls_{task}_{agg}_C{C}.pkl`` -- one JSON header line (``cfg``, ``test_acc``, ``n_classes``,
    ``class_names``), then the pickle of ``{"classifier", "test_pred", "test_y"}`` -- which ``eval_worker_fn`` reads."""
    log_format = "[%(asctime)s] [%(levelname)s] [%(name)s] %(message)s"
    logging.basicConfig(level=logging.DEBUG if cfg.debug else logging.INFO, format=log_format, force=True)
    logger = logging.getLogger("cls::train")
    logger.info("Started train_worker_fn().")

    if isinstance(cfg.cls, DecisionTree):
        raise NotImplementedError("cls=DecisionTree is not built here: a CPU decision tree has nothing for a kernel to win (DESIGN.md section 7); "
                                  "train it with the reference and audit its checkpoint with eval_worker_fn.")
    if not isinstance(cfg.cls, SparseLinear):
        raise ValueError(f"Unknown classifier type: {type(cfg.cls)}")

    run = disk.Run(cfg.run)
    train_shards_dpath, test_shards_dpath = pathlib.Path(cfg.train_shards), pathlib.Path(cfg.test_shards)
    assert train_shards_dpath.exists(), f"Train shards directory {train_shards_dpath} does not exist."
    assert test_shards_dpath.exists(), f"Test shards directory {test_shards_dpath} does not exist."
    train_inference_dpath = run.inference / train_shards_dpath.name
    assert train_inference_dpath.exists(), f"Train inference directory {train_inference_dpath} doesn't exist. Run inference.py."
    test_inference_dpath = run.inference / test_shards_dpath.name
    assert test_inference_dpath.exists(), f"Test inference directory {test_inference_dpath} doesn't exist. Run inference.py."
    train_token_acts_fpath = train_inference_dpath / "token_acts.npz"
    assert train_token_acts_fpath.exists(), f"Train SAE acts missing: '{train_token_acts_fpath}'. Run inference.py."
    test_token_acts_fpath = test_inference_dpath / "token_acts.npz"
    assert test_token_acts_fpath.exists(), f"Test SAE acts missing: '{test_token_acts_fpath}'. Run inference.py."

    train_md = saev_data.Metadata.load(train_shards_dpath)
    test_md = saev_data.Metadata.load(test_shards_dpath)
    logger.info("Loaded metadata: train=%d images, test=%d images.", train_md.n_examples, test_md.n_examples)

    logger.info("Loading image-level labels from train shards...")
    train_label_cols, train_labels = load_image_labels(train_shards_dpath)
    logger.info("Train label columns: %s", train_label_cols)
    logger.info("Loading image-level labels from test shards...")
    test_label_cols, test_labels = load_image_labels(test_shards_dpath)
    logger.info("Test label columns: %s", test_label_cols)

    source_col = cfg.task.source_col
    assert source_col in train_labels, f"Source column '{source_col}' not in train labels: {train_label_cols}"
    assert source_col in test_labels, f"Source column '{source_col}' not in test labels: {test_label_cols}"

    train_targets, class_names, train_mask = apply_grouping(train_labels[source_col], cfg.task)
    test_targets, _, test_mask = apply_grouping(test_labels[source_col], cfg.task)
    n_classes = len(class_names)
    logger.info("Task '%s': %d classes %s", cfg.task.name, n_classes, class_names)
    logger.info("Train: %d/%d images after filtering", train_mask.sum(), len(train_mask))
    logger.info("Test: %d/%d images after filtering", test_mask.sum(), len(test_mask))

    logger.info("Loading train SAE activations from %s...", train_token_acts_fpath)
    train_acts_csr = scipy.sparse.load_npz(train_token_acts_fpath).tocsr()
    logger.info("Train acts: shape=%s, nnz=%d", train_acts_csr.shape, train_acts_csr.nnz)
    logger.info("Loading test SAE activations from %s...", test_token_acts_fpath)
    test_acts_csr = scipy.sparse.load_npz(test_token_acts_fpath).tocsr()
    logger.info("Test acts: shape=%s, nnz=%d", test_acts_csr.shape, test_acts_csr.nnz)

    train_n_patches_per_image = train_md.content_tokens_per_example
    train_n_patches_expected = train_md.n_examples * train_n_patches_per_image
    assert train_acts_csr.shape[0] == train_n_patches_expected, f"Train acts have {train_acts_csr.shape[0]} rows, expected {train_n_patches_expected}"
    test_n_patches_per_image = test_md.content_tokens_per_example
    test_n_patches_expected = test_md.n_examples * test_n_patches_per_image
    assert test_acts_csr.shape[0] == test_n_patches_expected, f"Test acts have {test_acts_csr.shape[0]} rows, expected {test_n_patches_expected}"

    logger.info("Aggregating train patches to images using %s...", cfg.patch_agg.value)
    train_X_all = aggregate_to_images(train_acts_csr, train_md.n_examples, train_n_patches_per_image, cfg.patch_agg)
    logger.info("Train features (all): shape=%s", train_X_all.shape)
    logger.info("Aggregating test patches to images using %s...", cfg.patch_agg.value)
    test_X_all = aggregate_to_images(test_acts_csr, test_md.n_examples, test_n_patches_per_image, cfg.patch_agg)
    logger.info("Test features (all): shape=%s", test_X_all.shape)

    train_X, train_y = train_X_all[train_mask], train_targets[train_mask]
    test_X, test_y = test_X_all[test_mask], test_targets[test_mask]
    logger.info("Train features (filtered): shape=%s", train_X.shape)
    logger.info("Test features (filtered): shape=%s", test_X.shape)

    logger.info("Training SparseLinear (LogisticRegression L1) with C=%g...", cfg.cls.C)
    classifier = SparseLinearClassifier.fit(train_X, train_y, C=cfg.cls.C, kkt_tol=cfg.cls.kkt_tol, solver_iters=cfg.cls.solver_iters)
    logger.info("Training complete: %d iterations, KKT residual %.3g, objective %.6g, converged %s.", classifier.n_iter_, classifier.kkt_residual_,
                classifier.objective_, classifier.converged_)

    test_pred = classifier.predict(test_X)
    test_acc = (test_pred == test_y).mean()
    logger.info("Test accuracy: %.4f", test_acc)
    nonzero_i = np.where(np.any(classifier.coef_ != 0, axis=0))[0]
    logger.info("L1 selected %d features: %s", len(nonzero_i), nonzero_i.tolist())

    out_fpath = test_inference_dpath / f"cls_{cfg.task.name}_{cfg.patch_agg.value}_C{cfg.cls.C}.pkl"
    header = {"cfg": _jsonable(dataclasses.asdict(cfg)), "test_acc": float(test_acc), "n_classes": int(n_classes), "class_names": class_names}
    with open(out_fpath, "wb") as fd:
        fd.write(json.dumps(header).encode() + b"\n")
        pickle.dump({"classifier": classifier, "test_pred": test_pred, "test_y": test_y}, fd)
    logger.info("Saved checkpoint to %s", out_fpath)
    return 0
