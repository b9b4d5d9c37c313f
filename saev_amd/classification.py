"""The concept audit on sparse codes: the evaluation half of the reference's ``tdiscovery.classification`` (``compute_ap_for_latent``,
``compute_ap_batched``, ``extract_feature_ranking``, ``load_classifier_checkpoint``, ``EvalConfig``, ``eval_worker_fn``) over the HIP
kernels behind ``engine.latent_ap`` (include/saev_amd.h: LATENT AP).

The average precision of a latent's activation as a detector of each segmentation class is the exact tie-aware value of McSherry and
Najork (2008) -- the expectation over all orders of tied scores -- for every latent and every class, in one call on the device: the
stored entries are sorted once and each latent's zero rows enter as one tie group in closed form.  All sums are fp64 in a fixed
order (two runs give the same bits).  There is no CPU path: without a HIP device everything that computes raises."""

from __future__ import annotations

import dataclasses
import json
import logging
import pathlib
import pickle

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
