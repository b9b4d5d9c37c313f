"""Probe metrics: the reference's ``contrib/trait_discovery`` ``tdiscovery.metrics`` (``Config``, ``worker_fn``) over the HIP kernels
behind ``engine.probe_ap`` (include/saev_amd.h: PROBE AP).  The module is called ``probe_metrics`` because
``saev_amd.metrics`` is taken: that one mirrors the reference's ``saev.metrics``.

``worker_fn`` takes the probes ``probe1d.worker_fn`` fitted on the train split, picks per class the latent with the lowest train
loss, and scores ``w * a + b`` on the test split: average precision, precision, recall and F1 at score > 0, and the labels of every
latent's ``max_k`` highest rows.  It reads the files the reference reads, makes its checks with its messages, and writes its
``probe1d_metrics__train-<train shards>.npz`` with the same five keys, dtypes and shapes.

What differs, on purpose: the AP is the exact tie-aware value (the expectation over all orders of rows of equal score) where the
reference leaves tied rows -- all rows on which the latent is silent tie at score b -- in whatever order an unstable argsort puts
them; the two agree wherever the order of tied rows cannot matter.  All (latent, class) pairs are scored in one call on the sorted
sparse codes, never through an N x C array, and ``probe1d_ap_lc__train-<name>.npy`` (d_sae x classes float32) keeps every pair's
AP, not only the selected ones.  There is no CPU path."""

from __future__ import annotations

import dataclasses
import logging
import pathlib

import numpy as np
import scipy.sparse
import torch

from . import classification
from . import data as saev_data
from . import disk
from . import engine

log_format = "[%(asctime)s] [%(levelname)s] [%(name)s] %(message)s"


@dataclasses.dataclass(frozen=True)
class Config:
    """Configuration for AP evaluation pipeline on ImgSeg datasets (the reference's fields and defaults)."""

    run: pathlib.Path = pathlib.Path("./runs/abcdefg")
    """Run directory."""
    train_shards: pathlib.Path = pathlib.Path("./shards/01234567")
    """Training shards directory."""
    test_shards: pathlib.Path = pathlib.Path("./shards/abcdef01")
    """Test shards directory."""
    max_k: int = 256
    """How many patches to record labels (for purity@k)."""
    debug: bool = False
    """Debug logging."""
    mem_gb: int = 80
    """Node memory in GB."""
    slurm_acct: str = ""
    """Slurm account string. Empty means to not use Slurm."""
    slurm_partition: str = ""
    """Slurm partition."""
    n_hours: float = 6.0
    """Slurm job length in hours."""
    log_to: pathlib.Path = pathlib.Path("./logs")
    """Where to log Slurm job stdout/stderr."""


def purity_stats(top_labels_dk: np.ndarray, k: int) -> tuple[float, float, float]:
    """(mean, min, max) over the latents of the share of the most frequent label among a latent's first k recorded labels: the
    numbers of the reference's ``np.unique`` loop, from one bincount."""
    labels_dk = np.ascontiguousarray(top_labels_dk[:, :k], dtype=np.uint8)
    d = labels_dk.shape[0]
    counts = np.bincount((np.arange(d, dtype=np.int64)[:, None] * 256 + labels_dk).reshape(-1), minlength=d * 256).reshape(d, 256)
    purities = (counts.max(axis=1) / k).astype(np.float32)
    return purities.mean().item(), purities.min().item(), purities.max().item()


def scores_from_counts(tp_c: np.ndarray, n_pred_pos_c: np.ndarray, n_pos_c: np.ndarray):
    """(precision, recall, f1) float32 from integer counts, by the reference's float32 expressions (its counts are float32 sums of
    0/1 arrays, exact below 2^24)."""
    tp_c, n_pred_pos_c, n_pos_c = (np.asarray(v).astype(np.float32) for v in (tp_c, n_pred_pos_c, n_pos_c))
    pos_class_mask_c = n_pos_c > 0
    precision_c = np.divide(tp_c, n_pred_pos_c, out=np.zeros_like(tp_c), where=n_pred_pos_c > 0.0)
    precision_c = np.where(pos_class_mask_c, precision_c, np.zeros_like(precision_c))
    recall_c = np.divide(tp_c, n_pos_c, out=np.zeros_like(tp_c), where=n_pos_c > 0.0)
    recall_c = np.where(pos_class_mask_c, recall_c, np.zeros_like(recall_c))
    denom_c = precision_c + recall_c
    f1_c = np.divide(2.0 * precision_c * recall_c, denom_c, out=np.zeros_like(precision_c), where=denom_c > 0.0)
    return precision_c, recall_c, f1_c


def worker_fn(cfg: Config):
    level = logging.DEBUG if cfg.debug else logging.INFO
    logging.basicConfig(level=level, format=log_format)
    logger = logging.getLogger("metrics")
    logger.info("Started worker_fn().")

    run = disk.Run(cfg.run)
    train_inference_dpath = run.inference / cfg.train_shards.name
    train_token_acts_fpath = train_inference_dpath / "token_acts.npz"
    assert train_token_acts_fpath.exists(), f"Train SAE acts missing: '{train_token_acts_fpath}'. Run inference.py."
    val_inference_dpath = run.inference / cfg.test_shards.name
    val_token_acts_fpath = val_inference_dpath / "token_acts.npz"
    assert val_token_acts_fpath.exists(), f"Validation SAE acts missing: '{val_token_acts_fpath}'. Run inference.py."
    train_probe_metrics_fpath = train_inference_dpath / "probe1d_metrics.npz"
    assert train_probe_metrics_fpath.exists(), f"Probe metrics missing: '{train_probe_metrics_fpath}'. Run probe1d.py."
    val_labels_fpath = cfg.test_shards / "labels.bin"
    assert val_labels_fpath.exists(), f"Validation labels missing: '{val_labels_fpath}'."

    with np.load(train_probe_metrics_fpath) as fd:
        train_loss_lc = fd["loss"]
        weights_lc = fd["weights"]
        biases_lc = fd["biases"]
    assert train_loss_lc.ndim == 2, f"Expected train loss to be 2D (latents x classes); found shape {train_loss_lc.shape}."
    msg = f"Probe metric shapes are inconsistent: loss{train_loss_lc.shape}, weights{weights_lc.shape}, biases{biases_lc.shape}."
    assert weights_lc.shape == train_loss_lc.shape, msg
    assert biases_lc.shape == train_loss_lc.shape, msg
    n_latents, n_classes = train_loss_lc.shape

    best_latent_idx_c = np.argmin(train_loss_lc, axis=0)
    class_idx_c = np.arange(n_classes)
    best_train_loss_c = train_loss_lc[best_latent_idx_c, class_idx_c]
    logger.info(
        "Selected best latents per class: n_classes=%d, unique_latents=%d, train_loss[mean]=%.6f, train_loss[min]=%.6f, train_loss[max]=%.6f.",
        n_classes, np.unique(best_latent_idx_c).size, best_train_loss_c.mean().item(), best_train_loss_c.min().item(), best_train_loss_c.max().item())

    val_md = saev_data.Metadata.load(cfg.test_shards)
    val_token_acts_csr = scipy.sparse.load_npz(val_token_acts_fpath).tocsr()
    val_n_samples, val_n_latents = val_token_acts_csr.shape
    assert val_n_latents == n_latents, f"Validation activations have {val_n_latents} latents; expected {n_latents}."
    val_labels = np.memmap(val_labels_fpath, mode="r", dtype=np.uint8, shape=(val_md.n_examples, val_md.content_tokens_per_example)).copy().reshape(-1)
    assert val_labels.size == val_n_samples, f"Validation labels provide {val_labels.size} samples; expected {val_n_samples}."
    val_max_label = val_labels.max().item()
    assert val_max_label < n_classes, f"Validation labels include class id {val_max_label}; expected < {n_classes}."
    assert cfg.max_k > 0, f"max_k must be positive; got {cfg.max_k}."
    assert cfg.max_k <= val_n_samples, f"max_k ({cfg.max_k}) exceeds validation samples ({val_n_samples})."

    # every pair on the device in one call, in the arithmetic numpy would score in: float32 codes times the stored weights
    score_dtype = np.result_type(np.float32, weights_lc.dtype, biases_lc.dtype)
    if score_dtype not in (np.float32, np.float64):
        raise ValueError(f"probe weights of dtype {weights_lc.dtype} / {biases_lc.dtype} give scores of dtype {score_dtype}: float32 or float64 only")
    dev = classification._device()
    res = engine.probe_ap(*classification._csr_on(val_token_acts_csr, dev), val_n_samples, n_latents, n_classes,
                          labels=torch.from_numpy(val_labels).to(dev), weights=torch.from_numpy(np.ascontiguousarray(weights_lc, dtype=score_dtype)).to(dev),
                          biases=torch.from_numpy(np.ascontiguousarray(biases_lc, dtype=score_dtype)).to(dev), top_k=cfg.max_k)
    res.check()
    top_labels_dk = np.take(val_labels, res.top_rows.cpu().numpy()).astype(np.uint8, copy=False)
    logger.info("Captured top-%d labels for %d latents.", cfg.max_k, val_n_latents)
    for purity_k in (16, 64, 256):
        if purity_k > cfg.max_k:
            logger.info("Skipping purity@%d because max_k=%d.", purity_k, cfg.max_k)
            continue
        purity_mean, purity_min, purity_max = purity_stats(top_labels_dk, purity_k)
        logger.info("purity@%d across %d latents: mean=%.6f, min=%.6f, max=%.6f.", purity_k, val_n_latents, purity_mean, purity_min, purity_max)

    n_pos_c = res.n_pos.cpu().numpy()
    pos_class_mask_c = n_pos_c > 0
    ap_lc = res.ap.cpu().numpy()
    ap_c = np.where(pos_class_mask_c, ap_lc[best_latent_idx_c, class_idx_c], 0.0).astype(np.float32)
    precision_c, recall_c, f1_c = scores_from_counts(res.tp.cpu().numpy()[best_latent_idx_c, class_idx_c],
                                                     res.n_pred_pos.cpu().numpy()[best_latent_idx_c, class_idx_c], n_pos_c)

    n_pos_classes = pos_class_mask_c.sum().item()
    pos_precision_c, pos_recall_c, pos_f1_c = precision_c[pos_class_mask_c], recall_c[pos_class_mask_c], f1_c[pos_class_mask_c]
    logger.info(
        "Computed validation precision/recall/F1 on %d positive classes: precision[mean]=%.6f, precision[min]=%.6f, precision[max]=%.6f, recall[mean]=%.6f, recall[min]=%.6f, recall[max]=%.6f, f1[mean]=%.6f, f1[min]=%.6f, f1[max]=%.6f.",
        n_pos_classes, pos_precision_c.mean().item(), pos_precision_c.min().item(), pos_precision_c.max().item(), pos_recall_c.mean().item(),
        pos_recall_c.min().item(), pos_recall_c.max().item(), pos_f1_c.mean().item(), pos_f1_c.min().item(), pos_f1_c.max().item())
    logger.info("Computed validation AP on %d samples: n_pos_classes=%d, ap[mean]=%.6f, ap[min]=%.6f, ap[max]=%.6f.", val_n_samples,
                pos_class_mask_c.sum().item(), ap_c.mean().item(), ap_c.min().item(), ap_c.max().item())

    metrics_fpath = val_inference_dpath / f"probe1d_metrics__train-{cfg.train_shards.name}.npz"
    np.savez(metrics_fpath, ap=ap_c, precision=precision_c, recall=recall_c, f1=f1_c, top_labels=top_labels_dk)
    logger.info("Saved metrics to '%s'.", metrics_fpath)
    np.save(val_inference_dpath / f"probe1d_ap_lc__train-{cfg.train_shards.name}.npy", ap_lc.astype(np.float32))
