"""Per-latent activation histograms and exact quantiles of a run's stored codes (engine.LatentHist, engine.latent_quantiles;
include/saev_amd.h: LATENT HISTOGRAM).

``worker_fn`` reads ``<run>/inference/<metadata hash>/token_acts.npz`` and writes ``activation_stats.npz`` beside it:

    q            (Q,) float64                the quantiles asked for
    lower        (d_sae, Q) float32          element floor((count - 1) q) of every latent's sorted activations: exact
    higher       (d_sae, Q) float32          element ceil((count - 1) q)
    linear       (d_sae, Q) float64          numpy's default interpolation between the two
    count        (d_sae,) int64              the size of the latent's multiset: rows (over="rows") or non-zero codes ("entries")
    hist_counts  (d_sae, 8 (hi_exp - lo_exp) + 2) int64   non-zero activations per bin, eight bins to the octave; column 0 the
                                             positive ones below 2^lo_exp, the last column those at or above 2^hi_exp
    hist_n_neg   (d_sae,) int64              the negative ones
    hist_edges   (8 (hi_exp - lo_exp) + 1,) float32
    over, level  strings

``level="image"`` max-pools the tokens of every image first (the way ``mimics.score_run`` does: the maximum clamped at 0): its
0.95 quantile over rows is the per-latent threshold ``np.quantile(x, 0.95, axis=0)`` the reference's interactive/features.py takes
of a dense images x d_sae matrix.  The reference's stochastic ``PercentileEstimator`` (utils/statistics.py) is replaced by these
exact values.  ``thresholds`` hands one quantile out as the float32 vector that ``alignment.coactivation_match(thr_a=...)``,
``engine.ClassFireCounts(thresholds=...)`` or a probe takes.
"""

from __future__ import annotations

import dataclasses
import logging
import os
import pathlib

import numpy as np
import scipy.sparse
import torch

from . import classification, disk, engine
from .data import Metadata

logger = logging.getLogger("activation_stats.py")

FNAME = "activation_stats.npz"
KEYS = ("q", "lower", "higher", "linear", "count", "hist_counts", "hist_n_neg", "hist_edges", "over", "level")


@dataclasses.dataclass(frozen=True)
class Config:
    run: pathlib.Path = pathlib.Path("./runs/abcdefg")
    shards: pathlib.Path = pathlib.Path("./shards/abcdefg")
    q: tuple[float, ...] = (0.5, 0.9, 0.95, 0.99)
    over: str = "rows"
    level: str = "token"
    tokens_per_image: int | None = None
    """Tokens per image for ``level="image"`` (None: the shards' content tokens per example)."""
    chunk_rows: int = 2**20
    lo_exp: int = -16
    hi_exp: int = 16
    force_recompute: bool = False
    device: str = "cuda"


def _check(cfg: Config) -> None:
    if cfg.level not in ("token", "image"):
        raise ValueError(f"level must be 'token' or 'image', got {cfg.level!r}")
    if cfg.over not in ("rows", "entries"):
        raise ValueError(f"over must be 'rows' or 'entries', got {cfg.over!r}")
    if not 1 <= len(cfg.q) <= engine.LatentQuantiles.MAX_Q or not all(0.0 <= v <= 1.0 for v in cfg.q):
        raise ValueError(f"q must hold 1 to {engine.LatentQuantiles.MAX_Q} values in [0, 1], got {cfg.q}")
    if not -126 <= cfg.lo_exp < cfg.hi_exp <= 127:
        raise ValueError(f"need -126 <= lo_exp < hi_exp <= 127, got {cfg.lo_exp}, {cfg.hi_exp}")


def stats_path(cfg: Config) -> pathlib.Path:
    shards = pathlib.Path(os.path.expandvars(str(cfg.shards)))
    return disk.Run(cfg.run).inference / Metadata.load(shards).hash / FNAME


def _current(path: pathlib.Path, cfg: Config, d_sae: int | None = None) -> bool:
    """Whether ``path`` answers this config: the same quantiles, multiset, level and histogram window (and latents, when known).  A
    file of another question is rebuilt, never handed out as this one's."""
    if not path.exists():
        return False
    with np.load(path) as z:
        if sorted(z.files) != sorted(KEYS):
            return False
        same = (z["q"].shape == (len(cfg.q),) and np.array_equal(z["q"], np.asarray(cfg.q, dtype=np.float64)) and str(z["over"]) == cfg.over
                and str(z["level"]) == cfg.level and z["hist_edges"].shape == (8 * (cfg.hi_exp - cfg.lo_exp) + 1,)
                and z["hist_edges"][0] == np.float32(2.0**cfg.lo_exp))
        return bool(same and (d_sae is None or z["lower"].shape == (d_sae, len(cfg.q))))


@torch.inference_mode()
def worker_fn(cfg: Config) -> pathlib.Path:
    _check(cfg)
    out = stats_path(cfg)
    ta_fpath = out.parent / "token_acts.npz"
    if not ta_fpath.exists():
        raise FileNotFoundError(f"'{ta_fpath}' is missing: run framework.inference.worker_fn with save=True first")
    ta = scipy.sparse.load_npz(ta_fpath).tocsr()
    n_rows, d_sae = ta.shape
    if not cfg.force_recompute and _current(out, cfg, d_sae):
        logger.info("Current: '%s'.", out)
        return out
    dev = engine._hip_device("activation_stats", cfg.device)
    indptr, indices, data = classification._csr_on(ta, dev)
    del ta
    if cfg.level == "image":
        tpi = cfg.tokens_per_image or Metadata.load(pathlib.Path(os.path.expandvars(str(cfg.shards)))).content_tokens_per_example
        if tpi < 1 or n_rows % tpi:
            raise ValueError(f"{n_rows} token rows are no whole number of images of {tpi} tokens")
        n_rows //= tpi
        # the positive pooled maxima, in sparse form (what the non-zero entries of the clamped dense pooling were)
        indptr, indices, data = engine.pool_csr(indptr, indices, data, n_rows, tpi, d_sae).triple()
    hist = engine.LatentHist(d_sae, dev)
    got = engine.latent_quantiles(indptr, indices, data, n_rows, d_sae, cfg.q, over=cfg.over, chunk_rows=cfg.chunk_rows, device=dev, hist=hist)
    counts, n_neg, edges = hist.histogram(cfg.lo_exp, cfg.hi_exp)
    np.savez(out, q=np.asarray(cfg.q, dtype=np.float64), lower=got.lower.numpy(), higher=got.higher.numpy(), linear=got.linear.numpy(),
             count=got.count.numpy(), hist_counts=counts.numpy(), hist_n_neg=n_neg.numpy(), hist_edges=edges.numpy(), over=np.array(cfg.over),
             level=np.array(cfg.level))
    return out


def thresholds(path, q: float, method: str = "linear") -> np.ndarray:
    """The (d_sae,) float32 vector of quantile ``q`` in ``activation_stats.npz`` -- ``method`` "linear" (numpy's default, rounded to
    float32), "lower" or "higher" (exact elements).  A latent with an empty multiset gets NaN: it passes no threshold."""
    if method not in ("linear", "lower", "higher"):
        raise ValueError(f"method must be 'linear', 'lower' or 'higher', got {method!r}")
    with np.load(path) as z:
        at = np.flatnonzero(z["q"] == np.float64(q))
        if at.size == 0:
            raise ValueError(f"'{path}' holds the quantiles {z['q'].tolist()}, not {q}")
        return np.ascontiguousarray(z[method][:, at[0]].astype(np.float32))
