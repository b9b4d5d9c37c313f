"""Latents of two runs aligned by what they fire on (idea 8, "cross-run feature alignment", of the reference's
contrib/mimics/README.md: "if they activate on the same images, they capture the same trait"), on ``engine.coactivation_match``
(include/saev_amd.h: COACTIVATION).  The latents of different runs are unrelated by index and need not live in the
same activation space -- other layers, other backbones, other widths -- so they are compared by the SETS of tokens or images they
fire on: Jaccard similarity (or containment, for "which latent covers this one": split and absorbed features) of the sets, the best
partners in both directions, and whether the match is mutual.

``worker_fn`` reads both runs' ``token_acts.npz`` of the same shards and writes ``latent_alignment__<run_b id>.npz`` (``__self`` when
a run is aligned with itself) into run A's inference directory; ``robustness`` counts, over the files of one run against R others, in
how many runs each latent has a mutual partner -- the README's "if a trait appears in 8/10 runs, it's robust".  Everything that
touches activations runs on the HIP device; there is no CPU path.
"""

from __future__ import annotations

import dataclasses
import logging
import pathlib

import numpy as np
import scipy.sparse

from . import classification, engine, helpers

logger = logging.getLogger("alignment")

KEYS = ("partner", "intersection", "jaccard", "support_a", "support_b", "mutual", "reverse_partner")


@dataclasses.dataclass(frozen=True)
class Config:
    run_a: pathlib.Path = pathlib.Path("./runs/a")
    """Run directory (``<run root>/<run id>``) whose latents are matched."""
    run_b: pathlib.Path | None = None
    """Run directory whose latents are the partners; None aligns run A with itself (duplicate and split latents)."""
    shards: str = ""
    """Shards directory (or its name): both runs' ``inference/<name>/token_acts.npz`` are read."""
    level: str = "token"
    """"token": a latent's set is the tokens it fires on.  "image": the activations are max-pooled to images first."""
    tokens_per_image: int = 1
    """Rows of ``token_acts.npz`` per image (for ``level="image"``)."""
    top_k: int | None = None
    """If set, a latent's set is its ``top_k`` highest rows (the README's "top-K activated image sets") instead of all it fires on."""
    threshold: float = 0.0
    """An activation fires when it is > threshold."""
    measure: str = "jaccard"
    top_m: int = 1
    device: str = "cuda"


def alignment_fpath(cfg: Config) -> pathlib.Path:
    name = "self" if cfg.run_b is None else pathlib.Path(cfg.run_b).name
    return _inference_dpath(cfg.run_a, cfg.shards) / f"latent_alignment__{name}.npz"


def _inference_dpath(run: pathlib.Path, shards: str) -> pathlib.Path:
    return pathlib.Path(run) / "inference" / pathlib.Path(shards).name


def load_token_acts(cfg: Config) -> tuple[scipy.sparse.csr_matrix, scipy.sparse.csr_matrix | None]:
    """Both runs' token activations; ValueError if they do not cover the same rows."""
    fpath_a = _inference_dpath(cfg.run_a, cfg.shards) / "token_acts.npz"
    ta_a = scipy.sparse.load_npz(str(fpath_a)).tocsr()
    if cfg.run_b is None:
        return ta_a, None
    fpath_b = _inference_dpath(cfg.run_b, cfg.shards) / "token_acts.npz"
    ta_b = scipy.sparse.load_npz(str(fpath_b)).tocsr()
    if ta_a.shape[0] != ta_b.shape[0]:
        raise ValueError(f"the runs cover different rows: '{fpath_a}' has {ta_a.shape[0]}, '{fpath_b}' has {ta_b.shape[0]}")
    return ta_a, ta_b


def _top_k_sets(csr: scipy.sparse.csr_matrix, top_k: int, threshold: float) -> scipy.sparse.csr_matrix:
    """Per latent its ``top_k`` highest rows among those > threshold, back as a row-major CSR matrix (``helpers.csr_topk`` selects on
    the device; a latent with fewer such rows keeps them all)."""
    top = helpers.csr_topk(csr, k=top_k, axis=0)
    keep = (top.values != 0) & (top.values > threshold)  # csr_topk pads short latents with value 0
    cols = np.broadcast_to(np.arange(csr.shape[1]), top.values.shape)
    return scipy.sparse.csr_matrix((top.values[keep].astype(np.float32), (top.indices[keep], cols[keep])), shape=csr.shape)


def _sets_on_device(ta: scipy.sparse.csr_matrix, cfg: Config, dev):
    """(CSR triple on the device, number of rows) of one run at the configured level, with the top-k restriction applied."""
    n_rows = ta.shape[0]
    if cfg.level == "image":
        tpi = cfg.tokens_per_image
        if tpi < 1 or n_rows % tpi:
            raise ValueError(f"{n_rows} rows are not a whole number of images of {tpi} tokens")
        n_rows //= tpi
        # the positive maxima only, as mimics.max_pool_csr: the reference's pooling starts from zeros
        pooled = engine.pool_csr(*classification._csr_on(ta, dev), n_rows, tpi, ta.shape[1]).triple()
        if cfg.top_k is None:
            return pooled, n_rows
        indptr, indices, data = (t.cpu().numpy() for t in pooled)
        ta = scipy.sparse.csr_matrix((data, indices, indptr), shape=(n_rows, ta.shape[1]))
    elif cfg.level != "token":
        raise ValueError(f"level must be 'token' or 'image', got {cfg.level!r}")
    if cfg.top_k is not None:
        ta = _top_k_sets(ta, cfg.top_k, cfg.threshold)
    return classification._csr_on(ta, dev), n_rows


def arrays_of(index, intersection, support_a, support_b, reverse_partner) -> dict[str, np.ndarray]:
    """The file's arrays from the integers of a match and of its reverse: ``partner`` and ``intersection`` (Sa, top_m) int32,
    ``jaccard`` (Sa, top_m) float64 (I / (n_a + n_b - I), NaN where there is no partner), ``support_a`` (Sa) and ``support_b`` (Sb)
    int32, ``reverse_partner`` (Sb) int32 (the best latent of A for each of B) and ``mutual`` (Sa) bool."""
    partner = np.ascontiguousarray(index, dtype=np.int32)
    inter = np.ascontiguousarray(intersection, dtype=np.int32)
    n_a, n_b = np.ascontiguousarray(support_a, dtype=np.int32), np.ascontiguousarray(support_b, dtype=np.int32)
    rev = np.ascontiguousarray(reverse_partner, dtype=np.int32)
    found = partner >= 0
    union = n_a.astype(np.int64)[:, None] + n_b.astype(np.int64)[np.maximum(partner, 0)] - inter
    with np.errstate(divide="ignore", invalid="ignore"):
        jaccard = np.where(found, inter.astype(np.float64) / union.astype(np.float64), np.nan)
    best = partner[:, 0]
    mutual = (best >= 0) & (rev[np.maximum(best, 0)] == np.arange(len(best)))
    return dict(partner=partner, intersection=inter, jaccard=jaccard, support_a=n_a, support_b=n_b, mutual=mutual, reverse_partner=rev)


def align_runs(cfg: Config) -> dict[str, np.ndarray]:
    """The alignment of run A's latents with run B's (or with each other) as the arrays of ``arrays_of``."""
    ta_a, ta_b = load_token_acts(cfg)
    dev = classification._device(cfg.device)
    A, n_rows = _sets_on_device(ta_a, cfg, dev)
    B = None if ta_b is None else _sets_on_device(ta_b, cfg, dev)[0]
    res = engine.coactivation_match(A, B, n_rows=n_rows, n_latents_a=ta_a.shape[1], n_latents_b=None if ta_b is None else ta_b.shape[1],
                                    thr_a=cfg.threshold, thr_b=cfg.threshold, measure=cfg.measure, top_m=cfg.top_m)
    host = lambda t: t.cpu().numpy()  # noqa: E731
    return arrays_of(host(res.index), host(res.intersection), host(res.support_a), host(res.support_b), host(res.reverse.index[:, 0]))


def worker_fn(cfg: Config) -> pathlib.Path:
    """Align and write ``latent_alignment__<run_b id>.npz`` (keys ``KEYS``) into run A's inference directory; returns its path."""
    out = align_runs(cfg)
    fpath = alignment_fpath(cfg)
    np.savez(fpath, **out)
    logger.info("Wrote the alignment of %d latents (%.1f%% mutual) to '%s'.", len(out["mutual"]), 100.0 * out["mutual"].mean(), fpath)
    return fpath


def robustness(paths, *, min_jaccard: float = 0.5) -> np.ndarray:
    """Per latent of run A, in how many of the alignment files ``paths`` (run A against one other run each) it has a MUTUAL best
    partner with Jaccard >= ``min_jaccard``: (Sa) int32."""
    count = None
    for p in paths:
        with np.load(p) as z:
            with np.errstate(invalid="ignore"):
                hit = z["mutual"] & (z["jaccard"][:, 0] >= min_jaccard)
        if count is None:
            count = np.zeros(len(hit), dtype=np.int32)
        if len(hit) != len(count):
            raise ValueError(f"'{p}' aligns {len(hit)} latents, the files before it {len(count)}")
        count += hit
    if count is None:
        raise ValueError("robustness takes at least one alignment file")
    return count
