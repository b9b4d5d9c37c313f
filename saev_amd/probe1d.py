"""Per-latent logistic probes on sparse codes: the surface of the reference's ``tdiscovery.probe1d`` (``Sparse1DProbe``, ``Config``,
``worker_fn``) over the HIP kernels behind ``engine.Probe1D`` (include/saev_amd.h: PROBE1D).

For each of the ``n_latents x n_classes`` (latent, class) pairs a two-parameter logistic regression is fitted on the sparse codes
and scored; ``worker_fn`` writes ``probe1d_metrics.npz`` next to ``token_acts.npz`` for a train and a test split.  All arithmetic
is fp64 on the device in a fixed order (two fits of the same inputs give the same bits); ``dtype`` is what the results are rounded
to on the way out.  There is no CPU path: without a HIP device everything that computes raises."""

from __future__ import annotations

import dataclasses
import logging
import pathlib

import numpy as np
import scipy.sparse
import torch

from . import data as saev_data
from . import disk
from .engine import Probe1D, Probe1DHyper


def _csr_parts(x):
    """(indptr int64, indices int32, data float32, shape) as CPU or device tensors from a torch CSR tensor or a scipy CSR."""
    if isinstance(x, torch.Tensor):
        if x.layout != torch.sparse_csr:
            raise TypeError("x must be a torch.sparse_csr_tensor or a scipy CSR matrix.")
        return x.crow_indices(), x.col_indices(), x.values(), tuple(x.shape)
    if scipy.sparse.issparse(x) and x.format == "csr":
        return torch.from_numpy(np.asarray(x.indptr)), torch.from_numpy(np.asarray(x.indices)), torch.from_numpy(np.asarray(x.data)), tuple(x.shape)
    raise TypeError("x must be a torch.sparse_csr_tensor or a scipy CSR matrix.")


class Sparse1DProbe:
    """Levenberg-Marquardt fits of per-latent, per-class logistic probes on a sparse design matrix, as the reference's class of
    the same name: same constructor, ``fit``, ``loss_matrix``, ``loss_matrix_with_aux``, ``coef_``, ``intercept_``, ``n_iter_``,
    ``latent_qx_``.  ``row_batch_size`` is accepted and ignored (the kernels stream the events themselves)."""

    def __init__(self, *, n_latents: int, n_classes: int, ridge: float = 1e-8, tol: float = 1e-6, max_iter: int = 200, lam_init: float = 1e-3,
                 lam_shrink: float = 0.1, lam_grow: float = 10.0, delta_logit: float = 6.0, device: str = "cuda", dtype=torch.float32,
                 class_slab_size: int = 8, row_batch_size: int = 1024) -> None:
        if lam_shrink <= 0 or lam_shrink >= 1:
            raise ValueError(f"lam_shrink must lie in (0,1), got {lam_shrink}.")
        if lam_grow <= 1:
            raise ValueError(f"lam_grow must be >1, got {lam_grow}.")
        if delta_logit <= 0:
            raise ValueError(f"delta_logit must be >0, got {delta_logit}.")
        if dtype not in (torch.float32, torch.float64):
            raise ValueError(f"dtype must be torch.float32 or torch.float64, got {dtype}.")
        if n_latents < 1 or n_classes < 1 or n_classes > Probe1D.MAX_CLASSES:
            raise ValueError(f"n_latents must be >= 1 and n_classes in [1, {Probe1D.MAX_CLASSES}], got {n_latents} and {n_classes}.")
        if class_slab_size < 1:
            raise ValueError(f"class_slab_size must be >= 1, got {class_slab_size}.")
        self.n_latents, self.n_classes = n_latents, n_classes
        self.hyper = Probe1DHyper(ridge=float(ridge), tol=float(tol), max_iter=int(max_iter), lam_init=float(lam_init), lam_shrink=float(lam_shrink),
                                  lam_grow=float(lam_grow), delta_logit=float(delta_logit), class_slab_size=int(class_slab_size))
        self.ridge, self.tol, self.max_iter, self.lam_init = self.hyper.ridge, tol, max_iter, lam_init
        self.lam_shrink, self.lam_grow, self.delta_logit = lam_shrink, lam_grow, delta_logit
        self.class_slab_size, self.row_batch_size = class_slab_size, row_batch_size
        self.device, self.dtype = torch.device(device), dtype
        self.log = logging.getLogger("sparse1d")
        self.coef_ = self.intercept_ = self.n_iter_ = self.latent_qx_ = None
        self._prepared: tuple | None = None  # (x, y, Probe1D) of the last call: fit followed by loss_matrix on the same split

    def _labels(self, y, n_samples: int):
        """('labels', class ids) or ('y', N x C uint8 matrix), checked on the host where that is cheap."""
        y = torch.as_tensor(y)
        if y.ndim == 1:
            if y.shape[0] != n_samples:
                raise ValueError(f"y has {y.shape[0]} class ids, expected {n_samples}.")
            if y.dtype not in (torch.uint8, torch.int32, torch.int64):
                raise ValueError(f"class ids must be uint8, int32 or int64, got {y.dtype}.")
            return "labels", y
        if tuple(y.shape) != (n_samples, self.n_classes):
            raise ValueError(f"y has shape {tuple(y.shape)}, expected ({n_samples}, {self.n_classes}).")
        if y.dtype != torch.bool:
            if not bool(((y == 0) | (y == 1)).all()):
                raise ValueError("y must hold only 0 and 1.")
            y = y != 0
        return "y", y

    def _prepare(self, x, y) -> Probe1D:
        if self._prepared is not None and self._prepared[0] is x and self._prepared[1] is y:
            return self._prepared[2]
        indptr, indices, values, shape = _csr_parts(x)
        n_samples, n_latents = shape
        if n_latents != self.n_latents:
            raise ValueError(f"x has {n_latents} latents, expected {self.n_latents}.")
        form, labels = self._labels(y, n_samples)
        if self.device.type != "cuda" or not torch.cuda.is_available():
            raise RuntimeError("Sparse1DProbe runs on a HIP device only (there is no CPU path)")
        p = Probe1D(n_samples, n_latents, self.n_classes, int(values.numel()), self.device)
        dev = p.device
        p.prepare(indptr.to(dev, torch.int64), indices.to(dev, torch.int32), values.to(dev, torch.float32), **{form: labels.to(dev)})
        self._prepared = (x, y, p)
        return p

    @torch.no_grad()
    def fit(self, x, y) -> "Sparse1DProbe":
        p = self._prepare(x, y)
        self.coef_, self.intercept_, self.n_iter_ = p.fit(self.hyper, dtype=self.dtype)
        self.latent_qx_ = p.qx.to(self.dtype)
        return self

    def _fitted(self):
        if self.coef_ is None:
            raise RuntimeError("This Sparse1DProbe instance is not fitted yet. Call 'fit' first.")

    @torch.no_grad()
    def loss_matrix_with_aux(self, x, y, threshold: float = 0.5):
        """(loss, tp, fp, tn, fn), each (n_latents, n_classes) float32, of the fitted probes on (x, y)."""
        self._fitted()
        if not (0.0 < threshold < 1.0):
            raise ValueError("threshold must be between 0 and 1.")
        p = self._prepare(x, y)
        return p.evaluate(self.intercept_.to(torch.float64), self.coef_.to(torch.float64), threshold, dtype=torch.float32)

    def loss_matrix(self, x, y) -> torch.Tensor:
        return self.loss_matrix_with_aux(x, y)[0]


@dataclasses.dataclass(frozen=True)
class Config:
    run: pathlib.Path = pathlib.Path("./runs/abcdefg")
    """Run directory."""
    train_shards: pathlib.Path = pathlib.Path("./shards/01234567")
    """Training shards directory."""
    test_shards: pathlib.Path = pathlib.Path("./shards/abcdef01")
    """Test shards directory."""
    ridge: float = 1e-8
    """Ridge value."""
    class_slab_size: int = 8
    """Number of classes that stop together."""
    row_batch_size: int = 1024
    """Accepted for the reference's sweep files; ignored."""
    max_iter: int = 30
    """Number of iterations in the solver."""
    debug: bool = False
    """Debug logging."""
    device: str = "cuda"
    """Which accelerator to use."""
    mem_gb: int = 80
    slurm_acct: str = ""
    slurm_partition: str = ""
    n_hours: float = 4.0
    log_to: pathlib.Path = pathlib.Path("./logs")


def _save(fpath: pathlib.Path, probe: Sparse1DProbe, metrics) -> None:
    loss, tp, fp, tn, fn = (m.cpu().numpy() for m in metrics)
    fpath.parent.mkdir(parents=True, exist_ok=True)
    np.savez(fpath, loss=loss, weights=probe.coef_.cpu().numpy(), biases=probe.intercept_.cpu().numpy(), tp=tp, fp=fp, tn=tn, fn=fn)


def worker_fn(cfg: Config) -> int:
    """Fit on the train split's ``token_acts.npz`` and ``labels.bin``, score both splits, write
    ``inference/<shards>/probe1d_metrics.npz`` (loss, weights, biases, tp, fp, tn, fn) for each.  1 when an input is missing."""
    logging.basicConfig(level=logging.DEBUG if cfg.debug else logging.INFO, format="[%(asctime)s] [%(levelname)s] [%(name)s] %(message)s", force=True)
    logger = logging.getLogger("probe1d")
    run = disk.Run(cfg.run)
    splits = {"Train": pathlib.Path(cfg.train_shards), "Test": pathlib.Path(cfg.test_shards)}
    for name, dpath in splits.items():
        if not dpath.exists():
            logger.error("%s shards directory %s does not exist.", name, dpath)
            return 1
    for name, dpath in splits.items():
        if not (dpath / "labels.bin").exists():
            logger.error("%s shards directory %s is missing labels.bin.", name, dpath)
            return 1
    for name, dpath in splits.items():
        if not (run.inference / dpath.name).exists():
            logger.error("%s inference directory %s doesn't exist. Use inference.py to run inference.", name, run.inference / dpath.name)
            return 1
    for name, dpath in splits.items():
        if not (run.inference / dpath.name / "token_acts.npz").exists():
            logger.error("%s inference directory %s is missing token_acts.npz.", name, run.inference / dpath.name)
            return 1

    acts, labels = {}, {}
    for name, dpath in splits.items():
        md = saev_data.Metadata.load(dpath)
        csr = scipy.sparse.load_npz(run.inference / dpath.name / "token_acts.npz").tocsr()
        logger.info("Loaded %s activations: shape=%s, nnz=%d.", name.lower(), csr.shape, csr.nnz)
        n_expected = md.n_examples * md.content_tokens_per_example
        if n_expected != csr.shape[0]:
            logger.error("%s labels expect %d samples but activations have %d.", name, n_expected, csr.shape[0])
            return 1
        acts[name] = csr
        labels[name] = np.memmap(dpath / "labels.bin", mode="r", dtype=np.uint8, shape=(n_expected,))
    n_classes = max(int(v.max()) for v in labels.values()) + 1
    logger.info("Found %d classes across train/test labels.", n_classes)
    if acts["Train"].shape[1] != acts["Test"].shape[1]:
        logger.error("Train latents %d differ from test latents %d.", acts["Train"].shape[1], acts["Test"].shape[1])
        return 1

    # the class ids go to the device as they are: the N x C one-hot matrix the reference builds is never needed
    probe = Sparse1DProbe(n_latents=acts["Train"].shape[1], n_classes=n_classes, device=cfg.device, ridge=cfg.ridge, max_iter=cfg.max_iter,
                          class_slab_size=cfg.class_slab_size, row_batch_size=cfg.row_batch_size)
    y = {name: torch.from_numpy(np.array(v)) for name, v in labels.items()}  # (a copy: the files are mapped read-only)
    logger.info("Fitting probe on train split with %d samples.", acts["Train"].shape[0])
    probe.fit(acts["Train"], y["Train"])
    for name, dpath in splits.items():
        out_fpath = run.inference / dpath.name / "probe1d_metrics.npz"
        _save(out_fpath, probe, probe.loss_matrix_with_aux(acts[name], y[name]))
        logger.info("Saved %s probe outputs to %s.", name.lower(), out_fpath)
    return 0
