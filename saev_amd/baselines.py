"""The k-means baseline beside the SAEs: the surface of the reference's ``tdiscovery.baselines`` (``MiniBatchKMeans``, ``TrainConfig``,
``InferenceConfig``, ``train_worker_fn``, ``eval_kmeans``, ``dump`` / ``load``, ``inference_worker_fn``) over the HIP kernels of
include/saev_amd.h: K-MEANS.  Written from that module's contract: same names, same checkpoint file, same
artifacts; a step never forms an n x k or k x k distance matrix.

``method="pca"`` and ``method="semi-nmf"`` are not built (an eigendecomposition and dense GEMMs with a solve: nothing for a
kernel of this package to win); asking for them raises NotImplementedError.  ``partial_fit`` needs a HIP device; ``load`` and
``transform`` work on the CPU."""

from __future__ import annotations

import dataclasses
import io
import json
import logging
import pathlib
import time
import typing as tp
import uuid

import numpy as np
import scipy.sparse
import torch

from . import __version__, disk, engine
from . import data as saev_data
from .framework.inference import Filepaths, _jsonable
from .metrics import Metrics
from .utils import scheduling

BaselineMethod = tp.Literal["kmeans", "pca", "semi-nmf"]
BASELINE_SCHEMA_VERSION = 1
BASELINE_CKPT_NAME = "baseline.pt"

logger = logging.getLogger("baselines.py")


def _require_kmeans(method: str) -> None:
    if method in ("pca", "semi-nmf"):
        raise NotImplementedError(f"baseline method {method!r} is not built in saev_amd (only 'kmeans' is; DESIGN.md 7)")
    if method != "kmeans":
        raise ValueError(f"unknown baseline method {method!r} (the reference has 'kmeans', 'pca', 'semi-nmf')")


def _draw(fn: str, *args, **kwargs) -> torch.Tensor:
    """Every random draw of this module: ``torch.<fn>(*args, **kwargs)`` with the reference's arguments (the initial
    ``randperm(n, device=...)``, the replacement rows ``randint(0, n, (m,), device=...)``).  A test replays recorded draws by
    patching this one function."""
    return getattr(torch, fn)(*args, **kwargs)


def _baseline_ckpt(run: disk.Run) -> pathlib.Path:
    """Baseline runs reuse the SAE run layout and write their weights to ``checkpoint/baseline.pt``."""
    return run.ckpt.parent / BASELINE_CKPT_NAME


class MiniBatchKMeans(torch.nn.Module):
    """Mini-batch k-means with the reference estimator's API and arithmetic: fp32 state, the running-mean update in the order of
    a one-thread ``index_add_``, empty clusters replaced by drawn rows, collapsed centres (pairs closer than ``collapse_tol``)
    re-seeded from the batch's farthest points.  Every decision (nearest centre, pairs under the tolerance, farthest points) is
    taken on exactly recomputed fp32 distances with ties to the lower index."""

    method = "kmeans"

    def __init__(self, k: int, device: str = "cuda", collapse_tol: float = 0.5):
        super().__init__()
        self.k = k
        self.device = torch.device(device)
        self.cluster_centers_: torch.Tensor | None = None
        self.cluster_counts_: torch.Tensor | None = None
        self.n_steps_: int = 0
        self.n_features_in_: int | None = None
        self.last_batch_inertia_: float | None = None
        self.collapse_tol = collapse_tol
        self.last_assign_: dict | None = None  # route, candidates, capacity, overflow, tiles_refiltered of the last step's assign
        self._zero_counts = True  # some centre may have count 0 (only then can a cluster be "empty")

    def partial_fit(self, batch: torch.Tensor) -> "MiniBatchKMeans":
        assert batch.ndim == 2, f"batch must be 2D, got {batch.shape}"
        if self.device.type != "cuda":
            raise RuntimeError("saev_amd MiniBatchKMeans.partial_fit runs on a HIP device only (there is no CPU path)")
        x = batch.to(self.device)
        if x.dtype != torch.float32:
            raise ValueError(f"partial_fit takes float32 activations, got {x.dtype}")
        x = x.contiguous()
        n, d = x.shape
        if self.n_features_in_ is not None and d != self.n_features_in_:
            raise ValueError(f"partial_fit: the model was fitted on rows of width {self.n_features_in_}, this batch has width {d}")
        fresh = self.cluster_centers_ is None
        # (the first batch seeds local tensors: they become the state only once that batch is known to be finite)
        centers, counts = self._initial_centers(x) if fresh else (self.cluster_centers_, self.cluster_counts_)
        # words 0-3 assign info | 4-7 collapsed info | 8 losers | 9 centres with count 0 | 10-11 the inertia (one double)
        words = torch.zeros(12, device=x.device, dtype=torch.int32)
        dist2, idx, _ = engine.kmeans_assign_device(x, centers, info=words[0:4])
        batch_counts, starts, rows = engine.kmeans_group(idx, self.k)
        repl = None
        if fresh or self._zero_counts:  # (the first steps, and the step after a re-seeding: one more small read-back)
            empty = (counts == 0) & (batch_counts == 0)
            head = torch.cat([words[0:1], empty.sum().to(torch.int32).reshape(1)]).cpu().tolist()
            engine._kmeans_info("partial_fit", [head[0], 0, 0, 0])  # raises on a non-finite batch, before anything is committed
            if fresh:
                self.cluster_centers_, self.cluster_counts_, self.n_features_in_ = centers, counts, int(d)
            if head[1] > 0:
                drawn = _draw("randint", 0, n, (head[1],), device=x.device)
                repl = torch.full((self.k,), -1, device=x.device, dtype=torch.int32)
                repl[empty] = drawn.to(torch.int32)
        # (a non-finite batch left every index at -1: no centre has rows, nothing below changes the state, and the read-back raises)
        engine.kmeans_update(x, starts, rows, centers, counts, repl_rows=repl, dist2=dist2, out_inertia=words[10:12].view(torch.float64))
        losers = None
        if self.k >= 2:
            losers, _ = engine.kmeans_collapsed_device(centers, counts, self.collapse_tol, info=words[4:8])
            words[8:9].copy_(losers.sum())
        words[9:10].copy_((counts == 0).sum())
        host = words.cpu()
        self.last_assign_ = engine._kmeans_info("partial_fit", host[0:4].tolist())
        self.last_batch_inertia_ = float(host[10:12].view(torch.float64).item())
        self._zero_counts = int(host[9]) > 0
        if int(host[8]) > 0:
            self._reseed(x, losers, int(host[8]))
        self.n_steps_ += 1
        return self

    def _initial_centers(self, batch: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
        """(centres, counts) seeded from the first batch: k rows of a random permutation, or the batch repeated when it is short."""
        n = batch.shape[0]
        if n >= self.k:
            initial = batch[_draw("randperm", n, device=batch.device)[: self.k]]
        else:
            initial = batch.repeat((-(-self.k // n), 1))[: self.k]
        return initial.clone().contiguous(), torch.zeros(self.k, device=batch.device, dtype=batch.dtype)

    def _reseed(self, batch: torch.Tensor, losers: torch.Tensor, n_needed: int) -> None:
        """The losers become the batch's points farthest from every centre (largest distance to its farthest centre first, ties to
        the lower row; the batch repeated when it has fewer rows than losers), with count 0."""
        far = engine.kmeans_assign(batch, self.cluster_centers_, farthest=True)
        scores = torch.sqrt(far.dist2)
        n = batch.shape[0]
        if n < n_needed:
            scores = scores.repeat(-(-n_needed // n))
        pick = torch.argsort(scores, descending=True, stable=True)[:n_needed] % n
        self.cluster_centers_[losers] = batch[pick]
        self.cluster_counts_[losers] = 0.0
        self._zero_counts = True

    def transform(self, batch: torch.Tensor) -> torch.Tensor:
        if self.cluster_centers_ is None:
            raise RuntimeError("transform needs centres: call partial_fit or load a checkpoint first")
        return -torch.cdist(batch.to(self.device), self.cluster_centers_)


@dataclasses.dataclass(frozen=True)
class TrainConfig:
    """The reference's field names and defaults.  The fields of the other methods (z_iters .. d_update_every) and the SLURM,
    wandb and logging fields (slurm_*, n_hours, mem_gb, log_to, debug, track, wandb_project, tag) are accepted and ignored."""

    method: BaselineMethod = "kmeans"
    train_data: saev_data.ShuffledConfig = saev_data.ShuffledConfig()
    val_data: saev_data.ShuffledConfig = saev_data.ShuffledConfig()
    n_train: int = 100_000_000
    n_val: int = 10_000_000
    k: int = 1024 * 16
    collapse_tol: float = 0.5
    z_iters: int = 10
    encode_iters: int = 300
    ridge: float = 1e-6
    eps: float = 1e-8
    forget_factor: float = 0.7
    d_update_every: int = 10
    device: tp.Literal["cuda", "cpu"] = "cuda"
    seed: int = 42
    runs_root: pathlib.Path = pathlib.Path("./tdiscovery/runs")
    slurm_acct: str = ""
    slurm_partition: str = ""
    n_hours: float = 24.0
    mem_gb: int = 128
    log_to: pathlib.Path = pathlib.Path("./logs")
    debug: bool = False
    track: bool = True
    wandb_project: str = "tdiscovery"
    tag: str = ""
    log_every: int = 50


@dataclasses.dataclass(frozen=True)
class InferenceConfig:
    """The reference's field names and defaults; n_iters (Semi-NMF) and the SLURM fields are accepted and ignored."""

    run: pathlib.Path = pathlib.Path("./tdiscovery/runs/example")
    data: saev_data.OrderedConfig = saev_data.OrderedConfig()
    device: tp.Literal["cuda", "cpu"] = "cuda"
    seed: int = 42
    n_dists: int = 25
    n_iters: int = 300
    save: bool = True
    force: bool = False
    slurm_acct: str = ""
    slurm_partition: str = ""
    n_hours: float = 4.0
    mem_gb: int = 80
    log_to: pathlib.Path = pathlib.Path("./logs")


def _git_commit() -> str:
    import subprocess

    try:
        out = subprocess.run(["git", "rev-parse", "HEAD"], cwd=pathlib.Path(__file__).resolve().parent, capture_output=True, text=True,
                             timeout=10)
        return out.stdout.strip() if out.returncode == 0 and out.stdout.strip() else "unknown"
    except (OSError, subprocess.SubprocessError):
        return "unknown"


def load(run: disk.Run, *, device: str = "cpu") -> MiniBatchKMeans:
    """The model of ``checkpoint/baseline.pt``: one JSON header line, then a ``torch.save`` of the state dict -- the reference's
    format, so its files load here and the files of ``dump`` load there."""
    with open(_baseline_ckpt(run), "rb") as fd:
        header = json.loads(fd.readline())
        buffer = io.BytesIO(fd.read())
    _require_kmeans(header["method"])
    state = torch.load(buffer, map_location=device, weights_only=False)
    assert isinstance(state, dict), f"Unexpected checkpoint payload in {_baseline_ckpt(run)}"
    centers = state["cluster_centers"]
    model = MiniBatchKMeans(k=centers.shape[0], device=device, collapse_tol=state["collapse_tol"])
    model.cluster_centers_ = centers.to(device).contiguous()
    model.cluster_counts_ = state["cluster_counts"].to(device)
    model.n_steps_ = state["n_steps"]
    model.n_features_in_ = centers.shape[1]
    return model


def dump(run: disk.Run, cfg: TrainConfig, model: MiniBatchKMeans) -> pathlib.Path:
    """``checkpoint/config.json`` and ``checkpoint/baseline.pt`` (header keys method, schema, commit, lib; state keys
    cluster_centers, cluster_counts, n_steps, n_features_in, collapse_tol)."""
    _require_kmeans(model.method)
    assert model.cluster_centers_ is not None and model.cluster_counts_ is not None and model.n_features_in_ is not None
    header = {"method": model.method, "schema": BASELINE_SCHEMA_VERSION, "commit": _git_commit(), "lib": __version__}
    state = {
        "cluster_centers": model.cluster_centers_.cpu(),
        "cluster_counts": model.cluster_counts_.cpu(),
        "n_steps": model.n_steps_,
        "n_features_in": model.n_features_in_,
        "collapse_tol": float(model.collapse_tol),
    }
    ckpt_dir = run.ckpt.parent
    ckpt_dir.mkdir(parents=True, exist_ok=True)
    with open(ckpt_dir / "config.json", "w") as fd:
        json.dump(_jsonable(cfg), fd, indent=2)
    path = _baseline_ckpt(run)
    with open(path, "wb") as fd:
        fd.write(json.dumps(header).encode() + b"\n")
        torch.save(state, fd)
    return path


def get_training_metrics(model: MiniBatchKMeans, n_samples: int) -> dict[str, float]:
    return {"train/inertia": model.last_batch_inertia_ or 0.0, "train/l0": 1.0, "train/n_samples": n_samples}


def _loader_device(model: MiniBatchKMeans) -> torch.device:
    if model.device.type != "cuda":
        raise RuntimeError("saev_amd baselines run on a HIP device only (there is no CPU path)")
    return model.device


def eval_kmeans(cfg: TrainConfig, model: MiniBatchKMeans) -> dict[str, float]:
    """eval/inertia, eval/utilization, eval/mean_pop, eval/max_pop over min(n_val, the cache) validation rows; the populations
    are accumulated on the device from the batch counts of kmeans_group."""
    if cfg.n_val <= 0:
        return {}
    device = _loader_device(model)
    dl = saev_data.ShuffledDataLoader(cfg.val_data, device=device)
    limiter = scheduling.BatchLimiter(dl, min(cfg.n_val, dl.n_samples))
    centers = model.cluster_centers_
    hits = torch.zeros(centers.shape[0], device=device, dtype=torch.int64)
    sse = torch.zeros((), device=device, dtype=torch.float64)
    total = 0
    for batch in limiter:
        acts = batch["act"].to(device)
        res = engine.kmeans_assign(acts, centers)
        hits += engine.kmeans_group(res.indices, centers.shape[0])[0]
        sse += res.dist2.double().sum()
        total += acts.shape[0]
    if total == 0:
        return {}
    pop = hits.to(torch.float32)
    return {"eval/inertia": sse.item() / total, "eval/utilization": (hits > 0).float().mean().item(), "eval/mean_pop": pop.mean().item(),
            "eval/max_pop": pop.max().item()}


def train_worker_fn(cfg: TrainConfig) -> disk.Run:
    """Fit on ``n_train`` shuffled rows, evaluate, lay out a run directory and write the checkpoint; returns the run."""
    _require_kmeans(cfg.method)
    torch.manual_seed(cfg.seed)
    model = MiniBatchKMeans(k=cfg.k, device=cfg.device, collapse_tol=cfg.collapse_tol)
    device = _loader_device(model)
    dl = scheduling.BatchLimiter(saev_data.ShuffledDataLoader(cfg.train_data, device=device), cfg.n_train)
    n_samples = 0
    t_start = time.perf_counter()
    for batch in dl:
        acts = batch["act"]
        assert acts.ndim == 2, f"Expected 2D activations, got shape {tuple(acts.shape)}"
        model.partial_fit(acts)
        n_samples += acts.shape[0]
        if model.n_steps_ % cfg.log_every == 0:
            logger.info(", ".join(f"{key}={value}" for key, value in get_training_metrics(model, n_samples).items()))
    logger.info("Training complete: method=%s steps=%d samples=%d elapsed=%.2fs", cfg.method, model.n_steps_, n_samples,
                time.perf_counter() - t_start)
    for key, value in eval_kmeans(cfg, model).items():
        logger.info("%s=%.6f", key, value)
    run = disk.Run.new(uuid.uuid4().hex[:8], train_shards_dir=pathlib.Path(cfg.train_data.shards).resolve(),
                       val_shards_dir=pathlib.Path(cfg.val_data.shards).resolve(), runs_root=cfg.runs_root)
    logger.info("Saved checkpoint to %s", dump(run, cfg, model))
    return run


@torch.inference_mode()
def inference_worker_fn(cfg: InferenceConfig) -> Metrics | None:
    """One ordered pass over a cache with a k-means run: ``token_acts.npz`` (CSR, one entry per token: column = the nearest
    centre, value = 1 / (1 + distance)), ``mean_values.pt``, ``sparsity.pt``, ``distributions.pt`` (``save=True`` only) and
    ``metrics.json`` with sse_recon = the sum of squared distances.  Nothing is recomputed unless a file is missing or ``force``."""
    run = disk.Run(cfg.run)
    md = saev_data.Metadata.load(cfg.data.shards)
    fpaths = Filepaths.from_run(run, md)
    required = list(fpaths) if cfg.save else [fpaths.metrics]
    missing = [f for f in required if not f.exists()]
    if not cfg.force and not missing:
        logger.info("Found all required files; skipping.")
        return None
    model = load(run, device=cfg.device)
    device = _loader_device(model)
    centers = model.cluster_centers_
    k, d_model = centers.shape
    T = md.content_tokens_per_example
    batch_size = cfg.data.batch_size // T * T
    if batch_size <= 0:
        raise ValueError(f"data.batch_size = {cfg.data.batch_size} holds no whole example ({T} tokens each)")
    dl = saev_data.OrderedDataLoader(dataclasses.replace(cfg.data, batch_size=batch_size), device=device)
    with open(fpaths.metrics.parent / "config.json", "w") as fd:
        json.dump(_jsonable(cfg), fd, indent=2)

    value_sum = torch.zeros(k, device=device, dtype=torch.float64)  # (fp64: the mean is then one rounding away from its values')
    n_hit = torch.zeros(k, device=device, dtype=torch.int64)
    distributions = torch.zeros((dl.n_samples, cfg.n_dists) if cfg.save else (0, 0), dtype=torch.float32)
    cols: list[np.ndarray] = []
    vals: list[np.ndarray] = []
    sse = torch.zeros((), dtype=torch.float64, device=device)
    sum_sq = torch.zeros((), dtype=torch.float64, device=device)
    sum_vec = torch.zeros(d_model, dtype=torch.float64, device=device)
    n_tokens, prev_i = 0, -1
    for batch in dl:
        acts = batch["act"].to(device)
        res = engine.kmeans_assign(acts, centers)
        if cfg.save:
            scores = 1.0 / (1.0 + torch.sqrt(res.dist2))
            assign = res.indices.long()
            n_hit += engine.kmeans_group(res.indices, k)[0]
            value_sum.index_add_(0, assign, scores.double())
            g = batch["example_idx"] * T + batch["token_idx"]
            assert g[0].item() == prev_i + 1 and bool((g[1:] == g[:-1] + 1).all()), "batches must arrive in global order"
            prev_i = int(g[-1].item())
            assign_cpu, scores_cpu = assign.cpu(), scores.cpu()
            cols.append(assign_cpu.numpy().astype(np.int32))
            vals.append(scores_cpu.numpy())
            shown = torch.nonzero(assign_cpu < cfg.n_dists).flatten()  # tokens whose centre is one of the first n_dists
            if shown.numel() > 0:
                distributions[batch["example_idx"].cpu().long()[shown], assign_cpu[shown]] = scores_cpu[shown]
        sse += res.dist2.double().sum()
        acts64 = acts.double()
        sum_sq += (acts64 * acts64).sum()
        sum_vec += acts64.sum(dim=0)
        n_tokens += acts.shape[0]
    assert n_tokens == dl.n_samples and n_tokens > 0
    if cfg.save:
        col = np.concatenate(cols)
        token_acts = scipy.sparse.csr_matrix((np.concatenate(vals), col, np.arange(n_tokens + 1, dtype=np.int64)), shape=(n_tokens, k))
        scipy.sparse.save_npz(fpaths.token_acts, token_acts)
        pop = n_hit.cpu()
        torch.save((value_sum.cpu() / pop.double()).float(), fpaths.mean_values)  # 0 / 0 = NaN: a centre no token chose
        torch.save(pop.to(torch.float32) / dl.n_samples, fpaths.sparsity)  # (on the host: one correctly rounded division)
        torch.save(distributions, fpaths.distributions)
    sse_baseline = sum_sq.item() - torch.dot(sum_vec, sum_vec).item() / n_tokens
    if not sse_baseline > 0.0:
        raise ValueError(f"the activations have no variance about their mean (sum of squares {sse_baseline:.6e}): nothing to normalise the MSE by")
    metrics = Metrics.from_accumulators(sse_recon=sse.item(), sse_baseline=sse_baseline, n_tokens=n_tokens, d_model=d_model)
    with open(fpaths.metrics, "w") as fd:
        json.dump(metrics.to_dict(), fd, indent=2)
    return metrics
