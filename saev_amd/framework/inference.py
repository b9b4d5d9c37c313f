"""One ordered pass over a cache that dumps a trained SAE's inference artifacts
(reference src/saev/framework/inference.py:1-285).

Writes under ``<run>/inference/<metadata hash>/``:

    config.json        the inference config
    metrics.json       saev_amd.metrics.Metrics (fp64 accumulators: SSE of the SAE, SSE of the mean predictor)
    token_acts.npz     scipy CSR (n_tokens, d_sae) of the sparse codes            (save=True only)
    mean_values.pt     (d_sae,) sum of activations / number of tokens with f > 0   (save=True only)
    sparsity.pt        (d_sae,) fraction of tokens with f > 0                      (save=True only)
    distributions.pt   (n_tokens, n_dists), rows written at ``example_idx``        (save=True only)
    top_tokens.pt      {"values" (k, d_sae) float32, "indices" (k, d_sae) int64, "counts" (d_sae,) int64}: per latent the k largest
                       activations and the global token rows (rows of token_acts.npz) they sit in, what the reference's
                       ``helpers.csr_topk(token_acts, k=k, axis=0)`` returns   (``worker_fn(cfg, top_k_tokens=k)`` only)
    activation_hist.pt {"counts0" (d_sae, 4096) int32 (int64 once a count passes 2^31 - 1), "n_rows" int}: per latent the histogram
                       of its non-zero activations over sign, exponent and three mantissa bits (engine.LatentHist;
                       ``engine.hist_window`` cuts octaves out of it), and the kept tokens (rebuilt from token_acts.npz: its
                       rows)                                                   (``worker_fn(cfg, activation_hist=True)`` only)

The reference materialises the dense (B, d_sae) ``f_x`` per batch, copies it to the host and lets scipy compress it
(inference.py:189-246).  Here the codes never leave their sparse form: the HIP encoder returns (idx, val) with
ascending latent indices per row, which *is* a CSR block; per-latent sums are index-adds over the B*k codes.  A ReLU SAE
takes the same route with padded variable-length rows (SaeEngine.encode_relu: the first row_nnz entries of each row, also in
ascending latent order) and their decode (SaeEngine.decode_rows); its SSE is summed in fp64 from x_hat.
"""

from __future__ import annotations

import collections.abc
import dataclasses
import json
import logging
import os
import pathlib

import numpy as np
import scipy.sparse
import torch

from .. import disk, helpers, nn
from ..data import Metadata, OrderedConfig, OrderedDataLoader
from ..engine import BatchStats, LatentHist, LatentTopK
from ..metrics import Metrics

logger = logging.getLogger("inference.py")


@dataclasses.dataclass(frozen=True)
class Config:
    """Field names and defaults of inference.py:42-75."""

    run: pathlib.Path = pathlib.Path("./runs/abcdefg")
    data: OrderedConfig = OrderedConfig()
    n_dists: int = 25
    ignore_labels: list[int] = dataclasses.field(default_factory=list)
    force_recompute: bool = False
    save: bool = True
    device: str = "cuda"
    slurm_acct: str = ""
    slurm_partition: str = ""
    n_hours: float = 4.0
    mem_gb: int = 80
    log_to: str = os.path.join(".", "logs")


@dataclasses.dataclass(frozen=True)
class Filepaths:
    mean_values: pathlib.Path
    sparsity: pathlib.Path
    distributions: pathlib.Path
    token_acts: pathlib.Path
    metrics: pathlib.Path

    @classmethod
    def from_run(cls, run: disk.Run, md: Metadata) -> "Filepaths":
        root = run.inference / md.hash
        root.mkdir(exist_ok=True, parents=True)
        return cls(mean_values=root / "mean_values.pt", sparsity=root / "sparsity.pt",
                   distributions=root / "distributions.pt", token_acts=root / "token_acts.npz",
                   metrics=root / "metrics.json")

    def __iter__(self) -> collections.abc.Iterator[pathlib.Path]:
        yield from (self.mean_values, self.sparsity, self.distributions, self.token_acts, self.metrics)


def _shards_dir(cfg: Config) -> pathlib.Path:
    return pathlib.Path(os.path.expandvars(str(cfg.data.shards)))


def need_compute(cfg: Config) -> tuple[bool, str, Filepaths]:
    """(inference.py:108-134) recompute when forced or when a required output is missing."""
    run = disk.Run(cfg.run)
    fpaths = Filepaths.from_run(run, Metadata.load(_shards_dir(cfg)))
    required, mode = (list(fpaths), "full artifacts") if cfg.save else ([fpaths.metrics], "metrics only")
    missing = [f for f in required if not f.exists()]
    if cfg.force_recompute:
        return True, f"Force recompute flag set; computing {mode}.", fpaths
    if not missing:
        return False, f"Found all required files ({mode}).", fpaths
    return True, f"Missing files {', '.join(str(f) for f in missing)}; computing {mode}.", fpaths


def _jsonable(o):
    if dataclasses.is_dataclass(o) and not isinstance(o, type):
        return {f.name: _jsonable(getattr(o, f.name)) for f in dataclasses.fields(o)}
    if isinstance(o, pathlib.Path):
        return str(o)
    if isinstance(o, (list, tuple)):
        return [_jsonable(v) for v in o]
    if isinstance(o, dict):
        return {k: _jsonable(v) for k, v in o.items()}
    return o


TOP_TOKENS = "top_tokens.pt"


def _save_top_tokens(path: pathlib.Path, values, indices, counts) -> None:
    torch.save({"values": values, "indices": indices, "counts": counts}, path)


def _top_tokens_current(path: pathlib.Path, k: int, d_sae: int) -> bool:
    """Whether ``path`` holds lists of this k for this many latents (a file of another k is rebuilt, never handed out as k's)."""
    if not path.exists():
        return False
    values = torch.load(path)["values"]
    return tuple(values.shape) == (k, d_sae)


ACTIVATION_HIST = "activation_hist.pt"


def _save_activation_hist(path: pathlib.Path, hist: LatentHist) -> None:
    counts0 = hist.counts0  # uint32 counters in an int32 tensor: kept as int32 while every count fits, the file is half the size
    torch.save({"counts0": hist.read() if bool((counts0 < 0).any()) else counts0.cpu(), "n_rows": int(hist.n_rows.item())}, path)


def _activation_hist_current(path: pathlib.Path, d_sae: int) -> bool:
    """Whether ``path`` holds the table of this many latents."""
    return path.exists() and tuple(torch.load(path)["counts0"].shape) == (d_sae, 4096)


@torch.inference_mode()
def worker_fn(cfg: Config, *, top_k_tokens: int = 0, activation_hist: bool = False):
    """``top_k_tokens`` = k > 0 also keeps, per latent, the k largest activations of the pass and their global token rows
    (engine.LatentTopK, fed from the codes on the device) and writes them as ``top_tokens.pt``.  When the pass is up to date, a
    ``top_tokens.pt`` that is missing or holds another k is rebuilt from ``token_acts.npz``.  0 keeps no lists; a pass that rewrites
    ``token_acts.npz`` without them removes a ``top_tokens.pt`` left by an earlier pass, which would no longer describe it.

    ``activation_hist`` also keeps every latent's activation histogram (engine.LatentHist, fed from the codes on the device) and writes
    it as ``activation_hist.pt``, under the same policy: rebuilt from ``token_acts.npz`` when the pass is up to date and the file is
    missing or describes another pass, removed by a pass that rewrites ``token_acts.npz`` without it."""
    if top_k_tokens < 0 or top_k_tokens > LatentTopK.MAX_K:
        raise ValueError(f"top_k_tokens must lie in [0, {LatentTopK.MAX_K}], got {top_k_tokens}")
    run = disk.Run(cfg.run)
    md = Metadata.load(_shards_dir(cfg))
    root = run.inference / md.hash
    do, reason, fpaths = need_compute(cfg)
    logger.info(reason)
    if not do:
        if activation_hist and fpaths.token_acts.exists():
            token_acts = scipy.sparse.load_npz(fpaths.token_acts).tocsr()
            if not _activation_hist_current(root / ACTIVATION_HIST, token_acts.shape[1]):
                device = torch.device(cfg.device)
                if device.type != "cuda":
                    raise RuntimeError("saev_amd inference runs on a HIP device only (there is no CPU path)")
                hist = LatentHist(token_acts.shape[1], device)
                for r0 in range(0, token_acts.shape[0], 2**20):
                    block = token_acts[r0:r0 + 2**20]
                    hist.add_csr(torch.from_numpy(block.indptr.astype(np.int64)).to(device), torch.from_numpy(block.indices.astype(np.int32)).to(device),
                                 torch.from_numpy(block.data.astype(np.float32)).to(device))
                _save_activation_hist(root / ACTIVATION_HIST, hist)
        if top_k_tokens > 0 and fpaths.token_acts.exists():
            # the pass is up to date; lists that are missing, or were kept for another k, are selected from the saved codes
            token_acts = scipy.sparse.load_npz(fpaths.token_acts).tocsr()
            if _top_tokens_current(root / TOP_TOKENS, top_k_tokens, token_acts.shape[1]):
                return
            device = torch.device(cfg.device)
            if device.type != "cuda":
                raise RuntimeError("saev_amd inference runs on a HIP device only (there is no CPU path)")
            got = helpers._topk_axis0(token_acts, top_k_tokens, 1024, device)
            counts = np.minimum(np.bincount(token_acts.indices[token_acts.data != 0], minlength=token_acts.shape[1]), top_k_tokens)
            _save_top_tokens(root / TOP_TOKENS, torch.from_numpy(got.values.astype(np.float32)), torch.from_numpy(got.indices),
                             torch.from_numpy(counts.astype(np.int64)))
        return
    with open(root / "config.json", "w") as fd:
        json.dump(_jsonable(cfg), fd)
    assert cfg.data.tokens == "content"
    device = torch.device(cfg.device)
    if device.type != "cuda":
        raise RuntimeError("saev_amd inference runs on a HIP device only (there is no CPU path)")
    sae = nn.load(run.ckpt, device=device)
    S, D = sae.cfg.d_sae, sae.cfg.d_model
    T = md.content_tokens_per_example
    batch_size = cfg.data.batch_size // T * T  # whole examples per batch (inference.py:158-165)
    loader = OrderedDataLoader(dataclasses.replace(cfg.data, batch_size=batch_size), device=device)
    eng = sae._eng(batch_size)
    batch_topk = isinstance(sae.cfg.activation, nn.modeling.BatchTopK)
    # padded variable-length rows: a ReLU SAE's positives, a BatchTopK SAE's eval-mode codes (h > threshold, all positive too)
    relu = batch_topk or isinstance(sae.cfg.activation, nn.modeling.Relu)

    # every sum of the pass -- column sums of x, sum x^2 and sum (x - x_hat)^2 over the kept rows in fp64, per-latent positive
    # counts and value sums -- from one kernel per batch, TopK or ReLU, masked or not (engine.BatchStats)
    acc = BatchStats(D, S, device, want=("scalars", "col_sum", "n_pos", "value_sum") if cfg.save else ("scalars", "col_sum"))
    top = LatentTopK(S, top_k_tokens, device) if top_k_tokens > 0 else None
    hist = LatentHist(S, device) if activation_hist else None
    if cfg.save:
        distributions = np.zeros((loader.n_samples, cfg.n_dists), dtype=np.float32)
        csr_data: list[np.ndarray] = []
        csr_cols: list[np.ndarray] = []
        csr_counts: list[np.ndarray] = []
    ignore = torch.tensor(cfg.ignore_labels, dtype=torch.int64)
    sse_own, sum_sq_own = 0.0, 0.0  # unmasked TopK batches: the step's own fp64 reductions
    n_tokens = 0
    prev_i = -1
    logger.info("Loaded SAE and data.")

    for batch in loader:
        x = batch["act"]
        b = x.shape[0]
        if relu:
            idx, val, row_nnz = eng.encode_batch_topk(x, training=False) if batch_topk else eng.encode_relu(x)
            x_hat = eng.decode_rows(idx, val, row_nnz)[:, 0]
        else:
            eng.step_forward(x, training=False)
        keep_host = torch.ones(b, dtype=torch.bool)
        if "token_labels" in batch:  # segmentation caches: drop tokens whose label is ignored
            keep_host = torch.isin(batch["token_labels"], ignore, invert=True)
        n_keep = int(keep_host.sum())
        n_tokens += n_keep
        keep = keep_host.to(device)
        if n_keep > 0:
            mask = None if n_keep == b else keep
            if relu:
                acc.add(x, x_hat, idx, val, row_nnz, mask)
            elif mask is None:
                st = eng.read_stats()  # fp64 sums of this batch from the step's own reduction
                sse_own += st.sse
                sum_sq_own += st.sum_sq
                eng.add_batch_stats(acc, x, x_hat=False, scalars=False)
            else:
                eng.add_batch_stats(acc, x, mask)
            if top is not None:  # the batch's first global token index: the rows of token_acts.npz
                row_base = int(batch["example_idx"][0]) * T + int(batch["token_idx"][0])
                if relu:
                    top.add(idx, val, row_nnz, mask, row_base=row_base)
                else:
                    eng.add_latent_topk(top, mask, row_base=row_base)
            if hist is not None:
                if relu:
                    hist.add(idx, val, row_nnz, mask)
                else:
                    hist.add(*eng.last_codes(b, x_hat=False)[:2], None, mask)
        if not cfg.save:
            continue
        if not relu:
            idx, val, _ = eng.last_codes(b, x_hat=False)

        g = batch["example_idx"] * T + batch["token_idx"]
        assert g[0].item() == prev_i + 1 and bool((g[1:] == g[:-1] + 1).all()), "batches must arrive in global order"
        prev_i = int(g[-1].item())

        if relu:  # the row's first row_nnz entries, all > 0
            live = (torch.arange(idx.shape[1], device=device)[None, :] < row_nnz[:, None]) & keep[:, None]
        else:
            live = (val != 0) & keep[:, None]  # what a dense -> CSR conversion of the masked f_x would keep
        cols, vals = idx[live].long(), val[live]
        csr_counts.append(live.sum(dim=1).cpu().numpy())
        csr_cols.append(cols.to(torch.int32).cpu().numpy())
        csr_data.append(vals.cpu().numpy())
        # first n_dists latents of every kept token, stored at row example_idx (last token of an example wins)
        head = torch.zeros(b, cfg.n_dists, device=device)
        small = live & (idx < cfg.n_dists)
        rows = torch.arange(b, device=device)[:, None].expand_as(idx)[small]
        head[rows, idx[small].long()] = val[small]
        distributions[batch["example_idx"][keep_host].numpy()] = head.cpu().numpy()[keep_host.numpy()]

    got = acc.read()
    if top is not None:
        lists = top.read()
        _save_top_tokens(root / TOP_TOKENS, lists.values, lists.indices, lists.counts)
    elif cfg.save:
        (root / TOP_TOKENS).unlink(missing_ok=True)  # lists of an earlier pass do not describe the token_acts.npz written below
    if hist is not None:
        _save_activation_hist(root / ACTIVATION_HIST, hist)
    elif cfg.save:
        (root / ACTIVATION_HIST).unlink(missing_ok=True)
    if cfg.save:
        counts = np.concatenate(csr_counts) if csr_counts else np.zeros(0, dtype=np.int64)
        indptr = np.zeros(counts.shape[0] + 1, dtype=np.int64)
        np.cumsum(counts, out=indptr[1:])
        nnz = int(indptr[-1])
        itype = np.int32 if max(nnz, S) < 2**31 else np.int64
        token_acts = scipy.sparse.csr_array(
            (np.concatenate(csr_data) if csr_data else np.zeros(0, np.float32),
             (np.concatenate(csr_cols) if csr_cols else np.zeros(0, np.int32)).astype(itype), indptr.astype(itype)),
            shape=(counts.shape[0], S))
        scipy.sparse.save_npz(fpaths.token_acts, token_acts)
        torch.save((got.value_sum / got.n_pos.to(torch.float64)).to(torch.float32), fpaths.mean_values)  # 0 / 0 = NaN: never positive
        torch.save(got.n_pos.to(torch.float32) / loader.n_samples, fpaths.sparsity)
        torch.save(torch.from_numpy(distributions), fpaths.distributions)

    assert n_tokens > 0, "Inference dataloader yielded zero valid tokens; cannot compute metrics."
    sse, sum_sq, sum_vec = sse_own + got.sum_rr, sum_sq_own + got.sum_xx, got.col_sum
    sse_baseline = sum_sq - torch.dot(sum_vec, sum_vec).item() / n_tokens
    if sse_baseline <= 0.0:
        raise RuntimeError(
            f"Baseline variance is non-positive (sse_baseline={sse_baseline:.6e}); cannot compute normalized MSE.")
    metrics = Metrics.from_accumulators(sse_recon=sse, sse_baseline=sse_baseline, n_tokens=n_tokens, d_model=D)
    with open(fpaths.metrics, "w") as fd:
        json.dump(metrics.to_dict(), fd, indent=2)
    return metrics


def main(cfgs: Config | list[Config], *, top_k_tokens: int = 0, activation_hist: bool = False) -> int:
    """Run the configs one after another in this process (the reference can also submit them to Slurm,
    inference.py:288-364; cluster submission is outside this package)."""
    cfgs = [cfgs] if isinstance(cfgs, Config) else list(cfgs)
    for i, c in enumerate(cfgs, start=1):
        if c.slurm_acct:
            raise NotImplementedError("Slurm submission is not part of saev_amd; run worker_fn on the node directly")
        logger.info("Running config %d/%d locally.", i, len(cfgs))
        worker_fn(c, top_k_tokens=top_k_tokens, activation_hist=activation_hist)
    logger.info("Jobs done.")
    return 0
