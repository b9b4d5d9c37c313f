"""Host-side owner of one SAE's device state and the C-ABI context that runs its train step.

``SaeEngine`` allocates the four parameter-sized flat buffers (params, grads, Adam m, Adam v) as
torch tensors on a HIP device, exposes ``W_dec / b_dec / W_enc / b_enc`` as views into the flat
parameter buffer (state_dict order, reference nn/modeling.py:312-327), and forwards every compute
call to libsaev_amd.so.  PyTorch is used for memory, streams and ``torch.distributed`` only.
"""

from __future__ import annotations

import ctypes as C
import dataclasses
import math
import os

import numpy as np
import torch

from . import _lib


DEFAULT_ENCODER = "f16r"


@dataclasses.dataclass(frozen=True)
class EngineConfig:
    d_model: int
    d_sae: int
    top_k: int = 32
    k_aux: int = 512           # 0 disables the auxiliary loss
    alpha: float = 1.0 / 32.0
    dead_threshold_tokens: int = 10_000_000
    normalize_w_dec: bool = True
    remove_parallel_grads: bool = True
    max_batch: int = 16384
    aux_dead_cap: int = 0      # dead set the dense AuxK buffers are sized for at creation; 0 = min(d_sae, max(4096, 8 k_aux)).
                               # A step that meets more dead latents GROWS them (a device-synchronising free + allocate inside
                               # that step, reported on stderr; it fails only if the larger buffers do not fit the device)
    shard_world: int = 1       # > 1: flat buffers padded so that this many data-parallel ranks can each own 1/N of the tail
    max_backward_rows: int = 0  # 0 = max_batch; the GLOBAL batch for the sparse-state exchange (gathered backward over every
                                # rank's rows): sizes the backward's scratch only, the forward's buffers stay at max_batch
    # TopK candidate bounds of the fused encoder.  "guaranteed": running minimum over group maxima, always.  "norm" (default): the
    # same, except in the streamed f16r train step of a plain TopK engine, where a row's bound is predicted from its norm and the
    # previous step's exact k-th largest values, verified, and the step repeated on the device with guaranteed bounds if a row
    # fails.  "predicted": the older in-tile mean + z sigma predictor in every launch -- measured no faster over a
    # training run (tools/experiments/README.md), kept as an option.  Same codes in all three.  SAEV_AMD_BOUNDS overrides the default
    bounds: str = dataclasses.field(default_factory=lambda: os.environ.get("SAEV_AMD_BOUNDS", "norm"))
    # "f32": exact fp32 MFMA; "f16x3": split-fp16 MFMA at fp32 accuracy (16/3 of the f32 matrix rate);
    # "bf16": bf16-rounded encoder operands, one MFMA product, fp32 accumulate (everything else stays fp32);
    # "f16r": one fp16 MFMA product as a bounded-error first pass + exact fp32 recomputation of the surviving candidates.
    # The default can be overridden with the SAEV_AMD_ENCODER environment variable.
    encoder: str = dataclasses.field(default_factory=lambda: os.environ.get("SAEV_AMD_ENCODER", DEFAULT_ENCODER))
    # Route switches for A/B runs and for tests that must reach a particular kernel (saev_debug_cfg; same results on every
    # route).  The C library reads no environment variable; these defaults do, so that a test or a shell script can flip a
    # route without touching code:
    #   SAEV_AMD_DW=rows          weight gradients by whole-row gathers instead of column slices
    #   SAEV_AMD_DW=slices_a      column slices, but dval = <dL/dx_hat row, decoder row> formed by their first pass instead of by the decode
    #   SAEV_AMD_FWD=rows         exact refinement of the f16r encoder by whole-row gathers instead of 32-column slices
    #   SAEV_AMD_AUX_SMALL_MAX    largest dead set of the few-dead-latents AuxK kernels (-1: always the dense algebra)
    #   SAEV_AMD_CSC              1: the backward's pair-list build fills its bit map itself (default: the training decode does)
    #   SAEV_AMD_FIN              1: the backward's finalize re-reads the gradient rows for their statistics (round-4 kernels)
    #   SAEV_AMD_PREP             1: every f16r forward prepares its operands from x and W_enc itself (no streamed preparation)
    #   SAEV_AMD_AUX_DENSE        1: the dense AuxK algebra selects with the round-4 kernels (radix select, fills, scatter, absmax)
    #   SAEV_AMD_AUX_SMALL        1: 9-32 dead latents on the vector-ALU kernels of rounds 3-4 instead of the fp32 MFMA ones
    dw_route: str = dataclasses.field(default_factory=lambda: os.environ.get("SAEV_AMD_DW", "slices"))
    fwd_route: str = dataclasses.field(default_factory=lambda: os.environ.get("SAEV_AMD_FWD", "default"))
    aux_small_max: int = dataclasses.field(default_factory=lambda: int(os.environ.get("SAEV_AMD_AUX_SMALL_MAX", "0")))
    csc_route: int = dataclasses.field(default_factory=lambda: int(os.environ.get("SAEV_AMD_CSC", "0")))
    fin_route: int = dataclasses.field(default_factory=lambda: int(os.environ.get("SAEV_AMD_FIN", "0")))
    prep_route: int = dataclasses.field(default_factory=lambda: int(os.environ.get("SAEV_AMD_PREP", "0")))
    aux_dense_route: int = dataclasses.field(default_factory=lambda: int(os.environ.get("SAEV_AMD_AUX_DENSE", "0")))
    aux_small_route: int = dataclasses.field(default_factory=lambda: int(os.environ.get("SAEV_AMD_AUX_SMALL", "0")))
    group_route: int = dataclasses.field(default_factory=lambda: int(os.environ.get("SAEV_AMD_GROUP", "0")))
    aux_split_route: int = dataclasses.field(default_factory=lambda: int(os.environ.get("SAEV_AMD_AUX_SPLIT", "0")))
    aux_wide_route: int = dataclasses.field(default_factory=lambda: int(os.environ.get("SAEV_AMD_AUX_WIDE", "0")))
    # "topk" (default), or "relu": a forward-only context for a ReLU SAE (top_k is ignored, k_aux must be 0): encode_relu,
    # decode_rows, scatter_rows and the single ops run; the step entries raise NotImplementedError.
    # "relu_train" (include/saev_amd.h: RELU TRAINING): a ReLU SAE that TRAINS -- a context kind of its own, whose dense step runs on
    # the matrix cores: everything the "relu" engine runs, plus the phases, train_step (= the phases) and muon_tail with the
    # plain objective (no Matryoshka prefixes), one GPU, no share_x; last_codes compacts the dense f into padded rows.
    # "batch_topk" (include/saev_amd.h: BATCHTOPK): top_k codes per row ON AVERAGE, chosen over the whole batch in training mode
    # and by the learned threshold in eval mode; codes are padded rows of row_cap slots.  The phases, train_step (= the phases),
    # muon_tail, encode_batch_topk and batch_topk_dense run; one GPU, no share_x, no deferred gather.
    activation: str = "topk"
    row_cap: int = 0             # batch_topk: slots per code row; 0 = min(d_sae, max(64, 4 top_k)) rounded up to 64.  A forward that
                                 # meets a longer row rebuilds the context with the needed capacity (rounded up to 64) and repeats
    batch_momentum: float = 0.1  # batch_topk: EMA weight of the threshold update
    select_list_cap: int = 0     # batch_topk route switch for tests: capacity of the select's key list (0 = default; same results)
    l1_coeff: float = 0.0        # relu_train: L1Sparsity.coeff (0 = NoSparsity)


@dataclasses.dataclass(frozen=True)
class MuonConfig:
    """torch.optim.Muon's hyper-parameters (same names and defaults; lr is the per-step argument) -- include/saev_amd.h: MUON."""

    weight_decay: float = 0.1
    momentum: float = 0.95
    nesterov: bool = True
    ns_coefficients: tuple[float, float, float] = (3.4445, -4.7750, 2.0315)
    eps: float = 1e-07
    ns_steps: int = 5
    adjust_lr_fn: str | None = None

    def c_struct(self) -> "_lib.SaevMuonCfg":
        adj = {None: 0, "original": 0, "match_rms_adamw": 1, "none": 2}
        if self.adjust_lr_fn not in adj:
            raise ValueError(f"adjust_lr_fn must be None, 'original' or 'match_rms_adamw', got {self.adjust_lr_fn!r}")
        a, b, c = self.ns_coefficients
        return _lib.SaevMuonCfg(momentum=self.momentum, weight_decay=self.weight_decay, a=a, b=b, c=c, eps=self.eps,
                                nesterov=int(self.nesterov), ns_steps=self.ns_steps, adjust_lr=adj[self.adjust_lr_fn])


def newton_schulz(x: torch.Tensor, muon: MuonConfig | None = None, *, normalize: bool = True) -> torch.Tensor:
    """Newton-Schulz orthogonalisation of a 2-D device matrix on the HIP kernels of the Muon tail (torch's
    ``_zeropower_via_newtonschulz``): bf16 in and out, a taller matrix is transposed as torch does.  ``normalize=False``
    skips the division by the norm (the input is taken as already normalised)."""
    if x.ndim != 2 or not x.is_cuda:
        raise ValueError("newton_schulz takes a 2-D device matrix")
    lib = _lib.load()
    muon = muon or MuonConfig()
    tall = x.shape[0] > x.shape[1]
    xb = (x.t() if tall else x).to(torch.bfloat16).contiguous()
    rows, cols = xb.shape
    nbytes = int(lib.saev_muon_workspace_bytes(rows, cols))
    if nbytes < 0:
        raise _lib.SaevError(f"newton_schulz: unsupported shape {tuple(x.shape)}")
    ws = torch.empty(nbytes, device=x.device, dtype=torch.uint8)
    out = torch.empty_like(xb)
    cfg = muon.c_struct()
    with torch.cuda.device(x.device):
        rc = lib.saev_muon_newton_schulz(_ptr(xb), rows, cols, _ptr(out), C.byref(cfg), int(normalize), _ptr(ws), nbytes, _stream())
    if rc != 0:
        raise _lib.SaevError(f"saev_muon_newton_schulz failed (status {rc})")
    return out.t() if tall else out


@dataclasses.dataclass(frozen=True)
class CoherenceResult:
    """max_{i<j} |<w_i, w_j>| over the unit-normalised rows and the pair i < j that attains it (ties: the lexicographically
    smallest).  route: "filter" (fp16 filter + exact fp32 refinement) or "exact" (fp32 over every pair: asked for, or
    ``overflow`` -- more candidates than the list holds, ``candidates`` of ``capacity``)."""

    value: float
    i: int
    j: int
    route: str
    candidates: int = 0
    capacity: int = 0
    overflow: bool = False
    tiles_refiltered: int = 0  # 128 x 128 tiles the filter's second pass recomputed


_COHERENCE_ROUTES = {"auto": 0, "exact": 1}


def dictionary_coherence(W: torch.Tensor, *, route: str = "auto") -> CoherenceResult:
    """The log block's dictionary coherence (reference train.py:409-414), ``(W_n @ W_n.T).abs().triu(1).max()`` with
    ``W_n = W / W.norm(dim=1, keepdim=True)``, on the HIP kernels of saev_dictionary_coherence (include/saev_amd.h: COHERENCE):
    no S x S matrix, one read-back.  W: (S, D) float32 on a HIP device, D % 4 == 0, D <= 4096.  S = 1 gives 0.0 and the pair
    (-1, -1); a zero or non-finite row gives NaN.  ``route="exact"`` forces the fp32 route over every pair (A/B runs)."""
    if route not in _COHERENCE_ROUTES:
        raise ValueError(f"route must be one of {sorted(_COHERENCE_ROUTES)}, got {route!r}")
    if W.ndim != 2:
        raise ValueError(f"dictionary_coherence takes an (S, D) matrix, got shape {tuple(W.shape)}")
    lib = _lib.load()
    S, D = W.shape
    nbytes = int(lib.saev_coherence_workspace_bytes(S, D))
    if nbytes < 0:
        raise ValueError(f"dictionary_coherence: unsupported shape {(S, D)} (1 <= S <= 2**20, 4 <= D <= 4096, D % 4 == 0)")
    if not W.is_cuda or W.dtype != torch.float32:
        raise ValueError("dictionary_coherence takes a float32 device matrix")
    W = W.contiguous()
    if W.data_ptr() % 16:
        W = W.clone()
    ws = torch.empty(nbytes, device=W.device, dtype=torch.uint8)
    res = torch.empty(8, device=W.device, dtype=torch.int32)  # value bits | i, j | route, candidates, tiles, capacity
    with torch.cuda.device(W.device):
        rc = lib.saev_dictionary_coherence(_ptr(W), S, D, _COHERENCE_ROUTES[route], _ptr(ws), nbytes, _ptr(res), _ptr(res[1:]),
                                           _ptr(res[3:]), _stream())
    if rc != 0:
        raise _lib.SaevError(f"saev_dictionary_coherence failed (status {rc})")
    h = res.cpu()
    value = h[:1].view(torch.float32).item()
    i, j, code, cand, tiles, cap = h[1:7].tolist()
    return CoherenceResult(value=value, i=i, j=j, route="filter" if code == 0 else "exact", candidates=cand, capacity=cap,
                           overflow=code == 2, tiles_refiltered=tiles)


@dataclasses.dataclass(frozen=True)
class MatchResult:
    """Per row i of A its nearest neighbour among the rows of B: ``values[i]`` the largest cosine similarity (signed, or its
    absolute value) and ``indices[i]`` the smallest j that attains it, both device tensors.  route: "filter" (fp16 filter + exact
    fp32 refinement) or "exact" (fp32 over every pair: asked for, or ``overflow`` -- more candidates than the list holds,
    ``candidates`` of ``capacity``)."""

    values: torch.Tensor   # (Sa,) float32
    indices: torch.Tensor  # (Sa,) int32
    route: str
    candidates: int = 0
    capacity: int = 0
    overflow: bool = False
    tiles_refiltered: int = 0  # 128 x 128 tiles the filter's second pass recomputed

    @property
    def mmcs(self) -> float:
        """Mean max cosine similarity: the fp64 mean of ``values`` (NaN if any row is NaN)."""
        return self.values.double().mean().item()


_MATCH_LIMITS = "1 <= Sa, Sb <= 2**20, 4 <= D <= 4096, D % 4 == 0"


def dictionary_match(A: torch.Tensor, B: torch.Tensor | None = None, *, absolute: bool = False, route: str = "auto") -> MatchResult:
    """Nearest neighbour of every row of A among the rows of B by cosine similarity, ``(A_n @ B_n.T).max(dim=1)`` with
    ``X_n = X / X.norm(dim=1, keepdim=True)`` (``.abs()`` first if ``absolute``), on the HIP kernels of saev_dictionary_match
    (include/saev_amd.h: DICTIONARY MATCH): no Sa x Sb matrix, one small read-back.  ``B=None`` matches A against itself with
    the pair j == i excluded (one row: 0.0 and index -1).  A: (Sa, D), B: (Sb, D), float32 on one HIP device, D % 4 == 0,
    D <= 4096.  A row that meets a zero or non-finite row is NaN.  ``route="exact"`` forces the fp32 route over every pair."""
    if route not in _COHERENCE_ROUTES:
        raise ValueError(f"route must be one of {sorted(_COHERENCE_ROUTES)}, got {route!r}")
    if A.ndim != 2 or (B is not None and B.ndim != 2):
        raise ValueError(f"dictionary_match takes (S, D) matrices, got shapes {tuple(A.shape)}"
                         + ("" if B is None else f" and {tuple(B.shape)}"))
    Sa, D = A.shape
    Sb = Sa if B is None else B.shape[0]
    if B is not None and B.shape[1] != D:
        raise ValueError(f"dictionary_match: A and B must share D, got {D} and {B.shape[1]}")
    lib = _lib.load()
    nbytes = int(lib.saev_dictionary_match_workspace_bytes(Sa, Sb, D))
    if nbytes < 0:
        raise ValueError(f"dictionary_match: unsupported shape {(Sa, Sb, D)} ({_MATCH_LIMITS})")
    for X in (A,) if B is None else (A, B):
        if not X.is_cuda or X.dtype != torch.float32:
            raise ValueError("dictionary_match takes float32 device matrices")
    if B is not None and B.device != A.device:
        raise ValueError(f"dictionary_match: A and B must share a device, got {A.device} and {B.device}")

    def aligned(X):
        X = X.contiguous()
        return X.clone() if X.data_ptr() % 16 else X

    A = aligned(A)
    B = None if B is None else aligned(B)
    ws = torch.empty(nbytes, device=A.device, dtype=torch.uint8)
    values = torch.empty(Sa, device=A.device, dtype=torch.float32)
    indices = torch.empty(Sa, device=A.device, dtype=torch.int32)
    info = torch.empty(4, device=A.device, dtype=torch.int32)  # route, candidates, tiles, capacity
    with torch.cuda.device(A.device):
        rc = lib.saev_dictionary_match(_ptr(A), Sa, None if B is None else _ptr(B), Sb, D, int(bool(absolute)),
                                       _COHERENCE_ROUTES[route], _ptr(ws), nbytes, _ptr(values), _ptr(indices), _ptr(info), _stream())
    if rc != 0:
        raise _lib.SaevError(f"saev_dictionary_match failed (status {rc})")
    code, cand, tiles, cap = info.cpu().tolist()
    return MatchResult(values=values, indices=indices, route="filter" if code == 0 else "exact", candidates=cand, capacity=cap,
                       overflow=code == 2, tiles_refiltered=tiles)


@dataclasses.dataclass(frozen=True)
class AssignResult:
    """Per row i of X its nearest (or farthest) centre: ``dist2[i]`` the refined squared distance r_ij and ``indices[i]`` the smallest
    j that attains it, both device tensors.  route: "filter" (fp16 filter + exact fp32 refinement) or "exact" (every pair: asked
    for, or ``overflow`` -- the filter could not answer, ``candidates`` of ``capacity``)."""

    dist2: torch.Tensor    # (n,) float32
    indices: torch.Tensor  # (n,) int32
    route: str
    candidates: int = 0
    capacity: int = 0
    overflow: bool = False
    tiles_refiltered: int = 0  # 128 x 128 tiles the filter's second pass recomputed


@dataclasses.dataclass(frozen=True)
class CollapsedResult:
    """``losers``: (k,) bool device mask of the centres that lose a pair closer than the tolerance; the rest as AssignResult."""

    losers: torch.Tensor
    route: str
    candidates: int = 0
    capacity: int = 0
    overflow: bool = False
    tiles_refiltered: int = 0


_KMEANS_LIMITS = "1 <= n, k <= 2**20, 4 <= D <= 4096, D % 4 == 0"
KMEANS_NONFINITE = -1  # include/saev_amd.h: SAEV_KMEANS_NONFINITE


def _kmeans_matrix(what: str, X: torch.Tensor) -> torch.Tensor:
    if X.ndim != 2:
        raise ValueError(f"{what} takes (rows, D) matrices, got shape {tuple(X.shape)}")
    if not X.is_cuda or X.dtype != torch.float32:
        raise ValueError(f"{what} takes float32 device matrices")
    X = X.contiguous()
    return X.clone() if X.data_ptr() % 16 else X


def _kmeans_workspace(what: str, n: int, k: int, D: int, device) -> tuple[torch.Tensor, int]:
    nbytes = int(_lib.load().saev_kmeans_workspace_bytes(n, k, D))
    if nbytes < 0:
        raise ValueError(f"{what}: unsupported shape {(n, k, D)} ({_KMEANS_LIMITS})")
    return torch.empty(nbytes, device=device, dtype=torch.uint8), nbytes


def _kmeans_info(what: str, info) -> dict:
    code, cand, tiles, cap = info
    if code == KMEANS_NONFINITE:
        raise ValueError(f"{what}: the batch or the centres hold an inf or a NaN")
    return dict(route="filter" if code == 0 else "exact", candidates=cand, capacity=cap, overflow=code == 2, tiles_refiltered=tiles)


def kmeans_assign_device(X: torch.Tensor, C: torch.Tensor, *, farthest: bool = False, route: str = "auto",
                         info: torch.Tensor | None = None) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """saev_kmeans_assign without a read-back: (dist2, indices, info), ``info`` the four int32 words of the C entry on the device
    (written into the caller's tensor if one is given).  When word 0 reads KMEANS_NONFINITE every index is -1, which
    kmeans_group ignores, so a step built on this call touches no state before its one read-back can raise."""
    if route not in _COHERENCE_ROUTES:
        raise ValueError(f"route must be one of {sorted(_COHERENCE_ROUTES)}, got {route!r}")
    X, C = _kmeans_matrix("kmeans_assign", X), _kmeans_matrix("kmeans_assign", C)
    if X.shape[1] != C.shape[1]:
        raise ValueError(f"kmeans_assign: X and C must share D, got {X.shape[1]} and {C.shape[1]}")
    if X.device != C.device:
        raise ValueError(f"kmeans_assign: X and C must share a device, got {X.device} and {C.device}")
    (n, D), k = X.shape, C.shape[0]
    ws, nbytes = _kmeans_workspace("kmeans_assign", n, k, D, X.device)
    dist2 = torch.empty(n, device=X.device, dtype=torch.float32)
    indices = torch.empty(n, device=X.device, dtype=torch.int32)
    if info is None:
        info = torch.empty(4, device=X.device, dtype=torch.int32)
    with torch.cuda.device(X.device):
        rc = _lib.load().saev_kmeans_assign(_ptr(X), n, _ptr(C), k, D, int(bool(farthest)), _COHERENCE_ROUTES[route], _ptr(ws), nbytes,
                                            _ptr(dist2), _ptr(indices), _ptr(info), _stream())
    if rc != 0:
        raise _lib.SaevError(f"saev_kmeans_assign failed (status {rc})")
    return dist2, indices, info


def kmeans_assign(X: torch.Tensor, C: torch.Tensor, *, farthest: bool = False, route: str = "auto") -> AssignResult:
    """Nearest (``farthest``: farthest) centre of every row of X, ``torch.cdist(X, C).min(dim=1)`` squared, on the HIP kernels of
    saev_kmeans_assign (include/saev_amd.h: K-MEANS): no n x k matrix, one small read-back.  ``dist2[i]`` is the fp32
    difference-form sum of squares of the returned pair and ``indices[i]`` the smallest j attaining the optimum; both routes
    give the same bits.  X: (n, D), C: (k, D), float32 on one HIP device, D % 4 == 0, D <= 4096.  An inf or a NaN in either
    raises ValueError."""
    dist2, indices, info = kmeans_assign_device(X, C, farthest=farthest, route=route)
    return AssignResult(dist2=dist2, indices=indices, **_kmeans_info("kmeans_assign", info.cpu().tolist()))


def kmeans_group(indices: torch.Tensor, k: int) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(counts (k,), starts (k + 1,), rows (n,)), int32 on the device: the rows of a batch grouped by their centre, ascending within
    each centre -- a stable counting sort of ``indices`` (saev_kmeans_group).  Entries outside [0, k) are ignored."""
    if indices.ndim != 1 or not indices.is_cuda or indices.dtype != torch.int32:
        raise ValueError("kmeans_group takes a 1-D int32 device tensor")
    n = indices.shape[0]
    if not (1 <= n <= 2**20 and 1 <= k <= 2**20):
        raise ValueError(f"kmeans_group: unsupported shape {(n, k)} (1 <= n, k <= 2**20)")
    indices = indices.contiguous()
    counts = torch.empty(k, device=indices.device, dtype=torch.int32)
    starts = torch.empty(k + 1, device=indices.device, dtype=torch.int32)
    rows = torch.empty(n, device=indices.device, dtype=torch.int32)
    with torch.cuda.device(indices.device):
        rc = _lib.load().saev_kmeans_group(_ptr(indices), n, k, _ptr(counts), _ptr(starts), _ptr(rows), _stream())
    if rc != 0:
        raise _lib.SaevError(f"saev_kmeans_group failed (status {rc})")
    return counts, starts, rows


def kmeans_update(X: torch.Tensor, starts: torch.Tensor, rows: torch.Tensor, centers: torch.Tensor, cluster_counts: torch.Tensor, *,
                  repl_rows: torch.Tensor | None = None, dist2: torch.Tensor | None = None,
                  out_inertia: torch.Tensor | None = None) -> torch.Tensor | None:
    """The running-mean update of saev_kmeans_update, IN PLACE on ``centers`` (k, D) and ``cluster_counts`` (k,) float32: each
    centre with rows in the batch becomes (c * prev + sums) / (prev + count), sums in ascending row order.  ``repl_rows`` (k,)
    int32: >= 0 gives a centre without rows that one row with count 1.  With ``dist2`` the fp64 mean of it is returned as a
    one-element float64 device tensor (``out_inertia`` if given), else None."""
    X = _kmeans_matrix("kmeans_update", X)
    n, D = X.shape
    k = centers.shape[0]
    if centers.ndim != 2 or centers.shape[1] != D or not centers.is_cuda or centers.dtype != torch.float32 or not centers.is_contiguous() \
            or centers.data_ptr() % 16:
        raise ValueError("kmeans_update: centers must be a contiguous, 16-byte aligned (k, D) float32 device matrix (it is updated in place)")
    if cluster_counts.shape != (k,) or cluster_counts.dtype != torch.float32 or not cluster_counts.is_contiguous() \
            or cluster_counts.device != X.device or centers.device != X.device:
        raise ValueError("kmeans_update: cluster_counts must be a contiguous (k,) float32 tensor on the batch's device")
    if not (1 <= n <= 2**20 and 1 <= k <= 2**20 and 4 <= D <= 4096 and D % 4 == 0):
        raise ValueError(f"kmeans_update: unsupported shape {(n, k, D)} ({_KMEANS_LIMITS})")
    for name, t, shape in (("starts", starts, (k + 1,)), ("rows", rows, (n,)), ("repl_rows", repl_rows, (k,))):
        if t is not None and (t.shape != shape or t.dtype != torch.int32 or t.device != X.device or not t.is_contiguous()):
            raise ValueError(f"kmeans_update: {name} must be a contiguous {shape} int32 tensor on the batch's device")
    if dist2 is not None:
        if dist2.shape != (n,) or dist2.dtype != torch.float32 or dist2.device != X.device or not dist2.is_contiguous():
            raise ValueError("kmeans_update: dist2 must be a contiguous (n,) float32 tensor on the batch's device")
        if out_inertia is None:
            out_inertia = torch.empty(1, device=X.device, dtype=torch.float64)
    with torch.cuda.device(X.device):
        rc = _lib.load().saev_kmeans_update(_ptr(X), n, D, k, _ptr(starts), _ptr(rows), None if repl_rows is None else _ptr(repl_rows),
                                            _ptr(centers), _ptr(cluster_counts), None if dist2 is None else _ptr(out_inertia),
                                            None if dist2 is None else _ptr(dist2), _stream())
    if rc != 0:
        raise _lib.SaevError(f"saev_kmeans_update failed (status {rc})")
    return out_inertia if dist2 is not None else None


def kmeans_collapsed_device(C: torch.Tensor, cluster_counts: torch.Tensor, tol: float, *, route: str = "auto",
                            info: torch.Tensor | None = None) -> tuple[torch.Tensor, torch.Tensor]:
    """saev_kmeans_collapsed without a read-back: (losers (k,) bool, info (4,) int32), both on the device."""
    if route not in _COHERENCE_ROUTES:
        raise ValueError(f"route must be one of {sorted(_COHERENCE_ROUTES)}, got {route!r}")
    C = _kmeans_matrix("kmeans_collapsed", C)
    k, D = C.shape
    if cluster_counts.shape != (k,) or cluster_counts.dtype != torch.float32 or cluster_counts.device != C.device:
        raise ValueError("kmeans_collapsed: cluster_counts must be a (k,) float32 tensor on the centres' device")
    cluster_counts = cluster_counts.contiguous()
    ws, nbytes = _kmeans_workspace("kmeans_collapsed", k, k, D, C.device)
    losers = torch.empty(k, device=C.device, dtype=torch.uint8)
    if info is None:
        info = torch.empty(4, device=C.device, dtype=torch.int32)
    with torch.cuda.device(C.device):
        rc = _lib.load().saev_kmeans_collapsed(_ptr(C), k, D, float(tol), _ptr(cluster_counts), _COHERENCE_ROUTES[route], _ptr(ws),
                                               nbytes, _ptr(losers), _ptr(info), _stream())
    if rc != 0:
        raise _lib.SaevError(f"saev_kmeans_collapsed failed (status {rc})")
    return losers.view(torch.bool), info


def kmeans_collapsed(C: torch.Tensor, cluster_counts: torch.Tensor, tol: float, *, route: str = "auto") -> CollapsedResult:
    """The loser mask of the reference's collapsed-centre rule: for every pair i < j of centres closer than ``tol`` (the fp32
    distance ``sqrt(r_ij)``), i if ``cluster_counts[i] <= cluster_counts[j]`` else j -- on the HIP kernels of
    saev_kmeans_collapsed, no k x k matrix, one small read-back."""
    losers, info = kmeans_collapsed_device(C, cluster_counts, tol, route=route)
    return CollapsedResult(losers=losers, **_kmeans_info("kmeans_collapsed", info.cpu().tolist()))


def row_norm_mean(W: torch.Tensor) -> float:
    """``W.norm(dim=1).mean()`` of an (S, D) float32 device matrix on the HIP kernels of saev_row_norm_mean (the log block's
    metrics/avg_decoder_row_norm): exact fp64 squares, each norm rounded once to fp32, every sum in a fixed order; one read-back
    of one double."""
    if W.ndim != 2:
        raise ValueError(f"row_norm_mean takes an (S, D) matrix, got shape {tuple(W.shape)}")
    S, D = W.shape
    if S < 1 or D < 4 or D > 4096 or D % 4:
        raise ValueError(f"row_norm_mean: unsupported shape {(S, D)} (S >= 1, 4 <= D <= 4096, D % 4 == 0)")
    if not W.is_cuda or W.dtype != torch.float32:
        raise ValueError("row_norm_mean takes a float32 device matrix")
    lib = _lib.load()
    W = W.contiguous()
    if W.data_ptr() % 16:
        W = W.clone()
    ws = torch.empty(_lib.ROW_NORM_WORKSPACE_BYTES + 8, device=W.device, dtype=torch.uint8)  # [partials | the result]
    out = ws[_lib.ROW_NORM_WORKSPACE_BYTES:].view(torch.float64)
    with torch.cuda.device(W.device):
        rc = lib.saev_row_norm_mean(_ptr(W), S, D, _ptr(out), _ptr(ws), _lib.ROW_NORM_WORKSPACE_BYTES, _stream())
    _lib.check(lib, None, rc, "saev_row_norm_mean")
    return out.item()


def _on(t, dtype, shape, what, device):
    """``t`` made contiguous; ValueError unless it has this dtype and shape and lies on ``device``.  None passes through."""
    if t is None:
        return None
    if t.dtype != dtype or tuple(t.shape) != tuple(shape) or t.device != device:
        raise ValueError(f"{what} must be {dtype} of shape {tuple(shape)} on {device}, got {t.dtype} {tuple(t.shape)} on {t.device}")
    return t.contiguous()


def _hip_device(who: str, device) -> torch.device:
    """``device`` with its index filled in; RuntimeError unless it is a HIP device."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"{who} runs on a HIP device only (there is no CPU path)")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


def _csr_on(indptr, indices, data, n_rows: int, stored: int, device):
    """The CSR triple of the analysis entries: indptr (n_rows + 1) int64, indices and data (stored) int32 / float32."""
    return (_on(indptr, torch.int64, (n_rows + 1,), "indptr", device), _on(indices, torch.int32, (stored,), "indices", device),
            _on(data, torch.float32, (stored,), "data", device))


def _class_labels(who: str, labels, remap, n_rows: int, device):
    """``labels`` / ``remap`` of ``latent_ap`` as the C entry takes them: (class_u8, remap, class_i32), one label form set."""
    if labels.dtype == torch.uint8:
        return _on(labels, torch.uint8, (n_rows,), "labels", device), _on(remap, torch.int32, (256,), "remap", device), None
    if labels.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"labels must be uint8, int32 or int64, got {labels.dtype}")
    if remap is not None:
        raise ValueError(f"{who}: remap goes with uint8 labels")
    return None, None, _on(labels.to(torch.int32), torch.int32, (n_rows,), "labels", device)


def _check_err_word(err, errors: dict, who: str) -> None:
    """Reads the device's error word (one synchronisation); ValueError with the table's text if it is not 0."""
    code = int(err.item())
    if code != 0:
        raise ValueError(f"{who}: {errors.get(code, code)} (found on the device)")


class _Checked:
    """Results of a call that reports bad input through an error word on the device: the first read of a result -- or ``check()``
    -- reads the word once and raises ValueError if it is not 0; every later read of a bad call raises again."""

    def __init__(self, out: dict, err, errors: dict, who: str):
        self._out, self._err, self._errors, self._who = out, err, errors, who
        self._checked = False

    def check(self) -> None:
        if not self._checked:
            _check_err_word(self._err, self._errors, self._who)
            self._checked = True

    def _read(self, name):
        self.check()
        return self._out[name]


@dataclasses.dataclass(frozen=True)
class BatchStatsHost:
    """What ``BatchStats.read()`` brings back (CPU tensors; an output the accumulator was created without is None)."""

    n_kept: float
    sum_x: float
    sum_xx: float
    sum_r: float
    sum_rr: float
    extra: torch.Tensor              # (8) float64, the caller's own slots
    col_sum: torch.Tensor | None     # (D) float64
    n_pos: torch.Tensor | None       # (S) int64
    value_sum: torch.Tensor | None   # (S) float64
    live: torch.Tensor | None        # (S) int32


class BatchStats:
    """Accumulators of saev_batch_stats (include/saev_amd.h: BATCH STATISTICS) and its workspace, as torch tensors that alias
    ONE device buffer: ``sums`` = [extra (8) | scalars (8) | col_sum (D)] float64 -- ``extra`` belongs to the caller, so that
    a data-parallel run reduces its own per-batch scalars and the kernel's sums in one ``all_reduce`` --, then ``value_sum``
    (S float64), ``n_pos`` (S int64), ``live`` (S int32).  ``want`` names the outputs to keep; the others are not computed
    (without ``scalars`` and ``col_sum`` the pass over x and x_hat does not run at all).  ``add`` accumulates a batch, ``read`` is one device-to-host copy of everything."""

    OUTPUTS = ("scalars", "col_sum", "n_pos", "value_sum", "live")

    def __init__(self, d_model: int, d_sae: int, device, *, want=OUTPUTS, live_eps: float = 1e-12):
        unknown = set(want) - set(self.OUTPUTS)
        if unknown:
            raise ValueError(f"BatchStats: unknown outputs {sorted(unknown)} (known: {self.OUTPUTS})")
        if d_model < 4 or d_model > 4096 or d_model % 4:
            raise ValueError(f"BatchStats: unsupported d_model {d_model} (4 <= D <= 4096, D % 4 == 0)")
        self.lib = _lib.load()
        self.d_model, self.d_sae, self.live_eps = d_model, d_sae, live_eps
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        D, S = d_model, d_sae
        sizes = [("extra", 8 * 8), ("scalars", 8 * 8), ("col_sum", 8 * D if "col_sum" in want else 0),
                 ("value_sum", 8 * S if "value_sum" in want else 0), ("n_pos", 8 * S if "n_pos" in want else 0),
                 ("live", 4 * S if "live" in want else 0)]
        self._spans, off = {}, 0
        for name, nbytes in sizes:
            self._spans[name] = (off, off + nbytes)
            off += nbytes
        self.buf = torch.zeros(off, device=self.device, dtype=torch.uint8)
        dtypes = {"extra": torch.float64, "scalars": torch.float64, "col_sum": torch.float64, "value_sum": torch.float64,
                  "n_pos": torch.int64, "live": torch.int32}
        self._dtypes = dtypes
        for name, (lo, hi) in self._spans.items():
            setattr(self, name, self.buf[lo:hi].view(dtypes[name]) if hi > lo else None)
        self.sums = self.buf[:self._spans["col_sum"][1]].view(torch.float64)
        self._ws = None
        self._acc = _lib.SaevBatchAcc(struct_size=C.sizeof(_lib.SaevBatchAcc), flags=0, live_eps=live_eps,
                                      col_sum=_ptr(self.col_sum), scalars=_ptr(self.scalars) if "scalars" in want else None, n_pos=_ptr(self.n_pos),
                                      value_sum=_ptr(self.value_sum), live=_ptr(self.live))

    def zero_(self) -> "BatchStats":
        self.buf.zero_()
        return self

    def _workspace(self, n: int):
        need = int(self.lib.saev_batch_stats_workspace_bytes(n, self.d_model))
        if need < 0:
            raise _lib.SaevError(f"saev_batch_stats: unsupported shape n={n}, d_model={self.d_model}")
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, device=self.device, dtype=torch.uint8)
        return self._ws

    def _add_ptrs(self, x, x_hat, idx, val, row_nnz, keep, n: int, cap: int, overwrite: bool, scalars: bool = True):
        if keep is not None:
            if keep.dtype == torch.bool:
                keep = keep.view(torch.uint8)
            if keep.dtype != torch.uint8 or keep.shape != (n,) or keep.device != self.device or not keep.is_contiguous():
                raise ValueError(f"keep must be a contiguous bool / uint8 vector of {n} rows on {self.device}")
        ws = self._workspace(n)
        acc = self._acc
        if not scalars and acc.scalars:  # (this batch's scalar sums come from elsewhere: the step's own statistics)
            acc = _lib.SaevBatchAcc.from_buffer_copy(acc)
            acc.scalars = None
        acc.flags = _lib.BATCH_OVERWRITE if overwrite else 0
        with torch.cuda.device(self.device):
            rc = self.lib.saev_batch_stats(x, x_hat, idx, val, row_nnz, _ptr(keep), n, self.d_model, self.d_sae, cap,
                                           C.byref(acc), _ptr(ws), ws.numel(), _stream())
        _lib.check(self.lib, None, rc, "saev_batch_stats")

    def add(self, x: torch.Tensor, x_hat: torch.Tensor | None, idx: torch.Tensor | None, val: torch.Tensor | None,
            row_nnz: torch.Tensor | None = None, keep: torch.Tensor | None = None, *, overwrite: bool = False,
            scalars: bool = True) -> None:
        """One batch: x, x_hat (n, D) float32; padded code rows idx (n, cap) int32 / val (n, cap) float32 with row_nnz (n) int32
        (None: full rows); keep (n) bool.  ``overwrite`` stores instead of adding (``live`` is never cleared);
        ``scalars=False`` leaves the scalar sums out of this batch."""
        if x.ndim != 2:
            raise ValueError(f"x must be (n, {self.d_model}), got {tuple(x.shape)}")
        n = x.shape[0]
        x = _on(x, torch.float32, (n, self.d_model), "x", self.device)
        x_hat = _on(x_hat, torch.float32, (n, self.d_model), "x_hat", self.device)
        if (idx is None) != (val is None):
            raise ValueError("idx and val come together")
        cap = 0 if idx is None else idx.shape[-1]
        idx = _on(idx, torch.int32, (n, cap), "idx", self.device)
        val = _on(val, torch.float32, (n, cap), "val", self.device)
        row_nnz = _on(row_nnz, torch.int32, (n,), "row_nnz", self.device)
        self._add_ptrs(_ptr(x), _ptr(x_hat), _ptr(idx), _ptr(val), _ptr(row_nnz), keep, n, cap, overwrite, scalars)

    def read(self) -> BatchStatsHost:
        h = self.buf.cpu()  # the one device-to-host copy
        part = {name: (h[lo:hi].view(self._dtypes[name]) if hi > lo else None) for name, (lo, hi) in self._spans.items()}
        n_kept, sx, sxx, sr, srr = part["scalars"][:5].tolist()
        return BatchStatsHost(n_kept=n_kept, sum_x=sx, sum_xx=sxx, sum_r=sr, sum_rr=srr, extra=part["extra"], col_sum=part["col_sum"],
                              n_pos=part["n_pos"], value_sum=part["value_sum"], live=part["live"])


@dataclasses.dataclass(frozen=True)
class LatentTopKHost:
    """What ``LatentTopK.read()`` brings back (CPU tensors): ``values`` / ``indices`` as the reference's
    ``csr_topk(axis=0)`` shapes and pads them, and how many slots of each column are real."""

    values: torch.Tensor   # (k, S) float32, descending in each column, 0 past the latent's count
    indices: torch.Tensor  # (k, S) int64 row ids, 0 past the latent's count
    counts: torch.Tensor   # (S) int64


class LatentTopK:
    """Per-latent top-k activating rows over a stream of batches (include/saev_amd.h: LATENT TOP-K): the device
    state of saev_latent_topk_update -- ``top_val`` (S, k) float32, ``top_row`` (S, k) int64, ``top_cnt`` (S) int32 -- and its
    workspace.  ``add`` takes padded code rows, ``add_csr`` a CSR block; ``read`` is the only device-to-host copy.  Entries order
    by (value descending, row ascending), so the result does not depend on the order the batches arrive in."""

    MAX_K = 64

    def __init__(self, d_sae: int, k: int, device):
        if not 1 <= k <= self.MAX_K:
            raise ValueError(f"LatentTopK: unsupported k {k} (1 <= k <= {self.MAX_K})")
        if d_sae < 1 or d_sae >= 2**31:
            raise ValueError(f"LatentTopK: unsupported d_sae {d_sae}")
        self.device = _hip_device("LatentTopK", device)
        self.lib = _lib.load()
        self.d_sae, self.k = d_sae, k
        self.top_val = torch.zeros(d_sae, k, device=self.device, dtype=torch.float32)
        self.top_row = torch.zeros(d_sae, k, device=self.device, dtype=torch.int64)
        self.top_cnt = torch.zeros(d_sae, device=self.device, dtype=torch.int32)
        self._ws = None
        self._state = _lib.SaevLatentTopKState(struct_size=C.sizeof(_lib.SaevLatentTopKState), k=k, top_val=_ptr(self.top_val),
                                               top_row=_ptr(self.top_row), top_cnt=_ptr(self.top_cnt))

    def zero_(self) -> "LatentTopK":
        for t in (self.top_val, self.top_row, self.top_cnt):
            t.zero_()
        return self

    def _workspace(self, n_entries: int):
        need = int(self.lib.saev_latent_topk_workspace_bytes(n_entries, self.d_sae))
        if need < 0:
            raise _lib.SaevError(f"saev_latent_topk_update: {n_entries} entries in one batch (at most 2^31 - 1)")
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, device=self.device, dtype=torch.uint8)
        return self._ws

    def _keep(self, keep, n: int):
        if keep is None:
            return None
        if keep.dtype == torch.bool:
            keep = keep.view(torch.uint8)
        if keep.dtype != torch.uint8 or keep.shape != (n,) or keep.device != self.device or not keep.is_contiguous():
            raise ValueError(f"keep must be a contiguous bool / uint8 vector of {n} rows on {self.device}")
        return keep

    def _update(self, idx, val, row_nnz, cap: int, row_ptr, indices, data, nnz: int, keep, n: int, row_base: int) -> None:
        if row_base < 0:
            raise ValueError(f"row_base must be >= 0, got {row_base}")
        ws = self._workspace(n * cap if row_ptr is None else nnz)
        with torch.cuda.device(self.device):
            rc = self.lib.saev_latent_topk_update(idx, val, row_nnz, cap, row_ptr, indices, data, nnz, _ptr(self._keep(keep, n)), n,
                                                  self.d_sae, row_base, C.byref(self._state), _ptr(ws), ws.numel(), _stream())
        _lib.check(self.lib, None, rc, "saev_latent_topk_update")

    def add(self, idx: torch.Tensor, val: torch.Tensor, row_nnz: torch.Tensor | None = None, keep: torch.Tensor | None = None, *,
            row_base: int) -> None:
        """One batch of padded code rows: idx (n, cap) int32, val (n, cap) float32, row_nnz (n) int32 (None: full rows), keep (n)
        bool; local row b is row ``row_base + b``."""
        if idx.ndim != 2:
            raise ValueError(f"idx must be (n, cap), got {tuple(idx.shape)}")
        n, cap = idx.shape
        idx = _on(idx, torch.int32, (n, cap), "idx", self.device)
        val = _on(val, torch.float32, (n, cap), "val", self.device)
        row_nnz = _on(row_nnz, torch.int32, (n,), "row_nnz", self.device)
        if n == 0 or cap == 0:
            return
        self._update(_ptr(idx), _ptr(val), _ptr(row_nnz), cap, None, None, None, 0, keep, n, row_base)

    def add_csr(self, indptr: torch.Tensor, indices: torch.Tensor, data: torch.Tensor, keep: torch.Tensor | None = None, *,
                row_base: int) -> None:
        """One CSR block on the device: indptr (n + 1) int64 starting at 0, indices (nnz) int32, data (nnz) float32."""
        if indptr.ndim != 1 or indptr.numel() < 1:
            raise ValueError(f"indptr must be a vector of n + 1 offsets, got {tuple(indptr.shape)}")
        n, nnz = indptr.numel() - 1, indices.numel()
        indptr, indices, data = _csr_on(indptr, indices, data, n, nnz, self.device)
        if n == 0 or nnz == 0:
            return
        self._update(None, None, None, 0, _ptr(indptr), _ptr(indices), _ptr(data), nnz, keep, n, row_base)

    def read(self) -> LatentTopKHost:
        return LatentTopKHost(values=self.top_val.t().contiguous().cpu(), indices=self.top_row.t().contiguous().cpu(),
                              counts=self.top_cnt.to(torch.int64).cpu())


class _LatentHistStream:
    """What LatentHist and LatentQuantiles share: one batch, in either form, into the count table ``self._state`` describes
    (saev_latent_hist_update).  Counts are uint32 (held in int32 tensors): an accumulator offered 2^32 rows or more is refused."""

    MAX_ROWS = 2**32
    T_STRIDE = 16

    def _init_stream(self, who: str, d_sae: int, device) -> None:
        if d_sae < 1 or d_sae >= 2**31:
            raise ValueError(f"{who}: unsupported d_sae {d_sae}")
        self.device = _hip_device(who, device)
        self.lib = _lib.load()
        self.d_sae = d_sae
        self.n_rows = torch.zeros(1, device=self.device, dtype=torch.int64)  # kept rows of the current pass, on the device
        self._offered = 0
        self._ws = None
        self._no_codes = torch.zeros(1, device=self.device, dtype=torch.int32)  # stands in for the codes of a batch that has none

    _keep = LatentTopK._keep

    def _update(self, idx, val, row_nnz, cap: int, row_ptr, indices, data, nnz: int, keep, n: int) -> None:
        if self._offered + n >= self.MAX_ROWS:
            raise _lib.SaevError(f"saev_latent_hist_update: {self._offered + n} rows offered to one accumulator (uint32 counts: fewer than 2^32)")
        need = int(self.lib.saev_latent_hist_workspace_bytes(n * cap if row_ptr is None else nnz, self.d_sae))
        if need < 0:
            raise _lib.SaevError("saev_latent_hist_update: more than 2^31 - 1 entries in one batch")
        if self._ws is None:
            self._ws = torch.empty(need, device=self.device, dtype=torch.uint8)
        with torch.cuda.device(self.device):
            rc = self.lib.saev_latent_hist_update(idx, val, row_nnz, cap, row_ptr, indices, data, nnz, _ptr(self._keep(keep, n)), n, self.d_sae,
                                                  C.byref(self._state), _ptr(self._ws), self._ws.numel(), _stream())
        _lib.check(self.lib, None, rc, "saev_latent_hist_update")
        self._offered += n

    def add(self, idx: torch.Tensor, val: torch.Tensor, row_nnz: torch.Tensor | None = None, keep: torch.Tensor | None = None) -> None:
        """One batch of padded code rows: idx (n, cap) int32, val (n, cap) float32, row_nnz (n) int32 (None: full rows), keep (n) bool."""
        if idx.ndim != 2:
            raise ValueError(f"idx must be (n, cap), got {tuple(idx.shape)}")
        n, cap = idx.shape
        idx = _on(idx, torch.int32, (n, cap), "idx", self.device)
        val = _on(val, torch.float32, (n, cap), "val", self.device)
        row_nnz = _on(row_nnz, torch.int32, (n,), "row_nnz", self.device)
        self._accepts()
        if n == 0:
            return
        if cap == 0:  # rows without a slot are still rows
            idx = val = self._no_codes
        self._update(_ptr(idx), _ptr(val), _ptr(row_nnz), cap, None, None, None, 0, keep, n)

    def add_csr(self, indptr: torch.Tensor, indices: torch.Tensor, data: torch.Tensor, keep: torch.Tensor | None = None) -> None:
        """One CSR block on the device: indptr (n + 1) int64 starting at 0, indices (nnz) int32, data (nnz) float32."""
        if indptr.ndim != 1 or indptr.numel() < 1:
            raise ValueError(f"indptr must be a vector of n + 1 offsets, got {tuple(indptr.shape)}")
        n, nnz = indptr.numel() - 1, indices.numel()
        indptr, indices, data = _csr_on(indptr, indices, data, n, nnz, self.device)
        self._accepts()
        if n == 0:
            return
        if nnz == 0:
            indices = data = self._no_codes
        self._update(None, None, None, 0, _ptr(indptr), _ptr(indices), _ptr(data), nnz, keep, n)

    def _accepts(self) -> None:
        pass


def _u32(t: torch.Tensor) -> torch.Tensor:
    """uint32 counters held in an int32 tensor, as int64."""
    return t.to(torch.int64) & 0xFFFFFFFF


def hist_window(counts0: torch.Tensor, lo_exp: int = -16, hi_exp: int = 16):
    """The octaves [2^lo_exp, 2^hi_exp) of level-0 counts (S, 4096), eight bins each: ``(counts, n_neg, edges)`` with counts int64
    (S, 8 (hi_exp - lo_exp) + 2) -- column 0 the positive entries below the window, the last column those at or above it -- n_neg
    int64 (S,) the negative entries, and edges float32 (8 (hi_exp - lo_exp) + 1), exactly 2^e (1 + i / 8)."""
    if not -126 <= lo_exp < hi_exp <= 127:
        raise ValueError(f"histogram: need -126 <= lo_exp < hi_exp <= 127, got {lo_exp}, {hi_exp}")
    c = counts0 if counts0.dtype == torch.int64 else _u32(counts0)
    lo, hi = 2048 + 8 * (lo_exp + 127), 2048 + 8 * (hi_exp + 127)
    counts = torch.cat([c[:, 2048:lo].sum(1, keepdim=True), c[:, lo:hi], c[:, hi:].sum(1, keepdim=True)], dim=1)
    bits = (torch.arange(lo, hi + 1, dtype=torch.int64) - 2048) << 20  # the float whose key opens the bin
    return counts, c[:, :2048].sum(1), bits.to(torch.int32).view(torch.float32)


class LatentHist(_LatentHistStream):
    """Per-latent activation histogram over a stream of batches (include/saev_amd.h: LATENT HISTOGRAM): the level-0
    count table ``counts0`` (S, 4096) of saev_latent_hist_update -- sign, exponent and three mantissa bits of every code, eight
    bins to the octave -- and the kept rows ``n_rows``, both on the device.  Integer counts: exact, and the same for every order and
    every split of the batches.  ``read`` and ``histogram`` are the device-to-host copies."""

    def __init__(self, d_sae: int, device):
        self._init_stream("LatentHist", d_sae, device)
        if d_sae * 4096 >= 2**32 - 1:
            raise ValueError(f"LatentHist: unsupported d_sae {d_sae} (the table holds fewer than 2^32 - 1 counters)")
        self.counts0 = torch.zeros(d_sae, 4096, device=self.device, dtype=torch.int32)
        self._state = _lib.SaevLatentHistState(struct_size=C.sizeof(_lib.SaevLatentHistState), level=0, T=0, counts=_ptr(self.counts0),
                                               n_rows=_ptr(self.n_rows))

    def zero_(self) -> "LatentHist":
        self.counts0.zero_()
        self.n_rows.zero_()
        self._offered = 0
        return self

    def read(self) -> torch.Tensor:
        """Host ``counts0`` (S, 4096) int64."""
        return _u32(self.counts0).cpu()

    def histogram(self, lo_exp: int = -16, hi_exp: int = 16):
        """``hist_window`` of the table, merged on the device, on the host."""
        counts, n_neg, edges = hist_window(_u32(self.counts0), lo_exp, hi_exp)
        return counts.cpu(), n_neg.cpu(), edges


@dataclasses.dataclass(frozen=True)
class LatentQuantilesHost:
    """What ``LatentQuantiles.result()`` brings back (CPU tensors)."""

    lower: torch.Tensor   # (S, Q) float32: element floor(h) of the sorted multiset, h = (count - 1) q
    higher: torch.Tensor  # (S, Q) float32: element ceil(h)
    linear: torch.Tensor  # (S, Q) float64: lower + (h - floor(h)) (higher - lower)
    count: torch.Tensor   # (S) int64: the size of the latent's multiset (0: NaN in all three)


class LatentQuantiles(_LatentHistStream):
    """Exact per-latent quantiles by a three-pass radix select over the bits of the codes (include/saev_amd.h: LATENT HISTOGRAM;
    DESIGN.md 3.26).  Feed the SAME rows three times: ``add`` / ``add_csr`` the whole stream, ``next_pass()``, again, ``next_pass()``,
    again, ``next_pass()``; then ``result()``.  ``over="rows"`` takes every kept row as an element (the rows a latent is silent on are
    zeros, in closed form), ``over="entries"`` only the stored non-zero codes.  ``next_pass`` reads one device integer back -- the
    kept rows of the pass, which must be those of the first -- and nothing else leaves the device before ``result``."""

    MAX_Q = 8

    def __init__(self, d_sae: int, q, device, over: str = "rows"):
        q = [float(v) for v in (q if isinstance(q, (list, tuple)) else torch.as_tensor(q, dtype=torch.float64).reshape(-1).tolist())]
        if not 1 <= len(q) <= self.MAX_Q:
            raise ValueError(f"LatentQuantiles: unsupported number of quantiles {len(q)} (1 <= Q <= {self.MAX_Q})")
        if not all(0.0 <= v <= 1.0 for v in q):
            raise ValueError(f"LatentQuantiles: every q must lie in [0, 1], got {q}")
        if over not in ("rows", "entries"):
            raise ValueError(f"LatentQuantiles: over must be 'rows' or 'entries', got {over!r}")
        self._init_stream("LatentQuantiles", d_sae, device)
        self.q, self.over, self.Q, self.T = tuple(q), over, len(q), 2 * len(q)
        if d_sae * max(4096, self.T * 1024) >= 2**32 - 1:
            raise ValueError(f"LatentQuantiles: unsupported d_sae {d_sae} with {self.Q} quantiles (a table holds fewer than 2^32 - 1 counters)")
        S, dev = d_sae, self.device
        self.counts0 = torch.zeros(S, 4096, device=dev, dtype=torch.int32)
        self.counts = None  # (S, T, 1024), levels 1 and 2: made when level 0 is located
        self.prefix = torch.zeros(S, self.T_STRIDE, device=dev, dtype=torch.int32)
        self.rank = torch.zeros(S, self.T_STRIDE, device=dev, dtype=torch.int32)
        self.resolved = torch.zeros(S, self.T_STRIDE, device=dev, dtype=torch.int32)
        self.count = torch.zeros(S, device=dev, dtype=torch.int64)
        self.lower = torch.zeros(S, self.Q, device=dev, dtype=torch.float32)
        self.higher = torch.zeros(S, self.Q, device=dev, dtype=torch.float32)
        self.linear = torch.zeros(S, self.Q, device=dev, dtype=torch.float64)
        self._targets = _lib.SaevLatentHistTargets(struct_size=C.sizeof(_lib.SaevLatentHistTargets), Q=self.Q, over_rows=int(over == "rows"),
                                                   q=(C.c_double * 8)(*q), prefix=_ptr(self.prefix), rank=_ptr(self.rank),
                                                   resolved=_ptr(self.resolved), count=_ptr(self.count), lower=_ptr(self.lower),
                                                   higher=_ptr(self.higher), linear=_ptr(self.linear))
        self.n_passes = 0
        self._rows_first = None
        self._arm(0)

    def _arm(self, level: int) -> None:
        table = self.counts0 if level == 0 else self.counts
        self._state = _lib.SaevLatentHistState(struct_size=C.sizeof(_lib.SaevLatentHistState), level=level, T=0 if level == 0 else self.T,
                                               counts=_ptr(table), n_rows=_ptr(self.n_rows), prefix=None if level == 0 else _ptr(self.prefix))

    @property
    def done(self) -> bool:
        return self.n_passes == 3

    def _accepts(self) -> None:
        if self.done:
            raise _lib.SaevError("LatentQuantiles: the three passes are done (read result(); a new selection needs a new object)")

    def next_pass(self) -> None:
        """Locates every target in the tables of the pass just fed, and arms the next level."""
        self._accepts()
        with torch.cuda.device(self.device):
            rc = self.lib.saev_latent_hist_locate(C.byref(self._state), C.byref(self._targets), self.d_sae, _stream())
        _lib.check(self.lib, None, rc, "saev_latent_hist_locate")
        rows = int(self.n_rows.item())  # the one read-back of a pass
        if self._rows_first is None:
            self._rows_first = rows
        elif rows != self._rows_first:
            raise _lib.SaevError(f"LatentQuantiles: pass {self.n_passes + 1} was fed {rows} kept rows, the first pass {self._rows_first}")
        self.n_passes += 1
        if not self.done:
            if self.counts is None:
                self.counts0 = None  # level 0 is located: its table makes room for the refine table
                self.counts = torch.zeros(self.d_sae, self.T, 1024, device=self.device, dtype=torch.int32)
            else:
                self.counts.zero_()
            self.n_rows.zero_()
            self._offered = 0
            self._arm(self.n_passes)

    def result(self) -> LatentQuantilesHost:
        if not self.done:
            raise _lib.SaevError(f"LatentQuantiles: {self.n_passes} of 3 passes done")
        return LatentQuantilesHost(lower=self.lower.cpu(), higher=self.higher.cpu(), linear=self.linear.cpu(), count=self.count.cpu())


def latent_quantiles(indptr, indices, data, n_rows: int, n_latents: int, q, *, over: str = "rows", chunk_rows: int = 2**20,
                     device=None, hist: LatentHist | None = None) -> LatentQuantilesHost:
    """The quantiles ``q`` of every column of a CSR matrix (n_rows, n_latents), on the host (numpy / torch CPU) or on the device:
    the three passes of ``LatentQuantiles`` over row chunks of ``chunk_rows``.  ``hist`` also receives the chunks, once."""
    if chunk_rows < 1:
        raise ValueError(f"latent_quantiles: chunk_rows must be >= 1, got {chunk_rows}")
    indptr, indices, data = (torch.as_tensor(a) for a in (indptr, indices, data))
    if indptr.numel() != n_rows + 1:
        raise ValueError(f"latent_quantiles: indptr must hold n_rows + 1 = {n_rows + 1} offsets, got {indptr.numel()}")
    device = _hip_device("latent_quantiles", device if device is not None else indptr.device)
    acc = LatentQuantiles(n_latents, q, device, over)
    host_ptr = indptr.to(torch.int64).cpu()

    def chunk(r0: int):  # (host data crosses to the device once a pass)
        r1 = min(n_rows, r0 + chunk_rows)
        a, b = int(host_ptr[r0]), int(host_ptr[r1])
        return ((host_ptr[r0:r1 + 1] - a).to(device), indices[a:b].to(device=device, dtype=torch.int32),
                data[a:b].to(device=device, dtype=torch.float32))

    for level in range(3):
        for r0 in range(0, n_rows, chunk_rows):
            block = chunk(r0)
            acc.add_csr(*block)
            if level == 0 and hist is not None:
                hist.add_csr(*block)
        acc.next_pass()
    return acc.result()


@dataclasses.dataclass(frozen=True)
class Probe1DHyper:
    """The reference's Sparse1DProbe hyper-parameters (include/saev_amd.h: saev_probe1d_cfg)."""

    ridge: float = 1e-8
    tol: float = 1e-6
    max_iter: int = 200
    lam_init: float = 1e-3
    lam_shrink: float = 0.1
    lam_grow: float = 10.0
    delta_logit: float = 6.0
    class_slab_size: int = 8


class Probe1D:
    """Per-latent logistic probes on one prepared split (include/saev_amd.h: PROBE1D): the workspace of the
    saev_probe1d_* entries for a CSR matrix x (N, S) and labels over C classes, and views of what ``prepare`` leaves in it.
    ``prepare`` sorts the stored entries latent-major and packs the labels; ``stats`` gives the seven event sums of every pair at
    given (b, w); ``fit`` runs the solver on the device; ``evaluate`` gives loss and confusion counts at given (b, w).  All sums are
    fp64 in a fixed order: two runs give the same bits."""

    CHUNK = 512
    MAX_CLASSES = 4096
    _DTYPES = {torch.float32: 0, torch.float64: 1}
    _ERRORS = {1: "a class id lies outside [0, n_classes)", 2: "a column index lies outside [0, n_latents)", 3: "a label is neither 0 nor 1"}

    def __init__(self, n_rows: int, n_latents: int, n_classes: int, nnz: int, device):
        for name, v, hi in (("n_rows", n_rows, 2**31), ("n_latents", n_latents, 2**31), ("n_classes", n_classes, self.MAX_CLASSES + 1)):
            if not 1 <= v < hi:
                raise ValueError(f"Probe1D: unsupported {name} {v} (1 <= {name} < {hi})")
        if not 0 <= nnz < 2**31:
            raise ValueError(f"Probe1D: unsupported nnz {nnz} (0 <= nnz < 2^31)")
        self.device = _hip_device("Probe1D", device)
        self.lib = _lib.load()
        self.shape = (n_rows, n_latents, n_classes, nnz)
        self.layout = _lib.SaevProbe1DLayout()
        _lib.check(self.lib, None, self.lib.saev_probe1d_layout_of(*self.shape, C.byref(self.layout)), "saev_probe1d_layout_of")
        self._ws = torch.empty(self.layout.total_bytes, device=self.device, dtype=torch.uint8)
        self.prepared = False

    def _view(self, off: int, dtype, *shape):
        n = math.prod(shape) * torch.empty((), dtype=dtype).element_size()
        return self._ws[off:off + n].view(dtype).view(*shape)

    # what prepare leaves, and the solver state (views into the workspace)
    starts = property(lambda self: self._view(self.layout.off_starts, torch.int64, self.shape[1] + 1))
    chunk_starts = property(lambda self: self._view(self.layout.off_chunk_starts, torch.int32, self.shape[1] + 1))
    row = property(lambda self: self._view(self.layout.off_row, torch.int32, self.shape[3]))
    val = property(lambda self: self._view(self.layout.off_val, torch.float32, self.shape[3]))
    qx = property(lambda self: self._view(self.layout.off_qx, torch.float64, self.shape[1]))
    ybits = property(lambda self: self._view(self.layout.off_ybits, torch.int32, self.shape[0], self.layout.words))
    pos = property(lambda self: self._view(self.layout.off_pos, torch.int64, self.shape[2]))
    err = property(lambda self: self._view(self.layout.off_err, torch.int32, 1))
    done = property(lambda self: self._view(self.layout.off_done, torch.int32, self.shape[2]))

    def state(self, name: str) -> torch.Tensor:
        """b, w, lam, prev_pred, prev_loss (S, C) float64 or clipped (S, C) int32: the solver state, in place."""
        off = getattr(self.layout, "off_" + name)
        return self._view(off, torch.int32 if name == "clipped" else torch.float64, self.shape[1], self.shape[2])

    def _call(self, name: str, *args) -> None:
        with torch.cuda.device(self.device):
            rc = getattr(self.lib, name)(*args, _ptr(self._ws), self._ws.numel(), _stream())
        _lib.check(self.lib, None, rc, name)

    def prepare(self, indptr: torch.Tensor, indices: torch.Tensor, data: torch.Tensor, *, labels: torch.Tensor | None = None,
                y: torch.Tensor | None = None) -> "Probe1D":
        """x as CSR on the device (indptr (N + 1) int64 from 0, indices (nnz) int32, data (nnz) float32) and the labels in ONE form:
        ``labels`` (N) uint8 / int32 class ids, or ``y`` (N, C) bool / uint8 with entries 0 or 1.  Reads the error word back."""
        n, s, c, nnz = self.shape
        if (labels is None) == (y is None):
            raise ValueError("Probe1D.prepare: give the labels as class ids (labels=) or as an N x C matrix (y=), one of the two")
        indptr, indices, data = _csr_on(indptr, indices, data, n, nnz, self.device)
        u8 = i32 = mat = None
        if labels is not None:
            if labels.dtype == torch.uint8 and c <= 256:
                u8 = _on(labels, torch.uint8, (n,), "labels", self.device)
            elif labels.dtype in (torch.uint8, torch.int32, torch.int64):
                i32 = _on(labels.to(torch.int32), torch.int32, (n,), "labels", self.device)
            else:
                raise ValueError(f"labels must be uint8, int32 or int64 class ids, got {labels.dtype}")
        else:
            if y.dtype == torch.bool:
                y = y.view(torch.uint8)
            mat = _on(y, torch.uint8, (n, c), "y", self.device)
        self._call("saev_probe1d_prepare", _ptr(indptr), _ptr(indices), _ptr(data), nnz, n, s, c, _ptr(u8), _ptr(i32), _ptr(mat))
        _check_err_word(self.err, self._ERRORS, "Probe1D.prepare")
        self.prepared = True
        return self

    def _cfg(self, hp: Probe1DHyper, dtype=torch.float32, poll_every: int = 0) -> "_lib.SaevProbe1DCfg":
        if dtype not in self._DTYPES:
            raise ValueError(f"dtype must be torch.float32 or torch.float64, got {dtype}")
        return _lib.SaevProbe1DCfg(struct_size=C.sizeof(_lib.SaevProbe1DCfg), max_iter=hp.max_iter, class_slab_size=hp.class_slab_size,
                                   poll_every=poll_every, out_dtype=self._DTYPES[dtype], ridge=hp.ridge, tol=hp.tol, lam_init=hp.lam_init,
                                   lam_shrink=hp.lam_shrink, lam_grow=hp.lam_grow, delta_logit=hp.delta_logit)

    def _need(self):
        if not self.prepared:
            raise _lib.SaevError("Probe1D: prepare() first")

    def stats(self, b: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
        """The event sums (S, 7, C) float64 of every pair at (b, w), each (S, C) float64: mu, (mu - y) v, s, s v, s v^2, loss, y."""
        self._need()
        n, s, c, nnz = self.shape
        b, w = _on(b, torch.float64, (s, c), "b", self.device), _on(w, torch.float64, (s, c), "w", self.device)
        out = torch.empty(s, 7, c, device=self.device, dtype=torch.float64)
        self._call("saev_probe1d_stats", n, s, c, nnz, _ptr(b), _ptr(w), _ptr(out))
        return out

    def init(self, hp: Probe1DHyper) -> None:
        self._need()
        self._call("saev_probe1d_init", *self.shape, C.byref(self._cfg(hp)))

    def update(self, hp: Probe1DHyper, sums: torch.Tensor | None = None, *, debug: bool = False):
        """One solver iteration on the state in the workspace from ``sums`` (None: the workspace's own).  With ``debug`` returns
        (step (S, C, 4) float64: db, dw, pred, lam; flags (S, C) int32: SAEV_PROBE1D_STEP_* | tries << 8)."""
        self._need()
        n, s, c, nnz = self.shape
        sums = _on(sums, torch.float64, (s, 7, c), "sums", self.device)
        step = torch.zeros(s, c, 4, device=self.device, dtype=torch.float64) if debug else None
        flags = torch.zeros(s, c, device=self.device, dtype=torch.int32) if debug else None
        self._call("saev_probe1d_update", n, s, c, nnz, C.byref(self._cfg(hp)), _ptr(sums), _ptr(step), _ptr(flags))
        return (step, flags) if debug else None

    def fit(self, hp: Probe1DHyper, *, dtype=torch.float32, poll_every: int = 1):
        """(coef, intercept) (S, C) in ``dtype`` and n_iter (C) int32.  ``poll_every`` > 0: the host reads the number of running slabs
        every that many iterations and stops launching at 0 (same results as 0 = never)."""
        self._need()
        n, s, c, nnz = self.shape
        coef = torch.empty(s, c, device=self.device, dtype=dtype)
        intercept = torch.empty(s, c, device=self.device, dtype=dtype)
        n_iter = torch.empty(c, device=self.device, dtype=torch.int32)
        self._call("saev_probe1d_fit", n, s, c, nnz, C.byref(self._cfg(hp, dtype, poll_every)), _ptr(coef), _ptr(intercept), _ptr(n_iter))
        return coef, intercept, n_iter

    def evaluate(self, b: torch.Tensor, w: torch.Tensor, threshold: float = 0.5, *, dtype=torch.float32):
        """(loss, tp, fp, tn, fn), each (S, C) in ``dtype``, at (b, w) (S, C) float64."""
        self._need()
        if not 0.0 < threshold < 1.0:
            raise ValueError("threshold must be between 0 and 1.")
        if dtype not in self._DTYPES:
            raise ValueError(f"dtype must be torch.float32 or torch.float64, got {dtype}")
        n, s, c, nnz = self.shape
        b, w = _on(b, torch.float64, (s, c), "b", self.device), _on(w, torch.float64, (s, c), "w", self.device)
        outs = [torch.empty(s, c, device=self.device, dtype=dtype) for _ in range(5)]
        self._call("saev_probe1d_evaluate", n, s, c, nnz, _ptr(b), _ptr(w), float(threshold), self._DTYPES[dtype], *map(_ptr, outs))
        return tuple(outs)


class _APResult(_Checked):
    """What ``latent_ap`` and ``probe_ap`` both leave: the results, and the workspace with its error word and its sorted events."""

    def __init__(self, out: dict, ws, layout, shape):
        super().__init__(out, ws[layout.off_err:layout.off_err + 4].view(torch.int32), self._ERRORS, self._WHO)
        self._ws, self.layout, self.shape = ws, layout, shape

    def sorted_events(self):
        """(starts (S + 1) int64, key (E) int32 bit patterns of the uint32 keys, latent (E) int32, row (E) int32) of the E events in
        (latent, value descending, row ascending) order."""
        n, s, c, nnz = self.shape
        lay = self.layout
        view = lambda off, dtype, k: self._ws[off:off + k * torch.empty((), dtype=dtype).element_size()].view(dtype)  # noqa: E731
        starts = view(lay.off_starts, torch.int64, s + 1)
        e = int(starts[s].item())
        return starts, view(lay.off_key, torch.int32, nnz)[:e], view(lay.off_latent, torch.int32, nnz)[:e], view(lay.off_row, torch.int32, nnz)[:e]


class LatentAPResult(_APResult):
    """What ``latent_ap`` leaves on the device: ``ap`` (S, C) float64, ``n_pos`` (C) int64, ``best_ap`` (S) float64 and ``best_class``
    (S) int32, the lowest column that attains the row maximum.  The call itself does not synchronise; the first read of any of the
    four reads the device's error word (one synchronisation) and raises ValueError if it is not 0.  ``sorted_events()`` gives the
    workspace's sorted entries (include/saev_amd.h: LATENT AP)."""

    _WHO = "latent_ap"
    _ERRORS = {1: "a class id lies outside [-1, n_classes)", 2: "a column index lies outside [0, n_latents)"}

    ap = property(lambda self: self._read("ap"))
    n_pos = property(lambda self: self._read("n_pos"))
    best_ap = property(lambda self: self._read("best_ap"))
    best_class = property(lambda self: self._read("best_class"))


def _ap_open(who: str, indptr, indices, data, n_rows: int, n_latents: int, n_classes: int, labels, remap, nnz, top_k: int = 0, n_tasks: int | None = None,
             ws=None):
    """What ``latent_ap``, ``probe_ap``, ``latent_auroc`` and ``latent_operating`` do before their C entry: the size checks, the nnz
    rule, the CSR triple and the labels on the device, the layout and a workspace of its size (with ``n_tasks``: of ``latent_auroc``'s
    size, which begins with that layout; with ``ws``: that workspace, checked against the size).  Returns (lib, device, nnz, the ten
    leading arguments of either entry, ws, layout)."""
    for name, v, hi in (("n_rows", n_rows, 2**31), ("n_latents", n_latents, 2**31), ("n_classes", n_classes, 4097)):
        if not 1 <= v < hi:
            raise ValueError(f"{who}: unsupported {name} {v} (1 <= {name} < {hi})")
    if not 0 <= top_k <= n_rows:
        raise ValueError(f"{who}: top_k {top_k} must lie in [0, n_rows = {n_rows}]")
    device = _hip_device(who, indptr.device)
    stored = indices.numel()
    nnz = stored if nnz is None else int(nnz)
    if not 0 <= nnz < 2**31 or nnz > stored:
        raise ValueError(f"{who}: unsupported nnz {nnz} (0 <= nnz < 2^31, and at most the {stored} entries of indices)")
    csr = _csr_on(indptr, indices, data, n_rows, stored, device)
    classes = _class_labels(who, labels, remap, n_rows, device)
    lib = _lib.load()
    layout = _lib.SaevLatentAPLayout()
    _lib.check(lib, None, lib.saev_latent_ap_layout_of(n_rows, n_latents, n_classes, nnz, C.byref(layout)), "saev_latent_ap_layout_of")
    total = layout.total_bytes if n_tasks is None else lib.saev_latent_auroc_workspace_bytes(n_rows, n_latents, n_classes, n_tasks, nnz)
    if ws is None:
        ws = torch.empty(total, device=device, dtype=torch.uint8)
    elif ws.numel() != total or ws.device != device:
        raise ValueError(f"{who}: the workspace to reuse holds {ws.numel()} bytes on {ws.device}, this call needs {total} on {device}")
    return lib, device, nnz, csr, classes, ws, layout


def latent_ap(indptr: torch.Tensor, indices: torch.Tensor, data: torch.Tensor, n_rows: int, n_latents: int, n_classes: int, *,
              labels: torch.Tensor, remap: torch.Tensor | None = None, nnz: int | None = None) -> LatentAPResult:
    """Exact tie-aware average precision of every latent against every class (include/saev_amd.h: LATENT AP).
    x as CSR on the device (indptr (N + 1) int64, indices (nnz) int32, data (nnz) float32); ``labels`` (N) int32 / int64 columns with
    -1 for a row without a class, or uint8 bytes with an optional ``remap`` (256) int32 byte -> column or -1.  ``indptr`` holds
    absolute positions into ``indices`` / ``data``: when it does not start at 0 (a block cut out of a longer CSR) give
    ``nnz = indptr[-1] - indptr[0]``, which is otherwise taken to be ``indices.numel()`` -- the call reads no device value back to
    find it out, and ``indices`` and ``data`` must hold ``indptr[-1]`` entries.  One call, one workspace, no synchronisation; there
    is no CPU path."""
    lib, device, nnz, csr, classes, ws, layout = _ap_open("latent_ap", indptr, indices, data, n_rows, n_latents, n_classes, labels, remap, nnz)
    out = dict(ap=torch.empty(n_latents, n_classes, device=device, dtype=torch.float64),
               n_pos=torch.empty(n_classes, device=device, dtype=torch.int64),
               best_ap=torch.empty(n_latents, device=device, dtype=torch.float64),
               best_class=torch.empty(n_latents, device=device, dtype=torch.int32))
    with torch.cuda.device(device):
        rc = lib.saev_latent_ap(*map(_ptr, csr), nnz, n_rows, n_latents, n_classes, *map(_ptr, classes), *map(_ptr, out.values()), _ptr(ws),
                                ws.numel(), _stream())
    _lib.check(lib, None, rc, "saev_latent_ap")
    return LatentAPResult(out, ws, layout, (n_rows, n_latents, n_classes, nnz))


class ProbeAPResult(_APResult):
    """What ``probe_ap`` leaves on the device: ``ap`` (S, C) float64 (NaN for a pair whose w or b is not finite), ``n_pos`` (C) int64,
    ``tp`` and ``n_pred_pos`` (S, C) int64 (rows with score > 0, and those of them in the class) and ``top_rows`` (S, top_k) int64 or
    None.  The call itself does not synchronise; the first read of a result -- or ``check()`` -- reads the device's error word (one
    synchronisation) and raises ValueError if it is not 0.  ``layout`` is the workspace's, as of ``latent_ap``
    (include/saev_amd.h: PROBE AP)."""

    _WHO = "probe_ap"
    _ERRORS = {**LatentAPResult._ERRORS, 3: "a stored value is not finite"}

    ap = property(lambda self: self._read("ap"))
    n_pos = property(lambda self: self._read("n_pos"))
    tp = property(lambda self: self._read("tp"))
    n_pred_pos = property(lambda self: self._read("n_pred_pos"))
    top_rows = property(lambda self: self._read("top_rows"))


def probe_ap(indptr: torch.Tensor, indices: torch.Tensor, data: torch.Tensor, n_rows: int, n_latents: int, n_classes: int, *,
             labels: torch.Tensor, remap: torch.Tensor | None = None, weights: torch.Tensor, biases: torch.Tensor, top_k: int = 0,
             nnz: int | None = None) -> ProbeAPResult:
    """Exact tie-aware average precision of the score ``w * a + b`` of every (latent, class) pair, the counts behind precision and
    recall at score > 0, and the ``top_k`` highest rows of every latent (include/saev_amd.h: PROBE AP).  x, ``labels``,
    ``remap`` and ``nnz`` as for ``latent_ap``; ``weights`` and ``biases`` (S, C), both float32 or both float64: their dtype is the
    arithmetic the score is rounded in.  One call, one workspace, no synchronisation; there is no CPU path."""
    lib, device, nnz, csr, classes, ws, layout = _ap_open("probe_ap", indptr, indices, data, n_rows, n_latents, n_classes, labels, remap, nnz,
                                                          top_k)
    if weights.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"weights must be float32 or float64, got {weights.dtype}")
    weights = _on(weights, weights.dtype, (n_latents, n_classes), "weights", device)
    biases = _on(biases, weights.dtype, (n_latents, n_classes), "biases", device)
    pairs = dict(device=device, dtype=torch.int64)
    out = dict(ap=torch.empty(n_latents, n_classes, device=device, dtype=torch.float64),
               n_pos=torch.empty(n_classes, device=device, dtype=torch.int64),
               tp=torch.empty(n_latents, n_classes, **pairs), n_pred_pos=torch.empty(n_latents, n_classes, **pairs),
               top_rows=torch.empty(n_latents, top_k, **pairs) if top_k > 0 else None)
    with torch.cuda.device(device):
        rc = lib.saev_probe_ap(*map(_ptr, csr), nnz, n_rows, n_latents, n_classes, *map(_ptr, classes), _ptr(weights), _ptr(biases),
                               0 if weights.dtype == torch.float32 else 1, _ptr(out["ap"]), _ptr(out["n_pos"]), _ptr(out["tp"]),
                               _ptr(out["n_pred_pos"]), top_k, _ptr(out["top_rows"]), _ptr(ws), ws.numel(), _stream())
    _lib.check(lib, None, rc, "saev_probe_ap")
    return ProbeAPResult(out, ws, layout, (n_rows, n_latents, n_classes, nnz))


class LatentAUROCResult(_APResult):
    """What ``latent_auroc`` leaves on the device: ``auroc`` (S, T) float64 (NaN for a task without positives or without negatives),
    ``u2`` (S, T) int64 (twice the Mann-Whitney U: 2 x pairs ranked right + tied pairs), ``n_pos`` and ``n_neg`` (T) int64,
    ``fire_pos`` and ``fire_neg`` (S, T) int64 (included rows of the role with activation > 0), ``sum_pos`` and ``sum_neg`` (S, T)
    float64 (the role's activations summed) and ``class_counts`` (C) int64.  The call itself does not synchronise; the first read of
    a result -- or ``check()`` -- reads the device's error word (one synchronisation) and raises ValueError if it is not 0.
    ``layout`` is the leading part of the workspace, as of ``latent_ap`` (include/saev_amd.h: LATENT AUROC)."""

    _WHO = "latent_auroc"
    _ERRORS = {**LatentAPResult._ERRORS, 4: "a role byte is above 2"}

    auroc = property(lambda self: self._read("auroc"))
    u2 = property(lambda self: self._read("u2"))
    n_pos = property(lambda self: self._read("n_pos"))
    n_neg = property(lambda self: self._read("n_neg"))
    fire_pos = property(lambda self: self._read("fire_pos"))
    fire_neg = property(lambda self: self._read("fire_neg"))
    sum_pos = property(lambda self: self._read("sum_pos"))
    sum_neg = property(lambda self: self._read("sum_neg"))
    class_counts = property(lambda self: self._read("class_counts"))


def latent_auroc(indptr: torch.Tensor, indices: torch.Tensor, data: torch.Tensor, n_rows: int, n_latents: int, n_classes: int, *,
                 labels: torch.Tensor, remap: torch.Tensor | None = None, roles: torch.Tensor, nnz: int | None = None) -> LatentAUROCResult:
    """Exact tie-aware AUROC of every latent on every binary task, with the per-role supports and activation sums
    (include/saev_amd.h: LATENT AUROC).  x, ``labels``, ``remap`` and ``nnz`` as for ``latent_ap``; ``roles`` (T, C)
    uint8 on the device: 0 leaves the rows of class c out of task t, 1 makes them its negatives, 2 its positives; 1 <= T <= 4096.
    One call, one workspace, no synchronisation; there is no CPU path."""
    if roles.dim() != 2 or roles.dtype != torch.uint8:
        raise ValueError(f"latent_auroc: roles must be a (n_tasks, n_classes) uint8 matrix, got {roles.dtype} {tuple(roles.shape)}")
    n_tasks = roles.shape[0]
    if not 1 <= n_tasks <= 4096:
        raise ValueError(f"latent_auroc: unsupported n_tasks {n_tasks} (1 <= n_tasks <= 4096)")
    lib, device, nnz, csr, classes, ws, layout = _ap_open("latent_auroc", indptr, indices, data, n_rows, n_latents, n_classes, labels, remap, nnz,
                                                          n_tasks=n_tasks)
    roles = _on(roles, torch.uint8, (n_tasks, n_classes), "roles", device)
    pairs, tasks = (n_latents, n_tasks), (n_tasks,)
    i64, f64 = dict(device=device, dtype=torch.int64), dict(device=device, dtype=torch.float64)
    out = dict(auroc=torch.empty(pairs, **f64), u2=torch.empty(pairs, **i64), n_pos=torch.empty(tasks, **i64), n_neg=torch.empty(tasks, **i64),
               fire_pos=torch.empty(pairs, **i64), fire_neg=torch.empty(pairs, **i64), sum_pos=torch.empty(pairs, **f64),
               sum_neg=torch.empty(pairs, **f64), class_counts=torch.empty(n_classes, **i64))
    with torch.cuda.device(device):
        rc = lib.saev_latent_auroc(*map(_ptr, csr), nnz, n_rows, n_latents, n_classes, *map(_ptr, classes), _ptr(roles), n_tasks,
                                   *map(_ptr, out.values()), _ptr(ws), ws.numel(), _stream())
    _lib.check(lib, None, rc, "saev_latent_auroc")
    return LatentAUROCResult(out, ws, layout, (n_rows, n_latents, n_classes, nnz))


class LatentOperatingResult(_APResult):
    """What ``latent_operating`` leaves on the device, (S, T) each: ``f1`` float64 (NaN for a task without positives), ``f1_thr``
    float32, ``f1_tp`` and ``f1_fp`` int64 (the best F1 of the rule "a >= f1_thr", the threshold and the confusion counts there);
    ``j2`` int64 (TP n_neg - FP n_pos at its best), ``youden`` float64 (NaN for a task without positives or without negatives),
    ``j_thr`` float32, ``j_tp`` and ``j_fp`` int64; and ``n_pos``, ``n_neg`` (T) and ``class_counts`` (C) int64.  A threshold of +Inf
    with no predicted row is "predict nothing".  ``precision_f1``, ``recall_f1``, ``tpr_j`` and ``fpr_j`` (S, T) float64 are formed
    from the counts on the device (NaN where the denominator is 0).  The call itself does not synchronise; the first read of a
    result -- or ``check()`` -- reads the device's error word (one synchronisation) and raises ValueError if it is not 0
    (include/saev_amd.h: LATENT OPERATING POINTS)."""

    _WHO = "latent_operating"
    _ERRORS = LatentAUROCResult._ERRORS
    PAIRS = ("f1", "f1_thr", "f1_tp", "f1_fp", "j2", "youden", "j_thr", "j_tp", "j_fp")

    f1 = property(lambda self: self._read("f1"))
    f1_thr = property(lambda self: self._read("f1_thr"))
    f1_tp = property(lambda self: self._read("f1_tp"))
    f1_fp = property(lambda self: self._read("f1_fp"))
    j2 = property(lambda self: self._read("j2"))
    youden = property(lambda self: self._read("youden"))
    j_thr = property(lambda self: self._read("j_thr"))
    j_tp = property(lambda self: self._read("j_tp"))
    j_fp = property(lambda self: self._read("j_fp"))
    n_pos = property(lambda self: self._read("n_pos"))
    n_neg = property(lambda self: self._read("n_neg"))
    class_counts = property(lambda self: self._read("class_counts"))

    @staticmethod
    def _ratio(num, den):
        den = den.to(torch.float64)
        return torch.where(den > 0, num.to(torch.float64) / den.clamp_min(1.0), torch.full_like(den, float("nan")))

    precision_f1 = property(lambda self: self._ratio(self.f1_tp, self.f1_tp + self.f1_fp))
    recall_f1 = property(lambda self: self._ratio(self.f1_tp, self.n_pos[None, :].expand_as(self.f1_tp)))
    tpr_j = property(lambda self: self._ratio(self.j_tp, self.n_pos[None, :].expand_as(self.j_tp)))
    fpr_j = property(lambda self: self._ratio(self.j_fp, self.n_neg[None, :].expand_as(self.j_fp)))


def latent_operating(indptr: torch.Tensor, indices: torch.Tensor, data: torch.Tensor, n_rows: int, n_latents: int, n_classes: int, *,
                     labels: torch.Tensor, remap: torch.Tensor | None = None, roles: torch.Tensor, nnz: int | None = None,
                     reuse: "LatentAUROCResult | LatentOperatingResult | None" = None) -> LatentOperatingResult:
    """For every latent and every binary task the threshold at which "a >= theta => positive" has the best F1 and the one with the
    best Youden J, with the confusion counts at both, exact (include/saev_amd.h: LATENT OPERATING POINTS).  x,
    ``labels``, ``remap``, ``roles`` and ``nnz`` as for ``latent_auroc``.  ``reuse``: the result of a ``latent_auroc`` or
    ``latent_operating`` call ON THE SAME ARGUMENTS (the caller vouches for that; the shapes are checked here, before any device
    work): its workspace -- sorted events and role table -- and its counts are taken over and nothing is sorted again; the new result
    shares them.  One call, no synchronisation; there is no CPU path."""
    who = "latent_operating"
    if roles.dim() != 2 or roles.dtype != torch.uint8:
        raise ValueError(f"{who}: roles must be a (n_tasks, n_classes) uint8 matrix, got {roles.dtype} {tuple(roles.shape)}")
    n_tasks = roles.shape[0]
    if not 1 <= n_tasks <= 4096:
        raise ValueError(f"{who}: unsupported n_tasks {n_tasks} (1 <= n_tasks <= 4096)")
    stored = indices.numel() if nnz is None else int(nnz)
    if reuse is not None:
        if not isinstance(reuse, (LatentAUROCResult, LatentOperatingResult)):
            raise ValueError(f"{who}: reuse takes a LatentAUROCResult or a LatentOperatingResult, got {type(reuse).__name__}")
        have = (*reuse.shape, reuse._out["n_pos"].numel())
        if have != (n_rows, n_latents, n_classes, stored, n_tasks):
            raise ValueError(f"{who}: the result to reuse has (n_rows, n_latents, n_classes, nnz, n_tasks) = {have}, this call "
                             f"{(n_rows, n_latents, n_classes, stored, n_tasks)}")
    lib, device, nnz, csr, classes, ws, layout = _ap_open(who, indptr, indices, data, n_rows, n_latents, n_classes, labels, remap, nnz, n_tasks=n_tasks,
                                                          ws=None if reuse is None else reuse._ws)
    roles = _on(roles, torch.uint8, (n_tasks, n_classes), "roles", device)
    pairs = (n_latents, n_tasks)
    i64, f64, f32 = (dict(device=device, dtype=dt) for dt in (torch.int64, torch.float64, torch.float32))
    out = dict(f1=torch.empty(pairs, **f64), f1_thr=torch.empty(pairs, **f32), f1_tp=torch.empty(pairs, **i64), f1_fp=torch.empty(pairs, **i64),
               j2=torch.empty(pairs, **i64), youden=torch.empty(pairs, **f64), j_thr=torch.empty(pairs, **f32), j_tp=torch.empty(pairs, **i64),
               j_fp=torch.empty(pairs, **i64))
    if reuse is None:
        out.update(n_pos=torch.empty(n_tasks, **i64), n_neg=torch.empty(n_tasks, **i64), class_counts=torch.empty(n_classes, **i64))
    else:
        out.update({k: reuse._out[k] for k in ("n_pos", "n_neg", "class_counts")})
    with torch.cuda.device(device):
        rc = lib.saev_latent_operating(*map(_ptr, csr), nnz, n_rows, n_latents, n_classes, *map(_ptr, classes), _ptr(roles), n_tasks,
                                       0 if reuse is None else _lib.OPERATING_SORTED, *map(_ptr, out.values()), _ptr(ws), ws.numel(), _stream())
    _lib.check(lib, None, rc, "saev_latent_operating")
    return LatentOperatingResult(out, ws, layout, (n_rows, n_latents, n_classes, nnz))


class LatentSpatialResult(_Checked):
    """What ``latent_spatial`` leaves on the device.  (S, G) int64: ``n_events``, ``n_images_fire``, ``pairs_h``, ``pairs_v``,
    ``sum_m2`` and ``overlap``; ``moments`` (S, G, 5) float64 (sum v, sum v r, sum v c, sum v r^2, sum v c^2); ``count_map``
    (S, G, gh, gw) int32; ``sum_map`` (S, G, gh, gw) float64 or None; ``n_group_images`` (G) int64.  ``grid`` is (gh, gw).  The call
    itself does not synchronise; the first read of a result -- or ``check()`` -- reads the device's error word (one synchronisation)
    and raises ValueError if it is not 0 (include/saev_amd.h: LATENT SPATIAL).  ``saev_amd.spatial`` turns the integers into scores."""

    _WHO = "latent_spatial"
    _ERRORS = {1: "a group id lies outside [-1, n_groups)", 2: "a column index lies outside [0, n_latents)"}

    def __init__(self, out: dict, ws, grid):
        super().__init__(out, ws[0:4].view(torch.int32), self._ERRORS, self._WHO)
        self._ws, self.grid = ws, grid

    n_group_images = property(lambda self: self._read("n_group_images"))
    n_events = property(lambda self: self._read("n_events"))
    n_images_fire = property(lambda self: self._read("n_images_fire"))
    pairs_h = property(lambda self: self._read("pairs_h"))
    pairs_v = property(lambda self: self._read("pairs_v"))
    sum_m2 = property(lambda self: self._read("sum_m2"))
    overlap = property(lambda self: self._read("overlap"))
    moments = property(lambda self: self._read("moments"))
    count_map = property(lambda self: self._read("count_map"))
    sum_map = property(lambda self: self._read("sum_map"))


def latent_spatial(indptr: torch.Tensor, indices: torch.Tensor, data: torch.Tensor, *, n_images: int, grid: tuple[int, int], n_latents: int,
                   groups: torch.Tensor, n_groups: int, threshold: float = 0.0, sum_map: bool = True, nnz: int | None = None) -> LatentSpatialResult:
    """Where every latent fires on the (gh, gw) patch grid, per group of images: the exact counts behind the spatial-coherence scores
    of ``saev_amd.spatial`` and the per-cell maps (include/saev_amd.h: LATENT SPATIAL).  x as CSR on the device over
    ``n_images * gh * gw`` rows (indptr int64, indices int32, data float32; ``nnz`` as for ``latent_ap``), row ``i * gh * gw + p``
    being position p of image i; ``groups`` (n_images) int32 / int64 in [-1, n_groups), -1 leaving the image out; an entry fires when
    it is > ``threshold`` (>= 0).  ``sum_map=False`` leaves the (S, G, gh, gw) float64 map out.  One call, one workspace, no
    synchronisation; there is no CPU path."""
    who = "latent_spatial"
    gh, gw = (int(g) for g in grid)
    if gh < 1 or gw < 1 or gh * gw > 4096:
        raise ValueError(f"{who}: unsupported grid {gh} x {gw} (gh, gw >= 1 and at most 4096 positions)")
    tpi = gh * gw
    for name, v, hi in (("n_images", n_images, 2**31 // tpi + 1), ("n_latents", n_latents, 2**31), ("n_groups", n_groups, 65)):
        if not 1 <= v < hi:
            raise ValueError(f"{who}: unsupported {name} {v} (1 <= {name} < {hi})")
    n_rows = n_images * tpi
    if n_latents * n_groups * tpi >= 2**31:
        raise ValueError(f"{who}: n_latents * n_groups * gh * gw = {n_latents * n_groups * tpi} must stay below 2^31 (score the latents in slices)")
    if not threshold >= 0:
        raise ValueError(f"{who}: threshold {threshold} must be at least 0")
    device = _hip_device(who, indptr.device)
    stored = indices.numel()
    nnz = stored if nnz is None else int(nnz)
    if not 0 <= nnz < 2**31 or nnz > stored:
        raise ValueError(f"{who}: unsupported nnz {nnz} (0 <= nnz < 2^31, and at most the {stored} entries of indices)")
    csr = _csr_on(indptr, indices, data, n_rows, stored, device)
    if groups.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"groups must be int32 or int64, got {groups.dtype}")
    groups = _on(groups.to(torch.int32), torch.int32, (n_images,), "groups", device)
    lib = _lib.load()
    need = lib.saev_latent_spatial_workspace_bytes(n_images, tpi, n_latents, n_groups, nnz)
    if need < 0:
        raise ValueError(f"{who}: unsupported shape")
    ws = torch.empty(need, device=device, dtype=torch.uint8)
    pairs = (n_latents, n_groups)
    i64, f64 = dict(device=device, dtype=torch.int64), dict(device=device, dtype=torch.float64)
    out = dict(n_group_images=torch.empty(n_groups, **i64), n_events=torch.empty(pairs, **i64), n_images_fire=torch.empty(pairs, **i64),
               pairs_h=torch.empty(pairs, **i64), pairs_v=torch.empty(pairs, **i64), sum_m2=torch.empty(pairs, **i64),
               overlap=torch.empty(pairs, **i64), moments=torch.empty(*pairs, 5, **f64),
               count_map=torch.empty(*pairs, gh, gw, device=device, dtype=torch.int32),
               sum_map=torch.empty(*pairs, gh, gw, **f64) if sum_map else None)
    with torch.cuda.device(device):
        rc = lib.saev_latent_spatial(*map(_ptr, csr), nnz, n_rows, n_images, gh, gw, n_latents, _ptr(groups), n_groups, float(threshold),
                                     *map(_ptr, out.values()), _ptr(ws), ws.numel(), _stream())
    _lib.check(lib, None, rc, who)
    return LatentSpatialResult(out, ws, (gh, gw))


class LatentExemplarsResult(_Checked):
    """What ``latent_exemplars`` leaves on the device.  ``n_group_images`` (G) int64; ``n_fire`` (S, G) int32; (S, G, k) each:
    ``top_val`` float32, ``top_img`` and ``top_patch`` int32 -- the group's firing images by (max-pooled value descending, image
    ascending) --, ``bot_val``, ``bot_img``, ``bot_patch`` -- by (value ascending, image ascending) -- and ``silent_img`` int32, the
    first images of the group that do not fire.  Unused slots hold 0.0, -1, -1.  The call itself does not synchronise; the first read
    of a result -- or ``check()`` -- reads the device's error word (one synchronisation) and raises ValueError if it is not 0
    (include/saev_amd.h: LATENT EXEMPLARS)."""

    _WHO = "latent_exemplars"
    _ERRORS = {1: "a group id lies outside [-1, n_groups)", 2: "a column index lies outside [0, n_latents)"}
    ARRAYS = _lib.SaevLatentExemplarsOut.OUTPUTS

    def __init__(self, out: dict, ws, k: int, tokens_per_image: int):
        super().__init__(out, ws[0:4].view(torch.int32), self._ERRORS, self._WHO)
        self._ws, self.k, self.tokens_per_image = ws, k, tokens_per_image

    n_group_images = property(lambda self: self._read("n_group_images"))
    n_fire = property(lambda self: self._read("n_fire"))
    top_val = property(lambda self: self._read("top_val"))
    top_img = property(lambda self: self._read("top_img"))
    top_patch = property(lambda self: self._read("top_patch"))
    bot_val = property(lambda self: self._read("bot_val"))
    bot_img = property(lambda self: self._read("bot_img"))
    bot_patch = property(lambda self: self._read("bot_patch"))
    silent_img = property(lambda self: self._read("silent_img"))


def _exemplar_rows(who: str, n_images: int, tokens_per_image: int, n_latents: int) -> None:
    """The shape refusals ``latent_exemplars`` and ``latent_patch_rows`` share (they mirror the C entries')."""
    if not 1 <= tokens_per_image <= 4096:
        raise ValueError(f"{who}: unsupported tokens_per_image {tokens_per_image} (1 <= tokens_per_image <= 4096)")
    for name, v, hi in (("n_images", n_images, -(-2**31 // tokens_per_image)), ("n_latents", n_latents, 2**31)):
        if not 1 <= v < hi:
            raise ValueError(f"{who}: unsupported {name} {v} (1 <= {name} < {hi})")


def latent_exemplars(indptr: torch.Tensor, indices: torch.Tensor, data: torch.Tensor, *, n_images: int, tokens_per_image: int, n_latents: int,
                     groups: torch.Tensor, n_groups: int, k: int, threshold: float = 0.0, nnz: int | None = None) -> LatentExemplarsResult:
    """Which images to look at: for every latent and every group of images the ``k`` strongest firing images, the ``k`` weakest firing
    images and the first ``k`` silent ones, each firing image with its max-pooled value and the lowest patch that attains it
    (include/saev_amd.h: LATENT EXEMPLARS).  x as CSR on the device over ``n_images * tokens_per_image`` rows (indptr
    int64, indices int32, data float32; ``nnz`` as for ``latent_spatial``), row ``i * tokens_per_image + p`` being patch p of image i;
    ``groups`` (n_images) int32 / int64 in [-1, n_groups), -1 leaving the image out; an entry is an event when it is > ``threshold``
    (>= 0).  Pooled on the fly, exact and deterministic; one call, one workspace, no synchronisation; there is no CPU path."""
    who = "latent_exemplars"
    _exemplar_rows(who, n_images, tokens_per_image, n_latents)
    for name, v, hi in (("n_groups", n_groups, 65), ("k", k, 33)):
        if not 1 <= v < hi:
            raise ValueError(f"{who}: unsupported {name} {v} (1 <= {name} < {hi})")
    if n_latents * n_groups * k >= 2**31:
        raise ValueError(f"{who}: n_latents * n_groups * k = {n_latents * n_groups * k} must stay below 2^31 (score the latents in slices)")
    if not threshold >= 0:
        raise ValueError(f"{who}: threshold {threshold} must be at least 0")
    device = _hip_device(who, indptr.device)
    stored = indices.numel()
    nnz = stored if nnz is None else int(nnz)
    if not 0 <= nnz < 2**31 or nnz > stored:
        raise ValueError(f"{who}: unsupported nnz {nnz} (0 <= nnz < 2^31, and at most the {stored} entries of indices)")
    csr = _csr_on(indptr, indices, data, n_images * tokens_per_image, stored, device)
    if groups.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"groups must be int32 or int64, got {groups.dtype}")
    groups = _on(groups.to(torch.int32), torch.int32, (n_images,), "groups", device)
    lib = _lib.load()
    need = lib.saev_latent_exemplars_workspace_bytes(nnz, n_latents, n_images, n_groups)
    if need < 0:
        raise ValueError(f"{who}: unsupported shape")
    ws = torch.empty(need, device=device, dtype=torch.uint8)
    lists = (n_latents, n_groups, k)
    i32, f32 = dict(device=device, dtype=torch.int32), dict(device=device, dtype=torch.float32)
    out = dict(n_group_images=torch.empty(n_groups, device=device, dtype=torch.int64), n_fire=torch.empty(n_latents, n_groups, **i32),
               top_val=torch.empty(lists, **f32), top_img=torch.empty(lists, **i32), top_patch=torch.empty(lists, **i32),
               bot_val=torch.empty(lists, **f32), bot_img=torch.empty(lists, **i32), bot_patch=torch.empty(lists, **i32),
               silent_img=torch.empty(lists, **i32))
    struct = _lib.SaevLatentExemplarsOut(struct_size=C.sizeof(_lib.SaevLatentExemplarsOut), **{name: _ptr(t) for name, t in out.items()})
    with torch.cuda.device(device):
        rc = lib.saev_latent_exemplars(*map(_ptr, csr), nnz, _ptr(groups), n_images, tokens_per_image, n_latents, n_groups, k, float(threshold),
                                       C.byref(struct), _ptr(ws), ws.numel(), _stream())
    _lib.check(lib, None, rc, who)
    return LatentExemplarsResult(out, ws, k, tokens_per_image)


_PATCH_ROWS_ERRORS = {2: "a queried latent lies outside [0, n_latents)", 3: "a queried image lies outside [-1, n_images)"}


def latent_patch_rows(indptr: torch.Tensor, indices: torch.Tensor, data: torch.Tensor, latents: torch.Tensor, images: torch.Tensor, *,
                      n_images: int, tokens_per_image: int, n_latents: int) -> torch.Tensor:
    """The patch vectors behind chosen (latent, image) pairs: ``latents`` and ``images`` (int32 / int64, any equal shape) give
    ``(*shape, tokens_per_image)`` float32 with the STORED value of the latent in every row of the image, on the bits, and 0.0 where
    a row stores none; an image of -1 -- a padding slot of ``latent_exemplars``' lists -- gives zeros (include/saev_amd.h: LATENT
    EXEMPLARS).  x as ``latent_exemplars`` takes it.  Reads the device's error word before it returns (one synchronisation) and
    raises ValueError for a latent outside [0, n_latents) or an image outside [-1, n_images); there is no CPU path."""
    who = "latent_patch_rows"
    _exemplar_rows(who, n_images, tokens_per_image, n_latents)
    if tuple(latents.shape) != tuple(images.shape):
        raise ValueError(f"{who}: latents {tuple(latents.shape)} and images {tuple(images.shape)} must have one shape")
    for name, t in (("latents", latents), ("images", images)):
        if t.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"{name} must be int32 or int64, got {t.dtype}")
    shape, n_q = tuple(latents.shape), latents.numel()
    if n_q * tokens_per_image >= 2**31:
        raise ValueError(f"{who}: {n_q} queries of {tokens_per_image} tokens must stay below 2^31 values (gather in slices)")
    device = _hip_device(who, indptr.device)
    stored = indices.numel()
    if stored >= 2**31:
        raise ValueError(f"{who}: unsupported nnz {stored} (0 <= nnz < 2^31)")
    csr = _csr_on(indptr, indices, data, n_images * tokens_per_image, stored, device)
    q_latent = _on(latents.to(torch.int32).reshape(-1), torch.int32, (n_q,), "latents", device)
    q_image = _on(images.to(torch.int32).reshape(-1), torch.int32, (n_q,), "images", device)
    out = torch.empty(n_q, tokens_per_image, device=device, dtype=torch.float32)
    if n_q == 0:
        return out.reshape(*shape, tokens_per_image)
    err = torch.empty(1, device=device, dtype=torch.int32)
    lib = _lib.load()
    with torch.cuda.device(device):
        rc = lib.saev_latent_patch_rows(*map(_ptr, csr), stored, n_images, tokens_per_image, n_latents, _ptr(q_latent), _ptr(q_image), n_q, _ptr(out),
                                        _ptr(err), _stream())
    _lib.check(lib, None, rc, who)
    _check_err_word(err, _PATCH_ROWS_ERRORS, who)
    return out.reshape(*shape, tokens_per_image)


class PoolResult(_Checked):
    """What ``pool_images`` leaves on the device: ``pooled`` (n_images, n_latents) float32.  The call itself does not synchronise; the
    first read of ``pooled`` reads the device's error word (one synchronisation) and raises ValueError if it is not 0.  ``ranges`` is
    the number of latent ranges (workgroups per image) the launch ran, ``range_len`` the latents of one."""

    _ERRORS = {1: "a column index lies outside [0, n_latents)", 2: "a stored value is not finite", 3: "indptr is not a non-decreasing sequence of positions into indices"}

    def __init__(self, out, err, ranges, range_len):
        super().__init__(dict(pooled=out), err, self._ERRORS, "pool_images")
        self.ranges, self.range_len = ranges, range_len

    pooled = property(lambda self: self._read("pooled"))


def pool_images(indptr: torch.Tensor, indices: torch.Tensor, data: torch.Tensor, n_images: int, tokens_per_image: int, n_latents: int,
                agg: str = "max") -> PoolResult:
    """Pool a token CSR on the device (indptr (n_images * tokens_per_image + 1) int64, indices int32, data float32, as ``latent_ap``
    takes it) to one dense float32 row per image: ``PoolResult.pooled`` (n_images, n_latents) holds, per image and latent, the
    reference's ``aggregate_to_images`` value as numbers (include/saev_amd.h: SPARSE LINEAR).  ``"max"``: the largest
    of the image's ``tokens_per_image`` dense values -- a latent stored in fewer patches competes with an implicit 0, one stored in all
    of them with negative values only has a negative maximum.  ``"mean"``: the float32 sum of the stored values in patch order, then
    one float32 division by ``float32(tokens_per_image)``.  Rows must be canonical (no column twice in a row).  A column index outside
    [0, n_latents) or a non-finite value raises ValueError on the first read of ``pooled``.  There is no CPU path."""
    aggs = {"max": 0, "mean": 1}
    if agg not in aggs:
        raise ValueError(f"pool_images: agg must be 'max' or 'mean', got {agg!r}")
    for name, v in (("n_images", n_images), ("tokens_per_image", tokens_per_image), ("n_latents", n_latents)):
        if not 1 <= v < 2**31:
            raise ValueError(f"pool_images: unsupported {name} {v} (1 <= {name} < 2^31)")
    if n_images * tokens_per_image >= 2**31:
        raise ValueError(f"pool_images: unsupported n_images * tokens_per_image {n_images * tokens_per_image} (below 2^31)")
    device = _hip_device("pool_images", indptr.device)
    nnz = indices.numel()
    indptr, indices, data = _csr_on(indptr, indices, data, n_images * tokens_per_image, nnz, device)
    lib = _lib.load()
    out = torch.empty(n_images, n_latents, device=device, dtype=torch.float32)
    err = torch.empty(1, device=device, dtype=torch.int32)
    with torch.cuda.device(device):
        rc = lib.saev_pool_images(_ptr(indptr), _ptr(indices), _ptr(data), nnz, n_images, tokens_per_image, n_latents, aggs[agg], _ptr(out),
                                  _ptr(err), _stream())
    _lib.check(lib, None, rc, "saev_pool_images")
    range_len = int(lib.saev_pool_images_range())
    return PoolResult(out, err, -(-n_latents // range_len), range_len)


class PoolCsrResult(_Checked):
    """What ``pool_csr`` leaves on the device: the image-level CSR ``indptr`` (n_images + 1) int64, ``indices`` (nnz) int32 ascending
    inside every row, ``data`` (nnz) float32; with ``details=True`` also ``patch`` and ``count`` (nnz) int32, else None.  ``nnz`` is a
    host int.  The first read of an array -- or ``check()`` -- reads the device's error word (one synchronisation) and raises
    ValueError if it is not 0."""

    _ERRORS = {1: "a column index lies outside [0, n_latents)", 2: "a stored value is not finite",
               3: "indptr is not a non-decreasing sequence of positions into indices", 4: "an entry of the threshold vector is negative"}

    def __init__(self, out, err, nnz, ws):
        super().__init__(out, err, self._ERRORS, "pool_csr")
        self.nnz, self._ws = nnz, ws

    indptr = property(lambda self: self._read("indptr"))
    indices = property(lambda self: self._read("indices"))
    data = property(lambda self: self._read("data"))
    patch = property(lambda self: self._read("patch"))
    count = property(lambda self: self._read("count"))

    def triple(self):
        """(indptr, indices, data), as ``latent_auroc``, ``latent_operating``, ``latent_quantiles``, ``coactivation_match`` and
        ``latent_ap`` take them."""
        return self.indptr, self.indices, self.data


def pool_csr(indptr: torch.Tensor, indices: torch.Tensor, data: torch.Tensor, n_images: int, tokens_per_image: int, n_latents: int,
             threshold=0.0, details: bool = False) -> PoolCsrResult:
    """Pool a token CSR on the device (as ``pool_images`` takes it; unsorted rows and repeated columns are allowed) to the image-level
    CSR, without the (n_images, n_latents) matrix (include/saev_amd.h: POOL CSR).  Entry (i, l) exists iff some patch
    of image i stores a value of latent l ABOVE the latent's threshold (strict); its value is the maximum of those values.
    ``threshold`` is one finite float >= 0 or a (n_latents,) float32 vector (a device tensor, or a numpy array that is copied over)
    in the strict form ``operating.thresholds`` and ``activation_stats.thresholds`` hand out: NaN passes nothing, +Inf silences the
    latent, a negative entry raises on first read.  With threshold 0 the result is the non-zero pattern and the values of
    ``clamp_min(pool_images(..., "max").pooled, 0)``.  ``details=True`` adds ``patch`` (the lowest patch that attains the maximum)
    and ``count`` (the stored entries that pass).  The call runs the count pass, reads ``out_indptr[-1]`` once -- an 8-byte read-back,
    its only synchronisation --, allocates the arrays exactly and runs the fill pass.  Memory is that of the output and of
    ``saev_pool_csr_workspace_bytes``.  There is no CPU path."""
    who = "pool_csr"
    for name, v in (("n_images", n_images), ("tokens_per_image", tokens_per_image), ("n_latents", n_latents)):
        if not 1 <= v < 2**31:
            raise ValueError(f"{who}: unsupported {name} {v} (1 <= {name} < 2^31)")
    if n_images * tokens_per_image >= 2**31:
        raise ValueError(f"{who}: unsupported n_images * tokens_per_image {n_images * tokens_per_image} (below 2^31)")
    vector = isinstance(threshold, (torch.Tensor, np.ndarray))
    if not vector:
        threshold = float(threshold)
        if not (0.0 <= threshold < float("inf")):
            raise ValueError(f"{who}: a scalar threshold must be finite and at least 0, got {threshold}")
    elif tuple(threshold.shape) != (n_latents,) or threshold.dtype not in (torch.float32, np.float32):
        raise ValueError(f"{who}: a threshold vector must be float32 of shape ({n_latents},), got {threshold.dtype} {tuple(threshold.shape)}")
    device = _hip_device(who, indptr.device)
    nnz_in = indices.numel()
    indptr, indices, data = _csr_on(indptr, indices, data, n_images * tokens_per_image, nnz_in, device)
    thr_vec = None
    if vector:
        thr_vec = _on(torch.from_numpy(threshold).to(device) if isinstance(threshold, np.ndarray) else threshold, torch.float32, (n_latents,),
                      "threshold", device)
    lib = _lib.load()
    need = int(lib.saev_pool_csr_workspace_bytes(n_images, tokens_per_image, n_latents, nnz_in))
    if need < 0:
        raise ValueError(f"{who}: {n_images} images of {n_latents} latents are more than 2^31 (image, latent range) units: pool in slices of images")
    ws = torch.empty(need, device=device, dtype=torch.uint8)
    out_indptr = torch.empty(n_images + 1, device=device, dtype=torch.int64)
    err = torch.empty(1, device=device, dtype=torch.int32)
    shared = (_ptr(indptr), _ptr(indices), _ptr(data), nnz_in, n_images, tokens_per_image, n_latents, 0.0 if vector else threshold, _ptr(thr_vec))
    with torch.cuda.device(device):
        rc = lib.saev_pool_csr_count(*shared, _ptr(out_indptr), _ptr(ws), need, _ptr(err), _stream())
        _lib.check(lib, None, rc, "saev_pool_csr_count")
        nnz = int(out_indptr[-1].item())  # the call's one read-back
        i32 = dict(device=device, dtype=torch.int32)
        out = dict(indptr=out_indptr, indices=torch.empty(nnz, **i32), data=torch.empty(nnz, device=device, dtype=torch.float32),
                   patch=torch.empty(nnz, **i32) if details else None, count=torch.empty(nnz, **i32) if details else None)
        if nnz > 0:
            rc = lib.saev_pool_csr_fill(*shared, _ptr(out_indptr), _ptr(out["indices"]), _ptr(out["data"]), _ptr(out["patch"]), _ptr(out["count"]),
                                        _ptr(ws), need, _ptr(err), _stream())
            _lib.check(lib, None, rc, "saev_pool_csr_fill")
    return PoolCsrResult(out, err, nnz, ws)


class CoactResult(_Checked):
    """What ``coactivation_match`` leaves on the device: ``index`` (Sa, top_m) int32, per latent of A its best partners in B, best
    first, -1 where it has fewer; ``intersection`` (Sa, top_m) int32, the rows in which both fire; ``support_a`` (Sa) and
    ``support_b`` (Sb) int32, the sizes of the firing sets.  ``jaccard`` and ``containment`` (Sa, top_m) float64 are formed from those
    integers, NaN where the index is -1.  ``mutual`` (Sa) bool: a's best partner's best partner is a (for two matrices a second call
    with the roles swapped, made on first use; ``reverse`` is its result).  The call itself does not synchronise; the first read of
    a result -- or ``check()`` -- reads the device's error word (one synchronisation) and raises ValueError if it is not 0."""

    _ERRORS = {1: "a column index lies outside [0, n_latents)", 2: "a stored value is not finite", 3: "indptr is not a non-decreasing sequence of positions into indices"}

    def __init__(self, out, err, ws, measure, top_m, swapped):
        super().__init__(out, err, self._ERRORS, "coactivation_match")
        self.measure, self.top_m, self._ws, self._swapped, self._reverse = measure, top_m, ws, swapped, None

    index = property(lambda self: self._read("index"))
    intersection = property(lambda self: self._read("intersection"))
    support_a = property(lambda self: self._read("support_a"))
    support_b = property(lambda self: self._read("support_b"))

    def _partner_support(self):
        return self.support_b.to(torch.int64)[self.index.clamp_min(0).to(torch.int64)]

    @property
    def jaccard(self) -> torch.Tensor:
        inter = self.intersection.to(torch.int64)
        union = self.support_a.to(torch.int64)[:, None] + self._partner_support() - inter
        return torch.where(self.index >= 0, inter.double() / union.double(), torch.nan)

    @property
    def containment(self) -> torch.Tensor:
        inter = self.intersection.to(torch.int64)
        return torch.where(self.index >= 0, inter.double() / self.support_a.to(torch.int64)[:, None].double(), torch.nan)

    @property
    def reverse(self) -> "CoactResult":
        """B's latents matched against A's (the same measure, top_m = 1); of a self match the result itself."""
        if self._reverse is None:
            self._reverse = self if self._swapped is None else self._swapped()
        return self._reverse

    @property
    def mutual(self) -> torch.Tensor:
        best = self.index[:, 0].to(torch.int64)
        back = self.reverse.index[:, 0].to(torch.int64)
        own = torch.arange(best.numel(), device=best.device)
        return (best >= 0) & (back[best.clamp_min(0)] == own)


_COACT_MEASURES = {"jaccard": 0, "containment": 1}


def coactivation_match(A, B=None, *, n_rows: int, n_latents_a: int, n_latents_b: int | None = None, thr_a: float = 0.0, thr_b: float = 0.0,
                       measure: str = "jaccard", top_m: int = 1) -> CoactResult:
    """For every latent of A the ``top_m`` latents of B whose firing sets overlap its own most, on the HIP kernels of
    saev_coactivation (include/saev_amd.h: COACTIVATION): no Sa x Sb matrix, nothing read back.  A and B are CSR
    triples (indptr, indices, data) on one HIP device over the same ``n_rows`` rows (indptr int64, indices int32, data float32, rows
    canonical); an entry fires when its value is > the threshold.  ``B=None`` matches A against itself with the pair b == a
    excluded.  ``measure``: "jaccard" (I / (n_a + n_b - I)) or "containment" (I / n_a); the ranking is on integers (ties: the
    lower index for Jaccard; the smaller support, then the lower index for containment).  There is no CPU path."""
    if measure not in _COACT_MEASURES:
        raise ValueError(f"coactivation_match: measure must be one of {sorted(_COACT_MEASURES)}, got {measure!r}")
    if not 1 <= top_m <= 8:
        raise ValueError(f"coactivation_match: unsupported top_m {top_m} (1 <= top_m <= 8)")
    if B is None:
        if n_latents_b not in (None, n_latents_a):
            raise ValueError(f"coactivation_match: n_latents_b {n_latents_b} without B (a self match has n_latents_a = {n_latents_a} partners)")
        n_latents_b = n_latents_a
    elif n_latents_b is None:
        raise ValueError("coactivation_match: n_latents_b comes with B")
    for name, v in (("n_rows", n_rows), ("n_latents_a", n_latents_a), ("n_latents_b", n_latents_b)):
        if not 1 <= v < 2**31:
            raise ValueError(f"coactivation_match: unsupported {name} {v} (1 <= {name} < 2^31)")
    if not (math.isfinite(thr_a) and math.isfinite(thr_b)):
        raise ValueError(f"coactivation_match: thresholds must be finite, got {thr_a} and {thr_b}")
    device = _hip_device("coactivation_match", A[0].device)
    A = _csr_on(*A, n_rows, A[1].numel(), device)
    B = None if B is None else _csr_on(*B, n_rows, B[1].numel(), device)
    return _coactivation(A, B, n_rows, n_latents_a, n_latents_b, float(thr_a), float(thr_b), measure, top_m, device)


def _coactivation(A, B, n_rows, Sa, Sb, thr_a, thr_b, measure, top_m, device) -> CoactResult:
    lib = _lib.load()
    nnz_a = A[1].numel()
    nnz_b = nnz_a if B is None else B[1].numel()
    nbytes = int(lib.saev_coactivation_workspace_bytes(n_rows, Sa, Sb, nnz_a, nnz_b))
    if nbytes < 0:
        raise ValueError(f"coactivation_match: unsupported sizes {(n_rows, Sa, Sb, nnz_a, nnz_b)} (all below 2^31)")
    i32 = dict(device=device, dtype=torch.int32)
    ws = torch.empty(nbytes, device=device, dtype=torch.uint8)
    support_a = torch.empty(Sa, **i32)
    out = dict(index=torch.empty(Sa, top_m, **i32), intersection=torch.empty(Sa, top_m, **i32), support_a=support_a,
               support_b=support_a if B is None else torch.empty(Sb, **i32))
    err = torch.empty(1, **i32)
    none3 = (None, None, None)
    with torch.cuda.device(device):
        rc = lib.saev_coactivation(*map(_ptr, A), nnz_a, Sa, *(none3 if B is None else map(_ptr, B)), nnz_b, Sb, n_rows, thr_a, thr_b,
                                   _COACT_MEASURES[measure], top_m, _ptr(support_a), None if B is None else _ptr(out["support_b"]),
                                   _ptr(out["index"]), _ptr(out["intersection"]), _ptr(err), _ptr(ws), nbytes, _stream())
    _lib.check(lib, None, rc, "saev_coactivation")
    swapped = None if B is None else (lambda: _coactivation(B, A, n_rows, Sb, Sa, thr_b, thr_a, measure, 1, device))
    return CoactResult(out, err, ws, measure, top_m, swapped)


@dataclasses.dataclass
class L1LogisticResult:
    """A fit of ``l1_logistic``: ``coef_`` (1, S) for two classes and (K, S) otherwise and ``intercept_`` (float64, on the device; the
    intercepts of K >= 3 have mean zero), ``classes_`` (the sorted unique values of y), the iterations run, the KKT residual and the
    objective F = C * sum loss + ||W||_1 of the returned point, whether the residual reached ``kkt_tol``, and the step bound L the
    backtracking ended at."""

    coef_: torch.Tensor
    intercept_: torch.Tensor
    classes_: torch.Tensor
    n_iter_: int
    kkt_residual_: float
    objective_: float
    converged_: bool
    lipschitz_: float
    n_rejected_: int = 0
    n_restarts_: int = 0
    layout: object = None


def l1_logistic(X: torch.Tensor, y: torch.Tensor, C: float, *, kkt_tol: float = 1e-4, max_iter: int = 5000, check_every: int = 25) -> L1LogisticResult:
    """L1-penalised logistic regression on the device, scikit-learn's ``LogisticRegression(penalty="l1", C=C)`` problem solved to a
    certified optimum (include/saev_amd.h: SPARSE LINEAR): minimise ``C * sum_i loss_i + ||W||_1`` with an unpenalised
    intercept.  ``X`` (n, S) float32 on the device, ``y`` (n) int32 / int64 class ids; ``classes_ = unique(y)``.  Two classes give a
    binary logistic loss with one coefficient row (positive class ``classes_[1]``), three or more a softmax with one row per class.
    FISTA in fp64 with backtracking and restart; it stops when the KKT residual (the largest of ``|g + sign(w)|`` where ``w != 0``,
    ``max(|g| - 1, 0)`` where ``w == 0`` and ``|g_b|``, g the gradient of the C-scaled loss) is ``<= kkt_tol``.  The host reads the
    device's state block once per ``check_every`` iterations; the result does not depend on it.  Running out of ``max_iter`` returns
    the last iterate with ``converged_ = False`` and a warning.  One class, more than 64, ``C <= 0`` and a non-finite X raise
    ValueError.  There is no CPU path."""
    import warnings

    if X.dim() != 2 or y.dim() != 1 or X.shape[0] != y.shape[0] or X.shape[0] < 1 or X.shape[1] < 1:
        raise ValueError(f"l1_logistic: X must be (n, S) and y (n) with n, S >= 1, got {tuple(X.shape)} and {tuple(y.shape)}")
    if X.dtype != torch.float32 or y.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"l1_logistic: X must be float32 and y int32 or int64, got {X.dtype} and {y.dtype}")
    if not (C > 0 and math.isfinite(C)):
        raise ValueError(f"l1_logistic: C must be positive and finite, got {C}")
    if not kkt_tol >= 0 or max_iter < 0 or check_every < 1:
        raise ValueError(f"l1_logistic: kkt_tol >= 0, max_iter >= 0 and check_every >= 1, got {kkt_tol}, {max_iter}, {check_every}")
    device = X.device
    if device.type != "cuda" or y.device != device:
        raise RuntimeError("l1_logistic runs on a HIP device only (there is no CPU path)")
    n, s = X.shape
    classes, inverse = torch.unique(y, return_inverse=True)
    k = int(classes.numel())
    if k < 2:
        raise ValueError(f"This solver needs samples of at least 2 classes in the data, but the data contains only one class: {classes.tolist()[0]!r}")
    if k > 64:
        raise ValueError(f"l1_logistic: unsupported number of classes {k} (at most 64)")
    X = X.contiguous()
    yi = inverse.to(torch.int32).contiguous()
    lib = _lib.load()
    layout = _lib.SaevL1LogisticLayout()
    _lib.check(lib, None, lib.saev_l1_logistic_layout_of(n, s, k, _lib.C.byref(layout)), "saev_l1_logistic_layout_of")
    ws = torch.empty(layout.total_bytes, device=device, dtype=torch.uint8)
    common = (_ptr(X), _ptr(yi), n, s, k, float(C), float(kkt_tol))
    state = ws[layout.off_state:layout.off_state + 128].view(torch.float64)
    with torch.cuda.device(device):
        _lib.check(lib, None, lib.saev_l1_logistic_init(*common, _ptr(ws), ws.numel(), _stream()), "saev_l1_logistic_init")
        _check_err_word(ws[layout.off_err:layout.off_err + 4].view(torch.int32),
                        {1: "X holds a value that is not finite", 2: "a class index lies outside [0, K)"}, "l1_logistic")
        left = max_iter
        while left > 0:
            step = min(check_every, left)
            _lib.check(lib, None, lib.saev_l1_logistic_iterate(*common, step, _ptr(ws), ws.numel(), _stream()), "saev_l1_logistic_iterate")
            left -= step
            if state[8].item() != 0.0:  # SAEV_L1_STATE_DONE
                break
        coef = torch.empty(layout.coef_rows, s, device=device, dtype=torch.float64)
        intercept = torch.empty(layout.coef_rows, device=device, dtype=torch.float64)
        scalars = torch.empty(8, device=device, dtype=torch.float64)
        _lib.check(lib, None, lib.saev_l1_logistic_result(*common, _ptr(coef), _ptr(intercept), _ptr(scalars), _ptr(ws), ws.numel(), _stream()),
                   "saev_l1_logistic_result")
        sc = scalars.cpu().tolist()
    res = L1LogisticResult(coef, intercept, classes, int(sc[0]), float(sc[1]), float(sc[2]), bool(sc[3]), float(sc[4]), int(sc[5]), int(sc[6]), layout)
    if not res.converged_:
        warnings.warn(f"l1_logistic: the KKT residual is {res.kkt_residual_:.3g} after {res.n_iter_} iterations (kkt_tol {kkt_tol:g}): not converged",
                      RuntimeWarning, stacklevel=2)
    return res


def _row_bytes(who: str, name: str, t, n: int, device):
    """A per-row bool / uint8 vector as the C entries take it (None passes through)."""
    if t is None:
        return None
    if t.dtype == torch.bool:
        t = t.view(torch.uint8)
    if t.dtype != torch.uint8 or tuple(t.shape) != (n,) or t.device != device:
        raise ValueError(f"{who}: {name} must be a bool / uint8 vector of {n} rows on {device}")
    return t.contiguous()


def _padded_codes(who: str, idx, val, row_nnz, n: int, device):
    if idx.ndim != 2 or idx.shape[0] != n:
        raise ValueError(f"{who}: idx must be ({n}, cap), got {tuple(idx.shape)}")
    cap = idx.shape[1]
    return (_on(idx, torch.int32, (n, cap), "idx", device), _on(val, torch.float32, (n, cap), "val", device),
            _on(row_nnz, torch.int32, (n,), "row_nnz", device), cap)


def edit_records(edits) -> "C.Array":
    """``(latent, op, value, group)`` tuples as the saev_edit array of include/saev_amd.h (no device needed)."""
    arr = (_lib.SaevEdit * max(len(edits), 1))()
    for i, (latent, op, value, group) in enumerate(edits):
        arr[i] = _lib.SaevEdit(int(latent), int(op), float(value), int(group))
    return arr


def build_edit_plan(edits, d_sae: int, n_groups: int, device) -> torch.Tensor:
    """The device plan of ``saev_edit_plan_build`` for ``(latent, op, value, group)`` tuples (include/saev_amd.h: LATENT EDITS): the
    edits validated on the host -- ValueError with the library's message for an edit it refuses -- and regrouped on the device.
    One synchronisation; the plan serves every later ``intervene_rows`` call."""
    device = _hip_device("build_edit_plan", device)
    lib = _lib.load()
    need = int(lib.saev_edit_plan_bytes(len(edits), n_groups))
    if need < 0:
        raise ValueError(f"build_edit_plan: at most 65536 edits and 65536 groups, got {len(edits)} and {n_groups}")
    plan = torch.empty(need, device=device, dtype=torch.uint8)
    with torch.cuda.device(device):
        rc = lib.saev_edit_plan_build(edit_records(edits), len(edits), n_groups, d_sae, _ptr(plan), need, _stream())
    if rc in (-1, -3):
        raise ValueError((lib.saev_last_error(None) or b"saev_edit_plan_build refused the edits").decode())
    _lib.check(lib, None, rc, "saev_edit_plan_build")
    return plan


def intervene_rows(x: torch.Tensor, W_dec: torch.Tensor, idx: torch.Tensor, val: torch.Tensor, row_nnz: torch.Tensor | None,
                   plan: torch.Tensor, n_edits: int, n_groups: int, *, row_group: torch.Tensor | None = None,
                   row_keep: torch.Tensor | None = None, out: torch.Tensor | None = None,
                   rows_changed: torch.Tensor | None = None) -> torch.Tensor:
    """x' = x + sum_e (t_e(f_l) - f_l) W_dec[l_e, :] for the edits of ``plan`` (``build_edit_plan``) on padded code rows
    (include/saev_amd.h: LATENT EDITS).  x (n, D) float32, W_dec (S, D) float32, idx / val (n, cap), row_nnz (n)
    int32 or None (full rows), row_group (n) int32, row_keep (n) bool, rows_changed (n_edits) int64 (added to).  ``out`` may be
    ``x`` (in place); it is allocated when None.  Rows no edit touches come back bit for bit.  There is no CPU path."""
    who = "intervene_rows"
    device = _hip_device(who, x.device)
    if x.ndim != 2 or W_dec.ndim != 2 or x.shape[1] != W_dec.shape[1]:
        raise ValueError(f"{who}: x must be (n, D) and W_dec (S, D), got {tuple(x.shape)} and {tuple(W_dec.shape)}")
    n, D = x.shape
    S = W_dec.shape[0]
    if out is None:
        x = _on(x, torch.float32, (n, D), "x", device)
        out = torch.empty_like(x)
    elif out.dtype != torch.float32 or tuple(out.shape) != (n, D) or out.device != device or not out.is_contiguous():
        raise ValueError(f"{who}: out must be a contiguous float32 ({n}, {D}) tensor on {device}")
    elif not (x.dtype == torch.float32 and x.device == device and x.is_contiguous()):
        raise ValueError(f"{who}: with out given, x must be a contiguous float32 tensor on {device}")
    W_dec = _on(W_dec.detach(), torch.float32, (S, D), "W_dec", device)
    idx, val, row_nnz, cap = _padded_codes(who, idx, val, row_nnz, n, device)
    row_group = _on(row_group, torch.int32, (n,), "row_group", device)
    row_keep = _row_bytes(who, "row_keep", row_keep, n, device)
    if rows_changed is not None and (rows_changed.dtype != torch.int64 or tuple(rows_changed.shape) != (n_edits,) or rows_changed.device != device
                                     or not rows_changed.is_contiguous()):
        raise ValueError(f"{who}: rows_changed must be a contiguous int64 vector of {n_edits} edits on {device}")
    lib = _lib.load()
    with torch.cuda.device(device):
        rc = lib.saev_intervene_rows(_ptr(x), n, D, _ptr(W_dec), S, _ptr(idx), _ptr(val), _ptr(row_nnz), cap, _ptr(plan), n_edits, n_groups,
                                     _ptr(row_group), _ptr(row_keep), _ptr(out), _ptr(rows_changed), _stream())
    _lib.check(lib, None, rc, "saev_intervene_rows")
    return out


class ClassFireCounts:
    """Class-conditional firing counts of every latent over a stream of batches (include/saev_amd.h: CLASS FIRING COUNTS; the
    reference's semseg ``get_latent_lookup``): ``hist`` (C, T, S) / ``pos`` (T, S) uint32 as int32 tensors, ``n_rows_c`` (C) int64.
    ``add`` takes padded code rows and their labels, ``f1`` forms the best F1 over the thresholds, ``lookup`` the top latents of
    every class.  Nothing is read back before ``lookup``."""

    def __init__(self, d_sae: int, n_classes: int, device, thresholds=(0.0, 0.1, 0.3, 1.0)):
        self.device = _hip_device("ClassFireCounts", device)
        self.lib = _lib.load()
        self.d_sae, self.n_classes, self.thresholds = d_sae, n_classes, tuple(float(t) for t in thresholds)
        T = len(self.thresholds)
        if not 1 <= T <= 8:
            raise ValueError(f"ClassFireCounts: 1 to 8 thresholds, got {T}")
        if d_sae < 1 or n_classes < 1 or n_classes * T * d_sae >= 2**31:
            raise ValueError(f"ClassFireCounts: unsupported shape (n_classes * thresholds * d_sae = {n_classes * T * d_sae} must stay below 2^31)")
        self._thr = (C.c_float * T)(*self.thresholds)
        self.hist = torch.zeros(n_classes, T, d_sae, device=self.device, dtype=torch.int32)
        self.pos = torch.zeros(T, d_sae, device=self.device, dtype=torch.int32)
        self.n_rows_c = torch.zeros(n_classes, device=self.device, dtype=torch.int64)

    def zero_(self) -> "ClassFireCounts":
        for t in (self.hist, self.pos, self.n_rows_c):
            t.zero_()
        return self

    def add(self, idx: torch.Tensor, val: torch.Tensor, row_nnz: torch.Tensor | None, labels: torch.Tensor,
            keep: torch.Tensor | None = None) -> None:
        """One batch: idx (n, cap) int32, val (n, cap) float32, row_nnz (n) int32 or None (full rows), labels (n) integer class ids
        (a label outside [0, n_classes) drops the row), keep (n) bool."""
        n = idx.shape[0]
        idx, val, row_nnz, cap = _padded_codes("ClassFireCounts.add", idx, val, row_nnz, n, self.device)
        labels = _on(labels.to(torch.int32), torch.int32, (n,), "labels", self.device)
        keep = _row_bytes("ClassFireCounts.add", "keep", keep, n, self.device)
        with torch.cuda.device(self.device):
            rc = self.lib.saev_class_fire_counts(_ptr(idx), _ptr(val), _ptr(row_nnz), cap, n, _ptr(labels), _ptr(keep), self.d_sae,
                                                 self.n_classes, self._thr, len(self.thresholds), _ptr(self.hist), _ptr(self.pos),
                                                 _ptr(self.n_rows_c), _stream())
        _lib.check(self.lib, None, rc, "saev_class_fire_counts")

    def f1(self, latent_mask: torch.Tensor | None = None) -> tuple[torch.Tensor, torch.Tensor]:
        """``(f1, best_t)``, (C, S) float32 / uint8 on the device: the best F1 over the thresholds and the index of the (lowest)
        threshold that gives it; a latent whose ``latent_mask`` (S bool) is False gets -1."""
        latent_mask = _row_bytes("ClassFireCounts.f1", "latent_mask", latent_mask, self.d_sae, self.device)
        f1 = torch.empty(self.n_classes, self.d_sae, device=self.device, dtype=torch.float32)
        best_t = torch.empty(self.n_classes, self.d_sae, device=self.device, dtype=torch.uint8)
        with torch.cuda.device(self.device):
            rc = self.lib.saev_class_fire_f1(_ptr(self.hist), _ptr(self.pos), _ptr(self.n_rows_c), self.d_sae, self.n_classes,
                                             len(self.thresholds), _ptr(latent_mask), _ptr(f1), _ptr(best_t), _stream())
        _lib.check(self.lib, None, rc, "saev_class_fire_f1")
        return f1, best_t

    def lookup(self, top_k: int = 3, latent_mask: torch.Tensor | None = None):
        """``(latents, scores, thresholds)``, CPU tensors of shape (C, top_k): every class's best latents by F1, best first, and
        the threshold each score was reached at."""
        f1, best_t = self.f1(latent_mask)
        scores, latents = torch.topk(f1, k=min(top_k, self.d_sae), dim=1)
        thr = torch.tensor(self.thresholds, dtype=torch.float32)[best_t.gather(1, latents).long().cpu()]
        return latents.cpu(), scores.cpu(), thr


@dataclasses.dataclass
class StepStats:
    mse: float
    aux: float
    l0: float
    l1: float
    grad_norm: float
    upper: float
    n_dead: int
    n_overflow_rows: int
    cand_max: int
    dense_route: int
    sse: float
    sum_sq: float

    @property
    def loss(self) -> float:
        return self.mse + self.aux


def flat_layout(cfg: EngineConfig) -> "_lib.SaevLayout":
    """Offsets of the four tensors in the flat buffers, their length and the per-rank chunk lengths (saev_layout)."""
    lay = _lib.SaevLayout()
    ccfg = _lib.SaevCfg(d_model=cfg.d_model, d_sae=cfg.d_sae, shard_world=cfg.shard_world)
    rc = _lib.load().saev_layout(C.byref(ccfg), C.byref(lay))
    if rc != 0:
        raise _lib.SaevError(f"saev_layout failed with status {rc} for {cfg}")
    return lay


def _ptr(t: torch.Tensor | None):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class SaeEngine:
    def __init__(self, cfg: EngineConfig, device: torch.device | str | int = "cuda", *, with_optim: bool = True):
        if not torch.cuda.is_available():
            raise _lib.SaevError("saev_amd needs a HIP device (torch.cuda.is_available() is False); there is no CPU path")
        self.lib = _lib.load()
        self.cfg = cfg
        self.device = torch.device(device if not isinstance(device, int) else f"cuda:{device}")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        S, D = cfg.d_sae, cfg.d_model
        lay = flat_layout(cfg)
        self.n_params = lay.n_total  # floats per flat buffer (zero padding included when shard_world > 1)
        self.shard_world = cfg.shard_world
        self.chunk_a, self.chunk_b = lay.chunk_a, lay.chunk_b
        self.offsets = {"W_dec": lay.off_W_dec, "b_dec": lay.off_b_dec, "W_enc": lay.off_W_enc, "b_enc": lay.off_b_enc}
        self.shapes = {"W_dec": (S, D), "b_dec": (D,), "W_enc": (D, S), "b_enc": (S,)}
        if cfg.bounds not in ("guaranteed", "predicted", "norm"):
            raise ValueError(f"EngineConfig.bounds (SAEV_AMD_BOUNDS) must be 'guaranteed', 'predicted' or 'norm', got {cfg.bounds!r}")
        if cfg.encoder not in ("f32", "f16x3", "bf16", "f16r"):
            raise ValueError(f"EngineConfig.encoder (SAEV_AMD_ENCODER) must be one of f32, f16x3, bf16, f16r, got {cfg.encoder!r}")
        if cfg.activation not in ("topk", "relu", "batch_topk", "relu_train"):
            raise ValueError(f"EngineConfig.activation must be 'topk', 'relu', 'batch_topk' or 'relu_train', got {cfg.activation!r}")
        if cfg.activation == "relu_train" and cfg.encoder == "bf16":
            raise NotImplementedError("the bf16 encoder is not available for ReLU SAEs: use f32, f16x3 or f16r")
        if cfg.activation == "relu_train" and (cfg.shard_world > 1 or cfg.max_backward_rows > cfg.max_batch):
            raise NotImplementedError("a ReLU training engine runs on one GPU (world > 1 is not on this path)")
        if cfg.activation == "relu_train" and not (cfg.l1_coeff >= 0.0 and math.isfinite(cfg.l1_coeff)):
            raise ValueError(f"EngineConfig.l1_coeff must be a finite number >= 0, got {cfg.l1_coeff!r}")
        if cfg.activation == "batch_topk" and cfg.encoder == "bf16":
            raise NotImplementedError("the bf16 encoder is not available for BatchTopK SAEs: use f32, f16x3 or f16r")
        if cfg.activation == "batch_topk" and (cfg.shard_world > 1 or cfg.max_backward_rows > cfg.max_batch):
            raise NotImplementedError("a BatchTopK engine runs on one GPU (a batch-wide top-k over ranks needs a distributed select)")
        if cfg.activation in ("relu", "relu_train") and cfg.k_aux != 0:
            raise ValueError("a ReLU engine has no auxiliary loss: k_aux must be 0")
        with torch.cuda.device(self.device):
            self.params = torch.zeros(self.n_params, device=self.device, dtype=torch.float32)
            self.grads = torch.zeros_like(self.params) if with_optim else None
            self.adam_m = torch.zeros_like(self.params) if with_optim else None
            self.adam_v = torch.zeros_like(self.params) if with_optim else None
            self.toks_since_active = torch.zeros(S, device=self.device, dtype=torch.int64)
            self.fired = torch.zeros(S, device=self.device, dtype=torch.int32)
            if cfg.dw_route not in ("slices", "rows", "slices_a") or cfg.fwd_route not in ("default", "rows"):
                raise ValueError(f"EngineConfig.dw_route must be 'slices', 'slices_a' or 'rows' and fwd_route 'default' or 'rows', got {cfg.dw_route!r} / {cfg.fwd_route!r}")
            # the tail's sum of squares lives in a torch tensor from the start, so that a collective can reach it
            self.sumsq = torch.zeros(1, device=self.device, dtype=torch.float64)
            # BatchTopK: the inference threshold (the module's registered buffer aliases this word) and the rows' capacity
            self.threshold = torch.zeros((), device=self.device, dtype=torch.float32) if cfg.activation == "batch_topk" else None
            self.row_cap = 0
            self.row_regrows = 0  # forwards that met a row longer than row_cap and rebuilt the context
            self._w_enc_t = None
            self._prefixes = None
            self.ctx = None
            self._create_ctx()
            self._params_version = self._pversion()
        self.adam_steps = 0
        self._x_keepalive = None
        self._last_n = 0  # rows of the last step_forward (0: none, or a fused step ran since)
        # ReLU rows: capacity of the next encode_relu (grows to the largest count seen) and how many calls needed a second launch
        self.relu_row_cap = min(cfg.d_sae, 512)
        self.relu_second_launches = 0

    # ---- plumbing -------------------------------------------------------------------------
    def _create_ctx(self) -> None:
        """The C-ABI context for ``self.cfg``, bound to this engine's tensors.  Everything a context carries from step to step that
        matters to results -- parameters, gradients, moments, tracker, threshold -- lives in those tensors, so a context can be
        replaced (``_grow_rows``) without losing any of it."""
        cfg, S, D = self.cfg, self.cfg.d_sae, self.cfg.d_model
        ccfg = _lib.SaevCfg(
            d_model=D, d_sae=S, top_k=cfg.top_k, k_aux=cfg.k_aux, alpha=cfg.alpha,
            dead_threshold_tokens=cfg.dead_threshold_tokens,
            normalize_w_dec=int(cfg.normalize_w_dec), remove_parallel_grads=int(cfg.remove_parallel_grads),
            max_batch=cfg.max_batch, encoder_mode={"f32": 0, "f16x3": 1, "bf16": 2, "f16r": 3}[cfg.encoder],
            aux_dead_cap=cfg.aux_dead_cap, shard_world=cfg.shard_world,
            bound_mode={"guaranteed": 0, "predicted": 1, "norm": 2}[cfg.bounds], max_backward_rows=cfg.max_backward_rows,
            activation={"topk": _lib.ACT_TOPK, "relu": _lib.ACT_RELU, "batch_topk": _lib.ACT_BATCHTOPK, "relu_train": _lib.ACT_RELU}[cfg.activation],
        )
        dbg = _lib.SaevDebugCfg(
            struct_size=C.sizeof(_lib.SaevDebugCfg), dw_route={"slices": 0, "rows": 1, "slices_a": 2}[cfg.dw_route],
            aux_small_max=cfg.aux_small_max, fwd_route={"default": 0, "rows": 1}[cfg.fwd_route],
            csc_route=cfg.csc_route, fin_route=cfg.fin_route, prep_route=cfg.prep_route, aux_dense_route=cfg.aux_dense_route, aux_small_route=cfg.aux_small_route,
            group_route=cfg.group_route, aux_split_route=cfg.aux_split_route, aux_wide_route=cfg.aux_wide_route)
        ctx = C.c_void_p()
        if cfg.activation == "batch_topk":
            bt = _lib.SaevBatchTopKCfg(struct_size=C.sizeof(_lib.SaevBatchTopKCfg), row_cap=cfg.row_cap, batch_momentum=cfg.batch_momentum,
                                       list_cap=cfg.select_list_cap)
            rc = self.lib.saev_create_batch_topk(C.byref(ccfg), C.byref(dbg), C.byref(bt), self.device.index, C.byref(ctx))
        elif cfg.activation == "relu_train":
            rt = _lib.SaevReluTrainCfg(struct_size=C.sizeof(_lib.SaevReluTrainCfg), l1_coeff=float(cfg.l1_coeff))
            rc = self.lib.saev_create_relu_train(C.byref(ccfg), C.byref(dbg), C.byref(rt), self.device.index, C.byref(ctx))
        else:
            rc = self.lib.saev_create_ex(C.byref(ccfg), C.byref(dbg), self.device.index, C.byref(ctx))
        if rc != 0:
            raise _lib.SaevError(f"saev_create failed with status {rc} for {cfg}")
        self.ctx = ctx
        self._chk(self.lib.saev_bind(ctx, _ptr(self.params), _ptr(self.grads), _ptr(self.adam_m), _ptr(self.adam_v)), "saev_bind")
        self._chk(self.lib.saev_bind_tracker(ctx, _ptr(self.toks_since_active), _ptr(self.fired)), "saev_bind_tracker")
        self._chk(self.lib.saev_bind_sumsq(ctx, _ptr(self.sumsq)), "saev_bind_sumsq")
        if self._w_enc_t is not None:
            self._chk(self.lib.saev_bind_w_enc_t(ctx, _ptr(self._w_enc_t)), "saev_bind_w_enc_t")
        if self.threshold is not None:
            self._chk(self.lib.saev_bind_threshold(ctx, _ptr(self.threshold)), "saev_bind_threshold")
            self.row_cap = int(self.lib.saev_row_cap(ctx))
        if self._prefixes is not None:
            self.set_prefixes(self._prefixes)

    def _grow_rows(self, need: int) -> None:
        """BatchTopK: a forward met a row of ``need`` codes, more than the context's rows hold.  A context with row_cap = need
        rounded up to 64 takes its place; parameters, moments, tracker, threshold and adam_steps are this engine's tensors and
        attributes and carry over as they are (the tracker as after ``set_tracker``: the new context reads the dead count back
        for its first steps)."""
        if need <= self.row_cap:
            raise _lib.SaevError(f"BatchTopK row overflow reported {need} codes for rows of {self.row_cap}")
        torch.cuda.synchronize(self.device)
        self.lib.saev_destroy(self.ctx)
        self.ctx = None
        self.cfg = dataclasses.replace(self.cfg, row_cap=min(self.cfg.d_sae, (need + 63) // 64 * 64))
        with torch.cuda.device(self.device):
            self._create_ctx()
        self.row_regrows += 1
        self._last_n = 0

    def _chk(self, rc, what):
        _lib.check(self.lib, self.ctx, rc, what)

    def _topk_only(self, what: str):
        if self.cfg.activation == "batch_topk":
            raise NotImplementedError(f"{what} is not available for a BatchTopK SAE (one GPU, the phases or train_step, encode_batch_topk)")
        if self.cfg.activation == "relu_train":
            raise NotImplementedError(f"{what} is not available for a ReLU training engine (one GPU, the phases in one piece or train_step, "
                                      "encode_relu)")
        if self.cfg.activation != "topk":
            raise NotImplementedError(f"{what}: training and the TopK forward are not on the HIP path for a {self.cfg.activation} SAE "
                                      "(only its forward is: encode_relu / decode_rows)")

    def _trains(self, what: str):
        """TopK, BatchTopK and ReLU training engines run the step entries; a ReLU engine its forward only."""
        if self.cfg.activation == "relu":
            self._topk_only(what)

    def close(self):
        if getattr(self, "ctx", None):
            if getattr(self, "_leader", None) is not None and getattr(self._leader, "ctx", None):
                self.lib.saev_share_x(self.ctx, None)
            self.lib.saev_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def view(self, name: str, flat: torch.Tensor | None = None) -> torch.Tensor:
        flat = self.params if flat is None else flat
        off, shape = self.offsets[name], self.shapes[name]
        return flat[off : off + math.prod(shape)].view(shape)

    def param_views(self) -> dict[str, torch.Tensor]:
        return {k: self.view(k) for k in self.offsets}

    def grad_views(self) -> dict[str, torch.Tensor]:
        return {k: self.view(k, self.grads) for k in self.offsets}

    def set_tracker(self, toks: torch.Tensor | None) -> None:
        """Overwrite the dead-latent tracker (``None`` zeroes it) and tell the context it changed."""
        if toks is None:
            self.toks_since_active.zero_()
        else:
            self.toks_since_active.copy_(toks.to(self.device, torch.int64))
        self._chk(self.lib.saev_tracker_touched(self.ctx), "saev_tracker_touched")

    def set_prefixes(self, prefixes) -> None:
        """Matryoshka cut points for the following steps (ascending, last == d_sae); None / one entry = plain."""
        if self.cfg.activation == "relu_train" and prefixes is not None and len(list(prefixes)) > 1:
            raise NotImplementedError("set_prefixes: the dense ReLU step implements the plain objective only (n_prefixes = 1)")
        if prefixes is None:
            self._n_prefixes = 1
            self._prefixes = None
            self._chk(self.lib.saev_set_prefixes(self.ctx, None, 0), "saev_set_prefixes")
            return
        pre = [int(p) for p in prefixes]
        self._prefixes = pre
        self._n_prefixes = max(1, len(pre))
        arr = (C.c_int64 * len(pre))(*pre)
        self._chk(self.lib.saev_set_prefixes(self.ctx, arr, len(pre)), "saev_set_prefixes")

    def share_x(self, leader: "SaeEngine | None") -> None:
        """Borrow what a step derives from x alone (statistics, centring, operand images) from ``leader`` whenever it has
        just run its forward on the same batch tensor: several SAEs on the same batches (train()'s parallel groups)."""
        if leader is not None and "batch_topk" in (self.cfg.activation, leader.cfg.activation):
            raise NotImplementedError("share_x: a BatchTopK engine neither lends nor borrows what a step derives from x")
        if leader is not None and "relu_train" in (self.cfg.activation, leader.cfg.activation):
            raise NotImplementedError("share_x: a ReLU training engine neither lends nor borrows what a step derives from x")
        self._leader = leader  # keeps it alive for as long as the link exists
        self._chk(self.lib.saev_share_x(self.ctx, leader.ctx if leader is not None else None), "saev_share_x")

    def load_params(self, params: dict[str, torch.Tensor]) -> None:
        for k in self.offsets:
            self.view(k).copy_(params[k].to(self.device, torch.float32))
        self.params_touched()

    def params_touched(self) -> None:
        """Tell the context that the parameter buffer was written from outside the library (include/saev_amd.h: PARAMETER
        OWNERSHIP): it drops what it keeps of W_enc / W_dec between calls.  In-place torch operations on ``params`` or on views of
        it are noticed by themselves (torch's version counter, checked before every forward); writes that bypass it -- ``.data``,
        raw pointers, another library -- need this call."""
        self._chk(self.lib.saev_params_touched(self.ctx), "saev_params_touched")
        self._params_version = self._pversion()

    def _pversion(self):
        try:
            return self.params._version
        except RuntimeError:  # a buffer created under torch.inference_mode() has no version counter: nothing to go by
            return None

    def watch(self, tensors) -> None:
        """Tensors that alias the parameter buffer but carry version counters of their own -- the four Parameters of a
        ``SparseAutoencoder`` bound to this engine (``p.data = view`` keeps the Parameter's counter).  Every entry point that
        reads the parameters compares their counters too, so an in-place write through the module (``sae.W_enc.mul_()``,
        ``load_state_dict``, an initialiser) is noticed even when the caller drives the engine directly, as ``train()`` does."""
        import weakref

        self._watched = [weakref.ref(t) for t in tensors]
        self._watched_versions = self._wversions()

    def _wversions(self):
        out = []
        for r in getattr(self, "_watched", ()):
            t = r()
            try:
                out.append(None if t is None else t._version)
            except RuntimeError:  # inference tensors carry no version counter
                out.append(-1)
        return out

    def _note_param_writes(self) -> None:
        v = self._pversion()
        w = self._wversions()
        if v is None or v != self._params_version or w != getattr(self, "_watched_versions", []) or -1 in w:
            self.params_touched()
            self._watched_versions = w

    def _check_x(self, x: torch.Tensor) -> torch.Tensor:
        if x.device != self.device or x.dtype != torch.float32:
            raise _lib.SaevError(f"activations must be float32 on {self.device}, got {x.dtype} on {x.device}")
        if x.ndim != 2 or x.shape[1] != self.cfg.d_model:
            raise _lib.SaevError(f"activations must be (n, {self.cfg.d_model}), got {tuple(x.shape)}")
        return x.contiguous()

    # ---- single ops -----------------------------------------------------------------------
    def normalize_w_dec(self):
        self._chk(self.lib.saev_normalize_w_dec(self.ctx, _stream()), "saev_normalize_w_dec")

    def encode_dense(self, x: torch.Tensor) -> torch.Tensor:
        x = self._check_x(x)
        h = torch.empty(x.shape[0], self.cfg.d_sae, device=self.device, dtype=torch.float32)
        self._chk(self.lib.saev_encode_dense(self.ctx, _ptr(x), x.shape[0], _ptr(h), _stream()), "saev_encode_dense")
        return h

    def _check_dev(self, what: str, t: torch.Tensor, dtype: torch.dtype) -> None:
        if not isinstance(t, torch.Tensor) or t.device != self.device or t.dtype != dtype:
            got = f"{t.dtype} on {t.device}" if isinstance(t, torch.Tensor) else type(t).__name__
            raise _lib.SaevError(f"{what} must be {dtype} on {self.device}, got {got}")

    def _check_codes(self, idx: torch.Tensor, val: torch.Tensor):
        """(idx, val) of a fixed-length code matrix: int32 / float32 on the engine's device, both (n, k), contiguous."""
        self._check_dev("idx", idx, torch.int32)
        self._check_dev("val", val, torch.float32)
        if idx.ndim != 2 or idx.shape != val.shape or idx.shape[0] < 1 or idx.shape[1] < 1:
            raise _lib.SaevError(f"idx and val must both be (n, k), got {tuple(idx.shape)} and {tuple(val.shape)}")
        return idx.contiguous(), val.contiguous()

    def topk_dense(self, h: torch.Tensor, k: int, mask: torch.Tensor | None = None):
        """``(idx, val)``, (n, k) each, of the per-row top-k of ``h`` (n, d_sae), in ascending latent order (include/saev_amd.h,
        saev_topk_dense: the order of NaN and of the zeros, and the -1 / 0 slots of a mask with fewer than k eligible latents).
        ``h`` must be float32 on the engine's device.  ``mask`` is a (d_sae,) bool or integer tensor, non-zero = eligible; it is the
        one argument that may live on another device (the host, usually): it is a small vector that is converted to int32 words and
        copied here anyway."""
        S = self.cfg.d_sae
        self._check_dev("h", h, torch.float32)
        if h.ndim != 2 or h.shape[1] != S or h.shape[0] < 1:
            raise _lib.SaevError(f"h must be (n, {S}), got {tuple(h.shape)}")
        if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= S:
            raise _lib.SaevError(f"k must be an int in 1..{S}, got {k!r}")
        h = h.contiguous()
        if h.data_ptr() % 16:
            h = h.clone()
        n = h.shape[0]
        idx = torch.empty(n, k, device=self.device, dtype=torch.int32)
        val = torch.empty(n, k, device=self.device, dtype=torch.float32)
        if mask is not None:
            if not isinstance(mask, torch.Tensor) or mask.shape != (S,) or mask.is_floating_point() or mask.is_complex():
                raise _lib.SaevError(f"mask must be an integer or bool tensor of shape ({S},), got "
                                     f"{tuple(mask.shape) if isinstance(mask, torch.Tensor) else type(mask).__name__}")
            if mask.dtype != torch.int32:  # (an int64 word whose low half is zero must stay "eligible")
                mask = mask != 0
            mask = mask.to(self.device, torch.int32).contiguous()
            if mask.data_ptr() % 16:
                mask = mask.clone()
        self._chk(self.lib.saev_topk_dense(self.ctx, _ptr(h), n, k, _ptr(mask), _ptr(idx), _ptr(val), _stream()), "saev_topk_dense")
        return idx, val

    def encode_topk(self, x: torch.Tensor):
        self._topk_only("encode_topk")
        x = self._check_x(x)
        self._note_param_writes()
        n, k = x.shape[0], min(self.cfg.top_k, self.cfg.d_sae)
        idx = torch.empty(n, k, device=self.device, dtype=torch.int32)
        val = torch.empty(n, k, device=self.device, dtype=torch.float32)
        self._chk(self.lib.saev_encode_topk(self.ctx, _ptr(x), n, _ptr(idx), _ptr(val), _stream()), "saev_encode_topk")
        return idx, val

    def scatter_dense(self, idx: torch.Tensor, val: torch.Tensor) -> torch.Tensor:
        idx, val = self._check_codes(idx, val)
        n, k = idx.shape
        f = torch.zeros(n, self.cfg.d_sae, device=self.device, dtype=torch.float32)
        self._chk(self.lib.saev_scatter_dense(self.ctx, _ptr(idx), _ptr(val), n, k, _ptr(f), _stream()), "saev_scatter_dense")
        return f

    def decode_sparse(self, idx: torch.Tensor, val: torch.Tensor, prefixes=None) -> torch.Tensor:
        idx, val = self._check_codes(idx, val)
        n, k = idx.shape
        if prefixes is None:
            pre = [self.cfg.d_sae]
        else:
            pre = [int(p) for p in prefixes]
        if not pre:
            raise _lib.SaevError("prefixes must hold at least one cut")
        arr = (C.c_int64 * len(pre))(*pre)
        out = torch.empty(n, len(pre), self.cfg.d_model, device=self.device, dtype=torch.float32)
        self._chk(self.lib.saev_decode_sparse(self.ctx, _ptr(idx), _ptr(val), n, k, arr, len(pre), _ptr(out), _stream()), "saev_decode_sparse")
        return out

    # ---- ReLU SAE forward: padded variable-length rows (include/saev_amd.h, saev_encode_relu) ---------------------------
    def encode_relu(self, x: torch.Tensor, row_cap: int | None = None):
        """f = relu(x W_enc + b_enc) as padded rows: ``(idx, val, row_nnz)``, idx / val (n, cap), row b's entries in its first
        row_nnz[b] slots in ascending latent order (slots past it are unspecified).  ``cap`` starts at ``row_cap`` (default: the
        engine's ``relu_row_cap``); when a row has more positives the call reads the largest count back and runs the encoder
        once more with that capacity, so no row is truncated.  Without ``row_cap`` the engine's capacity then grows to it."""
        if self.cfg.activation not in ("relu", "relu_train"):
            raise _lib.SaevError("encode_relu needs an engine created with activation='relu' (or 'relu_train')")
        if self.cfg.encoder == "bf16":
            raise NotImplementedError("the bf16 encoder is not available for ReLU SAEs: use f32, f16x3 or f16r")
        x = self._check_x(x)
        self._note_param_writes()
        n, S = x.shape[0], self.cfg.d_sae
        cap = max(1, min(S, row_cap if row_cap is not None else self.relu_row_cap))
        over = torch.empty(1, device=self.device, dtype=torch.int32)
        row_nnz = torch.empty(n, device=self.device, dtype=torch.int32)
        for attempt in range(2):
            idx = torch.empty(n, cap, device=self.device, dtype=torch.int32)
            val = torch.empty(n, cap, device=self.device, dtype=torch.float32)
            self._chk(self.lib.saev_encode_relu(self.ctx, _ptr(x), n, cap, _ptr(row_nnz), _ptr(idx), _ptr(val), _ptr(over), _stream()),
                      "saev_encode_relu")
            need = int(over.item())  # the call's one read-back: 0, or the largest row count when a row overflowed
            if need == 0:
                return idx, val, row_nnz
            if attempt == 1:
                raise _lib.SaevError(f"saev_encode_relu overflowed a capacity of {cap} sized from its own count {need}")
            cap = need
            self.relu_second_launches += 1
            if row_cap is None:
                self.relu_row_cap = max(self.relu_row_cap, min(S, (need + 63) // 64 * 64))

    def decode_rows(self, idx: torch.Tensor, val: torch.Tensor, row_nnz: torch.Tensor, prefixes=None) -> torch.Tensor:
        """(n, n_prefixes, d_model) reconstructions of padded rows (ascending latents per row); the cost grows with row_nnz."""
        n, cap = idx.shape
        pre = [self.cfg.d_sae] if prefixes is None else [int(p) for p in prefixes]
        arr = (C.c_int64 * len(pre))(*pre)
        out = torch.empty(n, len(pre), self.cfg.d_model, device=self.device, dtype=torch.float32)
        self._chk(self.lib.saev_decode_rows(self.ctx, _ptr(idx.contiguous()), _ptr(val.contiguous()), _ptr(row_nnz.contiguous()), cap, n,
                                            arr, len(pre), _ptr(out), _stream()), "saev_decode_rows")
        return out

    def scatter_rows(self, idx: torch.Tensor, val: torch.Tensor, row_nnz: torch.Tensor) -> torch.Tensor:
        """Dense (n, d_sae) f_x of padded rows (API compatibility)."""
        n, cap = idx.shape
        f = torch.zeros(n, self.cfg.d_sae, device=self.device, dtype=torch.float32)
        self._chk(self.lib.saev_scatter_rows(self.ctx, _ptr(idx.contiguous()), _ptr(val.contiguous()), _ptr(row_nnz.contiguous()), cap, n,
                                             _ptr(f), _stream()), "saev_scatter_rows")
        return f

    # ---- BatchTopK activation: padded rows of row_cap slots, -1 / 0 past row_nnz (include/saev_amd.h: BATCHTOPK) -------------
    def _btk_rows(self, what: str, src: torch.Tensor, training: bool):
        if self.cfg.activation != "batch_topk":
            raise _lib.SaevError(f"{what} needs an engine created with activation='batch_topk'")
        n = src.shape[0]
        fn = getattr(self.lib, f"saev_{what}")
        over = torch.empty(1, device=self.device, dtype=torch.int32)
        row_nnz = torch.empty(n, device=self.device, dtype=torch.int32)
        for attempt in range(2):
            idx = torch.empty(n, self.row_cap, device=self.device, dtype=torch.int32)
            val = torch.empty(n, self.row_cap, device=self.device, dtype=torch.float32)
            self._chk(fn(self.ctx, _ptr(src), n, int(training), _ptr(row_nnz), _ptr(idx), _ptr(val), _ptr(over), _stream()), f"saev_{what}")
            need = int(over.item())  # the call's one read-back: 0, or the largest row count when a row overflowed
            if need == 0:
                return idx, val, row_nnz
            if attempt == 1:
                raise _lib.SaevError(f"saev_{what} overflowed rows of {self.row_cap} sized from its own count {need}")
            self._grow_rows(need)  # (the threshold has not moved: the repeated call applies the update, once)

    def encode_batch_topk(self, x: torch.Tensor, *, training: bool):
        """``(idx, val, row_nnz)`` of f = BatchTopK(x W_enc + b_enc): training mode selects over the whole batch and updates the
        threshold, eval mode keeps h > threshold.  A row longer than ``row_cap`` grows the engine's rows and repeats the call."""
        x = self._check_x(x)
        self._note_param_writes()
        return self._btk_rows("encode_batch_topk", x, training)

    def batch_topk_dense(self, h: torch.Tensor, *, training: bool = True):
        """The activation alone on a dense (n, d_sae) float32 device matrix: ``(idx, val, row_nnz)``."""
        if h.device != self.device or h.dtype != torch.float32 or h.ndim != 2 or h.shape[1] != self.cfg.d_sae:
            raise _lib.SaevError(f"batch_topk_dense takes a float32 (n, {self.cfg.d_sae}) matrix on {self.device}")
        h = h.contiguous()
        if h.data_ptr() % 16:
            h = h.clone()
        return self._btk_rows("batch_topk_dense", h, training)

    def batch_topk_state(self) -> dict:
        """What the last training-mode select left on the device: the cut value, the entries strictly above it, how many of the
        entries equal to it are kept (the tie quota) and how many there are."""
        cut = C.c_float()
        above, quota, ties = C.c_int64(), C.c_int64(), C.c_int64()
        self._chk(self.lib.saev_batch_topk_state(self.ctx, C.byref(cut), C.byref(above), C.byref(quota), C.byref(ties), _stream()),
                  "saev_batch_topk_state")
        return {"cut": cut.value, "n_above": above.value, "tie_quota": quota.value, "n_ties": ties.value}

    def remove_parallel_grads(self):
        self._chk(self.lib.saev_remove_parallel_grads(self.ctx, _stream()), "saev_remove_parallel_grads")

    def gather_rows(self, pool: torch.Tensor, rows: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        """``out[r] = pool[rows[r]]``: pool (rows, d_model) float32, contiguous; rows (n,) int64, every entry a row of the pool
        (the kernel does not check: the caller draws them); ``out`` (n, d_model) float32, contiguous, written in place."""
        D = self.cfg.d_model
        self._check_dev("pool", pool, torch.float32)
        self._check_dev("rows", rows, torch.int64)
        if pool.ndim != 2 or pool.shape[1] != D or not pool.is_contiguous() or pool.data_ptr() % 16:
            raise _lib.SaevError(f"pool must be a contiguous, 16-byte aligned (rows, {D}) matrix, got {tuple(pool.shape)} with strides {pool.stride()}")
        if rows.ndim != 1 or rows.shape[0] < 1:
            raise _lib.SaevError(f"rows must be (n,) with n >= 1, got {tuple(rows.shape)}")
        rows = rows.contiguous()
        n = rows.shape[0]
        if out is None:
            out = torch.empty(n, D, device=self.device, dtype=torch.float32)
        else:
            self._check_dev("out", out, torch.float32)
            if out.shape != (n, D) or not out.is_contiguous() or out.data_ptr() % 16:
                raise _lib.SaevError(f"out must be a contiguous, 16-byte aligned ({n}, {D}) matrix, got {tuple(out.shape)} with strides {out.stride()}")
        self._chk(self.lib.saev_gather_rows(self.ctx, _ptr(pool), _ptr(rows), n, _ptr(out), _stream()), "saev_gather_rows")
        return out

    # ---- the step -------------------------------------------------------------------------
    def step_forward(self, x: torch.Tensor, *, training: bool = True, n_rows_global: int | None = None):
        self._trains("step_forward")
        x = self._check_x(x)
        self._x_keepalive = x
        self._note_param_writes()
        n = x.shape[0]
        if self.cfg.activation == "relu_train" and (n_rows_global or n) != n:
            raise NotImplementedError("step_forward: a ReLU training engine runs on one GPU (n_rows_global must equal the batch)")
        rc = self.lib.saev_step_forward(self.ctx, _ptr(x), n, n_rows_global or n, int(training), _stream())
        if rc == _lib.ROW_OVERFLOW:
            # BatchTopK: nothing was decoded and the threshold has not moved; larger rows, then the same forward again
            self._grow_rows(int(self.lib.saev_row_overflow_need(self.ctx)))
            rc = self.lib.saev_step_forward(self.ctx, _ptr(x), n, n_rows_global or n, int(training), _stream())
        self._chk(rc, "saev_step_forward")
        self._last_n = n

    def step_dead(self, n_rows_global: int):
        self._trains("step_dead")
        self._chk(self.lib.saev_step_dead(self.ctx, n_rows_global, _stream()), "saev_step_dead")

    def step_backward(self):
        self._trains("step_backward")
        self._chk(self.lib.saev_step_backward(self.ctx, _stream()), "saev_step_backward")

    # backward in pieces (data-parallel overlap, see framework/ddp.py)
    def grad_w_enc_t(self) -> torch.Tensor:
        """(d_sae, d_model) transposed W_enc gradient the ranged backward writes; allocated on first use and handed to
        the context so that collectives can run on it."""
        if self._w_enc_t is None:
            self._w_enc_t = torch.zeros(self.cfg.d_sae, self.cfg.d_model, device=self.device, dtype=torch.float32)
            self._chk(self.lib.saev_bind_w_enc_t(self.ctx, _ptr(self._w_enc_t)), "saev_bind_w_enc_t")
        return self._w_enc_t

    def backward_begin(self):
        self._topk_only("backward_begin")
        self._chk(self.lib.saev_backward_begin(self.ctx, _stream()), "saev_backward_begin")

    def backward_rows(self, lo: int, hi: int, part: int = 0):
        """Gradient rows of the latents [lo, hi).  part 0: both matrices in one pass; 1: the decoder's only (after it the
        decoder half of the gradient -- W_dec and b_dec -- is final); 2: the encoder's (needs part 1 first)."""
        if self.cfg.activation == "relu_train":
            self._topk_only("backward_rows")
        self._chk(self.lib.saev_backward_rows_part(self.ctx, lo, hi, part, _stream()), "saev_backward_rows_part")

    def backward_end(self):
        if self.cfg.activation == "relu_train":
            self._topk_only("backward_end")
        self._chk(self.lib.saev_backward_end(self.ctx, _stream()), "saev_backward_end")

    def step_tail(self, lr: float, max_norm: float = 1.0, grad_scale: float = 1.0, *, trusted: bool = False):
        """``trusted``: nothing wrote the gradient buffer since ``backward_end`` -- the tail may use the row statistics the
        backward left behind (projection inside Adam, no rpg pass), as ``train_step`` does."""
        self._trains("step_tail")
        self.adam_steps += 1
        if trusted:
            self._chk(self.lib.saev_trust_gradients(self.ctx, 1), "saev_trust_gradients")
        try:
            self._chk(self.lib.saev_step_tail(self.ctx, lr, max_norm, grad_scale, self.adam_steps, _stream()), "saev_step_tail")
        finally:
            if trusted:
                self.lib.saev_trust_gradients(self.ctx, 0)

    def muon_tail(self, lr: float, max_norm: float = 1.0, grad_scale: float = 1.0, muon: MuonConfig | None = None):
        """The tail of a Muon step after the phases (saev_muon_tail): rpg, clip, Adam on the biases, Muon on W_dec / W_enc.
        The momentum buffers are the W_dec / W_enc segments of ``adam_m``."""
        self._trains("muon_tail")
        cfg = (muon or MuonConfig()).c_struct()
        self._chk(self.lib.saev_muon_tail(self.ctx, lr, max_norm, grad_scale, self.adam_steps + 1, C.byref(cfg), _stream()), "saev_muon_tail")
        self.adam_steps += 1  # (counted once the step is enqueued: a refused call -- d_model > d_sae -- is not an optimizer step)

    def train_step_muon(self, x: torch.Tensor, lr: float, max_norm: float = 1.0, muon: MuonConfig | None = None):
        """One optimizer step with Muon on the weight matrices: the phases, then ``muon_tail``."""
        n = x.shape[0]
        self.step_forward(x, training=True, n_rows_global=n)
        self.step_dead(n)
        self.step_backward()
        self.muon_tail(lr, max_norm, muon=muon)

    # ---- gathered backward (data-parallel runs that exchange the sparse step state instead of the gradient) -------------
    def gather_buffers(self, world: int, n_local: int):
        """(x_all, g_all, idx_all, val_all) for ``world`` ranks of ``n_local`` rows each, allocated once per shape."""
        P = getattr(self, "_n_prefixes", 1)  # Matryoshka: dL/dx_hat is P suffix-summed gradients per row
        key = (world, n_local, P)
        if getattr(self, "_gather_key", None) != key:
            n, D, K = world * n_local, self.cfg.d_model, min(self.cfg.top_k, self.cfg.d_sae)
            cap = max(self.cfg.max_batch, self.cfg.max_backward_rows)
            if n > cap:
                raise _lib.SaevError(f"gathered backward over {n} rows needs an engine with max_backward_rows >= {n} (the GLOBAL batch), "
                                     f"got {cap}")
            self._gather_bufs = (torch.empty(n, D, device=self.device), torch.empty(n, P * D, device=self.device),
                                 torch.empty(n, K, device=self.device, dtype=torch.int32), torch.empty(n, K, device=self.device))
            self._gather_key = key
        return self._gather_bufs

    def copy_step_state(self, n_rows: int, g_out: torch.Tensor, idx_out: torch.Tensor, val_out: torch.Tensor):
        """This rank's rows of dL/dx_hat and of the codes of the training forward in flight, into caller tensors."""
        if self.cfg.activation == "relu_train":
            self._topk_only("copy_step_state")
        self._chk(self.lib.saev_copy_step_state(self.ctx, n_rows, _ptr(g_out), _ptr(idx_out), _ptr(val_out), _stream()), "saev_copy_step_state")

    def backward_begin_gathered(self, x_all: torch.Tensor, g_all: torch.Tensor, idx_all: torch.Tensor, val_all: torch.Tensor):
        """``backward_begin`` over the rows of ALL ranks (rank-major); the following ``backward_rows`` cover them too."""
        if self.cfg.activation == "relu_train":
            self._topk_only("backward_begin_gathered")
        assert x_all.is_contiguous() and g_all.is_contiguous() and idx_all.is_contiguous() and val_all.is_contiguous()
        self._gather_keepalive = (x_all, g_all, idx_all, val_all)
        self._chk(self.lib.saev_backward_override(self.ctx, _ptr(x_all), _ptr(g_all), _ptr(idx_all), _ptr(val_all), x_all.shape[0]),
                  "saev_backward_override")
        self.backward_begin()

    def aux_compact_export(self) -> torch.Tensor | None:
        """The auxiliary term's local gradient -- the dead latents' rows of dW_dec and dW_enc^T, their db_enc, its share of
        db_dec -- packed into one tensor (None when the step has no auxiliary work); sum it over ranks, then import."""
        rows = int(self.lib.saev_aux_compact_rows(self.ctx))
        if rows == 0:
            return None
        buf = torch.empty(rows * (2 * self.cfg.d_model + 1) + self.cfg.d_model, device=self.device)
        self._chk(self.lib.saev_aux_compact_export(self.ctx, _ptr(buf), _stream()), "saev_aux_compact_export")
        return buf

    def aux_compact_import(self, buf: torch.Tensor):
        self._chk(self.lib.saev_aux_compact_import(self.ctx, _ptr(buf), _stream()), "saev_aux_compact_import")

    # tail in two parts over this rank's chunks (data-parallel runs with a sharded tail, framework/ddp.py)
    def halves(self, flat: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
        """The [W_dec | b_dec | pad] and [W_enc | b_enc | pad] halves of a flat buffer (shard_world equal chunks each)."""
        a = self.chunk_a * self.cfg.shard_world
        return flat[:a], flat[a:]


    def tail_prepare(self, shard_rank: int = -1):
        self._topk_only("tail_prepare")
        self._chk(self.lib.saev_tail_prepare(self.ctx, shard_rank, _stream()), "saev_tail_prepare")

    def tail_apply(self, lr: float, max_norm: float = 1.0, grad_scale: float = 1.0, shard_rank: int = -1):
        self._topk_only("tail_apply")
        self.adam_steps += 1
        self._chk(self.lib.saev_tail_apply(self.ctx, lr, max_norm, grad_scale, self.adam_steps, shard_rank, _stream()), "saev_tail_apply")

    def wdec_ready_after(self, event: "torch.cuda.Event | None"):
        """The next step_forward waits for ``event`` before it first touches W_dec (and renormalises W_dec there)."""
        self._wdec_event = event  # keep the handle alive until it has been consumed
        self._chk(self.lib.saev_wdec_ready_event(self.ctx, C.c_void_p(event.cuda_event) if event is not None else None),
                  "saev_wdec_ready_event")

    def wenc_ready_after(self, event: "torch.cuda.Event | None"):
        """The next forward prepares x first and waits for ``event`` only before it reads W_enc / b_enc."""
        self._wenc_event = event
        self._chk(self.lib.saev_wenc_ready_event(self.ctx, C.c_void_p(event.cuda_event) if event is not None else None),
                  "saev_wenc_ready_event")

    def train_step(self, x: torch.Tensor, lr: float, max_norm: float = 1.0):
        """Phases 1-4 on one GPU (reference train.py:332-460 loop body for one SAE).

        ``grad_views()`` is NOT a valid gradient afterwards: the W_enc gradient stays in the transposed scratch and the
        dW_dec rows are stored un-projected (the fused Adam projects them as it reads).  To look at gradients run the phases
        (``step_forward`` / ``step_dead`` / ``step_backward`` / ``step_tail``), as the log steps of ``train()`` do.
        (BatchTopK and ReLU training engines run the four phases back to back here: their ``grad_views()`` IS the step's
        gradient afterwards, projected by the tail.)"""
        self._trains("train_step")
        x = self._check_x(x)
        self._x_keepalive = x
        self._note_param_writes()
        rc = self.lib.saev_train_step(self.ctx, _ptr(x), x.shape[0], lr, max_norm, self.adam_steps + 1, _stream())
        if rc == _lib.ROW_OVERFLOW:  # (BatchTopK: the step stopped in its forward, before anything moved)
            self._grow_rows(int(self.lib.saev_row_overflow_need(self.ctx)))
            rc = self.lib.saev_train_step(self.ctx, _ptr(x), x.shape[0], lr, max_norm, self.adam_steps + 1, _stream())
        self._chk(rc, "saev_train_step")
        self._last_n = 0
        self.adam_steps += 1  # (counted once the step is enqueued: a refused call -- SAEV_STALE_PARAMS -- is not an optimizer step)

    # data parallel behind the C ABI (include/saev_amd.h: DATA PARALLEL): RCCL inside the library, two collectives per step
    def comm_unique_id(self) -> bytes:
        """128 bytes from ncclGetUniqueId: made on ONE rank, handed to all ranks (e.g. ``torch.distributed.broadcast_object_list``)."""
        buf = C.create_string_buffer(128)
        self._chk(self.lib.saev_comm_unique_id(buf), "saev_comm_unique_id")
        return buf.raw

    def comm_init(self, unique_id: bytes, rank: int, world: int):
        if len(unique_id) != 128:
            raise _lib.SaevError(f"a communicator id is 128 bytes, got {len(unique_id)}")
        self._chk(self.lib.saev_comm_init(self.ctx, C.create_string_buffer(unique_id, 128), rank, world), "saev_comm_init")

    def comm_world(self) -> int:
        return int(self.lib.saev_comm_world(self.ctx))

    def train_step_dp(self, x_local: torch.Tensor, lr: float, max_norm: float = 1.0):
        self._topk_only("train_step_dp")
        """One optimizer step on the global batch of which ``x_local`` is this rank's share (equal shares on all ranks): forward,
        all-reduce of the fired flags, AuxK + backward, all-reduce of the flat gradient, tail with the gradient averaged --
        all enqueued by ONE call into the library (saev_train_step_dp), RCCL on torch's current stream."""
        x = self._check_x(x_local)
        self._x_keepalive = x
        self._note_param_writes()
        self._chk(self.lib.saev_train_step_dp(self.ctx, _ptr(x), x.shape[0], lr, max_norm, self.adam_steps + 1, _stream()), "saev_train_step_dp")
        self._last_n = 0
        self.adam_steps += 1  # (counted once the step is enqueued: a refused call -- SAEV_STALE_PARAMS -- is not an optimizer step)

    def train_step_gather(self, pool: torch.Tensor, rows: torch.Tensor, lr: float, max_norm: float = 1.0, out: torch.Tensor | None = None) -> torch.Tensor:
        """``train_step`` on the batch ``pool[rows]``, drawn inside the step (saev_train_step_gather): the step's first kernel reads
        the pool rows and leaves the batch as a contiguous matrix -- returned -- on its way."""
        self._topk_only("train_step_gather")
        n = rows.shape[0]
        if pool.device != self.device or pool.dtype != torch.float32 or pool.ndim != 2 or pool.shape[1] != self.cfg.d_model or not pool.is_contiguous():
            raise _lib.SaevError(f"the pool must be a contiguous float32 (rows, {self.cfg.d_model}) matrix on {self.device}")
        if rows.device != self.device or rows.dtype != torch.int64 or not rows.is_contiguous():
            raise _lib.SaevError(f"rows must be contiguous int64 on {self.device}")
        if out is None:
            out = torch.empty(n, self.cfg.d_model, device=self.device, dtype=torch.float32)
        self._x_keepalive = (pool, rows, out)
        self._note_param_writes()
        self._chk(self.lib.saev_train_step_gather(self.ctx, _ptr(pool), _ptr(rows), _ptr(out), n, lr, max_norm, self.adam_steps + 1, _stream()),
                  "saev_train_step_gather")
        self._last_n = 0
        self.adam_steps += 1
        return out

    def read_stats(self) -> StepStats:
        st = _lib.SaevStepStats()
        self._chk(self.lib.saev_read_stats(self.ctx, C.byref(st), _stream()), "saev_read_stats")
        return StepStats(**{f: getattr(st, f) for f, _ in _lib.SaevStepStats._fields_})

    def add_batch_stats(self, acc: BatchStats, x: torch.Tensor, keep: torch.Tensor | None = None, *, overwrite: bool = False,
                        x_hat: bool = True, scalars: bool = True) -> None:
        """Accumulate the statistics of the last ``step_forward`` -- whose batch ``x`` was -- into ``acc`` straight from the
        context's own codes and reconstruction (saev_last_idx / _val / _x_hat): no copy of either is made.  ``x_hat=False``
        leaves the reconstruction unread (the residual sums then add 0); ``scalars=False`` leaves the scalar sums out."""
        self._trains("add_batch_stats")  # (BatchTopK rows are padded with idx = -1, which the kernel ignores: no row_nnz needed)
        if self.cfg.activation == "relu_train":
            raise NotImplementedError("add_batch_stats: a ReLU training engine keeps no padded rows (compact them with last_codes and call BatchStats.add)")
        x = self._check_x(x)
        if self._last_n == 0 or x.shape[0] != self._last_n:
            raise _lib.SaevError(f"add_batch_stats: x has {x.shape[0]} rows, the last step_forward had {self._last_n or 'none'}")
        if acc.d_model != self.cfg.d_model or acc.d_sae != self.cfg.d_sae or acc.device != self.device:
            raise _lib.SaevError("add_batch_stats: the accumulator was made for another shape or device")
        p = lambda v: C.c_void_p(v)  # noqa: E731
        acc._add_ptrs(_ptr(x), p(self.lib.saev_last_x_hat(self.ctx)) if x_hat else None, p(self.lib.saev_last_idx(self.ctx)),
                      p(self.lib.saev_last_val(self.ctx)), None, keep, x.shape[0], self._code_width(), overwrite, scalars)

    def add_latent_topk(self, acc: LatentTopK, keep: torch.Tensor | None = None, *, row_base: int) -> None:
        """Feed the codes of the last ``step_forward`` to ``acc`` straight from the context (saev_last_idx / _val): no copy is
        made.  TopK rows are full; BatchTopK rows are padded with idx = -1, which the kernel ignores."""
        self._trains("add_latent_topk")
        if self.cfg.activation == "relu_train":
            raise NotImplementedError("add_latent_topk: a ReLU training engine keeps no padded rows (compact them with last_codes and call LatentTopK.add)")
        if self._last_n == 0:
            raise _lib.SaevError("add_latent_topk: no step_forward to take codes from")
        if acc.d_sae != self.cfg.d_sae or acc.device != self.device:
            raise _lib.SaevError("add_latent_topk: the accumulator was made for another shape or device")
        p = lambda v: C.c_void_p(v)  # noqa: E731
        acc._update(p(self.lib.saev_last_idx(self.ctx)), p(self.lib.saev_last_val(self.ctx)), None, self._code_width(), None, None, None, 0,
                    keep, self._last_n, row_base)

    def _code_width(self) -> int:
        """Columns of the context's code rows: top_k, or the row capacity of a BatchTopK engine."""
        return self.row_cap if self.cfg.activation == "batch_topk" else min(self.cfg.top_k, self.cfg.d_sae)

    def last_codes(self, n_rows: int, *, x_hat: bool = True, row_nnz: bool = False):
        """Copies of the last forward's codes and (unless ``x_hat=False``: None then) reconstruction.  A BatchTopK engine's codes
        are its padded rows (n_rows, row_cap); ``row_nnz=True`` appends their counts: ``(idx, val, x_hat, row_nnz)``.  A ReLU
        training engine's codes are compacted from the dense f of its last forward (saev_copy_last_rows) into rows of the capacity
        ``encode_relu`` keeps, which grows to the longest row met (one read-back, a second launch when a row did not fit)."""
        if self.cfg.activation == "relu_train":
            return self._relu_last_rows(n_rows, x_hat, row_nnz)
        k = self._code_width()
        idx = torch.empty(n_rows, k, device=self.device, dtype=torch.int32)
        val = torch.empty(n_rows, k, device=self.device, dtype=torch.float32)
        x_hat = torch.empty(n_rows, self.cfg.d_model, device=self.device, dtype=torch.float32) if x_hat else None
        self._chk(self.lib.saev_copy_last(self.ctx, n_rows, _ptr(idx), _ptr(val), _ptr(x_hat), _stream()), "saev_copy_last")
        if not row_nnz:
            return idx, val, x_hat
        nnz = torch.empty(n_rows, device=self.device, dtype=torch.int32)
        self._chk(self.lib.saev_copy_last_row_nnz(self.ctx, n_rows, _ptr(nnz), _stream()), "saev_copy_last_row_nnz")
        return idx, val, x_hat, nnz

    def _relu_last_rows(self, n_rows: int, x_hat: bool, row_nnz: bool):
        S = self.cfg.d_sae
        cap = max(1, min(S, self.relu_row_cap))
        over = torch.empty(1, device=self.device, dtype=torch.int32)
        nnz = torch.empty(n_rows, device=self.device, dtype=torch.int32)
        for attempt in range(2):
            idx = torch.empty(n_rows, cap, device=self.device, dtype=torch.int32)
            val = torch.empty(n_rows, cap, device=self.device, dtype=torch.float32)
            self._chk(self.lib.saev_copy_last_rows(self.ctx, n_rows, cap, _ptr(nnz), _ptr(idx), _ptr(val), _ptr(over), _stream()),
                      "saev_copy_last_rows")
            need = int(over.item())  # the call's one read-back: 0, or the largest row count when a row overflowed
            if need == 0:
                break
            if attempt == 1:
                raise _lib.SaevError(f"saev_copy_last_rows overflowed a capacity of {cap} sized from its own count {need}")
            cap = need
            self.relu_second_launches += 1
            self.relu_row_cap = max(self.relu_row_cap, min(S, (need + 63) // 64 * 64))
        xh = None
        if x_hat:
            xh = torch.empty(n_rows, self.cfg.d_model, device=self.device, dtype=torch.float32)
            self._chk(self.lib.saev_copy_last(self.ctx, n_rows, None, None, _ptr(xh), _stream()), "saev_copy_last")
        return (idx, val, xh, nnz) if row_nnz else (idx, val, xh)

    def aux_route(self) -> int:
        """What the last step_dead did for the auxiliary loss: 0 nothing, 1 few-dead-latents kernels without reading
        n_dead back, 2 the same after a read-back, 3 dense algebra after a read-back."""
        return int(self.lib.saev_last_aux_route(self.ctx))

    def scratch_bytes(self, which: int = 0) -> int:
        """Device memory the context owns besides the four flat buffers: 0 all of it, 1 AuxK dead-set buffers, 2 Matryoshka blocks."""
        return int(self.lib.saev_scratch_bytes(self.ctx, which))

    def dead_readbacks(self) -> int:
        """Blocking reads of n_dead so far."""
        return int(self.lib.saev_dead_readbacks(self.ctx))

    def bound_state(self) -> dict:
        """z of the predicted bounds (``bounds="norm"``: their safety factor c), launches that used them, how many had to be
        repeated, mean list length of the last."""
        z, mc = C.c_float(), C.c_float()
        n, r = C.c_int64(), C.c_int64()
        self._chk(self.lib.saev_bound_state(self.ctx, C.byref(z), C.byref(n), C.byref(r), C.byref(mc), _stream()), "saev_bound_state")
        out = {"z": z.value, "launches": n.value, "repeats": r.value, "mean_candidates": mc.value}
        if self.cfg.bounds == "norm":  # (their ratio and what is left of a pause: saev_bound_ratio)
            rho, left = C.c_float(), C.c_int64()
            self._chk(self.lib.saev_bound_ratio(self.ctx, C.byref(rho), C.byref(left), _stream()), "saev_bound_ratio")
            out.update(rho_lo=rho.value, pause_left=left.value)
        return out

    def enable_kernel_timing(self, on: bool = True):
        self._chk(self.lib.saev_enable_kernel_timing(self.ctx, int(on)), "saev_enable_kernel_timing")

    def encoder_ms(self) -> float:
        return float(self.lib.saev_last_encoder_ms(self.ctx))
