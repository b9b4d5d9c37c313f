"""Plain restatements of what the Muon tail does on the host and of torch's Muon step on one matrix -- shared by
test_muon_restatement_host_cpu.py (which holds them to the library's host entries and to torch.optim.Muon on the CPU) and by
test_gpu_muon_geometry.py (which holds the kernels to them):

  layout(D, S)       gemm_splits and muon_layout of saev_amd/csrc/muon.hip: the padded shape, the number of per-workgroup squares,
                     the split-K decomposition of the two symmetric products and the workspace size;
  CASES              the (rows, cols) the GPU tests run, one per class of that decomposition, each with the values layout() must
                     give -- a shape that moves to another class fails a CPU test instead of quietly testing something else;
  CONFIGS            the hyper-parameter settings both files run;
  muon_step_fp64     torch's _single_tensor_muon on one matrix with an injectable orthogonaliser;
  norm_margin, margin_input   inputs whose bf16 norm is decided by the reference alone."""

import dataclasses
import math

import torch

GT, GK, MT, MAX_SPLITS = 128, 32, 64, 16  # GEMM tile, k step, tile of the element-wise passes, MUON_MAX_SPLITS (kernels.h)


@dataclasses.dataclass(frozen=True)
class Layout:
    Dp: int
    Sp: int
    nb: int
    gram: tuple  # (n, k tiles per split, splits, k tiles in the last split) of G = X X^T
    gg: tuple    # the same of G G
    bytes: int


def _splits(tm: int, kt: int) -> tuple:
    """gemm_splits for a symmetric product of tm x tm tiles over kt k-tiles: n is the number of splits asked for (about 512
    workgroups in flight, at most MAX_SPLITS, at most one per k tile), then the k tiles per split and the splits that leaves."""
    tiles = tm * (tm + 1) // 2
    n = min(MAX_SPLITS, max(1, -(-512 // tiles)), kt)
    kper = -(-kt // n)
    splits = -(-kt // kper)
    return n, kper, splits, kt - (splits - 1) * kper


def layout(D: int, S: int) -> Layout:
    up = lambda v, m: -(-v // m) * m
    Dp, Sp = up(D, GT), up(S, GT)
    nb = -(-S // MT) * -(-D // MT)
    gram, gg = _splits(Dp // GT, Sp // GK), _splits(Dp // GT, Dp // GK)
    parts = [Dp * Sp * 2] * 2 + [Dp * Dp * 2] * 2 + [max(gram[2], gg[2]) * Dp * Dp * 4, nb * 8, 4]
    return Layout(Dp, Sp, nb, gram, gg, sum(up(b, 256) for b in parts))


@dataclasses.dataclass(frozen=True)
class Case:
    rows: int
    cols: int
    padded: tuple
    gram: tuple
    gg: tuple
    why: str

    @property
    def shape(self):
        return (self.rows, self.cols)

    @property
    def id(self):
        return f"{self.rows}x{self.cols}"


CASES = (
    Case(4, 8, (128, 128), (4, 1, 4, 1), (4, 1, 4, 1), "one tile, splits capped by kt, everything but 32 elements padding"),
    Case(36, 260, (128, 384), (12, 1, 12, 1), (4, 1, 4, 1), "one tile, ragged in both, kt < 16"),
    Case(128, 128, (128, 128), (4, 1, 4, 1), (4, 1, 4, 1), "exact tile, square"),
    Case(132, 132, (256, 256), (8, 1, 8, 1), (8, 1, 8, 1), "just past a tile: 124 padded rows, rows == cols"),
    Case(100, 1250, (128, 1280), (16, 3, 14, 1), (4, 1, 4, 1), "uneven last split, fewer splits than n"),
    Case(300, 516, (384, 640), (16, 2, 10, 2), (12, 1, 12, 1), "tm = 3: six upper tiles, three skipped"),
    Case(200, 5201, (256, 5248), (16, 11, 15, 10), (8, 1, 8, 1), "nb = 4 x 82 = 328 > 256, S odd"),
)

# (MuonConfig / torch.optim.Muon keyword arguments, by name)
CONFIGS = {
    "defaults": {},
    "momentum0.3": {"momentum": 0.3},  # 1 - mu = 0.7 >= 0.5 for the buffer, mu < 0.5 for Nesterov: lerp's other two branch / use pairs
    "momentum0": {"momentum": 0.0},
    "no_nesterov": {"nesterov": False},
    "wd0.5": {"weight_decay": 0.5},
    "wd0": {"weight_decay": 0.0},
    "match_rms_adamw": {"adjust_lr_fn": "match_rms_adamw"},
    "ns_steps3": {"ns_steps": 3},
    "ns_steps0": {"ns_steps": 0},
}


def adjusted_lr(lr: float, adjust_lr_fn, shape) -> float:
    A, B = shape
    if adjust_lr_fn is None or adjust_lr_fn == "original":
        return lr * math.sqrt(max(1, A / B))
    if adjust_lr_fn == "match_rms_adamw":
        return lr * 0.2 * math.sqrt(max(A, B))
    return lr * 1.0


def f32(v: float) -> float:
    """A Python float rounded to fp32: what a Python scalar becomes inside an fp32 tensor operation."""
    return torch.tensor(v, dtype=torch.float32).item()


def muon_step_fp64(p, g, m, lr: float, cfg, ns=None, torch_update: bool = False):
    """One torch.optim.Muon step on the matrix ``p`` (fp32) with gradient ``g`` and momentum buffer ``m`` (updated in place), on
    whatever device they live.  The two lerps are torch's fp32 ops; the ratio and the decay are Python floats, as torch computes
    them, and enter the update rounded to fp32, as a Python scalar enters an fp32 tensor operation; ``ns(u)`` is the
    orthogonaliser (default: torch's own with cfg's coefficients, steps and eps).  The update is p * decay - adj_lr * O in fp64,
    with p * decay rounded to fp32 first, where torch's mul_ (and the tail's apply kernel) rounds it: what is left to an fp32
    evaluation is the final rounding alone.  ``torch_update=True`` runs torch's own two fp32 operations instead (mul_, add_ with
    alpha), which is what the CPU test compares with torch.optim.Muon bit for bit.  Returns (new p, u, O)."""
    if ns is None:
        from torch.optim._muon import _zeropower_via_newtonschulz

        ns = lambda u: _zeropower_via_newtonschulz(u, tuple(cfg.ns_coefficients), cfg.ns_steps, cfg.eps)
    m.lerp_(g, 1 - cfg.momentum)
    u = g.lerp(m, cfg.momentum) if cfg.nesterov else m
    O = ns(u)
    decay, adj = 1 - lr * cfg.weight_decay, adjusted_lr(lr, cfg.adjust_lr_fn, p.shape)
    if torch_update:
        q = p.clone()
        q.mul_(decay)
        q.add_(O, alpha=-adj)
    else:
        q = (p.double() * f32(decay)).float().double() - f32(adj) * O.double()  # (the fp64 product of two fp32 is exact: one rounding)
    return q, u, O


def ulp_of(mag: torch.Tensor, mantissa_bits: int) -> torch.Tensor:
    """The spacing of a format with ``mantissa_bits`` explicit mantissa bits (7: bf16, 23: fp32) at the magnitudes ``mag`` (fp64)."""
    return 2.0 ** (torch.floor(torch.log2(mag.clamp_min(1e-38))) - mantissa_bits)


def norm_margin(x: torch.Tensor) -> float:
    """How far the fp64 Frobenius norm of bf16(x) is from the nearest bf16 rounding boundary (the midpoint of two neighbouring
    bf16 values), relative to the norm.  inf for a zero matrix, whose norm is exact."""
    n = x.bfloat16().double().norm().item()
    if n == 0.0:
        return math.inf
    ulp = 2.0 ** (math.floor(math.log2(n)) - 7)
    frac = (n / ulp) % 1.0
    return abs(frac - 0.5) * ulp / n


NORM_MARGIN = 2.0 ** -20


def margin_input(shape, seed: int, scale: float = 1.0, edit=None):
    """A seeded normal matrix times ``scale`` (then passed through ``edit``, if given) whose bf16 norm the fp64 reference alone
    decides: the kernel sums the squares in double in a fixed order (relative error about 2^-52 per addition) and takes an fp32 square root (2^-24), so its norm is
    within about 2^-23 of the fp64 one; an input whose fp64 norm lies at least 2^-20 from a bf16 rounding boundary rounds the same
    way in both.  The first seed from ``seed`` upwards that has the margin is used; returns (x, the seed taken)."""
    for s in range(seed, seed + 64):
        x = torch.randn(*shape, generator=torch.Generator().manual_seed(s)) * scale
        if edit is not None:
            x = edit(x)
        if norm_margin(x) >= NORM_MARGIN:
            return x, s
    raise AssertionError(f"no seed in [{seed}, {seed + 64}) puts the norm of a {shape} matrix 2^-20 away from a bf16 boundary")
