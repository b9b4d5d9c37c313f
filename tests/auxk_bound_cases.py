"""AuxK with the dead count left on the device (tests/test_gpu_auxk_bound.py on the GPU, tests/test_auxk_bound_cases_host_cpu.py
without one): the scenario that makes saev_step_dead size a step's auxiliary work by a BOUND above the true count, its fp64 replay,
the dispatch the library's constants give that bound, and the table of rows -- one per (bound, count) class ("Parity":
the AuxK bound table).

The scenario.  thr = 100 n.  D dead latents carry toks = thr and b_enc = DEAD_BIAS: silent on every batch, dead on every step.  Sl
"sleepy" latents carry toks = thr - 4 n, b_enc = DEAD_BIAS and W_enc[0, sleepy] = WAKE_WEIGHT: silent while x[:, 0] = 0, firing (by ~200) in
the one "wake" batch with x[:, 0] = 1.  The warm-up steps run at learning rate 0.  The record of step i counts a latent as near when
toks >= thr - 4 n after that step's update (saev_amd/csrc/kernels.h: DeadRecord, tail.hip: dead_update_body), and step i + 4 is
sized by it.

  variant A (fresh buffers): wake on step 3, measure step 5.  Record 1 counts dead + sleepy (toks = thr - 3 n): bound D + Sl, count
      D; steps 1-4 read back a count of D, so the compact buffers never held more than D rows.
  variant B (stale buffers): wake on step 5, measure step 6.  The sleepy latents die on step 4 (toks = thr, a read-back step of
      count D + Sl: the compact buffers, dWd / dWe / dbe hold D + Sl rows), fire in step 5's forward, and step 6 is sized by record
      2 (toks = thr - 2 n): bound D + Sl, count D, rows past D stale."""

import dataclasses
import functools

import torch

from step_restatement import DEAD_BIAS, input_conditions

# ---- the library's constants, restated (tests/test_auxk_bound_cases_host_cpu.py derives every row's claim from them) ------------
DEAD_LAG = 4              # saev_amd/csrc/ctx.h: steps between a tracker record and the step it sizes
AUX_SMALL_MAX = 64        # saev_amd/csrc/kernels.h: row pitch of the few-dead-latents kernels' compact buffers
AUX_SMALL_DEFAULT = 40    # kernels.h: the vector-ALU kernels' largest dead set (d_model % 128 != 0)
AUX_FUSED_MAX = 8         # kernels.h: the one-pass kernel's largest dead set (a bound <= 4 takes its four-latent variant)
AUX_MFMA_MAX = 128        # kernels.h: the fp32-MFMA kernels' largest dead set; count windows [1, 32], [33, 64], [65, 128]
AUX_SMALL_D_MAX = 2048    # saev_amd/csrc/ctx_auxk.hip, saev_step_dead: above this d_model every dead set takes the dense algebra

# The issue's 300 is unreachable: the f16x3 encoder and, in EVERY encoder mode, the dense AuxK algebra split W_enc into fp16 halves
# at a fixed scale of 256 ("Limits": |W_enc| < 255), so a sleepy latent that dies (variant B, step 4) or meets the f16x3
# encoder turns the step into NaN at 300.  250 is the nearest weight inside the limit (250 * 256 = 64 000, an fp16 number); the
# sleepy latents still fire with a margin above 200.
WAKE_WEIGHT = 250.0
VARIANTS = {"A": (3, 5), "B": (5, 6)}  # variant -> (wake step, measured step), 1-based


def aux_fused_supported(d):  # saev_amd/csrc/auxk.hip
    return d % 256 == 0 and 256 <= d <= 1024


def aux_mfma_supported(d):  # saev_amd/csrc/auxk.hip
    return d % 128 == 0 and d >= 128


def dead_cap(s, k_aux):
    """Dead latents the dense buffers of a context created with aux_dead_cap = 0 hold (saev_amd/csrc/ctx.hip)."""
    return min((max(4096, 8 * k_aux) + 3) // 4 * 4, (s + 3) // 4 * 4)


def dispatch(d, s, k_aux, bound):
    """What saev_step_dead enqueues for a step whose record gives `bound` (ctx_auxk.hip: saev_step_dead, auxk_small_forward,
    auxk_forward), default debug switches: {"route": SaeEngine.aux_route(), "family": ..., and the family's own geometry}."""
    cap = dead_cap(s, k_aux)
    mfma_cap = AUX_MFMA_MAX if aux_mfma_supported(d) and max(cap, AUX_SMALL_MAX) >= AUX_MFMA_MAX else AUX_SMALL_MAX  # alloc_aux_buffers
    small_cap = max(AUX_SMALL_MAX, mfma_cap) if aux_mfma_supported(d) else AUX_SMALL_DEFAULT
    small_max = min(small_cap, k_aux)
    if bound == 0:
        return {"route": 0, "family": "none"}
    if bound <= small_max and d <= AUX_SMALL_D_MAX:
        if bound <= AUX_FUSED_MAX and aux_fused_supported(d):
            return {"route": 1, "family": "fused", "latents": 4 if bound <= 4 else AUX_FUSED_MAX}
        if bound <= mfma_cap and aux_mfma_supported(d):
            return {"route": 1, "family": "mfma", "windows": 1 + (bound > 32) + (bound > 64), "pitch": AUX_MFMA_MAX if bound > AUX_SMALL_MAX else AUX_SMALL_MAX}
        return {"route": 1, "family": "valu", "cap": small_max}
    ndp = (bound + 3) // 4 * 4
    assert ndp <= cap, "the dense buffers would have to grow: a read-back"
    ku = min(k_aux, bound)
    return {"route": 3, "family": "dense", "ndp": ndp, "ku": ku, "aux_all": ku == bound}


@dataclasses.dataclass(frozen=True)
class Case:
    n: int
    d: int
    s: int
    k: int
    k_aux: int
    n_dead: int             # D: the count of the measured step
    n_sleepy: int           # Sl: bound - count
    claim: tuple            # sorted items of what dispatch() must return for the bound D + Sl
    stale: bool = False     # runs in variant B as well (and in the fused-entry test)
    seed: int = 0           # fixed by tests/test_auxk_bound_cases_host_cpu.py: the scenario's conditions hold at this seed
    prefixes = None         # (input_conditions and restated_gradients take a Row: no Matryoshka here)

    @property
    def bound(self) -> int:
        return self.n_dead + self.n_sleepy

    @property
    def thr(self) -> int:
        return 100 * self.n

    @property
    def id(self) -> str:
        return f"{self.n}x{self.d}x{self.s}k{self.k}-aux{self.k_aux}-{self.n_dead}+{self.n_sleepy}"

    @property
    def variants(self) -> tuple:
        return ("A", "B") if self.stale else ("A",)


def _c(**kw):
    return tuple(sorted(kw.items()))


_VALU = (130, 100, 1004, 8)
_MFMA = (97, 128, 516, 8, 128)
_FUSED = (97, 256, 260, 8, 16)

# Sizes are the smallest that still reach the class; every row's numbers as the issue states them (only the wake weight had to move).
CASES = (
    # ---- vector-ALU kernels (d % 128 != 0; cap min(AUX_SMALL_DEFAULT, k_aux)) ----
    # route 1 at the cap of 40
    Case(*_VALU, 64, 20, 20, _c(route=1, family="valu", cap=40), seed=1),
    # route 1 with nothing dead: every kernel leaves at once, 40 stale rows in variant B
    Case(*_VALU, 64, 0, 40, _c(route=1, family="valu", cap=40), stale=True, seed=1),
    # route 1 at the NV = 8 templates, ragged in their last float4 (cap = k_aux = 16)
    Case(66, 2044, 260, 8, 16, 9, 7, _c(route=1, family="valu", cap=16), seed=0),
    # ---- dense algebra sized by the bound (no read-back) ----
    # bound 41 > 40: every column selected (ku = bound), ndp 44: 21 + 3 padding columns with bias 0
    Case(*_VALU, 64, 20, 21, _c(route=3, family="dense", ndp=44, ku=41, aux_all=True), seed=1),
    # select mode with ku_dev = 10 below the host's ku = 16
    Case(*_VALU, 16, 10, 30, _c(route=3, family="dense", ndp=40, ku=16, aux_all=False), stale=True, seed=1),
    # a real selection: 16 among 30 dead and 50 padding columns with bias -inf
    Case(*_VALU, 16, 30, 50, _c(route=3, family="dense", ndp=80, ku=16, aux_all=False), seed=0),
    # bound 129 > AUX_MFMA_MAX at an MFMA width: ndp 132, ku 128 of 129, ku_dev = 20
    Case(*_MFMA, 20, 109, _c(route=3, family="dense", ndp=132, ku=128, aux_all=False), seed=0),
    # above d_model 2048 every dead set is dense
    Case(34, 2560, 260, 8, 16, 5, 3, _c(route=3, family="dense", ndp=8, ku=8, aux_all=True), seed=0),
    # ---- fp32-MFMA kernels: the count in a lower window than the bound ----
    # two windows enqueued, the first runs
    Case(*_MFMA, 32, 1, _c(route=1, family="mfma", windows=2, pitch=64), seed=0),
    # three windows, the second runs at its first count, pitch 128
    Case(*_MFMA, 33, 67, _c(route=1, family="mfma", windows=3, pitch=128), stale=True, seed=0),
    # pitch 128 with a count <= 64
    Case(*_MFMA, 64, 1, _c(route=1, family="mfma", windows=3, pitch=128), seed=0),
    # the second 64-latent weight-gradient block holds one latent
    Case(*_MFMA, 65, 63, _c(route=1, family="mfma", windows=3, pitch=128), stale=True, seed=0),
    Case(*_MFMA, 1, 127, _c(route=1, family="mfma", windows=3, pitch=128), seed=1),
    Case(*_MFMA, 0, 128, _c(route=1, family="mfma", windows=3, pitch=128), stale=True, seed=1),
    # ---- one-pass kernel (d % 256 == 0, d <= 1024, bound <= 8) ----
    Case(*_FUSED, 3, 1, _c(route=1, family="fused", latents=4), seed=0),
    Case(*_FUSED, 4, 4, _c(route=1, family="fused", latents=8), stale=True, seed=0),
    Case(*_FUSED, 0, 8, _c(route=1, family="fused", latents=8), seed=0),
    # bound 9 leaves it for MFMA window 1
    Case(*_FUSED, 8, 1, _c(route=1, family="mfma", windows=1, pitch=64), seed=0),
    # NW = 4, 64 KB of LDS
    Case(34, 1024, 260, 8, 16, 5, 3, _c(route=1, family="fused", latents=8), seed=0),
)

DENSE_CASES = tuple(c for c in CASES if dict(c.claim)["family"] == "dense")
SMALL_CASES = tuple(c for c in CASES if dict(c.claim)["family"] != "dense")
STALE_CASES = tuple(c for c in CASES if c.stale)


def scenario(case: Case, variant: str):
    """(params, toks, batches, dead, sleepy): rand_params of tests/test_gpu_parity.py at the row's seed with the planted latents,
    the tracker to set before step 1, and the batches of steps 1 .. measured (the last one is the measured step's)."""
    from test_gpu_parity import rand_params  # (plain functions of a GPU test module: importing it needs no GPU)

    wake, measured = VARIANTS[variant]
    p = rand_params(case.d, case.s, seed=case.seed)
    perm = torch.randperm(case.s, generator=torch.Generator().manual_seed(case.seed + 2))
    dead, sleepy = perm[:case.n_dead], perm[case.n_dead:case.bound]
    p["b_enc"][dead] = DEAD_BIAS
    p["b_enc"][sleepy] = DEAD_BIAS
    p["W_enc"][0, sleepy] = WAKE_WEIGHT
    toks = torch.zeros(case.s, dtype=torch.int64)
    toks[dead] = case.thr
    toks[sleepy] = case.thr - DEAD_LAG * case.n
    g = torch.Generator().manual_seed(case.seed + 1)
    xs = []
    for step in range(1, measured + 1):
        x = torch.randn(case.n, case.d, generator=g)
        x[:, 0] = 1.0 if step == wake else 0.0
        xs.append(x)
    return p, toks, xs, dead, sleepy


@dataclasses.dataclass
class Step:
    mask: torch.Tensor       # (n, s) bool: the fp64 top-k
    toks: torch.Tensor       # the tracker after this step's update
    dead: torch.Tensor       # (s) bool: toks >= thr after the update
    n_near: int              # DeadRecord.n_near: toks >= thr - DEAD_LAG n after the update
    undecided: int           # latents whose firing fp32 rounding could change (see fired_bounds)


def fired_bounds(h, x, W, k):
    """(surely fired, possibly fired) as (s) bool.  Two fp32 evaluations of h[r, j] differ by at most t = 8 * 2^-24 |x_r| |w_j|
    (tol_b of tests/topk_exactness.py with the latent's own norm), so latent j is in EVERY fp32 top-k of row r when fewer than k
    others can reach h[r, j] - t, and in NONE when k others surely exceed h[r, j] + t.  Where the two sets are equal the fired
    set -- and with it the tracker -- is the same for every encoder."""
    t = 8.0 * 2.0 ** -24 * x.norm(dim=1, keepdim=True) * W.norm(dim=0, keepdim=True)
    lo, hi = h - t, h + t
    s = h.shape[1]
    n_reach = s - torch.searchsorted(hi.sort(dim=1).values, lo.contiguous(), right=False)   # others with hi >= lo[r, j], and j itself
    n_above = s - torch.searchsorted(lo.sort(dim=1).values, hi.contiguous(), right=True)    # others with lo > hi[r, j]
    return (n_reach <= k).any(dim=0), (n_above < k).any(dim=0)


def effective_w_enc(W_enc, x):
    """W_enc as a batch sees it: where x[:, 0] = 0 exactly, row 0 (the wake weights) adds exact zeros to every pre-activation and
    no rounding error, so the selection's fp32 tolerance is that of the matrix without it."""
    if bool((x[:, 0] == 0).all()):
        W_enc = W_enc.clone()
        W_enc[0] = 0
    return W_enc


@functools.lru_cache(maxsize=None)
def replay(case: Case, variant: str):
    """The scenario in fp64, step by step: [Step] for steps 1 .. measured."""
    p, toks, xs, _, _ = scenario(case, variant)
    b = p["b_enc"].double()
    toks = toks.clone()
    k = min(case.k, case.s)
    steps = []
    for x in xs:
        x = x.double()
        W = effective_w_enc(p["W_enc"], x).double()
        h = x @ W + b
        mask = torch.zeros(case.n, case.s, dtype=torch.bool).scatter_(1, h.topk(k, dim=1).indices, True)
        sure, maybe = fired_bounds(h, x, W, k)
        fired = mask.any(dim=0)
        assert bool((sure <= fired).all()) and bool((fired <= maybe).all())
        toks = torch.where(fired, 0, toks + case.n)
        steps.append(Step(mask, toks.clone(), toks >= case.thr, int((toks >= case.thr - DEAD_LAG * case.n).sum()), int((sure != maybe).sum())))
    return steps


def measured_conditions(case: Case, variant: str):
    """input_conditions on the measured step (tracker as it stands BEFORE that step: the dead are the planted D).  Returns its
    (mask, dead mask, gap ratios)."""
    p, _, xs, _, _ = scenario(case, variant)
    steps = replay(case, variant)
    return input_conditions(case, effective_w_enc(p["W_enc"], xs[-1]), p["b_enc"], xs[-1], steps[-2].toks, thr=case.thr)
