"""What the ReLU geometry and scale tests share (tests/test_gpu_relu_geometry.py and tests/test_gpu_relu_train_scale.py on the GPU,
tests/test_relu_cases_host_cpu.py without one): the forward geometry table, a planted batch whose every entry is known exactly, the
hand-built rows and prefix lists of the decode test, and the scale cases of the dense train step.

Planted batch.  d_model = 4, b_enc = 0, row c of W_enc a +-1 pattern P_c over the latents, batch row b = a_b * e_c(b) with a_b > 0
distinct per row: h[b, s] = +-a_b exactly in fp32 (three products are +-0, one is +-a_b), so row b's entries are the +1 latents of
its pattern, ascending, each with the value a_b bit for bit.  No tolerance band: idx, val and row_nnz are compared with equality.

Scale cases.  A base row of tests/relu_step_restatement.py: RELU_SHAPES with one of: every activation-side quantity (x, b_enc,
b_dec) times a power of two; one channel of x times 300 with its W_enc row divided by 300; an encoder bias under which no latent
fires; that and x = b_dec, so that the residual is exactly zero too.  Bounds: BOUND = 2e-5 of tests/step_restatement.py, the fp32
torch restatement of every case being held to a quarter of it in tests/test_relu_cases_host_cpu.py (worst measured there: 5.6e-7
per tensor, 1.2e-6 row by row, both at 257x512x516)."""

import dataclasses

import torch

from relu_step_restatement import L1_COEFF, RELU_SHAPES, SILENT_BIAS, ReluRow, relu_bound, relu_row_inputs
from step_restatement import BOUND

# ------------------------------------------------------------------------------------------------
# forward geometry: relu_encode_kernel's tiles of 32 rows x 128 latents x 16 d_model columns, relu_decode_kernel's four float4 trips
# ------------------------------------------------------------------------------------------------

FORWARD_SHAPES = (
    (1, 4, 4),         # the smallest of everything: one row, one float4 of d_model, one float4 of latents
    (31, 20, 36),      # one short row tile; d_model not a multiple of 16 (a second stage that holds one float4); d_sae under one tile
    (70, 16, 124),     # the last float4 of the only latent tile is missing; a third row tile of 6 rows
    (32, 48, 128),     # every tile exactly full: 32 rows, three whole stages, one whole latent tile
    (33, 36, 132),     # the 33rd row opens a second workgroup; the second latent tile holds one float4
    (65, 100, 1004),   # eight latent tiles; row counts near the default capacity of 512
    (34, 4092, 516),   # the widest ragged d_model: the decode's fourth trip ends one float4 short
    (40, 4096, 260),   # the widest d_model: all four trips of every decode thread
)


def forward_inputs(n, d, s, seed=0):
    """(params, x): rand_params of tests/test_gpu_parity.py and a standard normal batch, as the other tables use."""
    from test_gpu_parity import rand_params  # (plain functions of a GPU test module: importing it needs no GPU)

    return rand_params(d, s, seed=seed), torch.randn(n, d, generator=torch.Generator().manual_seed(seed + 1))


# ------------------------------------------------------------------------------------------------
# the planted batch
# ------------------------------------------------------------------------------------------------

PLANTED = ((260, 37), (1004, 131))  # (d_sae, cap): three and eight latent tiles; odd capacities (rows of idx / val at odd offsets)


def planted_patterns(S: int, cap: int) -> torch.Tensor:
    """(4, S) of +-1.  P0: no positive.  P1: exactly cap positives, none at latent 0, the last three at S - 3 .. S - 1 (columns 1 .. 3
    of the float4 of the LAST thread of the last tile: 4t + 1 .. 4t + 3 with 4t = S - 4), the others spread over every tile.
    P2: P1 and latent 0, cap + 1 positives: at a capacity of cap the cut falls between columns 2 and 3 of that thread.  P3: all S."""
    assert S % 4 == 0 and 4 <= cap <= S - 5
    P = -torch.ones(4, S)
    spread = 1 + (torch.arange(cap - 3) * (S - 5)) // (cap - 3)  # cap - 3 distinct latents of [1, S - 4)
    P[1, spread] = 1.0
    P[1, S - 3:] = 1.0
    P[2] = P[1]
    P[2, 0] = 1.0
    P[3] = 1.0
    return P


def planted_batch(S: int, cap: int, rows):
    """``rows``: the pattern number (0 .. 3) of each batch row.  Returns (params, x, want) with want = [(latents, a_b) per row]."""
    P = planted_patterns(S, cap)
    g = torch.Generator().manual_seed(S + cap)
    W_dec = torch.randn(S, 4, generator=g)
    params = {"W_enc": P.clone(), "b_enc": torch.zeros(S), "W_dec": W_dec / W_dec.norm(dim=1, keepdim=True), "b_dec": torch.zeros(4)}
    n = len(rows)
    a = 1.0 + torch.arange(n, dtype=torch.float32) / 64.0  # distinct, exact in fp32
    x = torch.zeros(n, 4)
    x[torch.arange(n), torch.tensor(rows)] = a
    want = [(torch.nonzero(P[c] > 0)[:, 0].to(torch.int32), float(a[b])) for b, c in enumerate(rows)]
    return params, x, want


def assert_planted_rows(idx, val, nnz, want, what=""):
    """Equality of every row with what was planted: the count, the latents in order, the value in every live slot."""
    idx, val, nnz = idx.cpu(), val.cpu(), nnz.cpu()
    assert idx.shape == val.shape and idx.shape[0] == len(want) == nnz.shape[0]
    for b, (lat, a) in enumerate(want):
        k = lat.numel()
        assert int(nnz[b]) == k, f"{what}row {b}: row_nnz {int(nnz[b])}, planted {k}"
        assert k <= idx.shape[1], f"{what}row {b}: {k} entries in rows of {idx.shape[1]}"
        assert torch.equal(idx[b, :k], lat), f"{what}row {b}: latents differ from the planted ones"
        assert torch.equal(val[b, :k], torch.full((k,), a)), f"{what}row {b}: a value is not a_b = {a}"


# ------------------------------------------------------------------------------------------------
# hand-built rows for relu_decode_kernel
# ------------------------------------------------------------------------------------------------

DECODE_D = (4, 20, 1028, 4092, 4096)  # one float4; under one trip; a second trip of one float4; the fourth trip ragged, and whole
DECODE_S, DECODE_CAP = 516, 40
# every inner cut is an entry's latent (100, 200, 476: the entry belongs to the LATER prefix only) or one above an entry (1 above
# latent 0, 100 above 99, 200 above 199, 516 above 515); the sixteen use every prefix slot of the kernel's argument block
DECODE_PREFIXES = (None, (1, 516), (100, 200, 516), (100, 476, 516),
                   (1, 2, 3, 4, 40, 99, 100, 101, 199, 200, 201, 300, 476, 477, 515, 516))


def decode_rows_case(seed=21):
    """(idx, val, nnz) on the CPU: padding index out of range, padding value NaN (neither may be read).  Row counts 0, 1 and cap;
    rows wholly below 100 (all their prefixes of a list that starts at >= 100 are equal), wholly at or past 476 (their prefixes cut
    at <= 476 equal b_dec exactly), and entries on and next to every cut of DECODE_PREFIXES."""
    S, cap = DECODE_S, DECODE_CAP
    g = torch.Generator().manual_seed(seed)
    rows = [[], [0], [S - 1], [100], [1],
            torch.randperm(S, generator=g)[:cap].sort().values.tolist(),
            list(range(cap)),                    # all below 100, and 0, 1, 2, 3 next to the smallest cuts
            list(range(S - cap, S)),             # all at or past 476 = S - cap
            [99, 100, 101, 199, 200, 300, 515],
            [0, 99, 199, 475, 476, 477]]
    for k in (2, 17, cap - 1):
        rows.append(torch.randperm(S, generator=g)[:k].sort().values.tolist())
    n = len(rows)
    idx = torch.full((n, cap), S + 1000, dtype=torch.int32)
    val = torch.full((n, cap), float("nan"))
    nnz = torch.tensor([len(r) for r in rows], dtype=torch.int32)
    for r, lat in enumerate(rows):
        idx[r, : len(lat)] = torch.tensor(lat, dtype=torch.int32)
        val[r, : len(lat)] = 0.25 + torch.rand(len(lat), generator=g) * 2
    return idx, val, nnz


# ------------------------------------------------------------------------------------------------
# the dense train step away from unit scale
# ------------------------------------------------------------------------------------------------

SCALE_BASES = tuple(r for r in RELU_SHAPES if r.id in ("65x36x260-extremes", "257x512x516"))
MASSIVE_CHANNEL, MASSIVE_FACTOR = 3, 300.0
BAND_SHARE = 0.01  # massive channel: at most this share of the pre-activations within two fp32 bounds of zero


@dataclasses.dataclass(frozen=True)
class ScaleCase:
    base: ReluRow
    kind: str             # "scale" | "massive" | "silent" | "zero_residual"
    log2: int = 0         # "scale": x, b_enc and b_dec are multiplied by 2^log2
    # 2e-5, or 4 x the case's measured fp32-restatement error where that exceeds a quarter of it (none does:
    # tests/test_relu_cases_host_cpu.py::test_fp32_restatement_of_every_scale_case measures each against fp64)
    bound: float = BOUND

    @property
    def id(self) -> str:
        return f"{self.base.id}-{self.kind}" + (f"{self.log2:+d}" if self.kind == "scale" else "")

    @property
    def l1_coeff(self) -> float:
        return 0.0 if self.kind == "zero_residual" else L1_COEFF


SCALE_CASES = tuple(ScaleCase(b, "scale", log2=e) for b in SCALE_BASES for e in (18, -20)) \
    + tuple(ScaleCase(b, kind) for b in SCALE_BASES for kind in ("massive", "silent", "zero_residual"))


def scale_case_inputs(case: ScaleCase):
    """(params, x) of a case.  "scale": powers of two leave every pre-activation's distance from zero unchanged in units of the
    bound.  "massive": h is the base row's up to the rounding of W_enc[3] / 300.  "silent": b_enc = 3 * SILENT_BIAS on every latent
    (the largest fp64 pre-activation is -13.0 at these shapes: nothing fires).  "zero_residual": the silent parameters and x = b_dec on every row, so
    x_hat = b_dec = x."""
    p, x = relu_row_inputs(case.base)
    if case.kind == "scale":
        c = 2.0 ** case.log2
        p["b_enc"], p["b_dec"], x = p["b_enc"] * c, p["b_dec"] * c, x * c
    elif case.kind == "massive":
        x[:, MASSIVE_CHANNEL] *= MASSIVE_FACTOR
        p["W_enc"][MASSIVE_CHANNEL] /= MASSIVE_FACTOR
    elif case.kind in ("silent", "zero_residual"):
        p["b_enc"] = torch.full_like(p["b_enc"], 3 * SILENT_BIAS)
        if case.kind == "zero_residual":
            x = p["b_dec"][None, :].repeat(case.base.n, 1)
    else:
        raise ValueError(case.kind)
    return p, x


def band_of(p, x):
    """(fp64 pre-activations, the mask of those within two fp32 bounds of zero)"""
    h = x.double() @ p["W_enc"].double() + p["b_enc"].double()
    return h, h.abs() <= 2 * relu_bound(x, p["W_enc"], p["b_enc"])


def assert_rows_close(got, ref64, bound, what=""):
    """A (d_model, d_sae) gradient ROW BY ROW: every d_model row against that row's own largest fp64 element.  (A bound relative to
    the whole tensor would let one massive row hide every other.)  Returns the worst row's error / its max |fp64|."""
    g, r = got.detach().cpu().double(), ref64.detach().cpu().double()
    assert g.shape == r.shape and r.ndim == 2
    err = (g - r).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err).amax(dim=1)
    scale = r.abs().amax(dim=1)
    bad = ~(err <= bound * scale)
    ratio = torch.where(scale > 0, err / scale.clamp_min(1e-300), torch.where(err == 0, 0.0, float("inf")))
    if bad.any():
        j = int(torch.nonzero(bad)[0])
        raise AssertionError(f"{what}row {j} of {tuple(r.shape)}: |difference| {err[j].item():.3e} > {bound:.1e} * the row's max|fp64| "
                             f"{scale[j].item():.3e} (= {ratio[j].item():.3e} of it); {int(bad.sum())} rows off")
    return float(ratio.max())
