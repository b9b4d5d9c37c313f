"""What the step-geometry tests share (tests/test_gpu_step_geometry.py on the GPU, tests/test_step_restatement_host_cpu.py without one):
a dense autograd restatement of the objective on a GIVEN selection, the element-wise comparison of gradients with it, the table of
shapes -- one row per dispatch class of d_model, d_sae and top_k ("Parity": the class table) -- and the inputs of a row.

The restatement is teacher-forced: f = h * mask with the mask taken from the codes the step itself selected, so a pre-activation
pair closer than fp32 can tell apart never decides the comparison.  The AuxK selection inside it is the reference's own top-k over
the dead pre-activations; `input_conditions` asserts that fp32 and fp64 cannot disagree on either selection for a row's inputs.
The bf16 encoder's step is the same restatement with `bf16_codes=True` (tests/test_gpu_bf16_geometry.py, tests/bf16_cases.py)."""

import dataclasses

import torch

import sae_ref as R

DEAD_THR = 1000     # dead_threshold_tokens of the AuxK rows: a latent with toks = DEAD_THR that stays silent is dead, nobody else is
DEAD_BIAS = -6.0    # b_enc of the dead latents: ~5 sigma below every top-k cut of the table, and small enough to leave the dead
                    # pre-activations their fp32 resolution (an offset of -100 quantises them: fp32 and fp64 then select differently)
BOUND = 2e-5        # of each tensor's largest element (tests/test_gpu_dw_slices.py holds 16384-row sums to the same)
MAX_PREFIXES = 16


def restated_gradients(params, x, mask, dead_mask, prefixes, k_aux, alpha, dtype=torch.float64, *, bf16_codes=False):
    """loss = mean over prefixes of the rescaled MSE + AuxK, with f = h * mask (df/dh = the mask; a threshold has no gradient), in
    ``dtype``.  Returns (mse, aux, {name: gradient}).

    ``bf16_codes``: the bf16 encoder (oracle/sae_ref.py: encode_pre_bf16).  The VALUE of the h that enters f is the product of the
    bf16-rounded x and W_enc (round to nearest even) plus b_enc, evaluated in ``dtype``; its gradient stays that of the unrounded
    formula, and the AuxK term keeps the unrounded h."""
    leaves = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in params.items()}
    x = x.to(dtype)
    if dead_mask is None:
        dead_mask = torch.zeros(mask.shape[1], dtype=torch.bool)
    if prefixes is not None and not torch.is_tensor(prefixes):
        prefixes = torch.tensor([int(p) for p in prefixes], dtype=torch.int64)
    h = x @ leaves["W_enc"] + leaves["b_enc"]
    h_codes = h
    if bf16_codes:
        with torch.no_grad():
            h_bf = params["W_enc"].detach().to(torch.bfloat16).to(dtype)
            h_bf = x.to(torch.bfloat16).to(dtype) @ h_bf + leaves["b_enc"]
        h_codes = h + (h_bf - h).detach()
    f = h_codes * mask.to(dtype)
    x_hats = R.decode(f, leaves["W_dec"], leaves["b_dec"], prefixes)
    P = x_hats.shape[1]
    mse = R.mean_squared_err(x_hats, x[:, None, :].expand(-1, P, -1)).mean()
    aux = R.auxk_loss(x=x, h=h, x_hat_last=x_hats[:, -1, :], dead_mask=dead_mask, W_dec=leaves["W_dec"], b_dec=leaves["b_dec"],
                      k_aux=k_aux, alpha=alpha)
    (mse + aux).backward()
    return mse.item(), aux.item(), {k: v.grad for k, v in leaves.items()}


def assert_grads_close(got, ref64, bound, what=""):
    """Per tensor: max |got - ref64| <= bound * max |ref64| over EVERY element (no allowance for outliers, no absolute floor).  The
    failure names the tensor, the flat index and the (row, column) of the worst element.  Returns {name: worst error / max |ref64|}."""
    ratios = {}
    for name in R.PARAM_ORDER:
        g, r = got[name].detach().cpu().double(), ref64[name].detach().cpu().double()
        assert g.shape == r.shape, f"{what}{name}: shape {tuple(g.shape)} against {tuple(r.shape)}"
        scale = r.abs().max().item()
        err = (g - r).abs()
        err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)  # (a NaN is the worst element, not an ignored one)
        flat = int(err.argmax())
        worst = err.flatten()[flat].item()
        ratios[name] = worst / scale if scale > 0 else (0.0 if worst == 0 else float("inf"))
        if not worst <= bound * scale:
            cols = r.shape[1] if r.ndim == 2 else 1
            pos = (flat // cols, flat % cols) if r.ndim == 2 else (flat,)
            raise AssertionError(f"{what}{name}.grad: flat index {flat} = (row, column) {pos} of {tuple(r.shape)}: got {g.flatten()[flat].item():.9e}, "
                                 f"fp64 {r.flatten()[flat].item():.9e}, |difference| {worst:.3e} > {bound:.1e} * max|fp64| {scale:.3e} "
                                 f"(= {ratios[name]:.3e} of it)")
    return ratios


@dataclasses.dataclass(frozen=True)
class Row:
    n: int
    d: int
    s: int
    k: int
    prefixes: tuple | None = None
    n_dead: int = 0
    k_aux: int = 0
    aux_route: int = 0      # SaeEngine.aux_route() the row must report: 0 none, 2 the few-dead-latents kernels, 3 the dense algebra
    seed: int = 0           # fixed by tests/test_step_restatement_host_cpu.py: the input conditions hold at this seed
    bound: float = BOUND    # 2e-5, or 4 x the row's measured fp32-oracle error where that is larger (none is: DESIGN.md)
    spread: float = 0.0     # BTK_SHAPES: batch row b is scaled by exp(spread * N(0, 1)), so the batch-wide select leaves rows of very different lengths
    dead_bias: float = DEAD_BIAS  # b_enc of the row's dead latents
    lengths: tuple | None = None  # BTK_SHAPES: (shortest row, longest row, empty rows) of the fp64 select, fixed by tests/test_batch_topk_restatement_host_cpu.py

    @property
    def id(self) -> str:
        tail = (f"-p{len(self.prefixes)}" if self.prefixes else "") + (f"-dead{self.n_dead}of{self.k_aux}" if self.n_dead else "")
        return f"{self.n}x{self.d}x{self.s}k{self.k}{tail}"


_P16 = (1, 7, 30, 64, 65, 130, 200, 255, 256, 300, 411, 512, 640, 777, 901, 1000)

# The classes (predicate and file of each: DESIGN.md, "Parity").  Sizes are the smallest that still reach the class.
SHAPES = (
    # one row, Dp = 32 (d_model % 32 != 0: no slices, no streaming), S < 64: a single partial tile of everything
    Row(1, 20, 36, 4, seed=48),
    # k clipped to d_sae: every latent selected in every row
    Row(5, 16, 24, 64, seed=0),
    # k = 1; a 65th row (colsum block of 64 + 1); S = one 256-latent tile + 4
    Row(65, 36, 260, 1, seed=6),
    # k = 33 on the plain decode_kernel (second register half, no decode_q at this width), rows route only (d % 32 != 0)
    Row(3, 100, 1004, 33, seed=27),
    # AuxK at d % 32 != 0 (d % 128 != 0: no aux_mfma, no aux_fused): 20 dead <= AUX_SMALL_DEFAULT = 40 on the vector-ALU kernels ...
    Row(200, 100, 1004, 8, n_dead=20, k_aux=64, aux_route=2, seed=0),
    # ... and 80 dead > k_aux = 64 on the dense algebra (a selection among the dead)
    Row(200, 100, 1004, 8, n_dead=80, k_aux=64, aux_route=3, seed=0),
    # three 32-column slices; Matryoshka cuts at 1 and off every multiple of 4; plain Matryoshka decode (d < 256)
    Row(130, 96, 1000, 8, prefixes=(1, 7, 130, 1000), seed=0),
    # S = 1024 + 4: a second scan block that holds 4 latents; vector-ALU AuxK (40 dead, the most they take) with slices
    Row(130, 96, 1028, 8, n_dead=40, k_aux=64, aux_route=2, seed=0),
    # decode_q_kernel<1, 2> (33 <= k <= 64 at d = 256) plain ...
    Row(97, 256, 260, 33, seed=0),
    # ... and with prefixes, where k > 32 leaves decode_matry_q for the plain Matryoshka decode; aux_small_fused (<= 8 dead, d % 256 == 0)
    Row(97, 256, 260, 33, prefixes=(5, 260), n_dead=3, k_aux=16, aux_route=2, seed=0),
    # decode_q_kernel<2, 2>
    Row(257, 512, 1028, 64, seed=9),
    # decode_matry_q<2> at the prefix limit (MAX_PREFIXES cuts, the first = 1)
    Row(150, 512, 1000, 16, prefixes=_P16, seed=3),
    # k = 65 > 64 at a decode_q width: fused_supported false, the exact dense route, decode_kernel, no lists; aux_mfma at 65..128 dead.
    # (The issue's 70 / 64 is unreachable: the few-dead-latents route ends at min(cap, k_aux), so 70 dead of k_aux 64 go to the dense
    # algebra.  k_aux = 128 keeps the class.)
    Row(70, 1280, 516, 65, n_dead=70, k_aux=128, aux_route=2, seed=0),
    # k = 100: exact dense route
    Row(34, 768, 516, 100, seed=0),
    # NV = 6; slices without a decode-formed dval (d % 256 == 0 above 1280); aux_mfma at <= 32 dead
    Row(130, 1536, 1000, 32, n_dead=20, k_aux=64, aux_route=2, seed=0),
    # the NV = 8 templates at 7 (partly filled); d % 128 == 0 and % 256 != 0; plain Matryoshka decode
    Row(70, 1664, 516, 32, prefixes=(100, 516), seed=0),
    # NV = 8 full; dense AuxK (200 dead of k_aux 64) with prefixes
    Row(130, 2048, 1000, 32, prefixes=(100, 300, 1000), n_dead=200, k_aux=64, aux_route=3, seed=0),
    # the NV = 12 templates at 10; dense AuxK above d_model 2048 (140 dead of k_aux 128)
    Row(66, 2560, 260, 16, n_dead=140, k_aux=128, aux_route=3, seed=0),
    # the NV = 16 templates at 14
    Row(34, 3584, 516, 32, seed=0),
    # the largest ragged width, Dp = 4096.  (The issue's "VALU AuxK" is unreachable here: above d_model 2048 every dead set takes the
    # dense algebra, saev_step_dead.  The row keeps its 9 / 16 on that route -- all dead selected, d % 32 != 0 -- and the next row
    # holds the vector-ALU kernels at the largest ragged width they take.)
    Row(130, 4092, 260, 8, n_dead=9, k_aux=16, aux_route=3, seed=0),
    # vector-ALU AuxK (9 dead) at d = 2044: Dp = 2048, the NV = 8 templates ragged in their last float4
    Row(66, 2044, 260, 8, n_dead=9, k_aux=16, aux_route=2, seed=3),
    # ragged everything at once: d % 32 != 0, S = 4 x 1024 + 908, k = 64, 300 rows, dense AuxK selecting 128 of 300
    Row(300, 772, 5004, 64, n_dead=300, k_aux=128, aux_route=3, seed=12),
)


def row_inputs(row: Row):
    """(params, x, toks): the row's parameters (rand_params of tests/test_gpu_parity.py at its seed), batch and tracker; the dead
    latents carry toks = DEAD_THR and b_enc = DEAD_BIAS."""
    from test_gpu_parity import rand_params  # (plain functions of a GPU test module: importing it needs no GPU)

    p = rand_params(row.d, row.s, seed=row.seed)
    x = torch.randn(row.n, row.d, generator=torch.Generator().manual_seed(row.seed + 1))
    toks = torch.zeros(row.s, dtype=torch.int64)
    if row.n_dead:
        dead = torch.randperm(row.s, generator=torch.Generator().manual_seed(row.seed + 2))[:row.n_dead]
        toks[dead] = DEAD_THR
        p["b_enc"][dead] = DEAD_BIAS
    return p, x, toks


def input_conditions(row: Row, W_enc, b_enc, x, toks, thr=DEAD_THR):
    """Asserts what makes the fp32 and the fp64 selections of a row's inputs the same sets: on every batch row the fp64 k-th and
    (k+1)-th pre-activation lie more than 2 tol_b apart (tol_b of tests/topk_exactness.py: two fp32 evaluations differ by at most
    that), no dead latent is among the k, and for n_dead > k_aux the same gap separates the k_aux-th and (k_aux+1)-th DEAD
    pre-activation.  `thr`: the dead threshold the tracker `toks` is read against (tests/auxk_bound_cases.py has its own).
    Returns (mask of the fp64 top-k as bool, dead mask, smallest gap / tol_b of either kind)."""
    h = x.double() @ W_enc.double() + b_enc.double()
    tol = 8.0 * 2.0 ** -24 * x.double().norm(dim=1) * W_enc.double().norm(dim=0).max()
    k = min(row.k, row.s)
    top = h.topk(min(k + 1, row.s), dim=1).values
    worst = [float("inf"), float("inf")]
    if k < row.s:
        gap = (top[:, k - 1] - top[:, k]) / tol
        worst[0] = gap.min().item()
        assert worst[0] > 2.0, f"{row.id}: batch row {int(gap.argmin())}: the k-th and (k+1)-th pre-activation are {worst[0]:.2f} tol_b apart"
    mask = torch.zeros(row.n, row.s, dtype=torch.bool).scatter_(1, h.topk(k, dim=1).indices, True)
    dead = toks >= thr
    assert int(dead.sum()) == row.n_dead
    assert not mask[:, dead].any(), f"{row.id}: a dead latent is among the top-k"
    if row.n_dead > row.k_aux:
        td = h[:, dead].topk(row.k_aux + 1, dim=1).values
        gap = (td[:, row.k_aux - 1] - td[:, row.k_aux]) / tol
        worst[1] = gap.min().item()
        assert worst[1] > 2.0, f"{row.id}: batch row {int(gap.argmin())}: the k_aux-th and (k_aux+1)-th dead pre-activation are {worst[1]:.2f} tol_b apart"
    return mask, dead, worst


# ------------------------------------------------------------------------------------------------
# BatchTopK: the same step on rows of variable length (tests/test_gpu_batch_topk_geometry.py, tests/test_batch_topk_restatement_host_cpu.py)
# ------------------------------------------------------------------------------------------------

BTK_SPREAD = 0.5  # batch rows scaled by exp(0.5 N(0, 1)): the batch-wide select gives the quiet rows nothing and the loud ones hundreds of codes


def btk_default_row_cap(row: Row) -> int:
    """The slots per code row of a context created with row_cap = 0 (saev_create_batch_topk)."""
    return min(row.s, (max(64, 4 * min(row.k, row.s)) + 63) // 64 * 64)


# The classes of the BatchTopK step ("Parity": the BatchTopK class table).  A BatchTopK context sizes by row_cap what a TopK
# context sizes by top_k, and its downstream kernels are the generic ones that skip idx < 0: decode_kernel / decode_matry_kernel, the
# CSC build, gather_rows_accum, dw_rows, AuxK.  `lengths` = (shortest, longest, empty) batch rows of the fp64 select.
BTK_SHAPES = (
    # NV = 1 ragged (d_model % 32 != 0), k = 1: nearly every batch row is empty; S = one 256-latent tile + 4
    Row(65, 36, 260, 1, seed=0, spread=BTK_SPREAD, lengths=(0, 25, 53)),
    # NV = 1 ragged, S off every tile, vector-ALU AuxK (20 dead <= 40) over rows with idx = -1 slots
    Row(200, 100, 1004, 8, n_dead=20, k_aux=64, aux_route=2, seed=0, spread=BTK_SPREAD, lengths=(0, 175, 123)),
    # Matryoshka cuts at 1 and off every multiple of 4 over variable rows, d_model < 256: an empty row, and a row with no code below 7
    Row(130, 96, 1000, 8, prefixes=(1, 7, 130, 1000), seed=0, spread=BTK_SPREAD, lengths=(0, 141, 79)),
    # NV = 2; S = 1024 + 4: a second CSC scan block that holds 4 latents
    Row(257, 512, 1028, 16, seed=1, spread=BTK_SPREAD, lengths=(0, 307, 124)),
    # NV = 6 with the few-dead-latents AuxK route it takes (20 dead of k_aux 64)
    Row(130, 1536, 1000, 32, n_dead=20, k_aux=64, aux_route=2, seed=3, dead_bias=-12.0, spread=BTK_SPREAD, lengths=(0, 290, 30)),
    # the NV = 8 templates at 7, two prefixes
    Row(70, 1664, 516, 32, prefixes=(100, 516), seed=0, spread=BTK_SPREAD, lengths=(0, 147, 14)),
    # NV = 8 full; dense AuxK (200 dead of k_aux 64) with three prefixes
    Row(130, 2048, 1000, 32, prefixes=(100, 300, 1000), n_dead=200, k_aux=64, aux_route=3, seed=7, dead_bias=-12.0, spread=BTK_SPREAD, lengths=(0, 201, 32)),
    # the NV = 12 templates at 10; dense AuxK (140 dead of k_aux 128)
    Row(66, 2560, 260, 16, n_dead=140, k_aux=128, aux_route=3, seed=7, dead_bias=-12.0, spread=BTK_SPREAD, lengths=(0, 46, 5)),
    # NV = 16 ragged in its last float4
    Row(130, 4092, 260, 8, seed=2, spread=BTK_SPREAD, lengths=(0, 72, 55)),
    # ragged everything, rows past 1024 codes (a 17th 64-slot chunk of a row), dense AuxK selecting 128 of 300
    Row(300, 772, 5004, 64, n_dead=300, k_aux=128, aux_route=3, seed=54, dead_bias=-12.0, spread=BTK_SPREAD, lengths=(0, 1086, 135)),
    # top_k >= d_sae: every entry kept, row_cap == d_sae, no padding anywhere
    Row(5, 16, 24, 64, seed=0, spread=BTK_SPREAD, lengths=(24, 24, 0)),
    # one row only: the batch-wide select is that row's top-k
    Row(1, 20, 36, 4, seed=0, spread=BTK_SPREAD, lengths=(4, 4, 0)),
    # MAX_PREFIXES cuts (the first = 1) on variable rows
    Row(150, 512, 1000, 16, prefixes=_P16, seed=0, spread=BTK_SPREAD, lengths=(0, 185, 54)),
    # aux_small_fused (<= 8 dead, d_model % 256 == 0) on variable rows
    Row(97, 256, 260, 16, n_dead=3, k_aux=16, aux_route=2, seed=0, spread=BTK_SPREAD, lengths=(0, 69, 22)),
)


def btk_row_inputs(row: Row):
    """(params, x, toks) of a BTK_SHAPES row: row_inputs with every batch row scaled by exp(row.spread * N(0, 1))."""
    from test_gpu_parity import rand_params

    p = rand_params(row.d, row.s, seed=row.seed)
    g = torch.Generator().manual_seed(row.seed + 1)
    x = torch.randn(row.n, row.d, generator=g)
    x = x * torch.exp(row.spread * torch.randn(row.n, 1, generator=g))
    toks = torch.zeros(row.s, dtype=torch.int64)
    if row.n_dead:
        dead = torch.randperm(row.s, generator=torch.Generator().manual_seed(row.seed + 2))[:row.n_dead]
        toks[dead] = DEAD_THR
        p["b_enc"][dead] = row.dead_bias
    return p, x, toks


def btk_tol(x, W_enc) -> float:
    """tol_b of tests/topk_exactness.py at the batch's largest row: two fp32 evaluations of any pre-activation of the batch differ by
    at most 2 of it."""
    return float(8.0 * 2.0 ** -24 * x.double().norm(dim=1).max() * W_enc.double().norm(dim=0).max())


def btk_input_conditions(row: Row, W_enc, b_enc, x, toks):
    """Asserts what makes the fp32 and the fp64 BATCH-WIDE selections of a row's inputs the same set: the fp64 (n k)-th and
    (n k + 1)-th largest pre-activation of the whole batch lie more than 2 tol_b apart (tol_b at the batch's largest row), no dead
    latent is selected, and for n_dead > k_aux the per-row gap of `input_conditions` between the k_aux-th and (k_aux+1)-th DEAD
    pre-activation.  Returns (mask of the fp64 batch top-(n k) as bool, dead mask, [cut gap / tol_b, smallest dead gap / tol_b])."""
    h = x.double() @ W_enc.double() + b_enc.double()
    tol_b = btk_tol(x, W_enc)
    t = row.n * min(row.k, row.s)
    worst = [float("inf"), float("inf")]
    if t < h.numel():
        top = h.flatten().topk(t + 1).values
        worst[0] = ((top[t - 1] - top[t]) / tol_b).item()
        assert worst[0] > 2.0, f"{row.id}: the (n k)-th and (n k + 1)-th pre-activation of the batch are {worst[0]:.2f} tol_b apart"
        mask = h >= top[t - 1]
    else:
        mask = torch.ones_like(h, dtype=torch.bool)
    assert int(mask.sum()) == t
    dead = toks >= DEAD_THR
    assert int(dead.sum()) == row.n_dead
    assert not mask[:, dead].any(), f"{row.id}: a dead latent is selected"
    if row.n_dead > row.k_aux:
        tol = 8.0 * 2.0 ** -24 * x.double().norm(dim=1) * W_enc.double().norm(dim=0).max()
        td = h[:, dead].topk(row.k_aux + 1, dim=1).values
        gap = (td[:, row.k_aux - 1] - td[:, row.k_aux]) / tol
        worst[1] = gap.min().item()
        assert worst[1] > 2.0, f"{row.id}: batch row {int(gap.argmin())}: the k_aux-th and (k_aux+1)-th dead pre-activation are {worst[1]:.2f} tol_b apart"
    return mask, dead, worst
