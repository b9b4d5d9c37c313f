"""CPU-only tests of the interventions' geometry cases (tests/interventions_cases.py): every ``holds`` against the restatement, the
vectorised restatements against the entry-by-entry ones that define them, and the constants the cases are built from against the
text of saev_amd/csrc/intervene.hip -- a retune must fail here and not move the cases off their edges without a word."""

import re

import numpy as np
import pytest

import interventions_cases as IC
import interventions_restatement as IR
from conftest import ROOT

HIP = (ROOT / "saev_amd" / "csrc" / "intervene.hip").read_text()


def _constexpr(name: str, text: str = HIP) -> int:
    m = re.search(r"constexpr\s+int\s+" + name + r"\s*=\s*(\d+)\s*;", text)
    assert m, f"{name} is not a constexpr int"
    return int(m.group(1))


def _kernel(name: str) -> str:
    """The text of a __global__ function, from its launch bounds to the line that closes it."""
    m = re.search(r"__global__\s+__launch_bounds__\(([^)]*)\)\s+void\s+" + name + r"\(.*?\n}\n", HIP, flags=re.S)
    assert m, name
    return m.group(0)


def test_constants_are_the_kernels():
    for name in ("IV_WAVES", "IV_TRIPS", "IV_MAX_GRID", "IV_MAX_LIST", "IV_CNT_SLOTS", "IV_MAX_EDITS", "IV_MAX_GROUPS", "CF_CODES_MAX_GRID",
                 "CF_ROWS_MAX_GRID", "CF_F1_MAX_GRID"):
        assert _constexpr(name) == getattr(IC, name), name
    assert _constexpr("ENTRY_MAX_C", (ROOT / "saev_amd" / "csrc" / "entry_util.h").read_text()) == IC.ENTRY_MAX_C
    # a pass of a wave over D, the row stride and the grid of the edit kernel, as the cases assume them
    assert "q0 += 64 * IV_TRIPS" in HIP and "const int q = q0 + 64 * u;" in HIP
    rows = _kernel("iv_rows_kernel")
    assert "__launch_bounds__(IV_WAVES * 64)" in rows
    assert "for (long b = (long)blockIdx.x * IV_WAVES + w; b < a.n; b += (long)gridDim.x * IV_WAVES)" in rows
    assert "slot = p & (IV_CNT_SLOTS - 1)" in rows
    assert "std::min<int64_t>((n_rows + IV_WAVES - 1) / IV_WAVES, IV_MAX_GRID)" in HIP
    # the three firing kernels: 256 threads, a grid-stride loop, the named cap in the launch
    for kernel, cap, count in (("cf_codes_kernel", "CF_CODES_MAX_GRID", "total"), ("cf_rows_kernel", "CF_ROWS_MAX_GRID", "n_rows"),
                               ("cf_f1_kernel", "CF_F1_MAX_GRID", "total")):
        text = _kernel(kernel)
        assert f"__launch_bounds__({IC.CF_THREADS})" in text
        assert re.search(rf"\(long\)blockIdx\.x \* {IC.CF_THREADS} \+ threadIdx\.x; \w+ < \w+; \w+ \+= \(long\)gridDim\.x \* {IC.CF_THREADS}\)", text), kernel
        assert re.search(rf"hipLaunchKernelGGL\({kernel}, dim3\(\(unsigned\)std::min<int64_t>\(\({count} \+ 255\) / 256, {cap}\)\), dim3\(256\)", HIP), kernel
    assert (IC.GRID_ROWS, IC.CODES_SPAN, IC.ROWS_SPAN, IC.F1_SPAN) == (8192, 8192 * 256, 1024 * 256, 8192 * 256)


def test_the_float4_route_asks_for_the_alignment_of_all_three_tensors():
    """Whether a 16-byte access one float off its alignment is tolerated, wrong or a fault is the device's business and is not
    tried on one; what can be pinned without a device is that the route is chosen from D and from x, out and W_dec together."""
    m = re.search(r"const bool vec = (.*);", HIP)
    assert m and m.group(1) == "D % 4 == 0 && (((uintptr_t)x | (uintptr_t)out | (uintptr_t)W_dec) & 15) == 0", m
    assert "if (vec) hipLaunchKernelGGL(iv_rows_kernel<true>" in HIP and "else hipLaunchKernelGGL(iv_rows_kernel<false>" in HIP
    assert re.search(r"if constexpr \(VEC\) \{\s*iv_apply<f32x4>", HIP) and re.search(r"\} else \{\s*iv_apply<float>", HIP)


ALL_EDIT_CASES = {**IC.EDIT_CASES, **IC.ALIGN_CASES, **IC.COUNT_CASES}


@pytest.mark.parametrize("name", list(ALL_EDIT_CASES))
def test_edit_case_holds(name):
    case = ALL_EDIT_CASES[name]()
    assert case.name == name
    e = case.expected
    case.holds(e)
    n, D = case.x.shape
    assert e["out"].shape == (n, D) and e["m"].shape == (n,) and e["rows_changed"].shape == (len(case.edits),)
    untouched = e["m"] == 0
    assert (e["out"][untouched] == case.x[untouched]).all() and np.isfinite(e["out"]).all()
    assert e["rows_changed"].sum() == e["m"].sum()


def test_every_asked_width_and_row_count_is_a_case():
    assert sorted(D for D, (vec, _, _) in IC.WIDTHS.items() if vec) == [1020, 1024, 1028, 1280, 2052, 4100]
    assert sorted(D for D, (vec, _, _) in IC.WIDTHS.items() if not vec) == [255, 257, 258, 511, 513, 1027]
    assert all(f"width_{'float4' if vec else 'scalar'}_{D}" in IC.EDIT_CASES for D, (vec, _, _) in IC.WIDTHS.items())
    R = IC.IV_MAX_GRID * IC.IV_WAVES
    assert all(f"row_stride_{n}" in IC.EDIT_CASES for n in (R - 1, R, R + 5, 2 * R + 3))
    assert {"inplace_512_edits_1028", "inplace_gap_2052", "plan_limits_65536"} <= set(IC.EDIT_CASES)
    assert set(IC.ALIGN_CASES) == {"align_1028", "align_8"} and all(c().offsets == (("x",), ("out",), ("W",), ("x", "out", "W")) for c in IC.ALIGN_CASES.values())


@pytest.mark.parametrize("name", list(IC.FIRE_CASES))
def test_fire_case_holds(name):
    case = IC.FIRE_CASES[name]()
    e = case.expected
    case.holds(e)
    T = len(case.thr)
    assert e["hist"].shape == (case.C, T, case.S) and e["pos"].shape == (T, case.S) and e["f1"].shape == (case.C, case.S)
    assert (e["hist"].sum(axis=0) <= e["pos"]).all() and e["hist"].max() < 2 ** 32
    assert e["f1"].dtype == np.float32 and e["best_t"].dtype == np.uint8


def test_the_2p24_case_tells_the_conversions_apart():
    """On the case's own integers: 2.f * float(TP) equals float(2 TP) (a power of two scales exactly), so the numerator alone cannot
    show a slip; the denominator summed in fp32 does, in f1's bits."""
    case = IC.FIRE_CASES["f1_past_2p24"]()
    e = case.expected
    TP, POS = IR.suffix(e["hist"], e["pos"])
    assert ((np.float32(2) * TP.astype(np.float32)) == (2 * TP).astype(np.float32)).all()
    FP, FN = POS[None] - TP, e["n_rows_c"][:, None, None] - TP
    exact = (2 * TP + FP + FN).astype(np.float32)
    summed = ((2 * TP).astype(np.float32) + FP.astype(np.float32)) + FN.astype(np.float32)
    assert (exact != summed).any()
    assert (IC.f1_mutated(TP, POS, e["n_rows_c"]).view(np.uint32) != e["f1"].view(np.uint32)).any()
    # one batch alone stays below 2^24: it is the repeated add that carries the counts past it
    one = IR.fire_counts_fast(case.idx, case.val, case.row_nnz, case.labels, case.keep, case.S, case.C, case.thr)
    assert 2 * one[0].max() < 2 ** 24 and (e["hist"] == case.repeats * one[0]).all()


# ---- the vectorised restatements against the loops that define them ---------------------------------------------------------------


def _same_counts(a, b):
    assert all(p.dtype == np.int64 and q.dtype == np.int64 and p.shape == q.shape and (p == q).all() for p, q in zip(a, b))


@pytest.mark.parametrize("T", [1, 4, 8])
@pytest.mark.parametrize("cap", [1, 5, 70])
def test_fire_counts_fast_on_the_shapes_of_the_gpu_test(T, cap):
    from test_gpu_interventions import THRESHOLDS, _fire_case

    rng = np.random.default_rng(100 * T + cap)
    n, S, C_ = 37, 70, 5
    idx, val, nnz, labels, keep = _fire_case(rng, n, S, C_, cap, THRESHOLDS[T])
    _same_counts(IR.fire_counts_fast(idx, val, nnz, labels, keep, S, C_, THRESHOLDS[T]), IR.fire_counts(idx, val, nnz, labels, keep, S, C_, THRESHOLDS[T]))
    _same_counts(IR.fire_counts_fast(idx, val, None, labels, None, S, C_, THRESHOLDS[T]), IR.fire_counts(idx, val, None, labels, None, S, C_, THRESHOLDS[T]))
    _same_counts(IR.fire_counts_fast(idx, val, nnz, labels.astype(np.int64), keep.astype(np.uint8), S, C_, THRESHOLDS[T]),
                 IR.fire_counts(idx, val, nnz, labels, keep, S, C_, THRESHOLDS[T]))


@pytest.mark.parametrize("seed", range(6))
def test_fire_counts_fast_on_random_small_shapes(seed):
    rng = np.random.default_rng(seed)
    n, S, C_, cap, T = (int(rng.integers(lo, hi)) for lo, hi in ((1, 90), (1, 40), (1, 9), (1, 12), (1, 9)))
    thr = np.sort(rng.choice(np.array([0.0, 0.05, 0.1, 0.2, 0.3, 0.5, 1.0, 2.0, 4.0], dtype=np.float32), T, replace=False))
    idx = rng.integers(-2, S + 2, (n, cap)).astype(np.int32)  # out-of-range latents on both sides, repeats inside a row
    val = rng.choice(np.concatenate([thr, np.nextafter(thr, np.float32(np.inf)), np.array([-1.0, 9.0, np.nan, np.inf], dtype=np.float32)]), (n, cap)).astype(np.float32)
    nnz = rng.integers(-2, cap + 3, n).astype(np.int32)
    labels = rng.integers(-2, C_ + 2, n).astype(np.int32)
    keep = rng.random(n) < 0.7
    _same_counts(IR.fire_counts_fast(idx, val, nnz, labels, keep, S, C_, thr), IR.fire_counts(idx, val, nnz, labels, keep, S, C_, thr))
    # the builders' own generator, cut to a size the loop can take
    small = IC._fire_inputs(rng, 300, S, C_, cap, thr, every_row=0 if seed % 2 else None)
    _same_counts(IR.fire_counts_fast(*small, S, C_, thr), IR.fire_counts(*small, S, C_, thr))


def _same_edit(case, **cut):
    args = dict(x=case.x, idx=case.idx, val=case.val, row_nnz=case.row_nnz, row_group=case.row_group, row_keep=case.row_keep)
    args.update(cut)
    fast = IR.intervene_fast(args["x"], case.W, args["idx"], args["val"], args["row_nnz"], case.edits, case.n_groups, row_group=args["row_group"],
                             row_keep=args["row_keep"])
    slow = IR.intervene(args["x"], case.W, args["idx"], args["val"], args["row_nnz"], case.edits, case.n_groups, row_group=args["row_group"],
                        row_keep=args["row_keep"])
    for key in ("out", "mag"):
        assert fast[key].dtype == np.float64 and (fast[key].view(np.uint64) == slow[key].view(np.uint64)).all(), key
    assert (fast["m"] == slow["m"]).all() and (fast["rows_changed"] == slow["rows_changed"]).all()
    at = {i: set() for i in range(len(case.edits))}
    lat_of = {}
    for i, (latent, _, _, group) in enumerate(case.edits):
        lat_of.setdefault((group, latent), i)
    for b, row in enumerate(slow["coef"]):
        g = -1 if args["row_group"] is None or not 0 <= int(args["row_group"][b]) < case.n_groups else int(args["row_group"][b])
        for latent, _ in row:
            at[lat_of[(g, latent)] if (g, latent) in lat_of else lat_of[(-1, latent)]].add(b)
    assert {i: set(r.tolist()) for i, r in fast["applied"].items()} == {i: r for i, r in at.items() if r}


@pytest.mark.parametrize("name", ["width_float4_1020", "width_scalar_257", "inplace_gap_2052", "align_8", "counts_prefilled_three_contenders",
                                  "inplace_512_edits_1028"])
def test_intervene_fast_is_intervene_on_the_small_cases(name):
    _same_edit(ALL_EDIT_CASES[name]())


def test_intervene_fast_is_intervene_on_the_head_and_the_seams_of_a_stride_case():
    case = IC.row_stride_case(2 * IC.GRID_ROWS + 3)
    rows = np.concatenate([np.arange(40), np.arange(IC.GRID_ROWS - 3, IC.GRID_ROWS + 40), np.arange(2 * IC.GRID_ROWS - 3, 2 * IC.GRID_ROWS + 3)])
    _same_edit(case, x=case.x[rows], idx=case.idx[rows], val=case.val[rows], row_nnz=case.row_nnz[rows], row_group=case.row_group[rows],
               row_keep=case.row_keep[rows])
    e = case.expected
    part = IR.intervene(case.x[rows], case.W, case.idx[rows], case.val[rows], case.row_nnz[rows], case.edits, case.n_groups,
                        row_group=case.row_group[rows], row_keep=case.row_keep[rows])
    assert (e["out"][rows].view(np.uint64) == part["out"].view(np.uint64)).all() and (e["m"][rows] == part["m"]).all()


def test_intervene_fast_without_optional_arguments_and_with_hard_scales():
    """No row_nnz, group or keep vector; SCALE values whose exact fmaf needs more than the 53 bits of the fast path's fp64 (the
    fall-back to the scalar coefficient), and SCALE by 1 (c = 0)."""
    rng = np.random.default_rng(3)
    S, D, n, cap = 50, 6, 40, 4
    W = rng.standard_normal((S, D)).astype(np.float32)
    x = rng.standard_normal((n, D)).astype(np.float32)
    idx, val, _ = IC._codes(rng, n, S, cap)
    val[:, 0] = np.float32(1 + 2.0 ** -12)
    idx[:, 0] = 40
    idx[:, 1:][idx[:, 1:] == 40] = IC.FREE
    edits = [(40, IR.SCALE, float(np.float32(1 + 2.0 ** -12)), -1), (41, IR.SCALE, 1e-30, -1), (42, IR.SCALE, 1.0, -1), (43, IR.SCALE, float(np.float32(1e30)), -1),
             (44, IR.SET | IR.IF_ACTIVE, 0.5, -1)]
    for b in range(n):
        for j, lat in enumerate((41, 42, 43), start=1):
            if b % (j + 1) == 0:
                IC._put(idx, val, b, j, lat, np.float32(rng.uniform(1e-3, 3.0)))
    fast = IR.intervene_fast(x, W, idx, val, None, edits, 0)
    slow = IR.intervene(x, W, idx, val, None, edits, 0)
    assert (fast["out"].view(np.uint64) == slow["out"].view(np.uint64)).all() and (fast["mag"] == slow["mag"]).all()
    assert (fast["m"] == slow["m"]).all() and (fast["rows_changed"] == slow["rows_changed"]).all() and fast["rows_changed"][2] == 0
    c, applies = IR._coefficients_fast(val[:, 0], IR.SCALE, np.float32(1 + 2.0 ** -12))
    assert applies.all() and (c == IR.coefficient(val[0, 0], IR.SCALE, np.float32(1 + 2.0 ** -12))).all()
