"""CPU-only tests of tests/relu_cases.py: the tables are well formed, the planted batch is what its docstring says (counts, the lanes
of the straddling entries, h = +-a_b exactly in fp32), the truncating-launch check of the GPU test tells `pos < row_cap` from `<=`
on a CPU model of the encoder's index arithmetic, the scale cases meet their input conditions, and the fp32 torch restatement
of every scale case passes the GPU test's checks against fp64 at a QUARTER of the GPU test's bound -- where the bounds of
tests/test_gpu_relu_train_scale.py come from (never from the HIP result)."""

import functools

import pytest
import torch

from relu_cases import (BAND_SHARE, DECODE_CAP, DECODE_D, DECODE_PREFIXES, DECODE_S, FORWARD_SHAPES, MASSIVE_CHANNEL, PLANTED, SCALE_BASES,
                        SCALE_CASES, assert_planted_rows, assert_rows_close, band_of, decode_rows_case, forward_inputs, planted_batch,
                        planted_patterns, scale_case_inputs)
from relu_step_restatement import RELU_SHAPES, relu_bound, relu_input_conditions, relu_restated_gradients, relu_row_inputs
from step_restatement import BOUND, assert_grads_close


def test_the_tables_are_well_formed():
    assert set(FORWARD_SHAPES) >= {(1, 4, 4), (31, 20, 36), (70, 16, 124), (32, 48, 128), (33, 36, 132), (65, 100, 1004), (34, 4092, 516),
                                   (40, 4096, 260)}
    for n, d, s in FORWARD_SHAPES:
        assert n >= 1 and d % 4 == 0 and s % 4 == 0 and 4 <= d <= 4096
    assert set(DECODE_D) == {4, 20, 1028, 4092, 4096} and (DECODE_S, DECODE_CAP) == (516, 40)
    assert {S for S, _ in PLANTED} == {260, 1004}
    assert {b.id for b in SCALE_BASES} == {"65x36x260-extremes", "257x512x516"}
    assert len({c.id for c in SCALE_CASES}) == len(SCALE_CASES) == 5 * len(SCALE_BASES)
    assert {c.log2 for c in SCALE_CASES if c.kind == "scale"} == {18, -20}
    for c in SCALE_CASES:
        assert c.base.d % 4 == 0 and c.base.s % 4 == 0 and c.base.d <= 4096 and c.bound >= BOUND
    # the train table's classes this pull request adds: Kp = n (no padding of the batch axis), one and two whole row tiles
    assert {(r.n, r.d, r.s) for r in RELU_SHAPES} >= {(256, 36, 260), (512, 20, 36)}
    p, x = forward_inputs(65, 100, 1004)
    counts = ((x.double() @ p["W_enc"].double() + p["b_enc"].double()) > 0).sum(dim=1)
    assert counts.min() < 512 < counts.max(), "the (65, 100, 1004) row must have counts on both sides of the default capacity"


def test_the_decode_rows_are_what_the_prefix_lists_need():
    idx, val, nnz = decode_rows_case()
    S, cap = DECODE_S, DECODE_CAP
    assert {0, 1, cap} <= set(nnz.tolist()) and idx.shape == val.shape == (nnz.numel(), cap)
    live = torch.arange(cap)[None, :] < nnz[:, None]
    assert (idx[~live] >= S).all() and torch.isnan(val[~live]).all() and (val[live] > 0).all()
    assert ((idx[:, 1:] > idx[:, :-1]) | ~live[:, 1:]).all() and (idx[live] >= 0).all() and (idx[live] < S).all()
    entries = set(idx[live].tolist())
    for pre in DECODE_PREFIXES[1:]:
        assert list(pre) == sorted(set(pre)) and pre[-1] == S and pre[0] >= 1 and len(pre) <= 16
        for cut in pre[:-1]:
            assert cut in entries or cut - 1 in entries  # a cut on an entry's latent, or one above an entry
    assert len(DECODE_PREFIXES[-1]) == 16 and DECODE_PREFIXES[0] is None
    full = nnz == cap
    assert ((idx < 100) | ~live)[full].all(dim=1).any(), "no full row with all entries below the first cut of (100, ...)"
    assert ((idx >= 476) | ~live)[full].all(dim=1).any(), "no full row with all entries at or past the cut 476"
    assert any(cut in entries for pre in DECODE_PREFIXES[1:] for cut in pre[:-1])


@pytest.mark.parametrize("S,cap", PLANTED)
def test_the_planted_batch_is_exact(S, cap):
    P = planted_patterns(S, cap)
    assert P.abs().eq(1).all()
    counts = (P > 0).sum(dim=1).tolist()
    assert counts == [0, cap, cap + 1, S]
    # P1: the cap-th positive is latent S - 1; its last three are columns 1 .. 3 of one thread's float4; latent 0 is negative
    pos1 = torch.nonzero(P[1] > 0)[:, 0]
    assert int(pos1[-1]) == S - 1 and pos1[-3:].tolist() == [S - 3, S - 2, S - 1] and P[1, S - 4] < 0 and P[1, 0] < 0
    t = (S - 4) // 4
    assert [4 * t + 1, 4 * t + 2, 4 * t + 3] == pos1[-3:].tolist()  # (thread tx = t % 32 of tile t // 32 holds latents 4t .. 4t + 3)
    assert len({int(q) // 128 for q in pos1}) == (S + 127) // 128, "P1 leaves a latent tile without a positive"
    # P2 = P1 + latent 0: at a capacity of cap its slots cap - 2, cap - 1 are latents S - 3, S - 2 and latent S - 1 is cut
    pos2 = torch.nonzero(P[2] > 0)[:, 0]
    assert pos2.tolist() == [0] + pos1.tolist() and pos2[cap - 2:].tolist() == [S - 3, S - 2, S - 1]
    rows = [0, 1, 2, 3, 3, 0, 3, 1]
    p, x, want = planted_batch(S, cap, rows)
    assert p["W_enc"].shape == (4, S) and not p["b_enc"].any() and x.shape == (len(rows), 4)
    a = x.sum(dim=1)
    assert (a > 0).all() and a.unique().numel() == len(rows) and (x != 0).sum(dim=1).eq(1).all()
    h = x @ p["W_enc"] + p["b_enc"]  # fp32 torch
    assert torch.equal(h, a[:, None] * P[rows]) and torch.equal(h.abs(), a[:, None].expand_as(h))
    # ... in the kernel's own order too: one fmaf per product, k ascending, from +0
    acc = torch.zeros(len(rows), S)
    for k in range(4):
        acc = torch.addcmul(acc, x[:, k:k + 1], p["W_enc"][k:k + 1])
    assert torch.equal(acc + p["b_enc"], h)
    for b, (lat, a_b) in enumerate(want):
        assert lat.numel() == counts[rows[b]] and a_b == float(a[b]) and torch.equal(lat.long(), torch.nonzero(h[b] > 0)[:, 0])
    # the comparison helper accepts the planted rows (with anything behind them) and refuses a wrong slot
    width = S
    idx = torch.full((len(rows), width), -7, dtype=torch.int32)
    val = torch.full((len(rows), width), float("nan"))
    for b, (lat, a_b) in enumerate(want):
        idx[b, : lat.numel()], val[b, : lat.numel()] = lat, a_b
    nnz = torch.tensor([w[0].numel() for w in want], dtype=torch.int32)
    assert_planted_rows(idx, val, nnz, want)
    idx[2, cap] += 1
    with pytest.raises(AssertionError, match="row 2"):
        assert_planted_rows(idx, val, nnz, want)


def _model_compaction(h, rc, n_slots, cut=lambda pos, rc: pos < rc):
    """relu_encode_kernel's index arithmetic on the CPU, thread by thread: tiles of 128 latents, thread tx holds latents
    n0 + 4 tx .. + 3 of a row, an entry's slot is the row's running count + the positives of the lanes before it + those of its own
    earlier columns, stored at row * rc + slot where ``cut`` allows.  Writes into flat buffers of ``n_slots`` entries."""
    n, S = h.shape
    idx, val = torch.full((n_slots,), -77, dtype=torch.int32), torch.full((n_slots,), -77.0)
    nnz = torch.zeros(n, dtype=torch.int32)
    for r in range(n):
        cnt = 0
        for n0 in range(0, S, 128):
            p = [[n0 + 4 * tx + j < S and bool(h[r, n0 + 4 * tx + j] > 0) for j in range(4)] for tx in range(32)]
            per_lane = [sum(q) for q in p]
            for tx in range(32):
                pos = cnt + sum(per_lane[:tx])
                for j in range(4):
                    if p[tx][j]:
                        if cut(pos, rc):
                            idx[r * rc + pos], val[r * rc + pos] = n0 + 4 * tx + j, h[r, n0 + 4 * tx + j]
                        pos += 1
            cnt += sum(per_lane)
        nnz[r] = cnt
    return idx, val, nnz


@pytest.mark.parametrize("short", [1, 2, 3])
def test_the_truncating_launch_check_tells_the_capacity_cut_apart(short):
    """What tests/test_gpu_relu_geometry.py::test_a_truncating_launch_stores_the_first_entries_and_nothing_past_its_rows asserts, on a
    CPU model of the kernel's index arithmetic: it holds with the cut `pos < row_cap`; with `pos <= row_cap` the longest row's entry
    number row_cap lands in slot 0 of the row behind it -- the guard row, for the last row of the batch -- inside the buffer the
    test allocates.  (That error is not run on a GPU: without the guard row it writes past the allocation.)"""
    S, cap = PLANTED[0]
    rows = [2, 0, 1, 2, 0, 2]
    p, x, want = planted_batch(S, cap, rows)
    n, rc = len(rows), cap + 1 - short
    h = x @ p["W_enc"]
    cutw = [(lat[:rc], a) for lat, a in want]
    kept = torch.tensor([w[0].numel() for w in cutw], dtype=torch.int32)
    idx, val, nnz = _model_compaction(h, rc, (n + 1) * rc)
    assert nnz.tolist() == [w[0].numel() for w in want] and int(nnz.max()) == cap + 1
    assert (idx[n * rc:] == -77).all() and (val[n * rc:] == -77.0).all()
    assert_planted_rows(idx[: n * rc].view(n, rc), val[: n * rc].view(n, rc), kept, cutw)
    idx, val, _ = _model_compaction(h, rc, (n + 1) * rc, cut=lambda pos, rc_: pos <= rc_)
    assert int(idx[n * rc]) == int(want[-1][0][rc]) and float(val[n * rc]) == want[-1][1]  # the guard row's slot 0: seen
    assert (idx[n * rc + 1:] == -77).all()


# ------------------------------------------------------------------------------------------------
# the scale cases
# ------------------------------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def _reference(case):
    p, x = scale_case_inputs(case)
    h, band = band_of(p, x)
    mask = h > 0
    return p, x, h, band, mask, relu_restated_gradients(p, x, mask, case.l1_coeff)


@pytest.mark.parametrize("case", SCALE_CASES, ids=lambda c: c.id)
def test_scale_cases_meet_their_input_conditions(case):
    p, x, h, band, mask, (mse, l1, ref) = _reference(case)
    bound = relu_bound(x, p["W_enc"], p["b_enc"])
    if case.kind == "scale":
        # a power of two moves every pre-activation and the bound alike: the base row's distance from zero, in bounds
        p0, x0 = relu_row_inputs(case.base)
        mask0, ratio0 = relu_input_conditions(p0["W_enc"], p0["b_enc"], x0)
        _, ratio = relu_input_conditions(p["W_enc"], p["b_enc"], x)
        print(f"{case.id}: smallest |h| {ratio:.2f} fp32 bounds from zero (base row: {ratio0:.2f})")
        assert torch.equal(mask, mask0) and abs(ratio - ratio0) <= 1e-6 * ratio0
        assert torch.equal(h, (x0.double() @ p0["W_enc"].double() + p0["b_enc"].double()) * 2.0 ** case.log2)
    elif case.kind == "massive":
        p0, x0 = relu_row_inputs(case.base)
        mask0, _ = relu_input_conditions(p0["W_enc"], p0["b_enc"], x0)
        share = band.double().mean().item()
        print(f"{case.id}: {share:.3%} of the pre-activations within two fp32 bounds ({bound:.2e}) of zero")
        assert share <= BAND_SHARE
        assert torch.equal(mask | band, mask0 | band)  # the plain row's mask wherever fp32 can tell
        # the channel dominates x, not h: a per-tensor bound on dW_enc would be that row's
        others = torch.arange(case.base.d) != MASSIVE_CHANNEL
        assert x[:, MASSIVE_CHANNEL].abs().max() > 30 * x[:, others].abs().max()
        assert ref["W_enc"][MASSIVE_CHANNEL].abs().max() > 30 * ref["W_enc"][others].abs().max()
    else:
        print(f"{case.id}: largest fp64 pre-activation {h.max().item():.2f}, fp32 bound {bound:.2e}")
        assert h.max() < -2 * bound and h.max() < -10 and not mask.any() and not band.any()
        assert l1 == 0 and not ref["W_dec"].any() and not ref["W_enc"].any() and not ref["b_enc"].any()
        if case.kind == "silent":
            assert mse > 0 and ref["b_dec"].abs().max() > 0
        else:
            assert mse == 0 and not ref["b_dec"].any() and torch.equal(x, p["b_dec"][None, :].expand_as(x))


@pytest.mark.parametrize("case", SCALE_CASES, ids=lambda c: c.id)
def test_fp32_restatement_of_every_scale_case(case):
    """The rule of test_relu_train_host_cpu.py::test_fp32_restatement_passes_its_own_check: the fp32 torch restatement against fp64
    at a quarter of the bound the GPU test uses, W_enc's gradient row by row included."""
    p, x, h, band, mask, (mse, l1, ref) = _reference(case)
    mse32, l132, got = relu_restated_gradients(p, x, mask, case.l1_coeff, dtype=torch.float32)
    ratios = assert_grads_close(got, ref, case.bound / 4, what=f"{case.id}: ")
    by_row = assert_rows_close(got["W_enc"], ref["W_enc"], case.bound / 4, what=f"{case.id}: W_enc.grad ")
    print(f"{case.id}: fp32 against fp64, worst |difference| / max|fp64|: " + "  ".join(f"{k} {v:.2e}" for k, v in ratios.items())
          + f"  W_enc row by row {by_row:.2e}")
    assert all(torch.isfinite(v).all() for v in got.values())
    assert abs(mse32 - mse) <= 1e-5 * mse and abs(l132 - l1) <= 1e-5 * l1
