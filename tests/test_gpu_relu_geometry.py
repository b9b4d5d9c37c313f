"""The ReLU forward kernels where they change behaviour, on the MI355X (needs -m gpu): relu_encode_kernel's tiles of 32 rows x 128
latents x 16 d_model columns and its capacity cut, relu_decode_kernel's four float4 trips and prefix cuts, relu_scatter_kernel, and
the module API on top of them (tables and builders in tests/relu_cases.py).

Tolerances.  Random rows: check_rows of tests/test_gpu_relu.py (values and membership against fp64 at the fp32 dot-product bound);
x_hat at BOUND = 2e-5 of tests/step_restatement.py times the largest fp64 element, against the fp64 decode of the rows the encoder
returned.  Planted rows: equality of idx, val and row_nnz, nothing else.  Hand-built decode rows: the tolerance of
test_gpu_relu.py::test_decode_rows_against_fp64; prefixes that must be equal, or equal to b_dec, are compared bit for bit.

Observed on an MI355X (f32; these kernels do not depend on the encoder arithmetic): x_hat within 6.1e-7 of max|fp64| in every
table row (bound 2e-5) and in the module test, whose f_x comes within 0.34 of check_rows' tolerance; the hand-built decode rows
within 1.0e-2 of their tolerance at every d_model.

What a one-line error does to these tests: with the prefix cut `i >= prefixes[p]` turned into `>` the decode test fails at every
d_model; with RD_NV = 3 it fails at 4092 and 4096, as do the table's two widest rows (both tried on the GPU).  `pos <= row_cap`
in the encoder writes a row's entry number row_cap into slot 0 of the NEXT row: test_a_truncating_launch_... ends its batch on the
longest row and keeps a guard row behind the buffer, so that write lands where it is seen and nowhere else."""

import ctypes as C

import pytest
import torch

from relu_cases import (DECODE_CAP, DECODE_D, DECODE_PREFIXES, DECODE_S, FORWARD_SHAPES, PLANTED, assert_planted_rows, decode_rows_case,
                        forward_inputs, planted_batch)
from step_restatement import BOUND
from test_gpu_relu import check_rows, relu_engine

pytestmark = [pytest.mark.gpu, pytest.mark.encoder_modes("f32")]


def _dense(idx, val, nnz, s):
    """The dense f of padded rows, built on the CPU from the first row_nnz slots alone."""
    idx, val, nnz = idx.cpu(), val.cpu(), nnz.cpu()
    live = torch.arange(idx.shape[1])[None, :] < nnz[:, None]
    f = torch.zeros(idx.shape[0], s)
    rows = torch.arange(idx.shape[0])[:, None].expand_as(idx)
    f[rows[live], idx[live].long()] = val[live]
    return f


# ------------------------------------------------------------------------------------------------
# random rows in every tile class
# ------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("shape", FORWARD_SHAPES, ids=lambda t: "x".join(map(str, t)))
def test_forward_in_every_tile_class(shape, encoder_mode):
    n, d, s = shape
    p, x = forward_inputs(n, d, s)
    eng = relu_engine(d, s, n, p)
    x = x.cuda()
    idx, val, nnz = eng.encode_relu(x)
    top = check_rows(eng, x, idx, val, nnz)
    assert idx.shape[1] >= top and int(nnz.min()) >= 0
    f = _dense(idx, val, nnz, s)
    assert torch.equal(eng.scatter_rows(idx, val, nnz).cpu(), f)
    x_hat64 = f.double() @ p["W_dec"].double() + p["b_dec"].double()
    got = eng.decode_rows(idx, val, nnz)
    assert got.shape == (n, 1, d)
    err = (got[:, 0].cpu().double() - x_hat64).abs().max().item()
    print(f"{n}x{d}x{s}: rows of {int(nnz.min())}..{top} entries in {idx.shape[1]} slots, second launches {eng.relu_second_launches}; "
          f"x_hat worst |difference| / max|fp64| {err / x_hat64.abs().max().item():.2e}")
    assert err <= BOUND * x_hat64.abs().max().item()


def test_module_api_at_a_ragged_shape(encoder_mode):
    from saev_amd.nn import modeling as M

    n, d, s = 65, 100, 1004
    p, x = forward_inputs(n, d, s)
    sae = M.SparseAutoencoder(M.SparseAutoencoderConfig(d_model=d, d_sae=s, activation=M.Relu()))
    sae.load_state_dict(p)
    sae = sae.to("cuda")
    out = sae(x.cuda())
    assert out.f_x.shape == (n, s) and out.x_hats.shape == (n, 1, d)
    h64 = x.double() @ p["W_enc"].double() + p["b_enc"].double()
    # check_rows' tolerance: inside it a latent may be on either side of the cut, and then either value is within it of the other
    tol = 8.0 * 2.0 ** -24 * x.double().norm(dim=1) * p["W_enc"].double().norm(dim=0).max() + 2.0 ** -23 * p["b_enc"].double().abs().max()
    f = out.f_x.cpu().double()
    err_f = ((f - h64.clamp_min(0)).abs() / tol[:, None]).max().item()
    x_hat64 = f @ p["W_dec"].double() + p["b_dec"].double()
    err_x = (out.x_hats[:, 0].cpu().double() - x_hat64).abs().max().item() / x_hat64.abs().max().item()
    print(f"module {n}x{d}x{s}: f_x worst |difference| / tolerance {err_f:.2e}; x_hat worst |difference| / max|fp64| {err_x:.2e}")
    assert err_f <= 1.0 and (f >= 0).all()
    assert err_x <= BOUND


# ------------------------------------------------------------------------------------------------
# planted rows: the compaction and the capacity cut, with equality
# ------------------------------------------------------------------------------------------------


def _planted_engine(S, cap, rows):
    p, x, want = planted_batch(S, cap, rows)
    return relu_engine(4, S, len(rows), p), x.cuda(), want


@pytest.mark.parametrize("S,cap", PLANTED)
def test_rows_that_fill_the_capacity_exactly_need_no_second_launch(S, cap, encoder_mode):
    rows = [0, 1] * 17 + [1, 1, 0]  # 37 rows: a second workgroup of five
    eng, x, want = _planted_engine(S, cap, rows)
    idx, val, nnz = eng.encode_relu(x, row_cap=cap)
    assert eng.relu_second_launches == 0 and idx.shape == (len(rows), cap)
    assert set(nnz.tolist()) == {0, cap}
    assert_planted_rows(idx, val, nnz, want)


@pytest.mark.parametrize("S,cap", PLANTED)
def test_a_row_one_past_the_capacity_takes_one_second_launch(S, cap, encoder_mode):
    rows = [0, 1] * 17 + [1, 2, 0]
    eng, x, want = _planted_engine(S, cap, rows)
    idx, val, nnz = eng.encode_relu(x, row_cap=cap)
    assert eng.relu_second_launches == 1 and idx.shape == (len(rows), cap + 1)
    assert_planted_rows(idx, val, nnz, want)
    wide = eng.encode_relu(x, row_cap=S)
    assert eng.relu_second_launches == 1 and wide[0].shape[1] == S
    assert torch.equal(wide[2], nnz)
    live = torch.arange(cap + 1, device="cuda")[None, :] < nnz[:, None]
    assert torch.equal(wide[0][:, :cap + 1][live], idx[live]) and torch.equal(wide[1][:, :cap + 1][live], val[live])
    assert eng.relu_row_cap == min(S, 512)  # (an explicit row_cap leaves the engine's own capacity alone)


@pytest.mark.parametrize("S,cap", PLANTED)
@pytest.mark.parametrize("short", [1, 2, 3])
def test_a_truncating_launch_stores_the_first_entries_and_nothing_past_its_rows(S, cap, short, encoder_mode):
    """The library entry itself at a capacity 1, 2 and 3 short of the longest row (P2: the cut falls after column 2, 1 and 0 of the
    last thread's float4): exact counts, the overflow word = the longest count, the first row_cap entries of every row, and a guard
    row behind the last batch row -- which is the longest -- untouched."""
    rows = [2, 0, 1, 2] * 9 + [0, 2]  # 38 rows; the last row of the batch overflows
    eng, x, want = _planted_engine(S, cap, rows)
    n, rc = len(rows), cap + 1 - short
    idx = torch.full((n + 1, rc), -77, dtype=torch.int32, device="cuda")
    val = torch.full((n + 1, rc), -77.0, device="cuda")
    nnz = torch.full((n + 1,), -77, dtype=torch.int32, device="cuda")
    over = torch.full((1,), -77, dtype=torch.int32, device="cuda")
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    assert eng.lib.saev_encode_relu(eng.ctx, P(x), n, rc, P(nnz), P(idx), P(val), P(over), C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    torch.cuda.synchronize()
    assert int(over.item()) == cap + 1
    assert (idx[n] == -77).all() and (val[n] == -77.0).all() and int(nnz[n]) == -77, "the launch wrote past its last row"
    assert nnz[:n].tolist() == [w[0].numel() for w in want]
    cut = [(lat[:rc], a) for lat, a in want]
    assert_planted_rows(idx[:n], val[:n], torch.tensor([w[0].numel() for w in cut], dtype=torch.int32), cut)


def test_an_all_positive_row_grows_the_engine_to_d_sae(encoder_mode):
    S, cap = 1004, 131
    rows = [1, 3, 0, 3] + [0, 1] * 16  # a P0 row between two P3 rows of one half-wave
    eng, x, want = _planted_engine(S, cap, rows)
    assert eng.relu_row_cap == 512
    idx, val, nnz = eng.encode_relu(x)
    assert eng.relu_second_launches == 1 and idx.shape[1] == S and eng.relu_row_cap == S
    assert_planted_rows(idx, val, nnz, want)
    again = eng.encode_relu(x)
    assert eng.relu_second_launches == 1 and again[0].shape[1] == S
    assert_planted_rows(*again, want)
    # the decode of an all-positive row: x_hat = a_b * (the column sums of W_dec), 1004 entries long
    got = eng.decode_rows(idx, val, nnz)[1, 0].cpu().double()
    ref = want[1][1] * eng.view("W_dec").double().cpu().sum(dim=0)
    assert (got - ref).abs().max() <= BOUND * max(ref.abs().max().item(), want[1][1])


@pytest.mark.parametrize("S,cap", PLANTED)
def test_capacities_at_and_past_the_ends(S, cap, encoder_mode):
    rows = [3, 0, 2, 1, 0]
    eng, x, want = _planted_engine(S, cap, rows)
    # above d_sae: clamped to it, no second launch even for the all-positive row
    idx, val, nnz = eng.encode_relu(x, row_cap=S + 1000)
    assert eng.relu_second_launches == 0 and idx.shape[1] == S
    assert_planted_rows(idx, val, nnz, want)
    # 1: everything but the empty rows overflows; the second launch is sized from the longest
    idx, val, nnz = eng.encode_relu(x, row_cap=1)
    assert eng.relu_second_launches == 1 and idx.shape[1] == S
    assert_planted_rows(idx, val, nnz, want)
    # ... and rows of at most one entry fit in it
    eng1, x1, want1 = _planted_engine(S, cap, [0, 0, 0])
    idx, val, nnz = eng1.encode_relu(x1, row_cap=1)
    assert eng1.relu_second_launches == 0 and idx.shape == (3, 1) and not nnz.any()


@pytest.mark.parametrize("S,cap", PLANTED)
def test_a_row_has_the_same_entries_wherever_it_sits(S, cap, encoder_mode):
    """70 rows of mixed patterns (three workgroups, the last of six rows), then the same rows permuted: every 32-row workgroup and
    every half-wave (four rows) mixes patterns, a P0 row sits between two P3 rows, and each row's entries follow it."""
    g = torch.Generator().manual_seed(5)
    rows = [3, 0, 3, 1, 2, 0, 1, 3] + torch.randint(0, 4, (62,), generator=g).tolist()
    p, x, want = planted_batch(S, cap, rows)
    eng = relu_engine(4, S, len(rows), p)
    idx, val, nnz = eng.encode_relu(x.cuda(), row_cap=S)
    assert_planted_rows(idx, val, nnz, want, what="in order: ")
    for seed in (6, 7):
        perm = torch.randperm(len(rows), generator=torch.Generator().manual_seed(seed))
        i2, v2, n2 = eng.encode_relu(x[perm].contiguous().cuda(), row_cap=S)
        assert_planted_rows(i2, v2, n2, [want[int(j)] for j in perm], what=f"permutation {seed}: ")
    assert eng.relu_second_launches == 0


# ------------------------------------------------------------------------------------------------
# relu_decode_kernel: every float4 trip, every kind of prefix cut
# ------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("d", DECODE_D)
def test_decode_rows_in_every_trip_class_and_at_every_cut(d, encoder_mode):
    s, cap = DECODE_S, DECODE_CAP
    idx, val, nnz = decode_rows_case()
    n = idx.shape[0]
    g = torch.Generator().manual_seed(22 + d)
    eng = relu_engine(d, s, n)
    eng.view("W_dec").copy_(torch.randn(s, d, generator=g).cuda())
    eng.view("b_dec").copy_(torch.randn(d, generator=g).cuda())
    eng.params_touched()
    W, bd32 = eng.view("W_dec").double().cpu(), eng.view("b_dec").cpu()
    bd = bd32.double()
    worst = 0.0
    for prefixes in DECODE_PREFIXES:
        pre = [s] if prefixes is None else list(prefixes)
        got32 = eng.decode_rows(idx.cuda(), val.cuda(), nnz.cuda(), prefixes=prefixes).cpu()
        assert got32.shape == (n, len(pre), d)
        got = got32.double()
        for r in range(n):
            k = int(nnz[r])
            ii, vv = idx[r, :k].long(), val[r, :k].double()
            for q, cut in enumerate(pre):
                m = ii < cut  # an entry ON the cut belongs to the later prefixes only
                want = bd + vv[m] @ W[ii[m]]
                tol = 1e-5 * want.abs() + 1e-4 * (1 + k) ** 0.5
                worst = max(worst, ((got[r, q] - want).abs() / tol).max().item())
                torch.testing.assert_close(got[r, q], want, rtol=1e-5, atol=1e-4 * (1 + k) ** 0.5, msg=lambda s_: f"d {d} prefixes {prefixes} row {r} prefix {q}: {s_}")
                if not m.any():
                    assert torch.equal(got32[r, q], bd32), f"d {d} prefixes {prefixes} row {r}: prefix {q} holds no entry and is not b_dec"
            if k == 0 or bool((ii < pre[0]).all()):  # all entries below the first cut: every prefix is the same sum
                assert all(torch.equal(got32[r, q], got32[r, 0]) for q in range(len(pre))), f"d {d} prefixes {prefixes} row {r}"
    print(f"decode d_model {d}: worst |difference| / tolerance {worst:.2e}")
