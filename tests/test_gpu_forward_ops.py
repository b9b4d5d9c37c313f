"""The single-op forward entries (include/saev_amd.h, "single ops": saev_topk_dense, saev_decode_sparse, saev_scatter_dense,
saev_gather_rows, saev_encode_dense) against tests/forward_ops_restatement.py on the cases of tests/forward_ops_cases.py
(needs an MI355X: -m gpu).

  A. select   -- codes and value bits equal the restated total order on every case; masks with fewer than k eligible latents through
                 the C entry with pre-filled outputs
  B. decode   -- decode_kernel<NV> with x == nullptr at every NV class, k around the 64-code chunk, four rows per workgroup: within
                 decode_tolerance of fp64, and bit-identical under -1 slots, prefix cuts and repetition
  C. scatter, gather -- equal to numpy on the bits
  D. encode_dense -- every element within tol_b (tests/topk_exactness.py) of fp64, in every encoder mode
  E. the walked dense route -- select_dense_kernel on a grid of 1 024 workgroups over 1 030 overflowing rows
  F. the module -- TopKActivation over leading dimensions, SparseAutoencoder.decode, the wrappers' refusals

The tolerances are derived (forward_ops_restatement.decode_tolerance, tol_b); the printed ratios are records ("Parity")."""

import numpy as np
import pytest
import torch

import forward_ops_cases as FC
import forward_ops_restatement as FR
from step_restatement import row_inputs
from test_gpu_parity import make_engine, rand_params

pytestmark = pytest.mark.gpu
f32_only = pytest.mark.encoder_modes("f32")


def bits(t) -> np.ndarray:
    a = t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def decode_engine(D, max_batch=8):
    W, b = FC.decode_params(D)
    eng = make_engine(D, FC.DEC_S, 8, max_batch=max_batch, normalize_w_dec=False)
    eng.load_params({"W_dec": torch.from_numpy(W), "b_dec": torch.from_numpy(b), "W_enc": torch.zeros(D, FC.DEC_S), "b_enc": torch.zeros(FC.DEC_S)})
    views = eng.param_views()
    assert np.array_equal(bits(views["W_dec"]), bits(W)) and np.array_equal(bits(views["b_dec"]), bits(b))
    return eng, W, b


# ---- A. select ---------------------------------------------------------------------------------------------------------------------


@f32_only
@pytest.mark.parametrize("S", FC.SELECT_WIDTHS)
def test_select_matches_the_restated_order(S):
    from saev_amd.engine import _ptr, _stream

    eng = make_engine(16, S, min(8, S), max_batch=8)
    for case in (c for c in FC.SELECT_CASES if c.S == S):
        h, k, mask = case.build()
        want_idx, want_val = FR.select(h, k, mask)
        hg = dev(h)
        mg = None if mask is None else dev(mask)
        if FC.is_short(case, k):
            # caller-owned outputs with a recognisable fill: an unwritten slot shows as -7 / NaN and no index is ever used
            idx = torch.full((len(h), k), -7, dtype=torch.int32, device="cuda")
            val = torch.full((len(h), k), float("nan"), dtype=torch.float32, device="cuda")
            rc = eng.lib.saev_topk_dense(eng.ctx, _ptr(hg), len(h), k, _ptr(mg), _ptr(idx), _ptr(val), _stream())
            assert rc == 0, case.id
            idx2, val2 = idx, val
        else:
            idx, val = eng.topk_dense(hg, k, mask=mg)
            idx2, val2 = eng.topk_dense(hg, k, mask=mg)
        got_idx = idx.cpu().numpy()
        bad = np.nonzero((got_idx != want_idx).any(axis=1) | (bits(val) != bits(want_val)).any(axis=1))[0]
        assert len(bad) == 0, (f"{case.id}: row {bad[0]}: idx {got_idx[bad[0]].tolist()[:12]}..{got_idx[bad[0]].tolist()[-4:]} against "
                               f"{want_idx[bad[0]].tolist()[:12]}..{want_idx[bad[0]].tolist()[-4:]}")
        assert torch.equal(idx, idx2) and np.array_equal(bits(val), bits(val2)), f"{case.id}: two calls differ"
    eng.close()


# ---- B. decode ---------------------------------------------------------------------------------------------------------------------


@f32_only
@pytest.mark.parametrize("D", FC.DEC_D)
def test_decode_sparse_every_nv_class(D):
    eng, W, b = decode_engine(D)
    worst = 0.0
    for c in FC.decode_cases(D):
        idx, val = FC.decode_codes(c)
        want, mag, m = FR.decode(idx, val, W, b, c.prefixes)
        ig, vg = dev(idx), dev(val)
        out = eng.decode_sparse(ig, vg, prefixes=c.prefixes)
        assert out.shape == (c.n, len(c.prefixes), D)
        got = out.cpu().numpy()
        ratio = np.abs(got.astype(np.float64) - want) / FR.decode_tolerance(mag, m)
        worst = max(worst, float(ratio.max()))
        assert (ratio <= 1.0).all(), f"{c.id}: element {np.unravel_index(ratio.argmax(), ratio.shape)} is {ratio.max():.2f} tolerances off fp64"
        assert np.array_equal(bits(eng.decode_sparse(ig, vg, prefixes=c.prefixes)), bits(got)), f"{c.id}: two calls differ"
        # -1 slots change nothing: each batch row without them
        for r in range(c.n):
            i2, v2 = FC.without_pads(idx[r], val[r])
            o2 = eng.decode_sparse(dev(i2[None]), dev(v2[None]), prefixes=c.prefixes)
            assert np.array_equal(bits(o2)[0], bits(got)[r]), f"{c.id}: row {r} changes when its -1 slots are removed"
        # prefix p of a multi-prefix call (scratch + strided copy) = a one-prefix call on the entries below the cut
        if len(c.prefixes) > 1:
            for p, cut in enumerate(c.prefixes):
                o1 = eng.decode_sparse(dev(np.where(idx >= cut, -1, idx).astype(np.int32)), vg)
                assert np.array_equal(bits(o1)[:, 0], bits(got)[:, p]), f"{c.id}: prefix {p} (cut {cut}) differs from the one-prefix decode"
            i2, v2 = FC.without_pads(np.where(idx[0] >= c.prefixes[0], -1, idx[0]).astype(np.int32), val[0])
            o1 = eng.decode_sparse(dev(i2[None]), dev(v2[None]))
            assert np.array_equal(bits(o1)[0, 0], bits(got)[0, 0]), f"{c.id}: prefix 0 differs from the decode of the entries below it alone"
    print(f"decode_sparse D={D} NV={FC.dispatch_nv(D)}: worst error {worst:.3f} of decode_tolerance")
    eng.close()


@f32_only
def test_decode_sparse_batch_limit_and_prefix_refusals():
    from saev_amd._lib import SaevError

    D = 260
    eng, W, b = decode_engine(D, max_batch=8)
    c = FC.DecodeCase(D, 65, 9, (FC.DEC_S,), seed=5)
    idx, val = FC.decode_codes(c)
    want, mag, m = FR.decode(idx, val, W, b, c.prefixes)
    got = eng.decode_sparse(dev(idx), dev(val)).cpu().numpy()  # n = 9 > max_batch = 8: one prefix needs no scratch
    assert (np.abs(got - want) <= FR.decode_tolerance(mag, m)).all()
    with pytest.raises(SaevError, match=r"status -1"):
        eng.decode_sparse(dev(idx), dev(val), prefixes=(5, FC.DEC_S))
    for pre in ((5, 5, FC.DEC_S), (6, 5, FC.DEC_S), (5, 60), (0, FC.DEC_S), (FC.DEC_S, FC.DEC_S + 4), ()):
        with pytest.raises(SaevError):
            eng.decode_sparse(dev(idx[:4]), dev(val[:4]), prefixes=pre)
    eng.close()


# ---- C. scatter and gather -----------------------------------------------------------------------------------------------------------


@f32_only
@pytest.mark.parametrize("S", sorted({S for _, _, S in FC.SCATTER_CASES}))
def test_scatter_dense_matches_numpy(S):
    eng = make_engine(16, S, 4, max_batch=8)
    for n, k, _ in (c for c in FC.SCATTER_CASES if c[2] == S):
        idx, val = FC.scatter_codes(n, k, S)
        f = eng.scatter_dense(dev(idx), dev(val))
        assert f.shape == (n, S) and np.array_equal(bits(f), bits(FR.scatter(idx, val, S))), f"n={n} k={k}"
    eng.close()


@f32_only
@pytest.mark.parametrize("D", FC.GATHER_D)
def test_gather_rows_matches_numpy(D):
    eng = make_engine(D, 64, 4, max_batch=8)
    for n in FC.GATHER_N:
        pool, rows = FC.gather_inputs(D, n)
        want = bits(FR.gather(pool, rows))
        pg, rg = dev(pool), dev(rows)
        assert np.array_equal(bits(eng.gather_rows(pg, rg)), want), f"n={n}"
        out = torch.full((n, D), float("nan"), device="cuda")
        assert eng.gather_rows(pg, rg, out=out) is out and np.array_equal(bits(out), want), f"n={n}, out= given"
    eng.close()


# ---- D. encode_dense -----------------------------------------------------------------------------------------------------------------


def encode_dense_ratio(eng, x, W_enc, b_enc) -> float:
    """Worst |h - fp64| / tol_b over every element, tol_b = 8 * 2^-24 * ||x_b|| * max_s ||W_enc[:, s]||."""
    h = eng.encode_dense(x.cuda()).cpu().double()
    ref = x.double() @ W_enc.double() + b_enc.double()
    tol = 8.0 * 2.0 ** -24 * x.double().norm(dim=1, keepdim=True) * W_enc.double().norm(dim=0).max()
    ratio = (h - ref).abs() / tol
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    return ratio.max().item()


@pytest.mark.parametrize("row", FC.encode_rows(), ids=lambda r: f"{r.n}x{r.d}x{r.s}")
def test_encode_dense_within_tol_b(row, encoder_mode):
    p, x, _ = row_inputs(row)
    eng = make_engine(row.d, row.s, row.k, max_batch=max(row.n, 8))
    eng.load_params(p)
    worst = encode_dense_ratio(eng, x, p["W_enc"], p["b_enc"])
    one = encode_dense_ratio(eng, x[-1:], p["W_enc"], p["b_enc"])
    print(f"encode_dense {encoder_mode} {row.n}x{row.d}x{row.s}: worst error {worst:.3f} tol_b, one row {one:.3f} tol_b")
    assert worst <= 1.0 and one <= 1.0
    eng.close()


@f32_only
def test_encode_dense_past_max_batch_in_f32():
    n, d, s = 40, 36, 260
    p = rand_params(d, s, seed=1)
    x = torch.randn(n, d, generator=torch.Generator().manual_seed(2))
    eng = make_engine(d, s, 4, max_batch=8)
    eng.load_params(p)
    worst = encode_dense_ratio(eng, x, p["W_enc"], p["b_enc"])
    print(f"encode_dense f32 n = {n} > max_batch = 8: worst error {worst:.3f} tol_b")
    assert worst <= 1.0
    eng.close()


# ---- E. the walked dense route -------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("varied", [False, True], ids=["same-h", "h-by-row"])
def test_dense_route_walks_past_its_grid(varied):
    """tests/test_gpu_parity.py::test_candidate_overflow_takes_the_exact_dense_route at n = 1030: every list overflows, the step takes
    the exact dense route, and select_dense_kernel runs on 1 024 workgroups that walk the rows -- six of them a second one.

    same-h: W_enc is zero, so every row's h is b_enc whatever x is, and every row's codes are select(b_enc, k).  That shows that rows
    1024..1029 are written and that the per-row state is set up again, not that the second trip reads ITS row of h.
    h-by-row: W_enc[0, 5000] = 1 and x[b, 0] = b % 7 - 3, so h[b, 5000] = b % 7 - 2 exactly in every encoder arithmetic (small integers
    times one; every other product is an exact zero).  Latent 5000 is a strict maximum of its own value in the rows with b % 7 >= 4, one
    more tie at 1.0 (left out: the lower indices win) at b % 7 = 3, below the cut elsewhere; row 1024 + j is handled by the workgroup of
    row j, whose b % 7 differs."""
    n, d, s, k = 1030, 32, 16384, 16
    p = rand_params(d, s, seed=3)
    p["W_enc"] = torch.zeros(d, s)
    p["b_enc"] = torch.ones(s)
    p["b_enc"][7], p["b_enc"][9000] = 2.0, 3.0
    x = torch.randn(n, d, generator=torch.Generator().manual_seed(4))
    kind = np.zeros(n, dtype=np.int64)
    if varied:
        p["W_enc"][0, 5000] = 1.0
        kind = np.arange(n) % 7
        x[:, 0] = torch.from_numpy(kind - 3).float()
    eng = make_engine(d, s, k, max_batch=1040)
    eng.load_params(p)
    eng.step_forward(x.cuda(), training=False)
    st = eng.read_stats()
    assert st.n_overflow_rows == n and st.dense_route == 1
    idx, val, x_hat = (t.cpu().numpy() for t in eng.last_codes(n))
    h = np.repeat(p["b_enc"].numpy()[None], 7 if varied else 1, axis=0)
    if varied:
        h[:, 5000] = np.arange(7, dtype=np.float32) - 2
    want_idx, want_val = FR.select(h, k)
    assert want_idx[0].tolist() == list(range(15)) + [9000], "the two strict maxima and the 14 lowest of the ties at 1.0"
    if varied:
        assert want_idx[3].tolist() == want_idx[0].tolist() and want_idx[6].tolist() == list(range(14)) + [5000, 9000] and want_val[6, 14] == 4.0
        assert len({tuple(want_idx[(1024 + j) % 7]) + tuple(want_val[(1024 + j) % 7]) for j in range(6)} | {tuple(want_idx[0]) + tuple(want_val[0])}) > 1
    want_idx, want_val = want_idx[kind], want_val[kind]
    bad = np.nonzero((idx != want_idx).any(axis=1) | (bits(val) != bits(want_val)).any(axis=1))[0]
    assert len(bad) == 0, (f"rows {bad[:8].tolist()} (of {len(bad)}): row {bad[0]} has idx {idx[bad[0]].tolist()}, val {val[bad[0]].tolist()}; "
                           f"want {want_idx[bad[0]].tolist()}, {want_val[bad[0]].tolist()}")
    views = eng.param_views()
    want, mag, m = FR.decode(idx, val, views["W_dec"].cpu().numpy(), views["b_dec"].cpu().numpy(), (s,))
    ratio = np.abs(x_hat.astype(np.float64) - want[:, 0]) / FR.decode_tolerance(mag, m)[:, 0]
    print(f"walked dense route ({'h by row' if varied else 'same h'}): overflow rows {st.n_overflow_rows}, x_hat worst error {ratio.max():.3f} of decode_tolerance")
    assert (ratio <= 1.0).all()
    eng.close()


# ---- F. the module -------------------------------------------------------------------------------------------------------------------


def small_sae(d=16, s=64, k=5):
    from saev_amd.nn import modeling as m

    return m.SparseAutoencoder(m.SparseAutoencoderConfig(d_model=d, d_sae=s, activation=m.TopK(top_k=k))).cuda()


@pytest.mark.parametrize("shape", [(3, 5, 64), (7, 64), (64,)], ids=str)
def test_topk_activation_selects_along_the_last_dimension(shape):
    sae = small_sae()
    h = torch.randn(*shape, generator=torch.Generator().manual_seed(len(shape)))
    f = sae.activation(h.cuda())
    assert f.shape == h.shape
    want = FR.scatter(*FR.select(h.reshape(-1, 64).numpy(), 5), 64).reshape(shape)
    assert np.array_equal(bits(f), bits(want))


def test_module_decode_of_dense_latents():
    sae = small_sae()
    S, D = 64, 16
    g = torch.Generator().manual_seed(11)
    with torch.no_grad():
        sae.b_dec.copy_(torch.randn(D, generator=g))
    f = torch.zeros(4, S)
    f[1, 40] = -1.5
    f[2, [0, 5, 6, 63]] = torch.randn(4, generator=g)
    f[3] = torch.randn(S, generator=g) + 3.0  # (no zero among them)
    assert (f != 0).sum(dim=1).tolist() == [0, 1, 4, S]
    pre = (5, 6, S)
    out = sae.decode(f.cuda(), prefixes=torch.tensor(pre)).cpu().numpy()
    assert out.shape == (4, 3, D)
    # the zero entries of a row reach the kernel as codes of value 0, whose products add exactly: the chain is that of the non-zeros
    idx = np.where(f.numpy() != 0, np.arange(S, dtype=np.int32)[None], np.int32(-1)).astype(np.int32)
    want, mag, m = FR.decode(idx, f.numpy(), sae.W_dec.detach().cpu().numpy(), sae.b_dec.detach().cpu().numpy(), pre)
    ratio = np.abs(out.astype(np.float64) - want) / FR.decode_tolerance(mag, m)
    print(f"SparseAutoencoder.decode: worst error {ratio.max():.3f} of decode_tolerance")
    assert (ratio <= 1.0).all()
    assert np.array_equal(bits(out[0]), np.broadcast_to(bits(sae.b_dec.detach()), (3, D))), "a row without latents decodes to b_dec"


def test_single_op_wrappers_refuse_what_they_cannot_read():
    """Each of these used to hand a pointer on and read (or write) out of bounds; now none reaches a kernel."""
    from saev_amd._lib import SaevError

    S, D = 64, 16
    eng = make_engine(D, S, 4, max_batch=8)
    h = torch.randn(3, S, device="cuda")
    idx = torch.zeros(3, 4, dtype=torch.int32, device="cuda")
    val = torch.ones(3, 4, device="cuda")
    pool = torch.randn(10, D, device="cuda")
    rows = torch.tensor([1, 2, 3], device="cuda")
    refused = [
        lambda: eng.topk_dense(h.cpu(), 4),
        lambda: eng.topk_dense(h.double(), 4),
        lambda: eng.topk_dense(h.half(), 4),
        lambda: eng.topk_dense(torch.randn(3, S + 4, device="cuda"), 4),
        lambda: eng.topk_dense(torch.randn(3, S - 4, device="cuda"), 4),
        lambda: eng.topk_dense(torch.randn(3, 5, S, device="cuda"), 4),
        lambda: eng.topk_dense(h[0], 4),
        lambda: eng.topk_dense(h, 0),
        lambda: eng.topk_dense(h, -1),
        lambda: eng.topk_dense(h, S + 1),
        lambda: eng.topk_dense(h, 4.0),
        lambda: eng.topk_dense(h, 4, mask=torch.ones(S - 4, dtype=torch.int32)),
        lambda: eng.topk_dense(h, 4, mask=torch.ones(2, S, dtype=torch.int32)),
        lambda: eng.topk_dense(h, 4, mask=torch.ones(S)),
        lambda: eng.scatter_dense(idx.long(), val),
        lambda: eng.scatter_dense(idx, val.double()),
        lambda: eng.scatter_dense(idx, val[:, :3]),
        lambda: eng.scatter_dense(idx[0], val[0]),
        lambda: eng.scatter_dense(idx.cpu(), val),
        lambda: eng.scatter_dense(idx, val.cpu()),
        lambda: eng.decode_sparse(idx.long(), val),
        lambda: eng.decode_sparse(idx, val.half()),
        lambda: eng.decode_sparse(idx, val[:2]),
        lambda: eng.decode_sparse(idx[0], val[0]),
        lambda: eng.decode_sparse(idx.cpu(), val.cpu()),
        lambda: eng.gather_rows(pool, rows.int()),
        lambda: eng.gather_rows(pool, rows.float()),
        lambda: eng.gather_rows(pool, rows[None]),
        lambda: eng.gather_rows(pool.double(), rows),
        lambda: eng.gather_rows(torch.randn(10, D + 4, device="cuda"), rows),
        lambda: eng.gather_rows(torch.randn(10, 2 * D, device="cuda")[:, :D], rows),
        lambda: eng.gather_rows(pool.reshape(-1), rows),
        lambda: eng.gather_rows(pool.cpu(), rows),
        lambda: eng.gather_rows(pool, rows.cpu()),
        lambda: eng.gather_rows(pool, rows, out=torch.empty(2, D, device="cuda")),
        lambda: eng.gather_rows(pool, rows, out=torch.empty(3, D, device="cuda", dtype=torch.float64)),
        lambda: eng.gather_rows(pool, rows, out=torch.empty(3, D)),
    ]
    for i, call in enumerate(refused):
        with pytest.raises(SaevError):
            call()
            pytest.fail(f"call {i} was accepted")
    # and what they must keep accepting: a bool or int64 mask on the host, views that need a copy
    want = FR.select(h.cpu().numpy(), 4, np.arange(S) % 2)
    for mask in (torch.arange(S) % 2 == 1, (torch.arange(S) % 2) << 32, (torch.arange(S, device="cuda") % 2).int()):
        got = eng.topk_dense(h, 4, mask=mask)
        assert np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(bits(got[1]), bits(want[1]))
    wide = torch.randn(3, 2 * S, device="cuda")
    got = eng.topk_dense(wide[:, 1:S + 1], 4)  # neither contiguous nor 16-byte aligned
    want = FR.select(wide[:, 1:S + 1].cpu().numpy(), 4)
    assert np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(bits(got[1]), bits(want[1]))
    f = eng.scatter_dense(got[0].t().contiguous().t(), got[1])
    assert np.array_equal(bits(f), bits(FR.scatter(want[0], want[1], S)))
    eng.close()
