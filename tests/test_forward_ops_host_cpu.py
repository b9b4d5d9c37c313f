"""The restatement and the cases of the single-op forward tests, checked without a GPU: the restatement against torch.topk and the
golden fixtures, every case against what it claims to reach, and the cases against wrong variants of the contract."""

import numpy as np
import pytest
import torch

import forward_ops_cases as FC
import forward_ops_restatement as FR
from conftest import load_golden


def built(case):
    h, k, mask = case.build()
    assert h.dtype == np.float32 and h.ndim == 2 and h.shape[1] == case.S and 1 <= k <= case.S
    assert mask is None or (mask.dtype == np.int32 and mask.shape == (case.S,))
    return h, k, mask


def sorted_keys(h, mask=None):
    """Per row the eligible keys from the largest down, as int64."""
    key = FR.keys(h).astype(np.int64)
    if mask is not None:
        key = key[:, mask != 0]
    return -np.sort(-key, axis=1)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------


def test_keys_are_the_documented_order():
    v = FC._bits([FC.N_NAN, 0xFF800000, 0xFF7FFFFF, 0xBF800000, 0x80000001, 0x80000000, 0x00000000, 0x00000001, 0x3F800000, 0x7F7FFFFF,
                  0x7F800000, 0x7F800001, FC.P_NAN])
    k = FR.keys(v).astype(np.int64)
    assert (np.diff(k) > 0).all(), "sign-bit NaN < -inf < ... < -0.0 < +0.0 < ... < +inf < +NaN"
    assert np.array_equal(FR.from_keys(FR.keys(v)).view(np.uint32), v.view(np.uint32))


@pytest.mark.parametrize("case", [c for c in FC.SELECT_CASES if c.tie_free], ids=lambda c: c.id)
def test_select_is_torch_topk_on_tie_free_rows(case):
    h, k, mask = built(case)
    assert np.isfinite(h).all() and all(len(np.unique(r)) == case.S for r in h)
    idx, val = FR.select(h, k, mask)
    want = torch.topk(torch.from_numpy(h), k, dim=-1)
    assert np.array_equal(np.sort(val, axis=1), np.sort(want.values.numpy(), axis=1))
    assert np.array_equal(idx, np.sort(want.indices.numpy(), axis=1))
    assert (np.diff(idx, axis=1) > 0).all() and np.array_equal(np.take_along_axis(h, idx.astype(np.int64), 1), val)


def test_select_reproduces_g1():
    g = load_golden("g1_encode_topk")
    idx, val = FR.select(g["h"].numpy(), 8)
    assert np.array_equal(FR.scatter(idx, val, 320), g["f"].numpy())


def test_decode_reproduces_g2():
    g = load_golden("g2_decode")
    f = g["f"].numpy()
    idx, _ = FR.select((f != 0).astype(np.float32), 8)  # ties to the lower index: the non-zeros first
    val = np.take_along_axis(f, idx.astype(np.int64), 1)
    for name, pre in (("x_hats_p1", (320,)), ("x_hats_p3", tuple(g["prefixes"].tolist()))):
        out, mag, m = FR.decode(idx, val, g["W_dec"].numpy(), g["b_dec"].numpy(), pre)
        # the fixture is the reference's fp32 matrix product: a chain of at most 320 terms, most of them zero; its own error is
        # bounded by the same kind of chain over the 8 non-zeros (zeros add exactly), in any summation order
        assert (m <= 8).all()
        assert (np.abs(out - g[name].numpy()) <= FR.decode_tolerance(mag, m)).all(), name


def test_decode_counts_duplicates_and_skips():
    W = np.arange(12, dtype=np.float32).reshape(4, 3)
    b = np.float32([1, 1, 1])
    idx = np.int32([[2, -1, 2, 3, 4, 0]])
    val = np.float32([[1, 9, 2, 1, 9, -1]])
    out, mag, m = FR.decode(idx, val, W, b, (1, 3, 4))
    assert np.array_equal(out[0, 0], 1 - W[0]) and np.array_equal(out[0, 1], 1 + 3 * W[2] - W[0]) and np.array_equal(out[0, 2], out[0, 1] + W[3])
    assert m.tolist() == [[1, 3, 4]] and np.array_equal(mag[0, 2], 1 + 3 * W[2] + W[0] + W[3])
    assert np.array_equal(FR.decode_tolerance(mag, m)[0, 0], 4 * 2.0 ** -24 * mag[0, 0] + 2.0 ** -149)


def test_scatter_and_gather():
    f = FR.scatter(np.int32([[0, -1, 3], [4, 2, 1]]), np.float32([[1, 2, 3], [4, 5, 6]]), 4)
    assert f.tolist() == [[1, 0, 0, 3], [0, 6, 5, 0]]
    assert FR.gather(np.arange(6).reshape(3, 2), [2, 0, 2]).tolist() == [[4, 5], [0, 1], [4, 5]]


# ---- the cases reach what they claim -----------------------------------------------------------------------------------------------


@pytest.mark.parametrize("case", FC.SELECT_CASES, ids=lambda c: c.id)
def test_select_case_claims(case):
    h, k, mask = built(case)
    eligible = case.S if mask is None else int((mask != 0).sum())
    if case.eligible is not None:
        assert eligible == case.eligible and mask is not None
    if eligible < k:
        idx, val = FR.select(h, k, mask)
        assert (idx[:, eligible:] == -1).all() and (val.view(np.uint32)[:, eligible:] == 0).all() and (idx[:, :eligible] >= 0).all()
        return
    sk = sorted_keys(h, mask)
    if case.byte is not None or case.digit is not None:
        p = case.byte if case.byte is not None else case.digit[0]
        kth, nxt = sk[:, k - 1], sk[:, k]
        assert ((kth >> (8 * (p + 1))) == (nxt >> (8 * (p + 1)))).all(), "the bytes above are shared"
        if case.byte is not None:
            assert (((kth >> (8 * p)) & 255) != ((nxt >> (8 * p)) & 255)).all(), f"the cut is decided in byte {p}"
        else:
            assert (((kth >> (8 * p)) & 255) == case.digit[1]).all()
            if case.digit[1] == 0xFF:
                assert (((nxt >> (8 * p)) & 255) < 0xFF).all()
    if case.bin_exact is not None:
        top = sk >> 24
        assert (top[:, k - 1] == case.bin_exact).all() and ((top >= case.bin_exact).sum(axis=1) == k).all()
    if case.tie_trips:
        idx, val = FR.select(h, k, mask)
        key = FR.keys(h).astype(np.int64)
        for b in range(len(h)):
            cut = sk[b, k - 1]
            kept = idx[b][key[b, idx[b]] == cut]
            assert kept.min() < FC.TRIP <= kept.max(), "kept ties on both sides of a trip border"
            if case.ties_run_out:
                later = np.nonzero(key[b] >= cut)[0]
                left = np.setdiff1d(later[key[b, later] == cut], kept)
                greater = later[key[b, later] > cut]
                assert (left > kept.max()).all() and len(left) + len(greater) > 0
                assert max(left.max(initial=0), greater.max(initial=0)) // FC.TRIP >= 1, "something follows in a later trip"


def test_select_cases_cover_the_issue():
    ids = {c.id for c in FC.SELECT_CASES}
    for S in FC.WIDTHS:
        for k in FC.KS + (S - 1, S):
            assert not 1 <= k <= S or f"w{S}k{k}" in ids
    assert {c.byte for c in FC.SELECT_CASES if c.byte is not None} == {0, 1, 2, 3}
    assert {c.digit for c in FC.SELECT_CASES if c.digit is not None} == {(p, d) for p in range(4) for d in (0, 255)}
    bins = {c.bin_exact for c in FC.SELECT_CASES if c.bin_exact is not None}
    assert {b & 3 for b in bins} >= {0, 3} and {b >> 2 for b in bins} >= {0, 33, 63}
    for S, k in ((1028, 33), (8, 3)):
        assert {c.eligible for c in FC.SELECT_CASES if c.S == S and c.eligible is not None} >= {k + 1, k, k - 1, 0}
    words = set()
    for c in FC.SELECT_CASES:
        if c.eligible:
            words |= set(np.unique(c.build()[2]).tolist())
    assert words == {0, 1, -1, 2}
    assert any(c.ties_run_out for c in FC.SELECT_CASES) and any(FC.is_short(c, c.build()[1]) for c in FC.SELECT_CASES)


def test_masked_cases_hide_the_largest_values():
    for c in FC.SELECT_CASES:
        if c.eligible is not None and c.id.startswith("mask-S"):
            h, k, mask = c.build()
            out = h[:, mask == 0]
            assert np.isinf(out).any() and np.isnan(out).any()
            if c.eligible:
                assert np.nanmax(h[:, mask != 0]) < 50.0 <= np.nanmax(np.where(np.isinf(out), 0, out))


def test_decode_cases_cover_every_class():
    assert tuple(FC.dispatch_nv(D) for D in FC.DEC_D) == FC.DEC_NV
    # every instantiation dispatch_nv can pick over the widths a context takes (d_model % 4 == 0, 4 .. 4096) is reached
    assert set(FC.DEC_NV) == {FC.dispatch_nv(D) for D in range(4, 4097, 4)} == {1, 2, 3, 4, 5, 6, 8, 12, 16}
    for D in FC.DEC_D:
        cases = FC.decode_cases(D)
        assert tuple(c.k for c in cases) == FC.DEC_K and {c.prefixes for c in cases} == set(FC.DEC_PREFIXES)
        for c in cases:
            idx, val = FC.decode_codes(c)
            assert idx.shape == val.shape == (c.n, c.k) and idx.min() >= -1 and idx.max() < FC.DEC_S
            assert c.prefixes[-1] == FC.DEC_S and all(b > a for a, b in zip(c.prefixes, c.prefixes[1:]))
            if c.k >= 8:
                r = idx[0]
                assert r[0] == r[-1] == r[c.k // 2] == -1 and 0 in r and FC.DEC_S - 1 in r
                assert (np.bincount(r[r >= 0]) > 1).any() and (np.diff(r[r >= 0]) < 0).any(), "a duplicate; not ascending"
    allc = [c for D in FC.DEC_D for c in FC.decode_cases(D)]
    assert {c.n for c in allc} == set(FC.DEC_N)
    assert {(c.k, len(c.prefixes) > 1) for c in allc} == {(k, m) for k in FC.DEC_K for m in (False, True)}
    assert len(FC.DEC_PREFIXES[3]) == 16


def test_scatter_gather_encode_cases():
    assert sorted(n * k for n, k, _ in FC.SCATTER_CASES) == [1, 257, 257, 65537]
    for n, k, S in FC.SCATTER_CASES:
        idx, val = FC.scatter_codes(n, k, S)
        assert idx.shape == (n, k) and idx.min() >= -1 and idx.max() <= S
        if n * k > 1:
            assert (idx == -1).any() and (idx == S).any()
        assert all(len(np.unique(r)) == k for r in idx[:300]), "no latent twice in a row: the scatter has no order among duplicates"
    for D in FC.GATHER_D:
        for n in FC.GATHER_N:
            pool, rows = FC.gather_inputs(D, n)
            assert rows.dtype == np.int64 and 0 <= rows.min() and rows.max() == FC.GATHER_POOL_ROWS - 1
            assert n < 3 or (0 in rows and len(np.unique(rows)) < n)
    from step_restatement import SHAPES
    assert {(r.d, r.s) for r in FC.encode_rows()} == {(r.d, r.s) for r in SHAPES}


# ---- the cases tell wrong variants apart -------------------------------------------------------------------------------------------


def ties_to_highest(h, k, mask):
    S = h.shape[1]
    idx, val = FR.select(h[:, ::-1], k, None if mask is None else mask[::-1])
    idx = np.where(idx >= 0, S - 1 - idx, np.int32(2 ** 31 - 1))
    order = np.argsort(idx, axis=1, kind="stable")
    idx, val = np.take_along_axis(idx, order, 1), np.take_along_axis(val, order, 1)
    return np.where(idx == 2 ** 31 - 1, -1, idx).astype(np.int32), val


def zeros_equal(h, k, mask):
    idx, _ = FR.select(h + np.float32(0.0), k, mask)  # -0.0 + 0.0 = +0.0
    val = np.where(idx >= 0, np.take_along_axis(h, np.maximum(idx, 0).astype(np.int64), 1), np.float32(0))
    return idx, val


def mask_ignored(h, k, mask):
    return FR.select(h, k, None)


@pytest.mark.parametrize("variant", [ties_to_highest, zeros_equal, mask_ignored], ids=lambda f: f.__name__)
def test_select_cases_tell_a_wrong_variant_apart(variant):
    differ = []
    for c in FC.SELECT_CASES:
        h, k, mask = c.build()
        with np.errstate(invalid="ignore"):
            got = variant(h, k, mask)
        want = FR.select(h, k, mask)
        if not (np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))):
            differ.append(c.id)
    assert differ, f"no case distinguishes {variant.__name__}"
    print(f"{variant.__name__}: {len(differ)} cases differ, e.g. {differ[:4]}")


def test_decode_cases_tell_an_unskipped_limit_apart():
    """A decode that applies no prefix cut (every entry below d_sae counted in every prefix) must leave the tolerance on some case."""
    differ = 0
    for D in FC.DEC_D[:3]:
        W, b = FC.decode_params(D)
        for c in FC.decode_cases(D):
            idx, val = FC.decode_codes(c)
            want, mag, m = FR.decode(idx, val, W, b, c.prefixes)
            wrong, _, _ = FR.decode(idx, val, W, b, (FC.DEC_S,) * len(c.prefixes))
            differ += bool((np.abs(wrong - want) > FR.decode_tolerance(mag, m)).any())
    assert differ > 0


def test_without_pads_keeps_the_row():
    c = FC.decode_cases(260)[3]
    idx, val = FC.decode_codes(c)
    W, b = FC.decode_params(260)
    for r in range(c.n):
        i2, v2 = FC.without_pads(idx[r], val[r])
        assert (i2 >= 0).all() and len(i2) == (idx[r] >= 0).sum()
        a, _, _ = FR.decode(idx[r:r + 1], val[r:r + 1], W, b, c.prefixes)
        o, _, _ = FR.decode(i2[None], v2[None], W, b, c.prefixes)
        assert np.array_equal(a, o)
