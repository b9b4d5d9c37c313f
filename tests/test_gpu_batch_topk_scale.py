"""The BatchTopK select and compaction where their loops turn over (needs -m gpu): sizes at which the kernels of
saev_amd/csrc/batchtopk.hip take a second trip of a grid-stride loop, flush the gather's staging buffer inside the loop, fill the key
list to its real capacity, carry the tie count past a block of 1024 rows, and sweep a partial 256-latent chunk.  Every case hands a
GIVEN h to SaeEngine.batch_topk_dense and compares with an fp64 sort under the flat-index tie rule at tolerance 0: the kept set, the
kept values bit for bit, row_nnz, the state words and the threshold.

The constants the arithmetic next to each case refers to (batchtopk.hip, kernels.h): the histogram and the gather run at most 2048
workgroups of 256 threads, one float4 per thread and tile, so a tile is 1024 entries and a second trip needs more than 2048 tiles
(> 2 097 152 entries); the gather stages up to BTK_GBUF = 4096 keys and flushes inside the loop once more than 3072 are staged; the
list holds BTK_LIST_CAP = 2^20 keys; a level-0 bin is 12 key bits = sign, exponent and three mantissa bits: one eighth of an octave.

NaN is out of scope: the reference's topk and this key order treat a negative-signed NaN differently, and neither is specified."""

import numpy as np
import pytest
import torch

from test_gpu_batch_topk import btk_engine, check_form, expected_mask, rows_to_dense

pytestmark = [pytest.mark.gpu, pytest.mark.encoder_modes("f32")]

TILE = 1024           # entries of a tile: 256 threads x one float4
MAX_GROUPS = 2048     # workgroups of btk_hist_kernel / btk_gather_kernel at most
GBUF = 4096           # BTK_GBUF
LIST_CAP = 1 << 20    # BTK_LIST_CAP
M = 0.1               # EngineConfig.batch_momentum


def tiles(n, s):
    return (n * s // 4 + 255) // 256


def bits(t):
    return t.contiguous().view(torch.int32)


def bin_count(h, cut):
    """Entries of h in the level-0 bin of the cut: same sign, exponent and three leading mantissa bits (-0 counts as +0)."""
    b = bits(h + 0.0) >> 20
    return int((b == (bits(torch.tensor([cut], dtype=torch.float32) + 0.0) >> 20)).sum())


def ema(t0, vmin):
    """threshold' as torch's mul_ / add_ round it."""
    return float(torch.tensor(t0, dtype=torch.float32).mul_(1 - M).add_(M * vmin))


def check_select(eng, h, k, *, t0=0.0):
    """Runs the training-mode select on h (CPU tensor) and asserts everything against expected_mask at tolerance 0.  Returns
    (mask, (cut, n_above, quota, n_ties), row_nnz on the CPU)."""
    n, s = h.shape
    eng.threshold.fill_(t0)
    idx, val, nnz = eng.batch_topk_dense(h.cuda(), training=True)
    mask, cut, n_above, quota, n_ties = expected_mask(h, n * k)
    check_form(idx, val, nnz)
    assert int(nnz.sum()) == min(n * k, n * s), "not exactly n * top_k codes"
    assert torch.equal(nnz.cpu().long(), mask.sum(dim=1))
    f, m = rows_to_dense(idx, val, nnz, s)
    m = m.cpu()
    rows = torch.arange(n)[:, None].expand_as(idx)
    got = torch.zeros(n, s, dtype=torch.bool)
    got[rows[m], idx.cpu()[m].long()] = True  # (from the indices: a kept zero is a member too)
    assert torch.equal(got, mask), f"{int((got != mask).sum())} entries of the kept set differ from the fp64 sort's"
    assert torch.equal(bits(val.cpu()[m]), bits(h[rows[m], idx.cpu()[m].long()])), "a kept value is not the given one, bit for bit"
    assert torch.equal(f.cpu(), torch.where(mask, h, torch.zeros(())))
    st = eng.batch_topk_state()
    assert (st["cut"], st["n_above"], st["tie_quota"], st["n_ties"]) == (float(np.float32(cut)), n_above, quota, n_ties)
    pos = h[mask & (h > 0) & (h < float("inf"))]
    want = ema(t0, pos.min()) if pos.numel() else t0
    assert float(eng.threshold) == want, (float(eng.threshold), want)
    return mask, (cut, n_above, quota, n_ties), nnz.cpu().long()


# ------------------------------------------------------------------------------------------------
# 1. a second trip of the grid-stride loops, ragged last tile
# ------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("list_cap", [0, 64])
def test_second_trip_of_the_grid_stride_loops_with_a_ragged_last_tile(list_cap, encoder_mode):
    # 521 x 4100 = 2 136 100 entries, n4 = 534 025 float4 = 2086 full tiles + 9 float4: 2087 tiles on 2048 workgroups, so workgroups
    # 0..38 take a second tile and workgroup 38's second tile is the ragged one (9 of 256 threads inside n4).
    n, s, k = 521, 4100, 8
    assert n * s // 4 > 524_288 and (n * s // 4) % 256 == 9 and tiles(n, s) - MAX_GROUPS == 39
    h = torch.randn(n, s, generator=torch.Generator().manual_seed(1))
    eng = btk_engine(16, s, k, n, select_list_cap=list_cap)
    _, (cut, *_), _ = check_select(eng, h, k)
    # the cut bin holds thousands of entries: the list (capacity 2^20) with list_cap = 0, the re-read of h with list_cap = 64
    assert 64 < bin_count(h, cut) <= LIST_CAP
    assert eng.row_regrows == 0
    eng.close()


# ------------------------------------------------------------------------------------------------
# 2. the real list capacity and the in-loop flush
# ------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("fill", ["all", "most"])
def test_one_crowded_bin_overflows_the_real_list_and_flushes_inside_the_loop(fill, encoder_mode):
    # 2052 x 4096 = 8 404 992 entries = 8208 full tiles = 4 x 2048 + 16: every workgroup takes four tiles, workgroups 0..15 a fifth.
    #   "all":  every entry lies in the bin [1, 1.125).  A tile stages 1024 keys: 3072 after the third tile (not above 3072: no flush),
    #           4096 = BTK_GBUF after the fourth -- the buffer exactly full, the in-loop flush fires -- and the fifth tile of workgroups
    #           0..15 starts from an empty buffer and leaves 1024 keys to the flush after the loop.
    #           Values 1 + j 2^-16, j < 2^13: 8192 distinct values, ~1026 entries each, so about a thousand ties straddle the cut.
    #   "most": ~85 % of the entries in the bin at its full resolution (2^20 distinct values), 15 % below it and 4000 above it:
    #           ~870 keys per tile, so the flush fires after the fourth tile at ~3480 staged keys, a count that differs per workgroup.
    # Either way the bin holds > 7e6 > 2^20 keys: the counter runs past the capacity and levels 1 and 2 re-read h (list_cap = 0).
    n, s, k = 2052, 4096, 4
    assert tiles(n, s) == 4 * MAX_GROUPS + 16 and n * s % TILE == 0 and 4 * TILE == GBUF > GBUF - TILE == 3072
    g = torch.Generator().manual_seed(2)
    if fill == "all":
        h = 1.0 + torch.randint(0, 1 << 13, (n, s), generator=g).float() * 2.0 ** -16
    else:
        h = 1.0 + torch.randint(0, 1 << 20, (n, s), generator=g).float() * 2.0 ** -23
        below = torch.rand(n, s, generator=g) < 0.15
        h = torch.where(below, torch.rand(n, s, generator=g) * 2 - 1, h)  # [-1, 1): other bins, both signs
        above = torch.randperm(n * s, generator=g)[:4000]  # fewer than n k = 8208, so the cut stays inside the crowded bin
        h.view(-1)[above] = 1.125 + 2 * torch.rand(4000, generator=g)
    eng = btk_engine(16, s, k, n)
    assert eng.row_cap == 64
    mask, (cut, n_above, quota, n_ties), nnz = check_select(eng, h, k)
    in_bin = bin_count(h, cut)
    assert 1.0 <= cut < 1.125 and in_bin > LIST_CAP, "the cut bin must hold more keys than the list"
    if fill == "all":
        assert in_bin == n * s and n_ties > 500 and 0 < quota < n_ties, (n_ties, quota)
    else:
        assert 0.8 * n * s < in_bin < 0.9 * n * s
        per_tile = (bits(h.flatten()) >> 20 == bits(torch.tensor([1.0])) >> 20).view(-1, TILE).sum(dim=1)
        four = per_tile[:4 * MAX_GROUPS].view(4, MAX_GROUPS).sum(dim=0)  # workgroup w takes tiles w, w + 2048, ...
        three = four - per_tile[3 * MAX_GROUPS:4 * MAX_GROUPS]
        assert int(three.max()) <= GBUF - TILE < int(four.min()) and int(four.max()) < GBUF and four.unique().numel() > 100
    assert eng.row_regrows == 0 and eng.row_cap == 64 and int(nnz.max()) <= 64
    eng.close()


# ------------------------------------------------------------------------------------------------
# 3. the boundary n_list == list_cap
# ------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("extra", [0, 1])
def test_a_cut_bin_of_exactly_the_list_capacity_and_one_more(extra, encoder_mode):
    # 32 x 64 entries, list_cap = 16.  56 entries of 100 + i lie above the cut bin [8, 9); the bin holds 16 + extra entries,
    # 8 + (j // 2) / 32 (pairs of equal values); everything else is below 4.  n k = 64: the cut is the 8th largest of the bin, the
    # lower one of a pair -- n_above = 63, one tie kept of two.  16 entries fit the list (n_list <= list_cap), 17 take the re-read.
    n, s, k, cap = 32, 64, 2, 16
    flat = (torch.arange(n * s) % 7).float() * 0.5
    g = torch.Generator().manual_seed(3 + extra)
    where = torch.randperm(n * s, generator=g)
    flat[where[:56]] = 100.0 + torch.arange(56)
    in_bin = cap + extra
    # from the top of the bin downwards, so that the extra entry is the smallest and the cut does not move
    flat[where[56:56 + in_bin]] = 8.0 + (31 - torch.arange(in_bin) // 2).float() / 32
    h = flat.view(n, s)
    eng = btk_engine(16, s, k, n, select_list_cap=cap)
    _, (cut, n_above, quota, n_ties), _ = check_select(eng, h, k)
    assert bin_count(h, cut) == in_bin
    assert (cut, n_above, quota, n_ties) == (8.0 + 28 / 32, 62, 2, 2) or (cut, n_above, quota, n_ties) == (8.0 + 28 / 32, 63, 1, 2), (cut, n_above, quota, n_ties)
    eng.close()


# ------------------------------------------------------------------------------------------------
# 4. more than 1024 rows with ties across the block boundary
# ------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("k,block", [(24, 1), (31, 2)])
def test_the_tie_quota_runs_out_past_the_first_block_of_1024_rows(k, block, encoder_mode):
    # 2200 x 64 of the values 0..3, 16 of each per row on average.  k = 24: the 35 200 threes are above the cut 2, the quota is
    # 17 600 of the twos at ~16 per row: it runs out near row 1100, in the second block of btk_tie_scan_kernel (rows 1024..2047), so
    # the count carried over from the first block decides.  k = 31: quota 33 000, it runs out near row 2062, in the third block
    # (rows 2048..2199): the carry of two blocks.
    n, s = 2200, 64
    h = torch.randint(0, 4, (n, s), generator=torch.Generator().manual_seed(4)).float()
    eng = btk_engine(16, s, k, n)
    assert eng.row_cap == s
    mask, (cut, n_above, quota, n_ties), nnz = check_select(eng, h, k)
    assert cut == 2.0 and n_ties > quota > 0
    ties = h == cut
    kept = (mask & ties).sum(dim=1)
    short = (kept < ties.sum(dim=1)).nonzero().flatten()
    r = int(short[0])  # the row in which the quota runs out
    assert 1024 * block <= r < min(1024 * (block + 1), n), r
    assert 0 < int(kept[r]) < int(ties[r].sum()), "that row keeps some of its ties"
    assert (kept[:r] == ties[:r].sum(dim=1)).all() and (kept[r + 1:] == 0).all() and int(ties[r + 1:].sum()) > 0
    eng.close()


# ------------------------------------------------------------------------------------------------
# 5. compaction at ragged d_sae
# ------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("s,k", [(4, 1), (60, 4), (260, 4), (1004, 4)])
def test_compaction_at_ragged_d_sae(s, k, encoder_mode):
    # One wave sweeps a row in 256-latent chunks of four 64-lane sub-loads.  d_sae = 4 and 60 leave the first sub-load partly filled,
    # 260 = one chunk + 4, 1004 = three chunks + 236 (the last sub-load holds 44).  n k "big" entries (4 + U[0, 1)) are the training
    # selection: row 0 has 2 or 3 of them, all in the last (partial) chunk; row 1 has exactly row_cap of them and nothing positive
    # else; the others are scattered over the remaining rows.  Everything else is N(-2.5, 1) capped at 2.9.
    n = 37
    g = torch.Generator().manual_seed(s)
    eng = btk_engine(16, s, k, n)
    cap = eng.row_cap
    assert cap == min(s, 64)
    last = (s - 1) // 256 * 256  # first latent of the last chunk
    h = (torch.randn(n, s, generator=g) - 2.5).clamp(max=2.9)
    big = torch.zeros(n, s, dtype=torch.bool)
    n0 = min(3, (s - last + 1) // 2)
    big[0, s - 1 - 2 * torch.arange(n0)] = True
    h[0, :last] = h[0, :last].clamp(max=-0.5)
    h[1] = -1.0 - torch.rand(s, generator=g)
    big[1, torch.randperm(s, generator=g)[:cap]] = True
    big[1, s - 1] = True  # (the last latent of the row among them)
    if int(big[1].sum()) > cap:
        big[1, int(big[1, :s - 1].nonzero()[0])] = False
    rest = n * k - int(big.sum())
    assert rest > 0
    flat = torch.randperm((n - 2) * s, generator=g)[:rest] + 2 * s
    big.view(-1)[flat] = True
    assert int(big.sum()) == n * k and int(big.sum(dim=1).max()) == cap
    h = torch.where(big, 4.0 + torch.rand(n, s, generator=g), h)
    h[5, 0], h[6, s - 1], h[7, 0], h[7, s - 1] = 0.25, 0.25, 0.0, -0.0  # equal to a threshold: never kept in eval mode
    mask, _, nnz = check_select(eng, h, k, t0=0.375)
    assert torch.equal(mask, big)
    assert int(nnz[0]) == n0 and int(nnz[1]) == cap
    idx, val, nnz_g = eng.batch_topk_dense(h.cuda(), training=True)
    assert int(idx[0, 0]) >= last and int(idx[1, cap - 1]) == s - 1 and int((nnz_g == 0).sum()) > 0
    # eval mode: h > threshold elementwise and strictly (h > 0 for a threshold <= 0), whatever the threshold's sign
    for thr in (0.25, 0.0, -1.0):
        eng.threshold.fill_(thr)
        idx, val, nnz_g = eng.batch_topk_dense(h.cuda(), training=False)
        check_form(idx, val, nnz_g)
        want = h > max(thr, 0.0)
        assert torch.equal(nnz_g.cpu().long(), want.sum(dim=1)) and int(nnz_g[1]) == cap
        f, _ = rows_to_dense(idx, val, nnz_g, s)
        assert torch.equal(f.cpu(), torch.where(want, h, torch.zeros(())))
        assert float(eng.threshold) == thr
    assert eng.row_regrows == 0 and eng.row_cap == cap
    eng.close()


# ------------------------------------------------------------------------------------------------
# 6. values at the edges of the key order
# ------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("k", [1, 16, 28])
def test_values_at_the_edges_of_the_key_order(k, encoder_mode):
    # 32 x 64 = 2048 entries: 300 positive (with +inf, the largest and the smallest normal and denormals), 500 zeros of both signs in
    # random order, the others negative (with the negative counterparts and -inf).  k = 1: the cut is among the positives; k = 16:
    # n k = 512, so 212 of the 500 zeros are kept, +0 and -0 alike as ONE tie run in flat order; k = 28: n k = 896, the cut is among
    # the negatives, and the negative denormals and the smallest normal lie above it.
    n, s = 32, 64
    g = torch.Generator().manual_seed(6)
    fi = torch.finfo(torch.float32)
    pos = torch.rand(300, generator=g) + 0.5
    neg = -(torch.rand(n * s - 800, generator=g) + 0.5)
    pos[:7] = torch.tensor([float("inf"), fi.max, fi.tiny, 2.0 ** -140, 2.0 ** -149, 3 * 2.0 ** -149, fi.tiny * (1 - 2.0 ** -23)])
    neg[:7] = -pos[:7]
    zeros = torch.zeros(500)
    zeros[torch.randperm(500, generator=g)[:250]] = -0.0
    flat = torch.cat([pos, zeros, neg])[torch.randperm(n * s, generator=g)]
    h = flat.view(n, s).contiguous()
    assert int((bits(h) == -(1 << 31)).sum()) == 250 and int((h == 0).sum()) == 500 and int((h == 2.0 ** -149).sum()) == 1
    eng = btk_engine(16, s, k, n)
    mask, (cut, n_above, quota, n_ties), _ = check_select(eng, h, k)
    kept_zero = mask & (h == 0)
    if k == 1:
        assert cut > 0 and mask[h == float("inf")].all()
    elif k == 16:
        assert cut == 0 and (n_above, quota, n_ties) == (300, 212, 500)
        signs = bits(h[kept_zero]) < 0
        assert 0 < int(signs.sum()) < 212, "both signs of zero must be among the kept ties"
    else:
        assert cut < 0 and kept_zero.sum() == 500 and mask[h == -fi.tiny].all() and mask[h == -(2.0 ** -149)].all()
        assert not mask[h == -float("inf")].any() and not mask[h == -fi.max].any()
    eng.close()
