"""Host-side tests of the analysis entries' scale designs (tests/analysis_scale_cases.py; no GPU needed): from the library's own layout
functions and from the kernels' launch lines, that the arrays tests/test_gpu_analysis_scale.py runs do pass the grid caps, do leave
parts of the sort unused, do take the latent passes they are named for and do make row chunks longer than 64 -- so that a change of a
constant cannot quietly turn those tests into small ones."""

import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import analysis_scale_cases as A
import latent_ap_restatement as R
import sparse_linear_restatement as SR
from conftest import ROOT
from latent_topk_restatement import restate_csr

CSRC = ROOT / "saev_amd" / "csrc"


def _lib():
    subprocess.run(["make", "-C", str(ROOT)], check=True, capture_output=True)
    from saev_amd import _lib

    return _lib, _lib.load()


@pytest.fixture(scope="module")
def past_cap():
    return A.past_cap()


def test_the_restated_caps_are_the_launch_lines():
    """Every grid-stride launch of the four units is capped as analysis_scale_cases restates it."""
    capped = r"std::min<(?:int64_t|size_t)>\(\((?:nnz|total|S \* \(int64_t\)top_k) \+ 255\) / 256, (\d+)\)"
    want = {"latentap.hip": [8192, 8192, 8192], "latenttopk.hip": [8192], "probe1d.hip": [8192], "sparselinear.hip": [8192, 4096]}
    for name, caps in want.items():
        assert [int(m) for m in re.findall(capped, (CSRC / name).read_text())] == caps, name
    assert A.GRID_CAP_ENTRIES == 8192 * 256 and A.SL_OUT_CAP_ENTRIES == 4096 * 256
    text = (CSRC / "latentap.hip").read_text()
    assert re.search(r"LA_MAX_PARTS = (\d+);", text).group(1) == str(A.LA_MAX_PARTS)


def test_past_cap_passes_the_caps_and_leaves_parts_unused(past_cap):
    lib_mod, lib = _lib()
    d = past_cap
    n, s, c, per_row = (A.PAST_CAP[k] for k in ("n", "s", "c", "per_row"))
    nnz = len(d["data"])
    assert (d["n"], d["s"], d["c"]) == (n, s, c) == (70_000, 48, 5) and nnz == n * per_row == 2_240_000 and d["indptr"][0] == 0
    assert (np.diff(d["indptr"]) == per_row).all() and (np.diff(d["indices"].reshape(n, per_row), axis=1) > 0).all()
    # the second trip: entries from the cap on, which are whole rows, and not just the last one
    assert nnz > A.GRID_CAP_ENTRIES
    last_below = int(np.searchsorted(d["indptr"], A.GRID_CAP_ENTRIES, side="right")) - 2  # the last row whose entries all lie below the cap
    assert last_below == A.GRID_CAP_ENTRIES // per_row - 1 == 65_535 < n - 1 and d["indptr"][last_below + 1] == A.GRID_CAP_ENTRIES
    # values: k / 4, every third latent signed with about 40 % negative values, a few dozen tie groups a latent
    dense_k = np.abs(d["data"]) * 4
    assert (dense_k == np.round(dense_k)).all() and dense_k.max() == 32
    for j in range(s):
        v = d["data"][d["indices"] == j]
        share = float((v < 0).mean())
        assert (0.37 < share < 0.43) if j % 3 == 0 else share == 0.0
        assert 30 <= len(np.unique(v[v != 0])) <= 64 and len(v) > 40_000
    # sentinels made by the second trip, of both signs, one of them in the last row
    zero_at = np.flatnonzero(d["data"] == 0)
    assert len(zero_at) == A.PAST_CAP_ZEROS and zero_at.min() >= A.GRID_CAP_ENTRIES and zero_at.max() >= d["indptr"][n - 1]
    assert 0 < np.signbit(d["data"][zero_at]).sum() < len(zero_at)
    assert (d["cls"] == -1).any() and set(d["cls"].tolist()) == set(range(-1, c))
    # latent AP's sort: all 2 048 parts laid out, 18 groups of 64 in each, and fewer of them used
    L = lib_mod.SaevLatentAPLayout()
    assert lib.saev_latent_ap_layout_of(n, s, c, nnz, C.byref(L)) == 0
    assert L.parts == A.LA_MAX_PARTS == 2048 and L.part_len >= 640 and L.part_len % 64 == 0 and L.part_len == 1152
    assert -(-nnz // L.part_len) == 1945 < L.parts and L.passes == 5
    # the probes' counting sort
    P = lib_mod.SaevProbe1DLayout()
    assert lib.saev_probe1d_layout_of(n, s, c, nnz, C.byref(P)) == 0
    assert A.P1.parts_of(s, nnz) == (1024, 2240) and P.parts == 1024
    assert -(-nnz // 2240) == 1000 and A.GRID_CAP_ENTRIES // 2240 < 999  # the second trip counts for several parts
    # seeded
    again = A.past_cap()
    assert all(np.array_equal(again[k].view(np.uint8), d[k].view(np.uint8)) for k in ("indptr", "indices", "data", "cls"))


def test_past_cap_views_for_top_k_and_the_probes(past_cap):
    d = past_cap
    first_row = A.GRID_CAP_ENTRIES // A.PAST_CAP["per_row"]
    doubled = A.past_cap_tail_doubled(d)
    assert np.array_equal(doubled["data"][:A.GRID_CAP_ENTRIES], d["data"][:A.GRID_CAP_ENTRIES])
    assert np.array_equal(doubled["data"][A.GRID_CAP_ENTRIES:], 2 * d["data"][A.GRID_CAP_ENTRIES:]) and doubled["indices"] is d["indices"]
    # which trip the lists come from: the lowest rows among the tied values as the design stands, the doubled tail otherwise
    for design, from_first in ((d, True), (doubled, False)):
        values, rows, counts = restate_csr(design["indptr"], design["indices"], design["data"], design["s"], 64)
        assert (counts == 64).all() and ((rows < first_row).all() if from_first else (rows >= first_row).all())
    idx, val, row_nnz, keep = A.past_cap_padded(d)
    assert idx.shape == val.shape == (d["n"], 32) and idx.size > A.GRID_CAP_ENTRIES and idx.dtype == np.int32 and val.dtype == np.float32
    assert row_nnz.min() == 0 and row_nnz.max() == 34 and row_nnz.dtype == np.int32 and 0.75 < keep.mean() < 0.85
    assert keep[first_row:].any() and (row_nnz[first_row:] > 0).any()
    p = A.past_cap_probe1d(d)
    assert (p.n, p.s, p.c, p.nnz) == (d["n"], d["s"], d["c"], len(d["data"])) and p.ymat.shape == (p.n, p.c)
    assert (p.ymat.sum(axis=1) == (d["cls"] >= 0)).all() and (p.ymat.sum(axis=0) == np.bincount(d["cls"][d["cls"] >= 0], minlength=p.c)).all()
    w, b = A.past_cap_weights(d)
    assert w.shape == b.shape == (d["s"], d["c"]) and ((w > 0).any(axis=1) & (w < 0).any(axis=1)).mean() > 0.8  # both signs inside a wave
    assert np.array_equal(w, w.astype(np.float32).astype(np.float64)) and np.array_equal(b, b.astype(np.float32).astype(np.float64))


def test_top_rows_design_has_lists_on_both_sides_of_the_cap():
    d = A.top_rows_design()
    n, s, c, k = (A.TOP_ROWS[key] for key in ("n", "s", "c", "top_k"))
    assert (d["n"], d["s"], d["c"]) == (n, s, c) and s * k == 2_099_200 > A.GRID_CAP_ENTRIES and k <= n
    first = A.GRID_CAP_ENTRIES // k
    assert first * k == A.GRID_CAP_ENTRIES and first == 8192 < s  # the second trip starts with a latent's first slot
    m = np.diff(R.sorted_events(d["indptr"], d["indices"], d["data"], s)[0])
    assert (m[list(A.TOP_ROWS_LONG)] > k).all() and min(A.TOP_ROWS_LONG) < first <= max(A.TOP_ROWS_LONG)
    short = m.copy()
    short[list(A.TOP_ROWS_LONG)] = 0
    assert short.max() <= 3 and (np.bincount(short, minlength=4) > 1000).all()  # most latents: 0 .. 3 events
    assert short[first - 8:first].any() and short[first:].any() and (m[first:] == 0).any()  # lists next to the border on both sides
    assert (d["data"] < 0).any() and d["w"].shape == (s, c)


@pytest.mark.parametrize("s", A.RADIX_S)
def test_radix_designs_put_the_sentinel_alone_in_its_byte(s):
    lib_mod, lib = _lib()
    wide, compact, used = A.radix_edges(s)
    c = 1 if s == 1 << 24 else 3
    assert (wide["n"], wide["s"], wide["c"]) == (A.RADIX_N, s, c) and (compact["n"], compact["s"], compact["c"]) == (A.RADIX_N, len(used) + 1, c)
    L = lib_mod.SaevLatentAPLayout()
    assert lib.saev_latent_ap_layout_of(wide["n"], s, c, len(wide["data"]), C.byref(L)) == 0
    assert L.passes == A.RADIX_PASSES[s]
    latent_bytes = L.passes - 4
    assert s >> (8 * latent_bytes) == 0 and (latent_bytes == 1 or s >> (8 * (latent_bytes - 1)) > 0)  # as many bytes as hold S
    if s in (256, 65_536, 1 << 24):  # no latent has a bit in the last pass's byte: the sentinel alone does
        assert (s - 1) >> (8 * (latent_bytes - 1)) == 0 and s >> (8 * (latent_bytes - 1)) == 1
    assert {0, 1, s - 1} <= set(used.tolist()) and set(used.tolist()) == {j for j in (0, 1, s - 1, 255, 256, 257, 65_535, 65_536, 65_537, (1 << 24) - 1) if j < s}
    assert set(np.unique(wide["indices"]).tolist()) == set(used.tolist()) and len(used) < s
    # the same entries under two numberings
    assert np.array_equal(wide["indptr"], compact["indptr"]) and np.array_equal(wide["data"].view(np.uint32), compact["data"].view(np.uint32))
    assert np.array_equal(wide["indices"], used[compact["indices"]]) and compact["indices"].max() == len(used) - 1
    assert np.array_equal(wide["cls"], compact["cls"])
    for j in used:  # quantised, signed, stored zeros of both signs in every used latent
        v = wide["data"][wide["indices"] == j]
        z = v[v == 0]
        assert len(z) == 2 * A.RADIX_ZEROS and np.signbit(z).sum() == A.RADIX_ZEROS and (v > 0).any() and (v < 0).any()
        assert (v * 4 == np.round(v * 4)).all() and len(v) - len(z) > 60
    assert compact["s"] <= 10  # (the exact evaluation walks the latents in Python: never the wide design)


@pytest.mark.parametrize("shape", list(A.LONG_CHUNKS), ids=["x".join(map(str, s)) for s in A.LONG_CHUNKS])
def test_solver_shapes_make_row_chunks_longer_than_64(shape):
    lib_mod, lib = _lib()
    n, s, k = shape
    L = lib_mod.SaevL1LogisticLayout()
    assert lib.saev_l1_logistic_layout_of(n, s, k, C.byref(L)) == 0
    assert (L.chunk_rows, L.n_chunks) == A.LONG_CHUNKS[shape] and L.chunk_rows > 64 and n > 2048
    assert n % L.chunk_rows != 0 and (n != 2049 or n - (L.n_chunks - 1) * L.chunk_rows == 1)  # a ragged last chunk
    x, y, c = A.long_chunk_design(shape)
    assert x.shape == (n, s) and x.dtype == np.float32 and len(np.unique(y)) == k
    own = SR.fista(x, y, c)
    assert own["converged"] and len(SR.ranked_support(own["coef"])) >= 1


def test_output_and_check_designs_pass_their_caps():
    lib_mod, lib = _lib()
    n, s, k = A.OUT_SHAPE
    assert k * s == 1_280_000 > A.SL_OUT_CAP_ENTRIES
    assert A.OUT_FIRST_ROW * s >= A.SL_OUT_CAP_ENTRIES > (A.OUT_FIRST_ROW - 1) * s and A.OUT_FIRST_ROW < k
    L = lib_mod.SaevL1LogisticLayout()
    assert lib.saev_l1_logistic_layout_of(n, s, k, C.byref(L)) == 0 and L.coef_rows == k
    x, y, c = A.out_design()
    assert x.shape == (n, s) and len(np.unique(y)) == k
    own = SR.fista(x, y, c, max_iter=A.OUT_MAX_ITER)
    assert not own["converged"] and own["n_iter"] == A.OUT_MAX_ITER
    assert np.count_nonzero(own["coef"][A.OUT_FIRST_ROW:]) > 0 and np.count_nonzero(own["coef"][:A.OUT_FIRST_ROW]) > 0
    n, s, k = A.CHECK_SHAPE
    assert A.GRID_CAP_ENTRIES < min(A.CHECK_FLAT) < max(A.CHECK_FLAT) == n * s - 1
    x, y, _ = A.check_design()
    assert x.shape == (n, s) and np.isfinite(x).all() and len(np.unique(y)) == k
