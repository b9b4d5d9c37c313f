"""The analysis entries on the MI355X past their grid caps and at the radix sort's byte borders (include/saev_amd.h: LATENT AP, PROBE AP,
LATENT TOP-K, PROBE1D, SPARSE LINEAR): the grid-stride kernels of latentap.hip, latenttopk.hip, probe1d.hip and sparselinear.hip on
inputs that take them a second time round their loops, the sort with parts of 1 152 entries and fewer parts used than laid out, the
third and fourth latent pass with the sentinel latent S alone in its top byte, and the solver with row chunks of 128 to 256 rows.

The inputs are the functions of tests/analysis_scale_cases.py; test_analysis_scale_host_cpu.py checks on the CPU, from the library's
own layout functions, that they reach all that.  The references are the restatements the entries' own suites use
(latent_ap_restatement, probe_ap_restatement, latent_topk_restatement, probe1d_restatement, sparse_linear_restatement).

No tolerance is new.  AP: |ap - exact| <= (n_{j,c} + 2) 2^-49 (tests/test_gpu_latent_ap.py).  The probes' sums: 1e-12 of the terms'
magnitudes, qx to 1e-14 (tests/test_gpu_probe1d_geometry.py).  The solver: the KKT, objective and rounding bounds of
tests/test_gpu_sparse_linear.py, through its ``check_fit``.  Everything else is bit or integer equality."""

import warnings

import numpy as np
import pytest
import scipy.sparse
import torch

import analysis_scale_cases as A
import latent_ap_restatement as R
import probe1d_restatement as P1R
import probe_ap_restatement as PR
import sparse_linear_restatement as SR
from latent_topk_restatement import restate_csr, restate_padded

pytestmark = [pytest.mark.gpu, pytest.mark.encoder_modes("f32")]
DEV = "cuda"
DTYPES = {"fp32": np.float32, "fp64": np.float64}


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _csr(d):
    return [_cuda(d[k]) for k in ("indptr", "indices", "data")]


def _latent_ap(d, csr=None, cls=None):
    from saev_amd import engine

    csr = _csr(d) if csr is None else csr
    return engine.latent_ap(*csr, d["n"], d["s"], d["c"], labels=_cuda(d["cls"] if cls is None else cls))


def _probe_ap(d, dtype, w, b, csr=None, cls=None, top_k=0):
    from saev_amd import engine

    csr = _csr(d) if csr is None else csr
    return engine.probe_ap(*csr, d["n"], d["s"], d["c"], labels=_cuda(d["cls"] if cls is None else cls), weights=_cuda(w.astype(dtype)),
                           biases=_cuda(b.astype(dtype)), top_k=top_k)


def _sorted(res):
    """(starts, key bits, latent, row of the events; the latent of every entry behind them) on the host."""
    starts, key, latent, row = (t.cpu().numpy() for t in res.sorted_events())
    nnz, lay = res.shape[3], res.layout
    every = res._ws[lay.off_latent:lay.off_latent + 4 * nnz].view(torch.int32).cpu().numpy()
    return starts, key.view(np.uint32), latent, row, every[len(latent):]


def _check_sorted(got, d):
    """The sort's one right answer: starts, latent, key and row equal numpy's lexsort, and every entry that is no event (a stored
    +-0.0) carries the sentinel latent S behind the events."""
    starts, key, latent, row, behind = got
    w_starts, w_lat, w_val, w_row = R.sorted_events(d["indptr"], d["indices"], d["data"], d["s"])
    np.testing.assert_array_equal(starts, w_starts)
    np.testing.assert_array_equal(latent, w_lat.astype(np.int32))
    np.testing.assert_array_equal(key, R.value_key(w_val))
    np.testing.assert_array_equal(row, w_row.astype(np.int32))
    assert starts[d["s"]] == len(w_lat) == int((d["data"] != 0).sum())
    assert len(behind) == int((d["data"] == 0).sum()) and (behind.view(np.uint32) == d["s"]).all()


def _check_ap(ap, exact, n_ev, what):
    miss = np.abs(ap - exact) / R.bound(n_ev)
    j, c = np.unravel_index(np.argmax(miss), miss.shape)
    print(f"{what}: largest |ap - exact| / bound = {miss.max():.3g} at latent {j}, class {c} ({n_ev[j, c]} events)")
    assert (miss <= 1.0).all()


# ---- past_cap: latent AP and probe AP -------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def past_cap():
    """The design, its CSR on the device and latent AP's result on it: built once, shared, left unchanged."""
    d = A.past_cap()
    csr = _csr(d)
    return d, csr, _latent_ap(d, csr)


def test_latent_ap_sorts_past_the_cap_to_the_one_right_answer(past_cap):
    """la_init_kernel's second trip (entries 2 097 152 .. 2 239 999: keys, sentinels and rows of the last 4 464 rows) and la_sort with
    1 945 of 2 048 parts used, 18 groups of 64 each."""
    d, _, res = past_cap
    assert (res.layout.parts, res.layout.part_len) == (A.LA_MAX_PARTS, 1152)
    _check_sorted(_sorted(res), d)


def test_latent_ap_past_the_cap_against_the_exact_evaluation(past_cap):
    d, _, res = past_cap
    exact, pos, n_ev = R.exact_ap(d["indptr"], d["indices"], d["data"], d["n"], d["s"], d["cls"], d["c"])
    ap = res.ap.cpu().numpy()
    assert ap.shape == (d["s"], d["c"]) and ap.dtype == np.float64
    np.testing.assert_array_equal(res.n_pos.cpu().numpy(), pos)
    _check_ap(ap, exact, n_ev, "past_cap")
    best_class = res.best_class.cpu().numpy()
    assert (best_class == np.argmax(ap, axis=1)).all() and best_class.dtype == np.int32
    np.testing.assert_array_equal(res.best_ap.cpu().numpy(), ap.max(axis=1))


@pytest.mark.parametrize("dt", list(DTYPES))
def test_probe_ap_past_the_cap_against_the_exact_evaluation(past_cap, dt):
    """pa_values_kernel's second trip on finite values, the shared sort, and the walk over latents of 46 000 events."""
    d, csr, latent = past_cap
    w, b = A.past_cap_weights(d)
    res = _probe_ap(d, DTYPES[dt], w, b, csr)
    x = PR.exact_ap(d["indptr"], d["indices"], d["data"], d["n"], d["s"], d["cls"], d["c"], w.astype(DTYPES[dt]), b.astype(DTYPES[dt]))
    np.testing.assert_array_equal(res.n_pos.cpu().numpy(), x["pos"])
    _check_ap(res.ap.cpu().numpy(), x["ap"], x["n_ev"], f"past_cap {dt}")
    np.testing.assert_array_equal(res.tp.cpu().numpy(), x["tp"])
    np.testing.assert_array_equal(res.n_pred_pos.cpu().numpy(), x["pred_pos"])
    for got, want in zip(_sorted(res), _sorted(latent)):  # the same sort, the same arrays left behind
        np.testing.assert_array_equal(got, want)


def _last_entry(csr, *, index=None, value=None):
    """The device CSR with its last stored entry replaced."""
    indptr, indices, data = csr
    if index is not None:
        indices = indices.clone()
        indices[-1] = index
    if value is not None:
        data = data.clone()
        data[-1] = value
    return [indptr, indices, data]


def test_a_column_index_out_of_range_in_the_last_entry_sets_the_error_word(past_cap):
    d, csr, _ = past_cap
    w, b = A.past_cap_weights(d)
    bad = _last_entry(csr, index=d["s"])
    res = _latent_ap(d, bad)
    with pytest.raises(ValueError, match="column index"):
        res.ap
    res = _probe_ap(d, np.float32, w, b, bad)
    with pytest.raises(ValueError, match="column index"):
        res.ap
    _latent_ap(d, csr).ap  # and a good call after them is good


@pytest.mark.parametrize("value", [np.inf, np.nan], ids=["inf", "nan"])
def test_a_value_that_is_not_finite_in_the_last_entry_sets_the_error_word(past_cap, value):
    d, csr, _ = past_cap
    w, b = A.past_cap_weights(d)
    res = _probe_ap(d, np.float32, w, b, _last_entry(csr, value=value))
    with pytest.raises(ValueError, match="not finite"):
        res.ap
    _probe_ap(d, np.float32, w, b, csr).ap


def test_a_class_id_out_of_range_on_the_last_row_sets_the_error_word(past_cap):
    d, csr, _ = past_cap
    w, b = A.past_cap_weights(d)
    bad = d["cls"].copy()
    bad[d["n"] - 1] = d["c"]
    with pytest.raises(ValueError, match="class id"):
        _latent_ap(d, csr, cls=bad).ap
    with pytest.raises(ValueError, match="class id"):
        _probe_ap(d, np.float64, w, b, csr, cls=bad).tp
    _probe_ap(d, np.float64, w, b, csr).tp


def test_top_rows_past_the_cap_equal_numpys_lexsort():
    """pa_top_rows_kernel with S * top_k = 2 099 200 outputs: the lists of latents 8 192 .. 8 199 are its second trip."""
    d = A.top_rows_design()
    k = A.TOP_ROWS["top_k"]
    assert d["s"] * k > A.GRID_CAP_ENTRIES
    got = _probe_ap(d, np.float32, d["w"], d["b"], top_k=k).top_rows.cpu().numpy()
    assert got.shape == (d["s"], k) and got.dtype == np.int64
    want = PR.top_rows(d["indptr"], d["indices"], d["data"], d["s"], k)
    first = A.GRID_CAP_ENTRIES // k
    assert want[first:].any() and want[:first].any()
    np.testing.assert_array_equal(got, want)


# ---- the radix byte edges of the latent key -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("s", A.RADIX_S)
def test_latent_passes_at_a_byte_border_of_the_key(s):
    """One to four latent passes with events on both sides of every byte border below S; at S = 256, 65 536 and 2^24 the sentinel S is
    the only key with a bit in the last pass's byte.  A latent stands alone, so the rows of the used latents are those of the same
    columns renumbered 0, 1, 2, ... in a design of at most ten latents, and every other row is the row of a latent without events."""
    wide, compact, used = A.radix_edges(s)
    res = _latent_ap(wide)
    assert res.layout.passes == A.RADIX_PASSES[s]
    _check_sorted(_sorted(res), wide)

    ap = res.ap.cpu().numpy()
    small = _latent_ap(compact).ap.cpu().numpy()
    bits, small_bits = ap.view(np.uint64), small.view(np.uint64)
    np.testing.assert_array_equal(bits[used], small_bits[:-1])
    exact, pos, n_ev = R.exact_ap(*(compact[k] for k in ("indptr", "indices", "data", "n", "s", "cls", "c")))
    np.testing.assert_array_equal(res.n_pos.cpu().numpy(), pos)
    _check_ap(small, exact, n_ev, f"S = {s}, compact")
    unused = np.ones(s, dtype=bool)
    unused[used] = False
    assert unused.sum() == s - len(used) > 0 and (n_ev[-1] == 0).all()
    assert (bits[unused] == small_bits[-1]).all()  # (small[-1] lies within the bound of the exact value of a latent without events, above)
    np.testing.assert_array_equal(res.best_ap.cpu().numpy(), ap.max(axis=1))
    np.testing.assert_array_equal(res.best_class.cpu().numpy(), np.argmax(ap, axis=1))


# ---- past_cap: latent top-k -----------------------------------------------------------------------------------------------------------------

def _lists(s, k):
    from saev_amd.engine import LatentTopK

    return LatentTopK(s, k, DEV)


def _same(acc, want):
    got = acc.read()
    values, rows = got.values.numpy(), got.indices.numpy()
    assert values.dtype == np.float32 and rows.dtype == np.int64 and values.shape == want[0].shape
    np.testing.assert_array_equal(values.view(np.int32), want[0].view(np.int32))
    np.testing.assert_array_equal(rows, want[1])
    np.testing.assert_array_equal(got.counts.numpy(), want[2])


TAILS = {"tail_as_is": lambda d: d, "tail_doubled": A.past_cap_tail_doubled}


def _first_trip_rows(want, k):
    """Whether the lists hold rows of the first trip, and of the second."""
    first_row = A.GRID_CAP_ENTRIES // A.PAST_CAP["per_row"]
    assert (want[2] == k).all()
    return bool((want[1] < first_row).any()), bool((want[1] >= first_row).any())


@pytest.mark.parametrize("tail", list(TAILS))
@pytest.mark.parametrize("k", [8, 64])
def test_latent_topk_of_the_whole_csr_in_one_call(past_cap, k, tail):
    """lt_count_kernel and lt_place_kernel over 2 240 000 stored entries, every one of them a candidate, the last 142 848 of them
    counted and placed in the second trip.  Among tied values the lowest rows win: as the design stands every list entry comes from
    the first trip, with the tail's values doubled every one comes from the second."""
    d = TAILS[tail](past_cap[0])
    acc = _lists(d["s"], k)
    acc.add_csr(*_csr(d), row_base=0)
    want = restate_csr(d["indptr"], d["indices"], d["data"], d["s"], k)
    assert _first_trip_rows(want, k) == ((True, False) if tail == "tail_as_is" else (False, True))
    _same(acc, want)


@pytest.mark.parametrize("tail", list(TAILS))
@pytest.mark.parametrize("k", [8, 64])
def test_latent_topk_of_padded_rows_in_one_call_and_in_eight(past_cap, k, tail):
    """The padded form over 70 000 x 32 slots with row counts of 0 .. 34 and a keep mask; one update and eight give the same bits."""
    d = TAILS[tail](past_cap[0])
    idx, val, row_nnz, keep = A.past_cap_padded(d)
    n = d["n"]
    assert idx.size > A.GRID_CAP_ENTRIES
    one = _lists(d["s"], k)
    one.add(_cuda(idx), _cuda(val), _cuda(row_nnz), _cuda(keep), row_base=0)
    want = restate_padded(idx, val, d["s"], k, row_nnz=row_nnz, keep=keep)
    assert _first_trip_rows(want, k) == ((True, False) if tail == "tail_as_is" else (False, True))
    _same(one, want)
    eight = _lists(d["s"], k)
    for part in np.array_split(np.arange(n), 8):
        lo, hi = int(part[0]), int(part[-1]) + 1
        assert (hi - lo) * idx.shape[1] < A.GRID_CAP_ENTRIES
        eight.add(_cuda(idx[lo:hi]), _cuda(val[lo:hi]), _cuda(row_nnz[lo:hi]), _cuda(keep[lo:hi]), row_base=lo)
    assert torch.equal(one.top_val.view(torch.int32), eight.top_val.view(torch.int32))
    assert torch.equal(one.top_row, eight.top_row) and torch.equal(one.top_cnt, eight.top_cnt)


def test_helpers_csr_topk_takes_the_array_as_one_block_past_the_cap(past_cap, monkeypatch):
    from saev_amd import helpers
    from saev_amd.engine import LatentTopK

    blocks = []
    orig = LatentTopK.add_csr
    monkeypatch.setattr(LatentTopK, "add_csr", lambda self, indptr, indices, *a, **kw: (blocks.append(indices.numel()), orig(self, indptr, indices, *a, **kw))[1])
    for tail in TAILS.values():
        d = tail(past_cap[0])
        arr = scipy.sparse.csr_array((d["data"], d["indices"], d["indptr"]), shape=(d["n"], d["s"]))
        del blocks[:]
        got = helpers.csr_topk(arr, k=8)
        assert blocks == [arr.nnz] and arr.nnz > A.GRID_CAP_ENTRIES  # the default block size: one update
        want = restate_csr(d["indptr"], d["indices"], d["data"], d["s"], 8)
        assert isinstance(got, helpers.NumpyTopK) and got.values.dtype == np.float32 and got.indices.dtype == np.int64
        np.testing.assert_array_equal(got.values.view(np.int32), want[0].view(np.int32))
        np.testing.assert_array_equal(got.indices, want[1])


# ---- past_cap: the probes' prepare ----------------------------------------------------------------------------------------------------------

def _prepare(d, indices=None):
    from saev_amd import engine

    assert engine.Probe1D.CHUNK == A.P1.CHUNK
    p = engine.Probe1D(d.n, d.s, d.c, d.nnz, DEV)
    return p.prepare(_cuda(d.indptr), _cuda(d.indices if indices is None else indices), _cuda(d.data), y=_cuda(d.ymat))


def test_probe1d_prepare_and_stats_past_the_cap(past_cap):
    """p1_count_kernel's second trip feeds the counters of the last 64 of 1 000 used parts (1 024 laid out, 35 groups of 64 each):
    everything prepare leaves as tests/test_gpu_probe1d_geometry.py checks it, and one stats call on the sorted events."""
    d = A.past_cap_probe1d(past_cap[0])
    p = _prepare(d)
    assert (p.layout.parts, A.P1.parts_of(d.s, d.nnz)[1]) == (1024, 2240)
    starts, rows, vals, qx = P1R.prepare(*d.csr, d.s)
    np.testing.assert_array_equal(p.starts.cpu().numpy(), starts)
    np.testing.assert_array_equal(p.chunk_starts.cpu().numpy(), np.concatenate([[0], np.cumsum(-(-np.diff(starts) // A.P1.CHUNK))]))
    np.testing.assert_array_equal(p.row.cpu().numpy(), rows)  # ascending inside every latent: the stable order
    np.testing.assert_array_equal(p.val.cpu().numpy().view(np.uint32), vals.view(np.uint32))
    np.testing.assert_allclose(p.qx.cpu().numpy(), qx, rtol=1e-14, atol=0)
    np.testing.assert_array_equal(p.pos.cpu().numpy(), d.ymat.sum(axis=0))
    np.testing.assert_array_equal(p.ybits.cpu().numpy().view(np.uint32), P1R.pack_bits(d.ymat))

    b, w = A.stats_coefficients(d)
    want, mag = P1R.event_sums(starts, rows, vals, d.ymat, b, w)
    got = p.stats(_cuda(b), _cuda(w)).cpu().numpy()
    err, band = np.abs(got - want), 1e-12 * mag + 1e-300
    print("largest error / band per sum:", dict(zip(P1R.SUM_NAMES, (err / band).max(axis=(0, 2)).round(6))))
    assert np.isfinite(want).all()
    for q, name in enumerate(P1R.SUM_NAMES):
        assert (err[:, q] <= band[:, q]).all(), name
    again = p.stats(_cuda(b), _cuda(w)).cpu().numpy()
    np.testing.assert_array_equal(again.view(np.uint64), got.view(np.uint64))


def test_probe1d_prepare_reports_a_column_out_of_range_in_the_last_entry(past_cap):
    d = A.past_cap_probe1d(past_cap[0])
    bad = d.indices.copy()
    bad[-1] = d.s
    with pytest.raises(ValueError, match="column index"):
        _prepare(d, bad)
    _prepare(d)  # and a good call after it is good


# ---- sparse linear --------------------------------------------------------------------------------------------------------------------------

def _fit(x, y, c, **kw):
    from saev_amd import engine

    return engine.l1_logistic(_cuda(np.ascontiguousarray(x, dtype=np.float32)), _cuda(np.asarray(y)), c, **kw)


@pytest.mark.parametrize("shape", list(A.LONG_CHUNKS), ids=["x".join(map(str, s)) for s in A.LONG_CHUNKS])
def test_row_chunks_longer_than_64(shape):
    """sl_grad_kernel over chunks of 128, 192 and 256 rows with a ragged last one, sl_step_kernel summing 17, 22 and 25 partial
    gradients: the fit against the float64 restatement, KKT and objective both ways."""
    from test_gpu_sparse_linear import check_fit

    x, y, c = A.long_chunk_design(shape)
    res = _fit(x, y, c)
    assert (res.layout.chunk_rows, res.layout.n_chunks) == A.LONG_CHUNKS[shape]
    own = SR.fista(x, y, c)
    assert own["converged"]
    check_fit(x, y, c, res, other=(own["coef"], own["intercept"]), label="long chunks")
    assert len(SR.ranked_support(res.coef_.cpu().numpy())) >= 1


def test_coefficients_past_the_cap_of_the_output_kernel():
    """sl_out_kernel with 1 280 000 coefficients: rows 53 .. 63 of coef_ are written in its second trip only.  An unfinished fit
    reports the residual and the objective of the iterate it returns, so both are recomputed on the host from that iterate."""
    n, s, k = A.OUT_SHAPE
    x, y, c = A.out_design()
    assert k * s > A.SL_OUT_CAP_ENTRIES and A.OUT_FIRST_ROW * s >= A.SL_OUT_CAP_ENTRIES
    with pytest.warns(RuntimeWarning, match="not converged"):
        short = _fit(x, y, c, max_iter=A.OUT_MAX_ITER)
    assert short.converged_ is False and short.n_iter_ == A.OUT_MAX_ITER
    w, b = short.coef_.cpu().numpy(), short.intercept_.cpu().numpy()
    assert w.shape == (k, s) and np.count_nonzero(w[A.OUT_FIRST_ROW:]) > 0 and np.count_nonzero(w[:A.OUT_FIRST_ROW]) > 0
    _, yi = SR.class_indices(y)
    eps, f = SR.kkt_residual(x, yi, k, w, b, c), SR.objective(x, yi, k, w, b, c)
    print(f"kkt host {eps:.6g} device {short.kkt_residual_:.6g}, F host {f:.17g} device {short.objective_:.17g}")
    assert abs(short.kkt_residual_ - eps) <= SR.gradient_rounding(x, n, k, c) + 1e-12 * short.kkt_residual_
    assert abs(short.objective_ - f) <= SR.objective_rounding(x, w, b, c, short.objective_)
    with pytest.warns(RuntimeWarning, match="not converged"):
        again = _fit(x, y, c, max_iter=A.OUT_MAX_ITER)
    assert torch.equal(short.coef_.view(torch.int64), again.coef_.view(torch.int64))
    assert torch.equal(short.intercept_.view(torch.int64), again.intercept_.view(torch.int64))
    assert (short.kkt_residual_, short.objective_, short.lipschitz_) == (again.kkt_residual_, again.objective_, again.lipschitz_)


def test_a_value_that_is_not_finite_past_the_cap_of_the_check_kernel():
    x, y, c = A.check_design()
    assert x.shape == A.CHECK_SHAPE[:2] and min(A.CHECK_FLAT) > A.GRID_CAP_ENTRIES and max(A.CHECK_FLAT) < x.size
    for at, value in zip(A.CHECK_FLAT, (np.inf, np.nan)):
        bad = x.copy()
        bad.reshape(-1)[at] = value
        with pytest.raises(ValueError, match="not finite"):
            _fit(bad, y, c, max_iter=1)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        assert _fit(x, y, c, max_iter=1).n_iter_ == 1  # and the same design without them is accepted
