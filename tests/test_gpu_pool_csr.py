"""GPU tests of POOL CSR (include/saev_amd.h): engine.pool_csr on every case of tests/pool_csr_cases.py against the
numpy restatement (tests/pool_csr_restatement.py) and, at threshold 0, against the path it replaces (pool_images, the clamp and
torch's nonzero conversion, kept inline here); determinism, independence of other images, the C entries on an exact workspace with
poisoned outputs, the error words, the hand-over to latent_auroc, mimics.max_pool_sparse, and one run whose dense form would not fit.

No tolerance anywhere: every output must EQUAL the restatement, floats compared on the bits.

The one-line errors the cases catch:
  ``>=`` for ``>``                   ``values_thr_half`` and ``vector_thresholds`` store values equal to the threshold, ``values_thr_0`` zeros of both signs
  a signed compare of value bits     ``values_*`` (denormals, FLT_MAX), every random design (a third of the values are negative)
  the higher patch on equal values   ``patches`` (latents 2, 3), the random designs (values on a grid of quarters)
  a repeat counted once / maxed twice ``columns``
  a slot from the wrong word prefix  ``s_65``, ``s_range_*``, ``full_row``, ``vector_random`` (sets with holes, past one word and one range)
  a range border                     ``s_range_minus_1``, ``s_range``, ``s_range_plus_1``, ``s_70001``, ``full_row``
  a span assumed short               ``long_span`` (70 000 entries of one image), ``full_row``
  units past the grid, the scan      ``many_images`` (70 000 units: two rounds of the grid, 18 chunks of the scan)
  an empty image's start             ``spans``, ``no_entries``, ``full_row`` (image 1), ``many_images``
  an output left as it was           the outputs are poisoned before the C entries run, and nothing past the end may change"""

import ctypes as C
import functools

import numpy as np
import pytest
import scipy.sparse
import torch

import pool_csr_cases as K
import pool_csr_restatement as R
from saev_amd.engine import pool_csr  # noqa: F401  (without the feature nothing here can run)

pytestmark = [pytest.mark.gpu, pytest.mark.encoder_modes("f32")]
DEV = "cuda"


@functools.lru_cache(maxsize=None)
def _case(name):
    return K.SMALL[name]()


@functools.lru_cache(maxsize=None)
def _expected(name):
    return R.restate(**_case(name))


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _run(c, details=True):
    from saev_amd import engine

    thr = c["thr"] if np.ndim(c["thr"]) == 0 else _t(c["thr"])
    return engine.pool_csr(_t(c["indptr"]), _t(c["indices"]), _t(c["data"]), c["n_images"], c["t"], c["s"], threshold=thr, details=details)


def _host(res, names=R.ARRAYS):
    return {name: getattr(res, name).cpu().numpy() for name in names}


def _assert_equal(got, want, names=R.ARRAYS):
    for name in names:
        assert got[name].dtype == want[name].dtype and got[name].shape == want[name].shape, (name, got[name].dtype, got[name].shape, want[name].shape)
        bad = np.flatnonzero(R.bits(got[name]) != R.bits(want[name]))
        assert bad.size == 0, (name, bad[:5].tolist(), got[name][bad[0]], want[name][bad[0]])


@pytest.mark.parametrize("name", list(K.SMALL))
def test_equals_the_restatement_with_and_without_details_twice(name):
    c = _case(name)
    res = _run(c)
    got = _host(res)
    _assert_equal(got, _expected(name))
    assert res.nnz == len(_expected(name)["indices"]) and got["indptr"][0] == 0
    plain = _run(c, details=False)
    assert plain.patch is None and plain.count is None
    _assert_equal(_host(plain, R.ARRAYS[:3]), _expected(name), R.ARRAYS[:3])  # the details change nothing else
    _assert_equal(_host(_run(c)), got)  # two calls give the same bits


def _parent_path(c):
    """What the workers did before: the dense pooled maximum, clamped at 0, and torch's conversion of its non-zero entries."""
    from saev_amd import engine

    pooled = torch.clamp_min(engine.pool_images(_t(c["indptr"]), _t(c["indices"]), _t(c["data"]), c["n_images"], c["t"], c["s"], "max").pooled, 0.0)
    at = pooled != 0
    indptr = torch.zeros(c["n_images"] + 1, device=DEV, dtype=torch.int64)
    indptr[1:] = torch.cumsum(at.sum(dim=1), dim=0)
    return indptr, at.nonzero()[:, 1].to(torch.int32), pooled[at]


# canonical rows only: pool_images leaves a column stored twice in a row unspecified
DENSE = [n for n, make in K.SMALL.items() if K.densifiable(make()) and np.ndim(make()["thr"]) == 0 and make()["thr"] == 0 and n != "columns"]


@pytest.mark.parametrize("name", DENSE)
def test_threshold_0_equals_the_dense_detour(name):
    c = _case(name)
    got = _run(c, details=False)
    for mine, theirs in zip(got.triple(), _parent_path(c)):
        assert mine.dtype == theirs.dtype and mine.shape == theirs.shape
        assert torch.equal(mine.view(torch.int32) if mine.dtype == torch.float32 else mine, theirs.view(torch.int32) if theirs.dtype == torch.float32 else theirs)


@pytest.mark.parametrize("name", ["tokens_16", "tokens_257", "s_range_plus_1", "vector_random"])
def test_an_image_alone_and_permuted_images(name):
    c, want = _case(name), _expected(name)
    n = c["n_images"]
    for i in (0, n // 2, n - 1):
        alone = _host(_run(K.one_image_of(c, i)))
        lo, hi = want["indptr"][i : i + 2]
        assert alone["indptr"].tolist() == [0, hi - lo]
        _assert_equal(alone, {k: want[k][lo:hi] for k in R.ARRAYS[1:]}, R.ARRAYS[1:])
    perm = np.random.default_rng(0).permutation(n)
    moved = _host(_run(K.permuted(c, perm)))
    assert np.array_equal(np.diff(moved["indptr"]), np.diff(want["indptr"])[perm])
    for q, i in enumerate(perm):
        lo, hi = want["indptr"][i : i + 2]
        at = moved["indptr"][q]
        _assert_equal({k: moved[k][at : at + hi - lo] for k in R.ARRAYS[1:]}, {k: want[k][lo:hi] for k in R.ARRAYS[1:]}, R.ARRAYS[1:])


POISON_I, POISON_F, TAIL = -77, -123.5, 64


@pytest.mark.parametrize("name", ["spans", "s_range_plus_1", "full_row", "no_entries", "vector_thresholds"])
def test_c_entries_on_an_exact_workspace_write_every_output_once_and_nothing_past_the_end(name):
    from saev_amd import _lib

    lib = _lib.load()
    c, want = _case(name), _expected(name)
    n, t, s, nnz_in = c["n_images"], c["t"], c["s"], len(c["data"])
    ptr = lambda x: None if x is None else C.c_void_p(x.data_ptr())  # noqa: E731
    indptr, indices, data = _t(c["indptr"]), _t(c["indices"]), _t(c["data"])
    thr_vec = None if np.ndim(c["thr"]) == 0 else _t(c["thr"])
    need = lib.saev_pool_csr_workspace_bytes(n, t, s, nnz_in)
    assert need == R.workspace_bytes(n, s, K.RANGE)
    ws = torch.full((need + 256,), 0x5A, device=DEV, dtype=torch.uint8)
    out_indptr = torch.full((n + 1 + TAIL,), POISON_I, device=DEV, dtype=torch.int64)
    err = torch.full((1,), 9, device=DEV, dtype=torch.int32)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    head = (ptr(indptr), ptr(indices) if nnz_in else None, ptr(data) if nnz_in else None, nnz_in, n, t, s, 0.0 if thr_vec is not None else float(c["thr"]), ptr(thr_vec))
    assert lib.saev_pool_csr_count(*head, ptr(out_indptr), ptr(ws), need, ptr(err), stream) == 0, lib.saev_last_error(None)
    assert err.item() == 0 and np.array_equal(out_indptr[: n + 1].cpu().numpy(), want["indptr"]) and (out_indptr[n + 1 :] == POISON_I).all()
    assert (ws[need:] == 0x5A).all()
    nnz = int(want["indptr"][-1])
    i32 = lambda: torch.full((nnz + TAIL,), POISON_I, device=DEV, dtype=torch.int32)  # noqa: E731
    out = dict(indices=i32(), data=torch.full((nnz + TAIL,), POISON_F, device=DEV), patch=i32(), count=i32())
    err.fill_(9)
    rc = lib.saev_pool_csr_fill(*head, ptr(out_indptr), ptr(out["indices"]), ptr(out["data"]), ptr(out["patch"]), ptr(out["count"]), ptr(ws), need, ptr(err), stream)
    assert rc == 0 and err.item() == 0, lib.saev_last_error(None)
    for key, poison in (("indices", POISON_I), ("data", POISON_F), ("patch", POISON_I), ("count", POISON_I)):
        assert (out[key][nnz:] == poison).all(), key
    _assert_equal({k: v[:nnz].cpu().numpy() for k, v in out.items()}, want, R.ARRAYS[1:])
    assert (ws[need:] == 0x5A).all() and (out_indptr[n + 1 :] == POISON_I).all()
    # one detail array alone, the other switched off
    only = i32()
    rc = lib.saev_pool_csr_fill(*head, ptr(out_indptr), ptr(out["indices"]), ptr(out["data"]), None, ptr(only), ptr(ws), need, ptr(err), stream)
    assert rc == 0 and err.item() == 0 and np.array_equal(only[:nnz].cpu().numpy(), want["count"]) and (only[nnz:] == POISON_I).all()


@pytest.mark.parametrize("kind", K.BROKEN)
def test_error_words(kind):
    c, code = K.broken(kind)
    res = _run(c)
    assert int(res._err.item()) == code
    with pytest.raises(ValueError, match="found on the device"):
        res.indices
    with pytest.raises(ValueError, match="found on the device"):  # a bad call raises on every read
        res.check()
    good = _run(K.random_design(21, 4, 3, 40, 8))  # the same design without the fault
    assert int(good._err.item()) == 0 and good.nnz > 0


def test_the_triple_feeds_latent_auroc_as_the_dense_detours_triple_did():
    from saev_amd import engine

    c = _case("tokens_16")
    n, s = c["n_images"], c["s"]
    cls = _t(np.asarray([0, 1, 0, 1, 1, -1, 0], dtype=np.int32))
    roles = _t(np.asarray([[1, 2], [2, 1]], dtype=np.uint8))
    mine = engine.latent_auroc(*_run(c, details=False).triple(), n, s, 2, labels=cls, roles=roles)
    theirs = engine.latent_auroc(*_parent_path(c), n, s, 2, labels=cls, roles=roles)
    for key in ("auroc", "u2", "n_pos", "n_neg", "fire_pos", "fire_neg", "sum_pos", "sum_neg"):
        a, b = getattr(mine, key).cpu().numpy(), getattr(theirs, key).cpu().numpy()
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8)), key
    assert np.isfinite(mine.auroc.cpu().numpy()).any()


@pytest.mark.parametrize("name", ["tokens_5", "values_thr_0", "s_range_plus_1"])
def test_max_pool_sparse_equals_the_csr_of_max_pool_csr(name):
    from saev_amd import mimics

    c = _case(name)
    ta = scipy.sparse.csr_matrix((c["data"], c["indices"], c["indptr"]), shape=(c["n_images"] * c["t"], c["s"]))
    got = mimics.max_pool_sparse(ta, c["n_images"], c["t"], device=DEV)
    want = scipy.sparse.csr_matrix(mimics.max_pool_csr(ta, c["n_images"], c["t"], device=DEV))
    assert isinstance(got, scipy.sparse.csr_matrix) and got.shape == want.shape and got.dtype == want.dtype == np.float32
    assert np.array_equal(got.indptr, want.indptr) and np.array_equal(got.indices, want.indices) and np.array_equal(R.bits(got.data), R.bits(want.data))
    assert got.has_sorted_indices


def test_a_run_whose_dense_form_would_not_fit():
    """200 000 images x 70 001 latents: 56 GB dense.  The result against the restatement, and the peak of device memory against the
    workspace, the outputs at their largest (every stored entry an output entry: 16 bytes each with the details) and the caching
    allocator's rounding (a large block is rounded up to a multiple of 2 MiB; seven allocations)."""
    from saev_amd import _lib

    c = K.huge()
    n, s, nnz_in = c["n_images"], c["s"], len(c["data"])
    assert n * s * 4 > 55e9
    want = R.restate(**c)
    args = (_t(c["indptr"]), _t(c["indices"]), _t(c["data"]))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    from saev_amd import engine

    res = engine.pool_csr(*args, n, c["t"], s, details=True)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    nnz = res.nnz
    assert nnz <= nnz_in
    bound = _lib.load().saev_pool_csr_workspace_bytes(n, c["t"], s, nnz_in) + 8 * (n + 1) + 16 * nnz_in + 7 * (2 << 20)
    assert peak <= bound < 64e6, (peak, bound)
    _assert_equal(_host(res), want)
