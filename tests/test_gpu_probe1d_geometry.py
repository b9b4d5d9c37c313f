"""The per-latent logistic probes on the MI355X where their kernels change behaviour (include/saev_amd.h: PROBE1D): the
counting sort with several groups of 64 per part and with the part count capped by S; int32 class ids and C up to 4 096; the fit
with slabs that stop at different iterations, inside and across 64-class groups, and one that never stops; evaluate in every lane
layout and at three thresholds; an absolute row_ptr, a second prepare, max_iter = 0.

The inputs are the functions of tests/probe1d_cases.py; test_probe1d_host_cpu.py checks on the CPU that they have the properties
relied on here (groups per part, which slab stops when and how far from tol, no probability on a threshold).  The references are the
fp64 restatement (tests/probe1d_restatement.py) and the device against itself: bands as in test_gpu_probe1d.py (1e-12 of the terms'
magnitudes for sums and loss, 1e-14 for qx, 1e-13 for the base intercept as for the solver step there); everything else is bit
equality or exact integers."""

import dataclasses

import numpy as np
import pytest
import torch

import csr_cases
import probe1d_cases as K
import probe1d_restatement as R

pytestmark = [pytest.mark.gpu, pytest.mark.encoder_modes("f32")]


def _engine():
    from saev_amd import engine

    assert engine.Probe1D.CHUNK == K.CHUNK
    return engine


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _probe(d, *, matrix=False, ids_dtype=None):
    p = _engine().Probe1D(d.n, d.s, d.c, d.nnz, "cuda")
    csr = [_cuda(a) for a in d.csr]
    if d.ids is None or matrix:
        return p.prepare(*csr, y=_cuda(d.ymat))
    return p.prepare(*csr, labels=_cuda(d.ids if ids_dtype is None else d.ids.astype(ids_dtype)))


def _left_by_prepare(p):
    """Everything prepare leaves, as integers (floats by their bits)."""
    return dict(starts=p.starts.cpu().numpy(), chunk_starts=p.chunk_starts.cpu().numpy(), row=p.row.cpu().numpy(),
                val=p.val.cpu().numpy().view(np.uint32), qx=p.qx.cpu().numpy().view(np.uint64), pos=p.pos.cpu().numpy(),
                ybits=p.ybits.cpu().numpy().view(np.uint32))


def _same_bits(got, want):
    assert got.keys() == want.keys()
    for key in want:
        np.testing.assert_array_equal(got[key], want[key], err_msg=key)


def _check_prepare(p, d, ref):
    starts, rows, vals, qx = ref
    got = _left_by_prepare(p)
    np.testing.assert_array_equal(got["starts"], starts)
    np.testing.assert_array_equal(got["chunk_starts"], np.concatenate([[0], np.cumsum(-(-np.diff(starts) // K.CHUNK))]))
    np.testing.assert_array_equal(got["row"], rows)  # ascending inside every latent: the stable order
    np.testing.assert_array_equal(got["val"], vals.view(np.uint32))
    np.testing.assert_allclose(p.qx.cpu().numpy(), qx, rtol=1e-14, atol=0)
    np.testing.assert_array_equal(got["pos"], d.ymat.sum(axis=0))
    np.testing.assert_array_equal(got["ybits"], R.pack_bits(d.ymat))


def _check_sums(got, want, mag, what=""):
    err = np.abs(got - want)
    band = 1e-12 * mag + 1e-300
    print(what, "largest error / band per sum:", dict(zip(R.SUM_NAMES, (err / band).max(axis=(0, 2)).round(6))))
    assert np.isfinite(want).all()
    for q, name in enumerate(R.SUM_NAMES):
        assert (err[:, q] <= band[:, q]).all(), (what, name)


def _check_stats(p, d, ref, seed):
    starts, rows, vals, _ = ref
    b, w = K.coefficients(d.s, d.c, seed)
    want, mag = R.event_sums(starts, rows, vals, d.ymat, b, w)
    got = p.stats(_cuda(b), _cuda(w)).cpu().numpy()
    _check_sums(got, want, mag)
    again = p.stats(_cuda(b), _cuda(w)).cpu().numpy()
    np.testing.assert_array_equal(again.view(np.uint64), got.view(np.uint64))
    return got


@pytest.fixture(scope="module")
def placed():
    """name -> (design, the restatement's prepare, the prepared device object), built once."""
    built = {}

    def get(name):
        if name not in built:
            d = K.PLACEMENT[name][0]()
            built[name] = (d, R.prepare(*d.csr, d.s), _probe(d))
        return built[name]

    return get


# ---- A: placement across groups and parts ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(K.PLACEMENT))
def test_prepare_and_stats_with_several_groups_of_64_per_part(placed, name):
    """The cursor that carries a latent's position from one group of 64 to the next inside a part (two_groups, four_groups), the part
    count capped by S and the scan's carries (many_latents), one latent in every lane (one_latent_rows), one row in every lane
    (long_rows): a stable sort all the same, and the sums of the sorted events."""
    d, ref, p = placed(name)
    _check_prepare(p, d, ref)
    _check_stats(p, d, ref, 400 + list(K.PLACEMENT).index(name))


def test_row_ptr_holds_absolute_positions(placed):
    """The C entry with row_ptr[0] = 777: indices and data are read from their base pointers at row_ptr's positions, and the 777
    entries in front (an index out of range, a NaN value) are never looked at."""
    engine = _engine()
    d, _, p = placed("two_groups")
    shift = K.ROW_PTR_SHIFT
    indptr = _cuda(d.indptr + shift)
    indices = _cuda(np.concatenate([np.full(shift, d.s, dtype=np.int32), d.indices]))
    data = _cuda(np.concatenate([np.full(shift, np.nan, dtype=np.float32), d.data]))
    ids = _cuda(d.ids)
    assert ids.dtype == torch.uint8 and indices.numel() == shift + d.nnz
    q = engine.Probe1D(d.n, d.s, d.c, d.nnz, "cuda")
    q._call("saev_probe1d_prepare", engine._ptr(indptr), engine._ptr(indices), engine._ptr(data), d.nnz, d.n, d.s, d.c, engine._ptr(ids), None, None)
    assert int(q.err.item()) == 0
    _same_bits(_left_by_prepare(q), _left_by_prepare(p))


def _prepare_raw(d):
    """saev_probe1d_prepare on a block whose indptr holds absolute positions, two classes, every row in class 0."""
    engine = _engine()
    q = engine.Probe1D(d["n"], d["s"], 2, d["nnz"], "cuda")
    csr = [_cuda(d[k]) for k in ("indptr", "indices", "data")]
    ids = _cuda(np.zeros(d["n"], dtype=np.uint8))
    q._call("saev_probe1d_prepare", *map(engine._ptr, csr), d["nnz"], d["n"], d["s"], 2, engine._ptr(ids), None, None)
    assert int(q.err.item()) == 0
    return q


@pytest.mark.parametrize("shift", [0, 333])
def test_rows_across_empty_rows_and_a_block_that_does_not_start_at_0(shift):
    """The row of a stored entry where indptr repeats (empty rows first, last and three in a run) and where it starts at ``shift``."""
    d = csr_cases.empty_rows_block(shift)
    q = _prepare_raw(d)
    order = csr_cases.by_latent(d, by_value=False)
    np.testing.assert_array_equal(q.starts.cpu().numpy(), np.concatenate([[0], np.cumsum(np.bincount(d["cols"], minlength=d["s"]))]))
    np.testing.assert_array_equal(q.row.cpu().numpy(), d["rows"][order])
    np.testing.assert_array_equal(q.val.cpu().numpy().view(np.uint32), d["vals"][order].view(np.uint32))


@pytest.mark.parametrize("s", [1023, 1024, 1025, 2049])
def test_starts_where_the_scan_ends_a_round(s):
    """One latent short of a round of 1 024, exactly one, one more, and one more than two: starts and chunk_starts are the running
    sums of the counts and of the chunk counts, the last latent holding two chunks."""
    d = csr_cases.scan_rounds_block(s)
    q = _prepare_raw(d)
    counts = np.bincount(d["indices"], minlength=s)
    assert counts[s - 1] == d["n"] > K.CHUNK
    np.testing.assert_array_equal(q.starts.cpu().numpy(), np.concatenate([[0], np.cumsum(counts)]))
    np.testing.assert_array_equal(q.chunk_starts.cpu().numpy(), np.concatenate([[0], np.cumsum(-(-counts // K.CHUNK))]))
    rows = np.repeat(np.arange(d["n"]), 6)
    np.testing.assert_array_equal(q.row.cpu().numpy(), rows[np.lexsort((rows, d["indices"]))])


def test_a_second_prepare_leaves_what_a_first_one_would(placed):
    d, ref, p = placed("four_groups")
    other = K.four_groups_other()
    q = _probe(other)
    _check_prepare(q, other, R.prepare(*other.csr, other.s))
    q.prepare(*[_cuda(a) for a in d.csr], labels=_cuda(d.ids))
    _same_bits(_left_by_prepare(q), _left_by_prepare(p))
    b, w = (_cuda(a) for a in K.coefficients(d.s, d.c, 410))
    np.testing.assert_array_equal(q.stats(b, w).cpu().numpy().view(np.uint64), p.stats(b, w).cpu().numpy().view(np.uint64))


# ---- B: labels ------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def labelled():
    built = {}

    def get(c):
        if c not in built:
            d = K.label_design(c)
            built[c] = (d, R.prepare(*d.csr, d.s), _probe(d, ids_dtype=np.int32))
        return built[c]

    return get


@pytest.mark.parametrize("c", K.LABEL_CLASSES)
def test_int32_and_int64_class_ids_above_256_classes(labelled, c):
    d, ref, p = labelled(c)
    assert d.ids.dtype == np.int64 and (d.ids == 0).any() and (d.ids == c - 1).any() and not (d.ids == c - 3).any()
    _check_prepare(p, d, ref)
    want = _left_by_prepare(p)
    _same_bits(_left_by_prepare(_probe(d, ids_dtype=np.int64)), want)
    _same_bits(_left_by_prepare(_probe(d, matrix=True)), want)
    if c != 1000:
        _check_stats(p, d, ref, 500 + c)


@pytest.mark.parametrize("cls", K.ALONE_CLASSES)
def test_a_class_alone_and_among_4096_gives_identical_bits(labelled, cls):
    """One class prepared on its own (eight sub-chunks side by side in a wave) against the same class as one lane of the 64 class
    groups of C = 4 096, at the edges of the groups and of the label words."""
    d, _, p = labelled(4096)
    assert d.ymat[:, cls].sum() >= 30
    b, w = K.coefficients(d.s, d.c, 590)
    full = p.stats(_cuda(b), _cuda(w)).cpu().numpy()
    alone = _probe(dataclasses.replace(d, c=1, ymat=d.ymat[:, cls:cls + 1].copy(), ids=None))
    one = alone.stats(_cuda(b[:, cls:cls + 1]), _cuda(w[:, cls:cls + 1])).cpu().numpy()
    np.testing.assert_array_equal(one[:, :, 0].view(np.uint64), full[:, :, cls].view(np.uint64))


# ---- C: the fit, slab by slab ---------------------------------------------------------------------------------------------------------------

def _fit(p, hp, poll=0):
    """(coef bits, intercept bits, n_iter per class, done per slab) of a float64 fit."""
    coef, icpt, n_iter = p.fit(hp, dtype=torch.float64, poll_every=poll)
    n_slabs = -(-p.shape[2] // hp.class_slab_size)
    return (coef.cpu().numpy().view(np.uint64), icpt.cpu().numpy().view(np.uint64), n_iter.cpu().numpy(), p.done.cpu().numpy()[:n_slabs].copy())


@pytest.fixture(scope="module")
def fitted():
    """(C, slab) -> (design, the engine's hyper-parameters, the restatement's trace, _fit of a fresh object), built once."""
    built = {}

    def get(pair):
        if pair not in built:
            d = K.fit_design(*pair)
            hp = K.fit_hyper(*pair, cls=_engine().Probe1DHyper)
            built[pair] = (d, hp, K.fit_trace(d, K.fit_hyper(*pair)), _fit(_probe(d), hp))
        return built[pair]

    return get


PAIR_IDS = [f"c{c}_slab{s}" for c, s in K.FIT_PAIRS]


@pytest.mark.parametrize("pair", list(K.FIT_PAIRS), ids=PAIR_IDS)
def test_fit_equals_init_and_max_iter_times_stats_then_update(fitted, pair):
    """fit skips the stopped slabs inside the events and the reduce kernels; stats passes no done array and recomputes every pair.
    A stopped slab's pairs are never read again, so the two agree bit for bit; and along the manual loop every iteration's sums lie
    in the band of the restatement's at the device's own (b, w)."""
    d, hp, _, (coef, icpt, n_iter, done) = fitted(pair)
    starts, rows, vals, _ = R.prepare(*d.csr, d.s)
    p = _probe(d)
    p.init(hp)
    for it in range(hp.max_iter):
        b, w = p.state("b"), p.state("w")
        sums = p.stats(b, w)
        want, mag = R.event_sums(starts, rows, vals, d.ymat, b.cpu().numpy(), w.cpu().numpy())
        _check_sums(sums.cpu().numpy(), want, mag, f"iteration {it + 1}")
        p.update(hp, sums)
    n_slabs = done.size
    np.testing.assert_array_equal(p.state("w").cpu().numpy().view(np.uint64), coef)
    np.testing.assert_array_equal(p.state("b").cpu().numpy().view(np.uint64), icpt)
    np.testing.assert_array_equal(p.done.cpu().numpy()[:n_slabs], done)
    per_slab = p._view(p.layout.off_n_iter, torch.int32, d.c).cpu().numpy()[:n_slabs]
    np.testing.assert_array_equal(np.repeat(per_slab, hp.class_slab_size)[:d.c], n_iter)


@pytest.mark.parametrize("pair", list(K.FIT_PAIRS), ids=PAIR_IDS)
def test_slabs_stop_where_the_restatement_stops_them(fitted, pair):
    """n_iter and done of every slab as the restatement's (the host tests hold its largest scaled gradient 10 x away from tol at
    every decision): stopped slabs at their iteration, the others still running at max_iter."""
    d, hp, (_, _, want_n_iter, _, want_done), (_, _, n_iter, done) = fitted(pair)
    np.testing.assert_array_equal(n_iter, want_n_iter)
    np.testing.assert_array_equal(done, want_done.astype(np.int32))
    for i, (c0, c1) in enumerate(K.slabs_of(d.c, hp.class_slab_size)):
        assert (n_iter[c0:c1] == hp.max_iter).all() or done[i] == 1


@pytest.mark.parametrize("pair", list(K.FIT_PAIRS), ids=PAIR_IDS)
def test_every_slab_fits_alone_to_the_same_bits(fitted, pair):
    """A slab's classes prepared and fitted on their own (C' = the slab's width, another lane layout, no other slab to skip):
    a pair's sums do not depend on C."""
    d, hp, _, (coef, icpt, n_iter, _) = fitted(pair)
    for c0, c1 in K.slabs_of(d.c, hp.class_slab_size):
        alone = dataclasses.replace(d, c=c1 - c0, ymat=d.ymat[:, c0:c1].copy())
        got = _fit(_probe(alone), dataclasses.replace(hp, class_slab_size=c1 - c0))
        np.testing.assert_array_equal(got[0], coef[:, c0:c1], err_msg=f"coef of classes {c0}..{c1}")
        np.testing.assert_array_equal(got[1], icpt[:, c0:c1], err_msg=f"intercept of classes {c0}..{c1}")
        np.testing.assert_array_equal(got[2], n_iter[c0:c1])


@pytest.mark.parametrize("pair", K.POLLED, ids=[f"c{c}_slab{s}" for c, s in K.POLLED])
def test_polling_changes_no_bit(fitted, pair):
    d, hp, _, want = fitted(pair)
    assert hp.max_iter % 3 != 0 and hp.max_iter > 3  # poll_every = 3 looks once, and not after the last iteration
    for poll in (0, 1, 3):
        for a, b in zip(_fit(_probe(d), hp, poll), want):
            np.testing.assert_array_equal(a, b, err_msg=f"poll_every={poll}")


@pytest.mark.parametrize("pair", [(5, 2), (151, 8)], ids=["c5_slab2", "c151_slab8"])
def test_max_iter_0_leaves_the_start(fitted, pair):
    d, hp, _, _ = fitted(pair)
    p = _probe(d)
    coef, icpt, n_iter = p.fit(dataclasses.replace(hp, max_iter=0), dtype=torch.float64)
    q = _probe(d)
    q.init(hp)
    np.testing.assert_array_equal(icpt.cpu().numpy().view(np.uint64), q.state("b").cpu().numpy().view(np.uint64))
    want = np.tile(R.base_intercept(d.ymat.sum(axis=0), d.n), (d.s, 1))
    np.testing.assert_allclose(icpt.cpu().numpy(), want, rtol=1e-13, atol=0)
    assert (coef == 0).all() and (n_iter == 0).all()


# ---- D: evaluate in every layout ------------------------------------------------------------------------------------------------------------

def _check_evaluate(p, d, b, w, thr):
    bt, wt = _cuda(b), _cuda(w)
    loss, tp, fp, tn, fn = (t.cpu().numpy() for t in p.evaluate(bt, wt, thr, dtype=torch.float64))
    want = R.evaluate(*d.csr, d.s, d.ymat, d.c, b, w, thr)
    assert (np.abs(loss - want[0]) <= 1e-12 * want[5] + 1e-300).all()
    for name, got, ref in zip(("tp", "fp", "tn", "fn"), (tp, fp, tn, fn), want[1:5]):
        np.testing.assert_array_equal(got, ref, err_msg=name)
    np.testing.assert_array_equal(tp + fp + tn + fn, float(d.n))
    np.testing.assert_array_equal(tp + fn, np.broadcast_to(d.ymat.sum(axis=0).astype(np.float64), tp.shape))
    for got, ref in zip(p.evaluate(bt, wt, thr), (loss, tp, fp, tn, fn)):  # float32: the same, rounded once on the way out
        assert got.dtype == torch.float32
        np.testing.assert_array_equal(got.cpu().numpy(), ref.astype(np.float32))


@pytest.fixture(scope="module")
def cases():
    built = {}

    def get(i):
        if i not in built:
            d = K.case_design(i)
            built[i] = (d, _probe(d))
        return built[i]

    return get


@pytest.mark.parametrize("thr", K.THRESHOLDS)
@pytest.mark.parametrize("i", range(len(K.CASES)), ids=K.CASE_IDS)
def test_evaluate_matches_the_restatement_in_every_layout(cases, i, thr):
    d, p = cases(i)
    _check_evaluate(p, d, *K.coefficients(d.s, d.c, K.EVAL_SEED + i), thr)


@pytest.mark.parametrize("thr", K.THRESHOLDS)
def test_evaluate_on_a_ten_chunk_latent_at_33_classes(placed, thr):
    """Four accumulators against the partials' stride of seven, over a cut latent, with two class groups."""
    d, _, p = placed("four_groups")
    _check_evaluate(p, d, *K.coefficients(d.s, d.c, K.EVAL_SEED - 1), thr)


def test_fit_evaluate_and_stats_share_their_scratch(fitted):
    """evaluate directly after fit, stats directly after evaluate on one object (all three use `sums` and `part`) against fresh ones."""
    pair = (33, 8)
    d, hp, _, want_fit = fitted(pair)
    b, w = (_cuda(a) for a in K.coefficients(d.s, d.c, 610))
    p = _probe(d)
    for a, ref in zip(_fit(p, hp), want_fit):
        np.testing.assert_array_equal(a, ref)
    ev = p.evaluate(b, w, 0.5, dtype=torch.float64)
    st = p.stats(b, w)
    for got, ref in zip(ev, _probe(d).evaluate(b, w, 0.5, dtype=torch.float64)):
        np.testing.assert_array_equal(got.cpu().numpy().view(np.uint64), ref.cpu().numpy().view(np.uint64))
    np.testing.assert_array_equal(st.cpu().numpy().view(np.uint64), _probe(d).stats(b, w).cpu().numpy().view(np.uint64))
    for a, ref in zip(_fit(p, hp), want_fit):  # and a fit after both
        np.testing.assert_array_equal(a, ref)
