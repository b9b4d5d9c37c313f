"""GPU tests of the interventions where the kernels of saev_amd/csrc/intervene.hip change behaviour: a second and
later pass of a wave over D on both routes, a wave that walks several rows past one grid, tensors one float off 16 bytes,
rows_changed added to a vector that is not zero with three contenders of one slot, the plan at 65536 edits and groups; the firing
counts past the grid caps of their three kernels, at 4096 classes, and F1 from counts that float32 does not hold.

The cases and what each exists for are in tests/interventions_cases.py (tests/test_interventions_cases_host_cpu.py runs every
``holds`` without a GPU).  The edits go through ``check_edit`` of tests/test_gpu_interventions.py and its tolerance: rows without a
remaining edit, in place, two calls and a NaN-filled output on the bits, the other rows within ``IR.tolerance(mag, m)``,
rows_changed on the integers.  The firing counts are compared as integers, f1 and best_t on the bits."""

import numpy as np
import pytest
import torch

import interventions_cases as IC
import interventions_restatement as IR
from test_gpu_interventions import _bits, _dev, check_edit

pytestmark = [pytest.mark.gpu, pytest.mark.encoder_modes("f32")]


@pytest.mark.parametrize("name", list(IC.EDIT_CASES))
def test_edit_geometry(name):
    case = IC.EDIT_CASES[name]()
    e = case.expected
    case.holds(e)
    check_edit(*case.args, row_group=case.row_group, row_keep=case.row_keep, expected=e)


def _off_by_one_float(a: np.ndarray) -> torch.Tensor:
    """``a`` on the device as a contiguous view that starts one float past a 16-byte boundary."""
    buf = torch.empty(a.size + 4, device="cuda", dtype=torch.float32)
    assert buf.data_ptr() % 16 == 0
    view = buf[1:1 + a.size].view(a.shape)
    view.copy_(torch.as_tensor(a))
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    return view


@pytest.mark.parametrize("name", list(IC.ALIGN_CASES))
def test_alignment_fall_back_gives_the_aligned_bits(name):
    """D % 4 == 0 with x, out or W_dec one float off 16 bytes takes the scalar route: the same fmaf chain per element, so the
    aligned call's bits; and the restatement within the tolerance."""
    from saev_amd import engine

    case = IC.ALIGN_CASES[name]()
    e = case.expected
    case.holds(e)
    check_edit(*case.args, row_group=case.row_group, row_keep=case.row_keep, expected=e)
    n, D = case.x.shape
    idxd, vald, nnzd = _dev(case.idx, torch.int32), _dev(case.val), _dev(case.row_nnz, torch.int32)
    rgd, rkd = _dev(case.row_group, torch.int32), _dev(case.row_keep, torch.bool)
    plan = engine.build_edit_plan(case.edits, case.W.shape[0], case.n_groups, "cuda")

    def run(xd, Wd, out):
        counts = torch.zeros(len(case.edits), device="cuda", dtype=torch.int64)
        res = engine.intervene_rows(xd, Wd, idxd, vald, nnzd, plan, len(case.edits), case.n_groups, row_group=rgd, row_keep=rkd, out=out,
                                    rows_changed=counts)
        assert res is out
        return res.cpu().numpy(), counts.cpu().numpy()

    xa, Wa, outa = _dev(case.x), _dev(case.W), torch.full((n, D), float("nan"), device="cuda")
    assert xa.data_ptr() % 16 == 0 and Wa.data_ptr() % 16 == 0 and outa.data_ptr() % 16 == 0
    aligned, counts = run(xa, Wa, outa)
    tol = IR.tolerance(e["mag"], e["m"])
    for moved in case.offsets:
        xd = _off_by_one_float(case.x) if "x" in moved else xa
        Wd = _off_by_one_float(case.W) if "W" in moved else Wa
        out = _off_by_one_float(np.full((n, D), np.nan, dtype=np.float32)) if "out" in moved else torch.full_like(outa, float("nan"))
        assert [t.data_ptr() % 16 for t in (xd, out, Wd)] == [4 if k in moved else 0 for k in ("x", "out", "W")], moved
        got, c = run(xd, Wd, out)
        assert (_bits(got) == _bits(aligned)).all(), f"{moved} off 16 bytes: not the aligned bits"
        assert (c == counts).all() and (c == e["rows_changed"]).all()
        assert (np.abs(got.astype(np.float64) - e["out"]) <= tol).all() and (_bits(got[e["m"] == 0]) == _bits(case.x[e["m"] == 0])).all()
    x2 = _off_by_one_float(case.x)  # in place, one float off
    got, c = run(x2, Wa, x2)
    assert (_bits(got) == _bits(aligned)).all() and (c == counts).all(), "in place off 16 bytes: not the aligned bits"


@pytest.mark.parametrize("name", list(IC.COUNT_CASES))
def test_rows_changed_is_added_to(name):
    from saev_amd import engine

    case = IC.COUNT_CASES[name]()
    e = case.expected
    case.holds(e)
    check_edit(*case.args, row_group=case.row_group, row_keep=case.row_keep, expected=e)
    xd, Wd, idxd, vald, nnzd = _dev(case.x), _dev(case.W), _dev(case.idx, torch.int32), _dev(case.val), _dev(case.row_nnz, torch.int32)
    rgd = _dev(case.row_group, torch.int32)
    plan = engine.build_edit_plan(case.edits, case.W.shape[0], case.n_groups, "cuda")
    counts = _dev(case.prefill, torch.int64)
    counted = engine.intervene_rows(xd, Wd, idxd, vald, nnzd, plan, len(case.edits), case.n_groups, row_group=rgd, rows_changed=counts)
    assert (counts.cpu().numpy() == case.prefill + e["rows_changed"]).all(), "the call must add the restated counts to what was there"
    engine.intervene_rows(xd, Wd, idxd, vald, nnzd, plan, len(case.edits), case.n_groups, row_group=rgd, rows_changed=counts)
    assert (counts.cpu().numpy() == case.prefill + 2 * e["rows_changed"]).all()
    plain = engine.intervene_rows(xd, Wd, idxd, vald, nnzd, plan, len(case.edits), case.n_groups, row_group=rgd, rows_changed=None)
    assert (_bits(plain.cpu().numpy()) == _bits(counted.cpu().numpy())).all(), "the output depends on whether the rows are counted"


@pytest.mark.parametrize("name", list(IC.FIRE_CASES))
def test_fire_geometry(name):
    from saev_amd import engine

    case = IC.FIRE_CASES[name]()
    e = case.expected
    case.holds(e)
    counts = engine.ClassFireCounts(case.S, case.C, "cuda", case.thr)
    batch = _dev(case.idx), _dev(case.val), _dev(case.row_nnz), _dev(case.labels), _dev(case.keep)
    for _ in range(case.repeats):
        counts.add(*batch)
    # uint32 counters held in int32 tensors: read as unsigned
    hist = counts.hist.cpu().numpy().view(np.uint32).astype(np.int64)
    pos = counts.pos.cpu().numpy().view(np.uint32).astype(np.int64)
    assert (hist == e["hist"]).all(), int((hist != e["hist"]).sum())
    assert (pos == e["pos"]).all(), int((pos != e["pos"]).sum())
    assert (counts.n_rows_c.cpu().numpy() == e["n_rows_c"]).all()
    f1, best_t = counts.f1(None if case.mask is None else torch.as_tensor(case.mask).cuda())
    f1, best_t = f1.cpu().numpy(), best_t.cpu().numpy()
    differ = _bits(f1) != _bits(e["f1"])
    assert not differ.any(), (int(differ.sum()), np.argwhere(differ)[:4].tolist())
    assert (best_t == e["best_t"]).all()
