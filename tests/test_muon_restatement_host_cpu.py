"""CPU-only tests of tests/muon_restatement.py, the restatements the GPU tests of test_gpu_muon_geometry.py lean on: the
split-K / workspace layout against the library's host entry (every case stays in the class it is there for), torch's Muon step
against torch.optim.Muon itself under every hyper-parameter setting, bit for bit, and MuonConfig.c_struct()."""

import ctypes
import itertools

import pytest
import torch

from muon_restatement import CASES, CONFIGS, NORM_MARGIN, layout, margin_input, muon_step_fp64, norm_margin, ulp_of


@pytest.fixture(scope="module")
def lib():
    from saev_amd import _lib

    return _lib.load()


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_every_case_is_in_the_class_it_is_there_for(case):
    L = layout(*case.shape)
    assert (L.Dp, L.Sp) == case.padded, case.why
    assert L.gram == case.gram and L.gg == case.gg, (case.why, L)
    n, kper, splits, last = L.gram
    assert (splits - 1) * kper + last == L.Sp // 32 and 1 <= last <= kper and splits <= n <= 16


def test_the_classes_the_cases_name():
    by = {c.shape: layout(*c.shape) for c in CASES}
    assert by[(200, 5201)].nb == 4 * 82 > 256                     # the norm kernel's strided loop takes a second round
    assert by[(200, 5201)] == layout(200, 5200)                   # the padded shape is the same: the odd column moves nothing
    assert by[(4, 8)].nb == 1 and by[(36, 260)].nb == 5 and by[(132, 132)].nb == 9
    for shape in ((4, 8), (36, 260), (128, 128)):                 # one diagonal tile: kt caps the splits, not MUON_MAX_SPLITS
        assert by[shape].Dp == 128 and by[shape].gg == (4, 1, 4, 1)
    assert by[(300, 516)].Dp // 128 == 3
    n, kper, splits, last = by[(100, 1250)].gram
    assert splits < n and last < kper
    # the shapes of test_gpu_muon.py: 16 even splits, an uneven last split, one split
    assert layout(200, 1000).gram == (16, 2, 16, 2) and layout(1024, 32768).gram == (15, 69, 15, 58) and layout(4096, 4224).gram == (1, 132, 1, 132)


def _sweep():
    edges = sorted({e + o for e in (128, 256, 384, 1024) for o in (-4, -1, 0, 1, 4)})
    pairs = [(r, c) for r, c in itertools.product(edges, edges) if r <= c]
    return pairs + [(1, 1), (1, 4096), (4, 8), (3, 1 << 20), (1, 1 << 30)]


def test_workspace_bytes_equal_the_library(lib):
    shapes = [c.shape for c in CASES] + [(1024, 32768), (768, 6144), (200, 1000), (4096, 4224)] + _sweep()
    assert len(_sweep()) >= 200
    for rows, cols in shapes:
        assert layout(rows, cols).bytes == lib.saev_muon_workspace_bytes(rows, cols), (rows, cols)
    for rows, cols in ((260, 36), (129, 128), (0, 8), (0, 0), (-1, 8), (4, (1 << 30) + 1), (4, 1 << 31)):
        assert lib.saev_muon_workspace_bytes(rows, cols) == -1, (rows, cols)


def _muon_config(**kw):
    from saev_amd.engine import MuonConfig

    return MuonConfig(**kw)


@pytest.mark.parametrize("name", list(CONFIGS))
@pytest.mark.parametrize("shape", [(260, 36), (36, 260)])
def test_restated_step_is_torchs_bit_for_bit(shape, name):
    """Three steps of torch.optim.Muon on the CPU against muon_step_fp64 with torch's own Newton-Schulz as the orthogonaliser and
    torch's two fp32 operations as the update: parameters and momentum buffer bit-equal.  The fp64 evaluation of the same update,
    which the GPU tests use and which rounds p * decay where mul_ does, is within one fp32 ulp of the result of it."""
    kw = CONFIGS[name]
    cfg = _muon_config(**kw)
    g = torch.Generator().manual_seed(shape[0])
    W = torch.nn.Parameter(torch.randn(*shape, generator=g) * 0.1)
    opt = torch.optim.Muon([W], lr=0.0, **kw)
    p, m = W.data.clone(), torch.zeros(shape)
    for step, lr in enumerate((1e-3, 2e-3, 0.02)):
        grad = torch.randn(*shape, generator=g) * 0.01
        W.grad = grad.clone()
        opt.param_groups[0]["lr"] = lr
        opt.step()
        q64, _, _ = muon_step_fp64(p, grad, m.clone(), lr, cfg)
        p, u, O = muon_step_fp64(p, grad, m, lr, cfg, torch_update=True)
        assert torch.equal(m, opt.state[W]["momentum_buffer"]), (name, step)
        assert torch.equal(p, W.data), (name, step)
        assert O.dtype == torch.bfloat16 and O.shape == p.shape
        assert ((p.double() - q64).abs() <= ulp_of(q64.abs(), 23)).all(), (name, step)
        if cfg.ns_steps == 0:
            assert torch.equal(O, (u.bfloat16() / u.bfloat16().norm().clamp(min=cfg.eps)))
    assert not torch.equal(p, W.data * 0)


def test_c_struct_round_trips_every_field():
    """Every field of the C struct is the MuonConfig field of the same meaning, to fp32; adjust_lr_fn: None and "original" are
    0, "match_rms_adamw" 1, "none" 2 (lr as it is, the branch torch takes for any other name), an unknown name a ValueError."""
    from saev_amd import _lib

    cfg = _muon_config(weight_decay=0.25, momentum=0.3, nesterov=False, ns_coefficients=(1.5, -2.5, 3.25), eps=1e-3, ns_steps=7,
                       adjust_lr_fn="match_rms_adamw")
    c = cfg.c_struct()
    got = {f: getattr(c, f) for f, _ in _lib.SaevMuonCfg._fields_}
    f = lambda v: ctypes.c_float(v).value
    assert got == {"momentum": f(0.3), "weight_decay": 0.25, "a": 1.5, "b": -2.5, "c": 3.25, "eps": f(1e-3), "nesterov": 0, "ns_steps": 7,
                   "adjust_lr": 1}
    assert _muon_config(nesterov=True).c_struct().nesterov == 1
    for name, code in ((None, 0), ("original", 0), ("match_rms_adamw", 1), ("none", 2)):
        assert _muon_config(adjust_lr_fn=name).c_struct().adjust_lr == code, name
    for bad in ("rms", "", "None", "Original"):
        with pytest.raises(ValueError, match="adjust_lr_fn"):
            _muon_config(adjust_lr_fn=bad).c_struct()


def test_margin_inputs_have_the_margin():
    for case in CASES:
        x, seed = margin_input(case.shape, 100 + case.rows)
        assert norm_margin(x) >= NORM_MARGIN and x.shape == case.shape and seed >= 100 + case.rows
    # a norm on a boundary has none: 1 + 2^-8 is the midpoint of the bf16 values 1 and 1 + 2^-7
    assert norm_margin(torch.tensor([[1.0, 0.0]])) > 0.001
    x = torch.zeros(1, 513)
    x[0, 0] = 1.0
    x[0, 1:513] = 2.0 ** -8  # sum of squares 1 + 512 * 2^-16 = 1 + 2^-7: the norm is 1 + 2^-8 - 2^-17 + ..., 2^-17 from the midpoint
    assert norm_margin(x) < 2.0 ** -16
    assert norm_margin(torch.zeros(3, 5)) == float("inf")
