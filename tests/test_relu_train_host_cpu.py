"""CPU-only tests of ReLU training's host side: the C-ABI additions against the header and the library, the refusals that need
no device, the gate of train() / evaluate(), the dense restatement against the reference's own trajectory (fixtures G22,
tools/gen_golden_relu_train.py) and the input conditions of the geometry table (this is where the seeds of
tests/relu_step_restatement.py: RELU_SHAPES are fixed)."""

import ctypes as C
import functools
import math
import re
import subprocess

import pytest
import torch

import sae_ref as R
from conftest import ROOT, load_golden
from relu_step_restatement import (L1_COEFF, RELU_SHAPES, relu_input_conditions, relu_restated_gradients, relu_row_inputs)
from step_restatement import BOUND, assert_grads_close

ENTRIES = ("saev_create_relu_train", "saev_copy_last_rows")
TAGS = ("l1", "nosparsity")


def _header() -> str:
    return (ROOT / "include" / "saev_amd.h").read_text()


# ------------------------------------------------------------------------------------------------
# the C ABI
# ------------------------------------------------------------------------------------------------


def test_entries_are_declared_exported_and_mirrored():
    subprocess.run(["make", "-C", str(ROOT)], check=True, capture_output=True)
    from saev_amd import _lib

    declared = set(re.findall(r"\b(saev_[a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)))
    lib = _lib.load()
    for name in ENTRIES:
        assert name in declared, f"{name} missing from include/saev_amd.h"
        assert hasattr(lib, name), f"{name} not exported by libsaev_amd.so"
        assert name in _lib.EXPORTED_SYMBOLS
    assert "saev_relu_train_cfg" in _header()
    m = re.search(r"#define SAEV_AMD_ABI_VERSION (\d+)", _header())
    assert int(m.group(1)) == _lib.ABI_VERSION == lib.saev_abi_version() == 12  # the additions are additive


def test_struct_layout_matches_the_header(tmp_path):
    from saev_amd import _lib

    fields = [f for f, _ in _lib.SaevReluTrainCfg._fields_]
    assert fields == ["struct_size", "reserved", "l1_coeff"]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "saev_amd.h"', "int main(void) {",
           'printf("size %zu\\n", sizeof(saev_relu_train_cfg));', 'printf("cfg %zu\\n", sizeof(saev_cfg));',
           'printf("last %zu\\n", offsetof(saev_cfg, activation) + sizeof(int32_t));']
    src += [f'printf("{f} %zu\\n", offsetof(saev_relu_train_cfg, {f}));' for f in fields]
    src.append("return 0; }")
    (tmp_path / "layout.c").write_text("\n".join(src))
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True)
    want = dict(line.split() for line in subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.splitlines())
    assert C.sizeof(_lib.SaevReluTrainCfg) == int(want["size"]) == 16
    for f in fields:
        assert getattr(_lib.SaevReluTrainCfg, f).offset == int(want[f]), f
    assert C.sizeof(_lib.SaevCfg) == int(want["cfg"])  # saev_cfg itself did not grow ...
    assert int(want["last"]) + (-int(want["last"])) % 8 == int(want["cfg"])  # ... and `activation` is still its last field


def test_create_refuses_bad_configurations_without_touching_a_device():
    """k_aux != 0 and a non-ReLU activation are SAEV_INVALID_ARG (-1) from the argument checks alone: there is no device here."""
    subprocess.run(["make", "-C", str(ROOT)], check=True, capture_output=True)
    from saev_amd import _lib

    lib = _lib.load()
    rt = _lib.SaevReluTrainCfg(struct_size=C.sizeof(_lib.SaevReluTrainCfg), l1_coeff=1e-2)
    base = dict(d_model=16, d_sae=32, top_k=4, max_batch=8)
    for kw in (dict(activation=_lib.ACT_RELU, k_aux=8), dict(activation=_lib.ACT_TOPK, k_aux=0), dict(activation=_lib.ACT_BATCHTOPK, k_aux=0)):
        ctx = C.c_void_p(0xDEAD)
        cfg = _lib.SaevCfg(**base, **kw)
        assert lib.saev_create_relu_train(C.byref(cfg), None, C.byref(rt), 0, C.byref(ctx)) == -1
        assert not ctx.value  # (*out is cleared)
    bad = _lib.SaevReluTrainCfg(struct_size=C.sizeof(_lib.SaevReluTrainCfg), l1_coeff=-1.0)
    cfg = _lib.SaevCfg(**base, activation=_lib.ACT_RELU, k_aux=0)
    assert lib.saev_create_relu_train(C.byref(cfg), None, C.byref(bad), 0, C.byref(C.c_void_p())) == -1
    assert lib.saev_create_relu_train(None, None, None, 0, C.byref(C.c_void_p())) == -1
    # the bf16 encoder and a sharded layout are out of scope: SAEV_UNSUPPORTED (-3), also before the device
    for kw in (dict(encoder_mode=2), dict(shard_world=2)):
        cfg = _lib.SaevCfg(**base, activation=_lib.ACT_RELU, k_aux=0, **kw)
        assert lib.saev_create_relu_train(C.byref(cfg), None, C.byref(rt), 0, C.byref(C.c_void_p())) == -3


# ------------------------------------------------------------------------------------------------
# the gate
# ------------------------------------------------------------------------------------------------


def _cfg(activation, n_prefixes):
    from saev_amd import nn
    from saev_amd.framework import train as T
    from saev_amd.nn import objectives as O

    return T.Config(sae=nn.SparseAutoencoderConfig(d_model=16, d_sae=32, activation=activation), objective=O.Matryoshka(n_prefixes=n_prefixes))


def test_the_gate_lets_the_plain_objective_through_and_refuses_the_rest():
    from saev_amd.framework import train as T
    from saev_amd.nn import modeling as M

    empty = torch.nn.ModuleList()
    for act in (M.Relu(), M.Relu(sparsity=M.NoSparsity())):
        # n_prefixes = 1 passes the activation check; what stops the call next is the missing device, as for a TopK config
        for cfg in (_cfg(act, 1), _cfg(M.TopK(top_k=4), 1)):
            with pytest.raises(RuntimeError, match="HIP device") as err:
                T.train([cfg])
            assert not isinstance(err.value, NotImplementedError)
        with pytest.raises(NotImplementedError, match=r"Relu.*n_prefixes"):
            T.train([_cfg(act, 4)])
        with pytest.raises(NotImplementedError, match=r"Relu.*n_prefixes"):
            T.evaluate([_cfg(act, 4)], empty, empty)
    aux = M.Relu(aux=M.AuxK())
    with pytest.raises(NotImplementedError, match="AuxK"):
        T.train([_cfg(aux, 1)])
    with pytest.raises(NotImplementedError, match="AuxK"):
        T.evaluate([_cfg(aux, 1)], empty, empty)
    # a TopK member next to it changes nothing, in either order
    for group in ([_cfg(M.TopK(top_k=4), 1), _cfg(M.Relu(), 4)], [_cfg(M.Relu(), 4), _cfg(M.TopK(top_k=4), 1)]):
        with pytest.raises(NotImplementedError, match="n_prefixes"):
            T.train(group)


def test_training_on_several_ranks_is_refused(monkeypatch):
    from saev_amd.framework import train as T
    from saev_amd.nn import modeling as M

    monkeypatch.setattr(T, "_dist", lambda: (None, 0, 2))
    with pytest.raises(NotImplementedError, match="one GPU"):
        T.train([_cfg(M.Relu(), 1)])


def test_engine_config_of_a_bound_module():
    """A Relu module builds the forward-only engine until an objective binds it, the training engine -- with the coefficient of
    its sparsity -- from then on; AuxK is refused."""
    from saev_amd.nn import modeling as M

    sae = M.SparseAutoencoder(M.SparseAutoencoderConfig(d_model=16, d_sae=32, activation=M.Relu(sparsity=M.L1Sparsity(coeff=3e-3))))
    assert sae._engine_cfg(64).activation == "relu"
    sae.__dict__["_relu_trains"] = True
    ecfg = sae._engine_cfg(64)
    assert ecfg.activation == "relu_train" and ecfg.l1_coeff == 3e-3 and ecfg.k_aux == 0
    none = M.SparseAutoencoder(M.SparseAutoencoderConfig(d_model=16, d_sae=32, activation=M.Relu(sparsity=M.NoSparsity())))
    none.__dict__["_relu_trains"] = True
    assert none._engine_cfg(64).l1_coeff == 0.0
    aux = M.SparseAutoencoder(M.SparseAutoencoderConfig(d_model=16, d_sae=32, activation=M.Relu(aux=M.AuxK())))
    aux.__dict__["_relu_trains"] = True
    with pytest.raises(NotImplementedError, match="AuxK"):
        aux._engine_cfg(64)


# ------------------------------------------------------------------------------------------------
# the restatement against the reference's own numbers (G22)
# ------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("tag", TAGS)
def test_the_fixture_is_what_the_issue_asks_for(tag):
    g = load_golden(f"g22_relu_train_{tag}")
    assert (int(g["d"]), int(g["s"]), int(g["bsz"]), int(g["n_steps"])) == (32, 128, 64, 4)
    assert float(g["l1_coeff"]) == (1e-2 if tag == "l1" else 0.0)
    assert (g["log_gap"] >= 16 * g["log_bound"]).all()  # no pre-activation near zero at any recorded forward
    assert int(g["thr_tokens"]) == 2 * int(g["bsz"]) and g["log_n_dead"][0] == 0 and (g["log_n_dead"][1:] >= 1).all()
    assert (g["log_grad_norm"] > float(g["grad_clip"])).all()  # every step clipped
    silent = g["silent"]
    assert (g["init_b_enc"][silent] == -6).all() and not g["f_x"][:, :, silent].any()
    # the silent latents' gradient rows are exactly zero
    assert not g["grad1_W_dec"][silent].any() and not g["grad1_W_enc"][:, silent].any() and not g["grad1_b_enc"][silent].any()


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_reproduces_the_reference_losses_and_gradients(tag):
    g = load_golden(f"g22_relu_train_{tag}")
    b, coeff = int(g["bsz"]), float(g["l1_coeff"])
    p = {k: g["init_" + k].clone() for k in R.PARAM_ORDER}
    p["W_dec"] = R.normalize_w_dec(p["W_dec"])  # the loop body renormalises first (train.py:334-335)
    x = g["acts"][:b]
    mask = g["f_x"][0] > 0
    mask64, ratio = relu_input_conditions(p["W_enc"], p["b_enc"], x)
    assert torch.equal(mask, mask64) and ratio >= 16
    mse, l1, ref = relu_restated_gradients(p, x, mask, coeff)
    assert math.isclose(mse, float(g["log_mse"][0]), rel_tol=1e-5) and math.isclose(l1, float(g["log_l1"][0]), rel_tol=1e-5)
    assert math.isclose(coeff * l1, float(g["log_sparsity"][0]), rel_tol=1e-5, abs_tol=0.0 if coeff else 1e-30)
    assert float(mask.sum(dim=1).float().mean()) == float(g["log_l0"][0])
    assert_grads_close({k: g["grad1_" + k] for k in R.PARAM_ORDER}, ref, BOUND, what=f"G22 {tag}: ")


# ------------------------------------------------------------------------------------------------
# the geometry table
# ------------------------------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def _reference(row):
    p, x = relu_row_inputs(row)
    mask, ratio = relu_input_conditions(p["W_enc"], p["b_enc"], x)
    return p, x, mask, ratio, relu_restated_gradients(p, x, mask, L1_COEFF)


def test_the_table_is_well_formed():
    assert len({r.id for r in RELU_SHAPES}) == len(RELU_SHAPES)
    assert {(r.n, r.d, r.s) for r in RELU_SHAPES} >= {(1, 20, 36), (65, 36, 260), (300, 100, 1004), (130, 256, 1028), (257, 512, 516),
                                                    (70, 1280, 516), (34, 4092, 260)}
    assert any(r.quiet_row for r in RELU_SHAPES) and any(r.extremes for r in RELU_SHAPES)
    for r in RELU_SHAPES:
        assert r.d % 4 == 0 and r.s % 4 == 0 and r.d <= 4096 and r.bound >= BOUND


@pytest.mark.parametrize("row", RELU_SHAPES, ids=lambda r: r.id)
def test_inputs_meet_the_mask_condition(row):
    p, x, mask, ratio, (mse, l1, ref) = _reference(row)
    print(f"{row.id}: smallest |h| {ratio:.2f} fp32 bounds from zero; codes per row {int(mask.sum(1).min())}..{int(mask.sum(1).max())}")
    assert mse > 0 and l1 > 0
    if row.quiet_row:  # an all-negative batch row: no code, and the latents' gradients hold nothing of it
        assert not mask[0].any() and mask[1:].any(dim=1).all()
    if row.extremes:   # a latent that never fires has zero rows in all three of its gradients; one fires on every row
        assert not mask[:, 1].any() and mask[:, 2].all()
        assert not ref["W_dec"][1].any() and not ref["W_enc"][:, 1].any() and ref["b_enc"][1] == 0
    # the edges carry gradient: a kernel that dropped the last latent or the last column could not hide behind a zero
    assert ref["b_enc"][-1] != 0 and ref["W_dec"][-1].abs().max() > 0 and ref["W_enc"][:, -1].abs().max() > 0
    assert ref["W_dec"][:, -1].abs().max() > 0 and ref["b_dec"][-1] != 0


@pytest.mark.parametrize("row", RELU_SHAPES, ids=lambda r: r.id)
def test_fp32_restatement_passes_its_own_check(row):
    """The margin of the bound is measured here, against an fp32 torch restatement, never against the HIP result: every row keeps
    BOUND = 2e-5 because the fp32 restatement's own error stays below a quarter of it."""
    p, x, mask, _, (mse, l1, ref) = _reference(row)
    mse32, l132, got = relu_restated_gradients(p, x, mask, L1_COEFF, dtype=torch.float32)
    ratios = assert_grads_close(got, ref, row.bound / 4, what=f"{row.id}: ")
    print(f"{row.id}: fp32 against fp64, worst |difference| / max|fp64|: " + "  ".join(f"{k} {v:.2e}" for k, v in ratios.items()))
    assert abs(mse32 - mse) <= 1e-5 * mse and abs(l132 - l1) <= 1e-5 * l1
