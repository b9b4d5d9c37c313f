"""CPU-only tests of the BatchTopK host side: the reference-written checkpoint with its ``activation.threshold`` (fixture G20,
tools/gen_golden_batch_topk.py), the round trip through dump / load, the C-ABI additions against the header and the library,
and the refusals that need no device."""

import ctypes as C
import io
import re
import subprocess

import pytest
import torch

from conftest import ROOT, load_golden

ENTRIES = ("saev_create_batch_topk", "saev_bind_threshold", "saev_threshold_device", "saev_row_cap", "saev_row_overflow_need",
           "saev_batch_topk_dense", "saev_encode_batch_topk", "saev_batch_topk_state", "saev_copy_last_row_nnz")
REFERENCE_KEYS = ["W_dec", "b_dec", "W_enc", "b_enc", "activation.threshold"]


def _header() -> str:
    return (ROOT / "include" / "saev_amd.h").read_text()


def _reference_state(g) -> dict:
    raw = g["ckpt"].numpy().tobytes()
    return torch.load(io.BytesIO(raw[raw.index(b"\n") + 1:]), weights_only=True, map_location="cpu")


def test_reference_checkpoint_with_a_threshold_loads(tmp_path):
    from saev_amd import nn
    from saev_amd.nn import modeling as M

    g = load_golden("g20_batch_topk_forward")
    path = tmp_path / "sae.pt"
    path.write_bytes(g["ckpt"].numpy().tobytes())
    sae = nn.load(path)
    state = _reference_state(g)
    assert list(state) == REFERENCE_KEYS  # what the reference wrote
    assert isinstance(sae.cfg.activation, M.BatchTopK) and sae.cfg.activation.top_k == int(g["k"])
    assert sae.cfg.activation.momentum == pytest.approx(float(g["momentum"]))
    assert isinstance(sae.activation, M.BatchTopKActivation)
    assert list(sae.state_dict()) == REFERENCE_KEYS
    for k in REFERENCE_KEYS:
        torch.testing.assert_close(sae.state_dict()[k], state[k], rtol=0, atol=0)
    assert float(sae.activation.threshold) == float(g["thr_before"]) > 0


def test_dump_then_load_round_trips_with_the_reference_keys_and_shapes(tmp_path):
    from saev_amd import nn

    g = load_golden("g20_batch_topk_forward")
    src = tmp_path / "ref.pt"
    src.write_bytes(g["ckpt"].numpy().tobytes())
    sae = nn.load(src)
    out = tmp_path / "out" / "sae.pt"
    nn.dump(out, sae)
    raw = out.read_bytes()
    written = torch.load(io.BytesIO(raw[raw.index(b"\n") + 1:]), weights_only=True, map_location="cpu")
    want = _reference_state(g)
    assert list(written) == list(want)
    for k, v in want.items():
        assert written[k].shape == v.shape and written[k].dtype == v.dtype, k
        torch.testing.assert_close(written[k], v, rtol=0, atol=0)
    again = nn.load(out)
    assert again.cfg == sae.cfg
    for k, v in want.items():
        torch.testing.assert_close(again.state_dict()[k], v, rtol=0, atol=0)


def test_a_fresh_module_has_the_threshold_buffer_at_zero():
    from saev_amd.nn import modeling as M

    sae = M.SparseAutoencoder(M.SparseAutoencoderConfig(d_model=16, d_sae=32, activation=M.BatchTopK(top_k=4)))
    assert list(sae.state_dict()) == REFERENCE_KEYS
    assert sae.activation.threshold.shape == () and float(sae.activation.threshold) == 0.0
    assert dict(sae.named_buffers()).keys() == {"activation.threshold"}
    # a TopK module's state dict keeps its four keys
    topk = M.SparseAutoencoder(M.SparseAutoencoderConfig(d_model=16, d_sae=32, activation=M.TopK(top_k=4)))
    assert list(topk.state_dict()) == REFERENCE_KEYS[:4]


def test_entries_are_declared_exported_and_mirrored():
    subprocess.run(["make", "-C", str(ROOT)], check=True, capture_output=True)
    from saev_amd import _lib

    declared = set(re.findall(r"\b(saev_[a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)))
    lib = _lib.load()
    for name in ENTRIES:
        assert name in declared, f"{name} missing from include/saev_amd.h"
        assert hasattr(lib, name), f"{name} not exported by libsaev_amd.so"
        assert name in _lib.EXPORTED_SYMBOLS
    m = re.search(r"#define SAEV_AMD_ABI_VERSION (\d+)", _header())
    assert int(m.group(1)) == _lib.ABI_VERSION == lib.saev_abi_version() == 12  # the additions are additive


def test_constants_and_struct_layouts_match_the_header(tmp_path):
    from saev_amd import _lib

    fields = [f for f, _ in _lib.SaevBatchTopKCfg._fields_]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "saev_amd.h"', "int main(void) {",
           'printf("size %zu\\n", sizeof(saev_batch_topk_cfg));', 'printf("cfg %zu\\n", sizeof(saev_cfg));',
           'printf("act %d\\n", SAEV_ACT_BATCHTOPK);', 'printf("overflow %d\\n", (int)SAEV_ROW_OVERFLOW);']
    src += [f'printf("{f} %zu\\n", offsetof(saev_batch_topk_cfg, {f}));' for f in fields]
    src.append("return 0; }")
    (tmp_path / "layout.c").write_text("\n".join(src))
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True)
    want = dict(line.split() for line in subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.splitlines())
    assert C.sizeof(_lib.SaevBatchTopKCfg) == int(want["size"])
    for f in fields:
        assert getattr(_lib.SaevBatchTopKCfg, f).offset == int(want[f]), f
    assert C.sizeof(_lib.SaevCfg) == int(want["cfg"])  # saev_cfg itself did not grow
    assert _lib.ACT_BATCHTOPK == int(want["act"]) == 2
    assert _lib.ROW_OVERFLOW == int(want["overflow"]) == -7


def test_training_on_several_ranks_is_refused(monkeypatch):
    from saev_amd import nn
    from saev_amd.framework import train as T
    from saev_amd.nn import modeling as M

    cfg = T.Config(sae=nn.SparseAutoencoderConfig(d_model=16, d_sae=32, activation=M.BatchTopK(top_k=4)))
    monkeypatch.setattr(T, "_dist", lambda: (None, 0, 2))
    with pytest.raises(NotImplementedError, match="one GPU"):
        T.train([cfg])
    # a TopK config next to it does not change that
    other = T.Config(sae=nn.SparseAutoencoderConfig(d_model=16, d_sae=32, activation=M.TopK(top_k=4)))
    with pytest.raises(NotImplementedError, match="one GPU"):
        T.train([other, cfg])


def test_there_is_no_cpu_path():
    from saev_amd import _lib
    from saev_amd.engine import EngineConfig, SaeEngine
    from saev_amd.nn import modeling as M

    sae = M.SparseAutoencoder(M.SparseAutoencoderConfig(d_model=16, d_sae=32, activation=M.BatchTopK(top_k=4)))
    with pytest.raises(NotImplementedError, match="no CPU path"):
        sae.activation(torch.zeros(2, 32))
    with pytest.raises(NotImplementedError):
        M.BatchTopKActivation(M.BatchTopK())(torch.zeros(2, 32))  # standalone: no engine to reach
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU path"):
            sae(torch.zeros(2, 16))
        with pytest.raises(_lib.SaevError, match="no CPU path"):
            SaeEngine(EngineConfig(d_model=16, d_sae=32, top_k=4, activation="batch_topk"))
    # the engine config of such a module: the activation's own settings, the objective's threshold
    ecfg = sae._engine_cfg(64)
    assert (ecfg.activation, ecfg.top_k, ecfg.batch_momentum, ecfg.row_cap, ecfg.k_aux) == ("batch_topk", 4, 0.1, 0, 512)
    l1 = M.SparseAutoencoder(M.SparseAutoencoderConfig(d_model=16, d_sae=32, activation=M.BatchTopK(sparsity=M.L1Sparsity())))
    with pytest.raises(NotImplementedError, match="sparsity"):
        l1._engine_cfg(64)
