"""CPU-only tests of the ReLU SAE forward's host side: the C-ABI entries, the ABI version, the reference-written ReLU
checkpoint (fixture G19, tools/gen_relu_golden.py) and the training entries that stay TopK-only."""

import io
import re
import subprocess

import pytest
import torch

from conftest import ROOT, load_golden

RELU_ENTRIES = ("saev_encode_relu", "saev_decode_rows", "saev_scatter_rows")


def _header() -> str:
    return (ROOT / "include" / "saev_amd.h").read_text()


def test_relu_entries_are_declared_and_exported():
    subprocess.run(["make", "-C", str(ROOT)], check=True, capture_output=True)
    from saev_amd import _lib

    declared = set(re.findall(r"\b(saev_[a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)))
    lib = _lib.load()
    for name in RELU_ENTRIES:
        assert name in declared, f"{name} missing from include/saev_amd.h"
        assert hasattr(lib, name), f"{name} not exported by libsaev_amd.so"
        assert name in _lib.EXPORTED_SYMBOLS


def test_abi_version_agrees_between_header_and_library():
    from saev_amd import _lib

    m = re.search(r"#define SAEV_AMD_ABI_VERSION (\d+)", _header())
    assert m is not None
    assert int(m.group(1)) == _lib.ABI_VERSION == _lib.load().saev_abi_version() == 12


def test_cfg_carries_the_activation_last():
    """The new field is appended: every TopK field keeps its offset, and zero (the default of a zeroed struct) is TopK."""
    from saev_amd import _lib

    assert [f for f, _ in _lib.SaevCfg._fields_][-1] == "activation"
    assert re.search(r"#define SAEV_ACT_TOPK 0\b", _header()) and re.search(r"#define SAEV_ACT_RELU 1\b", _header())
    assert _lib.SaevCfg().activation == 0


@pytest.mark.parametrize("tag", ["sparse", "dense"])
def test_reference_relu_checkpoint_loads(tmp_path, tag):
    from saev_amd import nn
    from saev_amd.nn import modeling as M

    g = load_golden(f"g19_relu_forward_{tag}")
    path = tmp_path / "sae.pt"
    path.write_bytes(g["ckpt"].numpy().tobytes())
    sae = nn.load(path)
    assert isinstance(sae.cfg.activation, M.Relu)
    assert sae.cfg.activation.sparsity == M.L1Sparsity(coeff=4e-4)
    assert isinstance(sae.activation, M.ReluActivation)
    assert (sae.cfg.d_model, sae.cfg.d_sae) == (g["x"].shape[1], g["h_x"].shape[1])
    raw = g["ckpt"].numpy().tobytes()
    state = torch.load(io.BytesIO(raw[raw.index(b"\n") + 1 :]), weights_only=True)
    for k in ("W_dec", "b_dec", "W_enc", "b_enc"):
        torch.testing.assert_close(getattr(sae, k).detach(), state[k], rtol=0, atol=0)


def test_relu_activation_module_matches_the_reference_fixture():
    from saev_amd.nn import modeling as M

    g = load_golden("g19_relu_forward_sparse")
    act = M.ReluActivation(M.Relu())
    torch.testing.assert_close(act(g["h_x"]), g["f_x"], rtol=0, atol=0)


def test_training_a_relu_sae_still_raises():
    from saev_amd import nn
    from saev_amd.framework import train as T
    from saev_amd.nn import modeling as M

    cfg = T.Config(sae=nn.SparseAutoencoderConfig(d_model=16, d_sae=32, activation=M.Relu()))
    with pytest.raises(NotImplementedError, match="Relu"):
        T.train([cfg])
    with pytest.raises(NotImplementedError, match="Relu"):
        T.evaluate([cfg], torch.nn.ModuleList(), torch.nn.ModuleList())


def test_batch_topk_stays_unsupported():
    from saev_amd.nn import modeling as M

    sae = M.SparseAutoencoder(M.SparseAutoencoderConfig(d_model=16, d_sae=32, activation=M.BatchTopK()))
    assert not isinstance(sae.activation, (M.ReluActivation, M.TopKActivation))
    with pytest.raises(NotImplementedError):
        sae.activation(torch.zeros(2, 32))
