"""CPU-only tests of the Muon tail's host side: the C-ABI entries, saev_muon_cfg's ctypes layout, MuonConfig's defaults against
torch.optim.Muon's signature, and the fp64 emulation of the bf16 Newton-Schulz iteration that the GPU tests (test_gpu_muon.py)
hold the kernels to -- validated here against torch's own CPU implementation."""

import inspect
import re
import subprocess

import torch

from conftest import ROOT

MUON_ENTRIES = ("saev_muon_tail", "saev_muon_default_cfg", "saev_muon_workspace_bytes", "saev_muon_newton_schulz")


def bf16(t: torch.Tensor) -> torch.Tensor:
    """fp64 -> bf16 the way the kernels round: through fp32 (their accumulator), then to nearest even -- back as fp64."""
    return t.float().bfloat16().double()


def ns_emulate(x: torch.Tensor, coeffs=(3.4445, -4.7750, 2.0315), steps: int = 5, eps: float = 1e-7, normalize: bool = True) -> torch.Tensor:
    """The Newton-Schulz iteration of torch.optim.Muon (rows <= cols) in fp64 with the bf16 roundings of the contract
    (include/saev_amd.h: MUON): the norm and the division rounded once each, every product rounded once after its epilogue."""
    a, b, c = coeffs
    X = bf16(x.double())
    if normalize:
        n = bf16(X.norm().reshape(1)).clamp(min=eps)
        X = bf16(X / bf16(n))
    for _ in range(steps):
        G = bf16(X @ X.T)
        U = bf16(c * (G @ G) + b * G)
        X = bf16(a * X + U @ X)
    return X


def test_muon_entries_are_declared_and_exported():
    subprocess.run(["make", "-C", str(ROOT)], check=True, capture_output=True)
    from saev_amd import _lib

    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "saev_amd.h").read_text(), flags=re.S)
    declared = set(re.findall(r"\b(saev_[a-z_0-9]+)\s*\(", text))
    lib = _lib.load()
    for name in MUON_ENTRIES:
        assert name in declared and hasattr(lib, name) and name in _lib.EXPORTED_SYMBOLS, name


def test_muon_cfg_layout_matches_header(tmp_path):
    import ctypes

    from saev_amd import _lib

    fs = [f for f, _ in _lib.SaevMuonCfg._fields_]
    src = ["#include <stdio.h>", "#include <stddef.h>", '#include "saev_amd.h"', "int main(void) {",
           'printf("size %zu\\n", sizeof(saev_muon_cfg));']
    src += [f'printf("{f} %zu\\n", offsetof(saev_muon_cfg, {f}));' for f in fs]
    src.append("return 0; }")
    (tmp_path / "m.c").write_text("\n".join(src))
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(tmp_path / "m.c"), "-o", str(tmp_path / "m")], check=True)
    want = dict(line.split() for line in subprocess.run([str(tmp_path / "m")], check=True, capture_output=True, text=True).stdout.splitlines())
    assert ctypes.sizeof(_lib.SaevMuonCfg) == int(want["size"])
    for f in fs:
        assert getattr(_lib.SaevMuonCfg, f).offset == int(want[f]), f


def test_library_defaults_equal_muon_config_defaults():
    import ctypes

    from saev_amd import _lib
    from saev_amd.engine import MuonConfig

    got = _lib.SaevMuonCfg()
    _lib.load().saev_muon_default_cfg(ctypes.byref(got))
    want = MuonConfig().c_struct()
    for f, _ in _lib.SaevMuonCfg._fields_:
        assert getattr(got, f) == getattr(want, f), f


def test_muon_config_defaults_are_torchs():
    import dataclasses

    from saev_amd.engine import MuonConfig

    sig = {k: v.default for k, v in inspect.signature(torch.optim.Muon).parameters.items() if k not in ("params", "lr")}
    ours = {f.name: f.default for f in dataclasses.fields(MuonConfig)}
    assert ours == sig


def test_emulation_agrees_with_torch_newton_schulz_on_cpu():
    """The fp64 emulation vs torch's CPU _zeropower_via_newtonschulz (bf16 matmuls): the two round at the same points, so
    they differ only where an fp32 accumulation crossed a bf16 rounding boundary.  One iteration: nearly every element
    equal, none more than one bf16 ulp apart; five iterations: relative Frobenius distance well under the bf16 step."""
    from torch.optim._muon import _zeropower_via_newtonschulz

    g = torch.Generator().manual_seed(0)
    for shape in ((64, 256), (96, 200)):
        x = torch.randn(*shape, generator=g)
        one = _zeropower_via_newtonschulz(x, (3.4445, -4.7750, 2.0315), 1, 1e-7).double()
        emu = ns_emulate(x, steps=1)
        ulp = torch.maximum(one.abs(), emu.abs()).clamp_min(1e-30)
        ulp = 2.0 ** (torch.floor(torch.log2(ulp)) - 7)
        d = (one - emu).abs()
        assert (d <= ulp).all(), (d / ulp).max()
        assert (d == 0).float().mean() > 0.97
        five = _zeropower_via_newtonschulz(x, (3.4445, -4.7750, 2.0315), 5, 1e-7).double()
        emu5 = ns_emulate(x)
        assert ((five - emu5).norm() / five.norm()).item() < 1e-2
    tall = torch.randn(300, 40, generator=g)
    t5 = _zeropower_via_newtonschulz(tall, (3.4445, -4.7750, 2.0315), 5, 1e-7).double()
    assert ((t5 - ns_emulate(tall.T).T).norm() / t5.norm()).item() < 1e-2


def test_train_accepts_muon_as_an_optimizer_choice():
    from saev_amd.framework import train as T

    cfgs = [T.Config(optim="adam"), T.Config(optim="muon")]
    assert "optim" not in T.CANNOT_PARALLELIZE
    assert len(T.split_cfgs(cfgs)) == 1
