"""CPU-only tests of the dictionary-coherence entries (include/saev_amd.h: COHERENCE): the ctypes signatures against the header's
prototypes, the workspace size, and the shape checks that reject a call before anything is launched."""

import ctypes as C
import re
import subprocess

import pytest
import torch

from conftest import ROOT

ENTRIES = ("saev_coherence_workspace_bytes", "saev_dictionary_coherence")
CTYPES = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64}
BAD_SHAPES = [(0, 64), (-1, 64), (10, 0), (10, 6), (10, 4100), (10, 2), ((1 << 20) + 1, 64)]


def _lib():
    subprocess.run(["make", "-C", str(ROOT)], check=True, capture_output=True)
    from saev_amd import _lib

    return _lib, _lib.load()


def _ctype(decl: str):
    decl = decl.replace("const", "").strip()
    if "*" in decl:
        return C.c_void_p
    return CTYPES[decl.split()[0]]


def test_signatures_match_the_header():
    lib_mod, lib = _lib()
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "saev_amd.h").read_text(), flags=re.S)
    for name in ENTRIES:
        m = re.search(r"(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, f"{name} is not declared"
        res = CTYPES[m.group(1)]
        args = [_ctype(re.sub(r"\w+\s*$", "", a.strip())) for a in m.group(2).split(",")]
        want_res, want_args = lib_mod._SIGNATURES[name]
        assert want_res is res, name
        assert list(want_args) == args, name
        assert hasattr(lib, name) and name in lib_mod.EXPORTED_SYMBOLS


def test_workspace_is_monotone_and_fits_configs3():
    _, lib = _lib()
    for D in (64, 1024, 4096):
        sizes = [lib.saev_coherence_workspace_bytes(S, D) for S in (1, 2, 37, 128, 129, 1000, 4097, 32768, 81920)]
        assert all(b > 0 and b % 256 == 0 for b in sizes)
        assert sizes == sorted(sizes), (D, sizes)
    for S in (2, 1000, 32768):
        sizes = [lib.saev_coherence_workspace_bytes(S, D) for D in (4, 64, 68, 1024, 1280, 4096)]
        assert sizes == sorted(sizes), (S, sizes)
    assert lib.saev_coherence_workspace_bytes(81920, 1280) < 256 * 2**20
    assert lib.saev_coherence_workspace_bytes(32768, 1024) < 128 * 2**20


@pytest.mark.parametrize("shape", BAD_SHAPES)
def test_bad_shapes_are_rejected_before_any_launch(shape):
    """The entry returns SAEV_INVALID_ARG from its argument checks alone: the (never dereferenced) device pointers below would
    fault any launch, and this machine needs no device for it."""
    _, lib = _lib()
    S, D = shape
    assert lib.saev_coherence_workspace_bytes(S, D) == -1
    fake = C.c_void_p(1 << 20)
    out = [C.c_void_p((1 << 20) + 256 * k) for k in range(3)]
    assert lib.saev_dictionary_coherence(fake, S, D, 0, fake, 1 << 40, *out, None) == -1


def test_bad_arguments_are_rejected():
    _, lib = _lib()
    fake = C.c_void_p(1 << 20)
    out = [C.c_void_p((1 << 20) + 256 * k) for k in range(3)]
    need = lib.saev_coherence_workspace_bytes(100, 64)
    assert lib.saev_dictionary_coherence(fake, 100, 64, 2, fake, need, *out, None) == -1      # route
    assert lib.saev_dictionary_coherence(fake, 100, 64, 0, fake, need - 1, *out, None) == -1  # workspace too small
    assert lib.saev_dictionary_coherence(C.c_void_p((1 << 20) + 4), 100, 64, 0, fake, need, *out, None) == -1  # W alignment
    assert lib.saev_dictionary_coherence(None, 100, 64, 0, fake, need, *out, None) == -1


def test_python_entry_rejects_bad_shapes():
    _lib()
    from saev_amd.engine import dictionary_coherence

    for S, D in [(0, 64), (10, 0), (10, 6), (10, 4100), (10, 2)]:
        with pytest.raises(ValueError, match="unsupported shape"):
            dictionary_coherence(torch.zeros(S, D))
    with pytest.raises(ValueError, match="matrix"):
        dictionary_coherence(torch.zeros(8))
    with pytest.raises(ValueError, match="route"):
        dictionary_coherence(torch.zeros(8, 8), route="fp16")
    with pytest.raises(ValueError, match="device"):
        dictionary_coherence(torch.zeros(8, 8))
