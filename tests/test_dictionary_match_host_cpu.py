"""CPU-only tests of the dictionary-match entries (include/saev_amd.h: DICTIONARY MATCH): the ctypes signatures against the
header's prototypes, the workspace size, and the argument checks that reject a call before anything is launched."""

import ctypes as C
import re
import subprocess

import pytest
import torch

from conftest import ROOT

ENTRIES = ("saev_dictionary_match_workspace_bytes", "saev_dictionary_match")
CTYPES = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64}
SMAX = 1 << 20
BAD_SHAPES = [(0, 10, 64), (10, 0, 64), (SMAX + 1, 10, 64), (10, SMAX + 1, 64), (10, 10, 0), (10, 10, 2), (10, 10, 6),
              (10, 10, 4100), (10, 10, 66)]
INVALID_ARG = -1


def _lib():
    subprocess.run(["make", "-C", str(ROOT)], check=True, capture_output=True)
    from saev_amd import _lib

    return _lib, _lib.load()


def _ctype(decl: str):
    decl = re.sub(r"/\*.*?\*/", "", decl).replace("const", "").strip()
    if "*" in decl:
        return C.c_void_p
    return CTYPES[decl.split()[0]]


def _fakes():
    """(Never dereferenced) device pointers: they would fault any launch, and this machine needs no device to refuse them."""
    fake = C.c_void_p(1 << 20)
    out = [C.c_void_p((1 << 20) + 256 * k) for k in range(3)]
    return fake, out


def test_both_symbols_are_declared_exported_and_listed():
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


def test_the_abi_version_is_still_12():
    lib_mod, lib = _lib()
    assert lib.saev_abi_version() == 12 == lib_mod.ABI_VERSION
    assert re.search(r"#define\s+SAEV_AMD_ABI_VERSION\s+12\b", (ROOT / "include" / "saev_amd.h").read_text())


@pytest.mark.parametrize("shape", BAD_SHAPES)
def test_unsupported_shapes_are_rejected_before_any_launch(shape):
    _, lib = _lib()
    fake, out = _fakes()
    assert lib.saev_dictionary_match_workspace_bytes(*shape) == -1
    Sa, Sb, D = shape
    assert lib.saev_dictionary_match(fake, Sa, fake, Sb, D, 0, 0, fake, 1 << 50, *out, None) == INVALID_ARG


def test_workspace_is_positive_aligned_monotone_and_never_sa_times_sb():
    _, lib = _lib()
    ws = lib.saev_dictionary_match_workspace_bytes
    for D in (4, 64, 68, 1024, 4096):
        for Sa, Sb in [(1, 1), (1, 300), (300, 1), (129, 37), (4097, 4097), (32768, 32768), (8192, 32768), (SMAX, 1), (1, SMAX)]:
            b = ws(Sa, Sb, D)
            assert b > 0 and b % 256 == 0, (Sa, Sb, D, b)
    for D in (64, 1024):
        sizes = [ws(S, S, D) for S in (1, 2, 37, 128, 129, 1000, 4097, 32768, 81920)]
        assert sizes == sorted(sizes), (D, sizes)
    # configs[1] against itself: two fp16 images (64 MiB each) and Sa x ceil(Sb / 128) floats (32 MiB), far below the 4 GiB product
    assert ws(32768, 32768, 1024) < 192 * 2**20
    assert ws(81920, 81920, 1280) < 1024 * 2**20


def test_bad_arguments_are_rejected_without_a_device():
    _, lib = _lib()
    fake, out = _fakes()
    odd = C.c_void_p((1 << 20) + 4)
    need = lib.saev_dictionary_match_workspace_bytes(100, 200, 64)
    call = lib.saev_dictionary_match
    assert call(None, 100, fake, 200, 64, 0, 0, fake, need, *out, None) == INVALID_ARG          # A
    assert call(fake, 100, fake, 200, 64, 0, 0, None, need, *out, None) == INVALID_ARG          # workspace
    for k in range(3):                                                                          # each output
        bad = list(out)
        bad[k] = None
        assert call(fake, 100, fake, 200, 64, 0, 0, fake, need, *bad, None) == INVALID_ARG
    assert call(odd, 100, fake, 200, 64, 0, 0, fake, need, *out, None) == INVALID_ARG           # A alignment
    assert call(fake, 100, odd, 200, 64, 0, 0, fake, need, *out, None) == INVALID_ARG           # B alignment
    assert call(fake, 100, fake, 200, 64, 0, 0, odd, need, *out, None) == INVALID_ARG           # workspace alignment
    for route in (-1, 2, 3):
        assert call(fake, 100, fake, 200, 64, 0, route, fake, need, *out, None) == INVALID_ARG
    assert call(fake, 100, fake, 200, 64, 0, 0, fake, need - 1, *out, None) == INVALID_ARG      # workspace too small
    assert call(fake, 100, None, 200, 64, 0, 0, fake, need, *out, None) == INVALID_ARG          # self mode: Sb repeats Sa


def test_python_entry_rejects_bad_arguments():
    _lib()
    from saev_amd.engine import MatchResult, dictionary_match

    with pytest.raises(ValueError, match="matrices"):
        dictionary_match(torch.zeros(8))
    with pytest.raises(ValueError, match="matrices"):
        dictionary_match(torch.zeros(8, 8), torch.zeros(8))
    with pytest.raises(ValueError, match="share D"):
        dictionary_match(torch.zeros(8, 8), torch.zeros(8, 12))
    for Sa, Sb, D in [(0, 4, 64), (4, 0, 64), (10, 10, 0), (10, 10, 6), (10, 10, 4100), (10, 10, 2)]:
        with pytest.raises(ValueError, match=r"unsupported shape.*2\*\*20.*4096"):
            dictionary_match(torch.zeros(Sa, D), torch.zeros(Sb, D))
    with pytest.raises(ValueError, match="float32"):
        dictionary_match(torch.zeros(8, 8, dtype=torch.float64))
    with pytest.raises(ValueError, match="device"):
        dictionary_match(torch.zeros(8, 8))
    with pytest.raises(ValueError, match="device"):
        dictionary_match(torch.zeros(8, 8), torch.zeros(4, 8))
    with pytest.raises(ValueError, match="route"):
        dictionary_match(torch.zeros(8, 8), route="fp16")
    assert {f.name for f in __import__("dataclasses").fields(MatchResult)} >= {"values", "indices", "route", "candidates",
                                                                                 "capacity", "overflow", "tiles_refiltered"}
    assert isinstance(MatchResult.mmcs, property)
