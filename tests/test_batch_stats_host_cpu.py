"""CPU-only tests of the batch-statistics entries (include/saev_amd.h: BATCH STATISTICS): declared, exported and bound with the
header's types; the ctypes mirror of saev_batch_acc against what gcc makes of the header; the workspace size; and every argument
check, which refuses a call before anything touches a device."""

import ctypes as C
import re
import subprocess

import pytest

from conftest import ROOT

ENTRIES = ("saev_batch_stats_workspace_bytes", "saev_batch_stats", "saev_row_norm_mean")
CTYPES = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64}
INVALID, UNSUPPORTED = -1, -3


def _lib():
    subprocess.run(["make", "-C", str(ROOT)], check=True, capture_output=True)
    from saev_amd import _lib

    return _lib, _lib.load()


def _ctype(decl: str, lib_mod):
    decl = decl.replace("const", "").strip()
    if "saev_batch_acc" in decl:
        return C.POINTER(lib_mod.SaevBatchAcc)
    if "*" in decl:
        return C.c_void_p
    return CTYPES[decl.split()[0]]


def test_entries_are_declared_exported_and_bound_with_the_headers_types():
    lib_mod, lib = _lib()
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "saev_amd.h").read_text(), flags=re.S)
    for name in ENTRIES:
        m = re.search(r"(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, f"{name} is not declared"
        res = CTYPES[m.group(1)]
        args = [_ctype(re.sub(r"\w+\s*$", "", a.strip()), lib_mod) for a in m.group(2).split(",")]
        want_res, want_args = lib_mod._SIGNATURES[name]
        assert want_res is res, name
        assert list(want_args) == args, name
        assert hasattr(lib, name) and name in lib_mod.EXPORTED_SYMBOLS
    assert lib.saev_abi_version() == 12  # additive entries: the version stays


def test_batch_acc_layout_matches_header(tmp_path):
    lib_mod, _ = _lib()
    cls = lib_mod.SaevBatchAcc
    fields = [f for f, _ in cls._fields_]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "saev_amd.h"', "int main(void) {",
           'printf("size %zu\\n", sizeof(saev_batch_acc));', 'printf("flag %d\\n", SAEV_BATCH_OVERWRITE);',
           'printf("rn %d\\n", SAEV_ROW_NORM_WORKSPACE_BYTES);']
    src += [f'printf("{f} %zu\\n", offsetof(saev_batch_acc, {f}));' for f in fields]
    src.append("return 0; }")
    (tmp_path / "layout.c").write_text("\n".join(src))
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True)
    want = dict(line.split() for line in subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.splitlines())
    assert C.sizeof(cls) == int(want["size"])
    for f in fields:
        assert getattr(cls, f).offset == int(want[f]), f
    assert lib_mod.BATCH_OVERWRITE == int(want["flag"])
    assert lib_mod.ROW_NORM_WORKSPACE_BYTES == int(want["rn"])


def test_workspace_is_monotone_and_refuses_unsupported_widths():
    _, lib = _lib()
    for D in (4, 256, 1024, 1280, 4096):
        sizes = [lib.saev_batch_stats_workspace_bytes(n, D) for n in (0, 1, 15, 16, 17, 1000, 4099, 16384, 16385, 1 << 20, (1 << 31) - 1)]
        assert all(b > 0 and b % 256 == 0 for b in sizes), (D, sizes)
        assert sizes == sorted(sizes), (D, sizes)
    assert lib.saev_batch_stats_workspace_bytes(16384, 1024) < 16 * 2**20
    for n, D in [(16, 6), (16, 8192), (16, 0), (16, -4), (-1, 64), (16, 4100)]:
        assert lib.saev_batch_stats_workspace_bytes(n, D) == -1, (n, D)


def _acc(lib_mod, **ptrs):
    fake = {k: C.c_void_p((1 << 21) + 4096 * i) for i, k in enumerate(("col_sum", "scalars", "n_pos", "value_sum", "live"))}
    fake.update(ptrs)
    return lib_mod.SaevBatchAcc(struct_size=C.sizeof(lib_mod.SaevBatchAcc), flags=0, live_eps=1e-12, **fake)


# (x, n, D, S, cap, workspace bytes relative to the need, status): the fake device pointers are never dereferenced -- a launch on
# them would fault, and this machine has no device to launch on
BAD_CALLS = [
    ("null_x", dict(x=None), INVALID),
    ("d_not_multiple_of_4", dict(D=6), UNSUPPORTED),
    ("d_above_4096", dict(D=8192), UNSUPPORTED),
    ("d_zero", dict(D=0), UNSUPPORTED),
    ("negative_n", dict(n=-1), INVALID),
    ("negative_d", dict(D=-4), INVALID),
    ("negative_s", dict(S=-1), INVALID),
    ("negative_cap", dict(cap=-1), INVALID),
    ("workspace_too_small", dict(ws_short=1), INVALID),
    ("workspace_null", dict(ws=None), INVALID),
    ("workspace_misaligned", dict(ws=C.c_void_p((1 << 20) + 8)), INVALID),
    ("x_misaligned", dict(x=C.c_void_p((1 << 22) + 4)), INVALID),
    ("null_idx", dict(idx=None), INVALID),
    ("null_acc", dict(acc=None), INVALID),
    ("unknown_flag", dict(flags=2), INVALID),
]


@pytest.mark.parametrize("case", BAD_CALLS, ids=[c[0] for c in BAD_CALLS])
def test_batch_stats_refuses_bad_arguments_without_a_device(case):
    lib_mod, lib = _lib()
    _, over, status = case
    a = dict(x=C.c_void_p(1 << 22), n=100, D=64, S=512, cap=8, ws=C.c_void_p(1 << 20), idx=C.c_void_p(1 << 23), ws_short=0, flags=0)
    acc = _acc(lib_mod)
    a["acc"] = C.byref(acc)
    a.update(over)
    acc.flags = a["flags"]
    need = lib.saev_batch_stats_workspace_bytes(100, 64)
    assert need > 0
    rc = lib.saev_batch_stats(a["x"], C.c_void_p(1 << 24), a["idx"], C.c_void_p(1 << 25), None, None, a["n"], a["D"], a["S"], a["cap"],
                              a["acc"], a["ws"], need - a["ws_short"], None)
    assert rc == status, case[0]
    msg = lib.saev_last_error(None).decode()
    assert msg.startswith("saev_batch_stats:"), msg  # refused with a message


def test_an_empty_batch_is_accepted_and_touches_nothing():
    lib_mod, lib = _lib()
    acc = _acc(lib_mod)
    assert lib.saev_batch_stats(None, None, None, None, None, None, 0, 64, 512, 8, C.byref(acc), None, 0, None) == 0


def test_row_norm_mean_refuses_bad_arguments_without_a_device():
    lib_mod, lib = _lib()
    W, out, ws, nb = C.c_void_p(1 << 22), C.c_void_p(1 << 23), C.c_void_p(1 << 20), lib_mod.ROW_NORM_WORKSPACE_BYTES
    for args, status in [((None, 10, 64, out, ws, nb), INVALID), ((W, 10, 64, None, ws, nb), INVALID), ((W, 0, 64, out, ws, nb), INVALID),
                         ((W, -1, 64, out, ws, nb), INVALID), ((W, 10, -4, out, ws, nb), INVALID), ((W, 10, 6, out, ws, nb), UNSUPPORTED),
                         ((W, 10, 8192, out, ws, nb), UNSUPPORTED), ((W, 10, 64, out, ws, nb - 1), INVALID), ((W, 10, 64, out, None, nb), INVALID),
                         ((C.c_void_p((1 << 22) + 4), 10, 64, out, ws, nb), INVALID)]:
        assert lib.saev_row_norm_mean(*args, None) == status, args
        assert lib.saev_last_error(None).decode().startswith("saev_row_norm_mean:")


def test_python_entries_refuse_bad_shapes():
    _lib()
    import torch

    from saev_amd.engine import BatchStats, row_norm_mean

    for S, D in [(0, 64), (10, 6), (10, 8192), (10, 0)]:
        with pytest.raises(ValueError, match="unsupported shape"):
            row_norm_mean(torch.zeros(S, D))
    with pytest.raises(ValueError, match="matrix"):
        row_norm_mean(torch.zeros(8))
    with pytest.raises(ValueError, match="device"):
        row_norm_mean(torch.zeros(8, 8))
    for D in (6, 8192, 0):
        with pytest.raises(ValueError, match="unsupported d_model"):
            BatchStats(D, 64, "cpu")
    with pytest.raises(ValueError, match="unknown outputs"):
        BatchStats(64, 64, "cpu", want=("col_sum", "histogram"))
