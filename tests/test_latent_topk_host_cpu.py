"""CPU-only tests of the per-latent top-k (include/saev_amd.h: LATENT TOP-K): the entries are declared, exported
and bound with the header's types; every argument check refuses a call before anything touches a device; the host-side helpers
(np_topk, csr_topk(axis=1)); and fixture G21, recorded from the reference, against the numpy restatement the GPU tests use."""

import ctypes as C
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse
import torch

from conftest import GOLDEN, ROOT
from latent_topk_restatement import restate_csr

ENTRIES = ("saev_latent_topk_workspace_bytes", "saev_latent_topk_update")
CTYPES = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64}
INVALID, UNSUPPORTED = -1, -3


def _lib():
    subprocess.run(["make", "-C", str(ROOT)], check=True, capture_output=True)
    from saev_amd import _lib

    return _lib, _lib.load()


def _ctype(decl: str, lib_mod):
    decl = decl.replace("const", "").strip()
    if "saev_latent_topk_state" in decl:
        return C.POINTER(lib_mod.SaevLatentTopKState)
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
    assert lib.saev_abi_version() == 12 and lib_mod.ABI_VERSION == 12  # additive entries: the version stays
    assert re.search(r"#define\s+SAEV_AMD_ABI_VERSION\s+12\b", text)


def test_state_layout_matches_header(tmp_path):
    lib_mod, _ = _lib()
    cls = lib_mod.SaevLatentTopKState
    fields = [f for f, _ in cls._fields_]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "saev_amd.h"', "int main(void) {",
           'printf("size %zu\\n", sizeof(saev_latent_topk_state));']
    src += [f'printf("{f} %zu\\n", offsetof(saev_latent_topk_state, {f}));' for f in fields]
    src.append("return 0; }")
    (tmp_path / "layout.c").write_text("\n".join(src))
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True)
    want = dict(line.split() for line in subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.splitlines())
    assert C.sizeof(cls) == int(want["size"])
    for f in fields:
        assert getattr(cls, f).offset == int(want[f]), f


def test_workspace_holds_every_entry_as_a_candidate():
    _, lib = _lib()
    for S in (0, 1, 60, 1004, 32768):
        sizes = [lib.saev_latent_topk_workspace_bytes(e, S) for e in (0, 1, 63, 64, 65, 96000, 16384 * 32, (1 << 31) - 1)]
        assert all(b > 0 and b % 256 == 0 for b in sizes), (S, sizes)
        assert sizes == sorted(sizes), (S, sizes)
        for e, b in zip((0, 1, 63, 64, 65, 96000, 16384 * 32), sizes):
            assert b >= 8 * e + 12 * S  # (value, row) per entry and three integers per latent
    assert lib.saev_latent_topk_workspace_bytes(16384 * 32, 32768) < 8 * 2**20  # configs[1]'s inference shape: a few megabytes
    for e, S in [(-1, 64), (1 << 31, 64), (10, -1), (10, 1 << 31)]:
        assert lib.saev_latent_topk_workspace_bytes(e, S) == -1, (e, S)


def _fake(i):
    return C.c_void_p((1 << 21) + 4096 * i)


def _state(lib_mod, k=5, **ptrs):
    fake = dict(top_val=_fake(0), top_row=_fake(1), top_cnt=_fake(2))
    fake.update(ptrs)
    return lib_mod.SaevLatentTopKState(struct_size=C.sizeof(lib_mod.SaevLatentTopKState), k=k, **fake)


PADDED = dict(idx=_fake(3), val=_fake(4))
CSR = dict(row_ptr=_fake(5), indices=_fake(6), data=_fake(7), nnz=800)
NO_PADDED = dict(idx=None, val=None)
# the fake device pointers are never dereferenced: a launch on them would fault, and this machine has no device to launch on
BAD_CALLS = [
    ("k_zero", dict(k=0), UNSUPPORTED),
    ("k_65", dict(k=65), UNSUPPORTED),
    ("negative_n", dict(n=-1), INVALID),
    ("negative_s", dict(S=-1), INVALID),
    ("negative_cap", dict(cap=-1), INVALID),
    ("negative_nnz", dict(NO_PADDED, **dict(CSR, nnz=-1)), INVALID),
    ("null_state", dict(state=None), INVALID),
    ("null_top_val", dict(top_val=None), INVALID),
    ("null_top_row", dict(top_row=None), INVALID),
    ("null_top_cnt", dict(top_cnt=None), INVALID),
    ("workspace_too_small", dict(ws_short=1), INVALID),
    ("workspace_too_small_csr", dict(NO_PADDED, ws_short=1, **CSR), INVALID),
    ("workspace_null", dict(ws=None), INVALID),
    ("workspace_misaligned", dict(ws=C.c_void_p((1 << 20) + 8)), INVALID),
    ("both_forms", dict(CSR), INVALID),
    ("neither_form", dict(NO_PADDED), INVALID),
    ("idx_without_val", dict(val=None), INVALID),
    ("csr_without_data", dict(NO_PADDED, **dict(CSR, data=None)), INVALID),
    ("row_nnz_with_csr", dict(NO_PADDED, row_nnz=_fake(8), **CSR), INVALID),
    ("negative_row_base", dict(row_base=-1), INVALID),
    ("too_many_entries", dict(n=1 << 20, cap=1 << 12), UNSUPPORTED),
]


def _update(lib_mod, lib, over):
    a = dict(PADDED, row_nnz=None, cap=8, row_ptr=None, indices=None, data=None, nnz=0, keep=None, n=100, S=512, row_base=0, k=5,
             ws=C.c_void_p(1 << 20), ws_short=0, top_val=_fake(0), top_row=_fake(1), top_cnt=_fake(2))
    a.update(over)
    st = _state(lib_mod, k=a["k"], top_val=a["top_val"], top_row=a["top_row"], top_cnt=a["top_cnt"])
    state = a.get("state", C.byref(st))
    need = lib.saev_latent_topk_workspace_bytes(800, 512)
    assert need > 0
    return lib.saev_latent_topk_update(a["idx"], a["val"], a["row_nnz"], a["cap"], a["row_ptr"], a["indices"], a["data"], a["nnz"], a["keep"],
                                       a["n"], a["S"], a["row_base"], state, a["ws"], need - a["ws_short"], None)


@pytest.mark.parametrize("case", BAD_CALLS, ids=[c[0] for c in BAD_CALLS])
def test_update_refuses_bad_arguments_without_a_device(case):
    lib_mod, lib = _lib()
    _, over, status = case
    rc = _update(lib_mod, lib, over)
    assert rc == status, case[0]
    msg = lib.saev_last_error(None).decode()
    assert msg.startswith("saev_latent_topk_update:"), msg  # refused with a message


# status and saev_last_error(NULL) word for word, as the library gave them when the entry carried the whole message in each check
EXACT = {
    "negative_n": "negative size", "k_65": "k must lie in [1, 64]", "null_state": "no saev_latent_topk_state (or its struct_size is unset)",
    "null_top_row": "a state pointer is NULL",
    "both_forms": "give the codes as padded rows (idx, val) or as CSR (row_ptr, indices, data), one of the two",
    "idx_without_val": "idx and val come together", "csr_without_data": "row_ptr, indices and data come together",
    "row_nnz_with_csr": "row_nnz belongs to the padded form", "negative_row_base": "row_base + n leaves int64",
    "too_many_entries": "more than 2^31 - 1 entries in one batch",
    "workspace_too_small": "workspace smaller than saev_latent_topk_workspace_bytes(entries, S)",
    "workspace_too_small_csr": "workspace smaller than saev_latent_topk_workspace_bytes(entries, S)",
    "workspace_null": "workspace smaller than saev_latent_topk_workspace_bytes(entries, S)",
    "workspace_misaligned": "workspace must be 256-byte aligned",
}


def test_refusals_keep_their_status_and_their_text():
    lib_mod, lib = _lib()
    cases = {name: (over, status) for name, over, status in BAD_CALLS}
    for name, text in EXACT.items():
        over, status = cases[name]
        assert _update(lib_mod, lib, over) == status, name
        assert lib.saev_last_error(None).decode() == "saev_latent_topk_update: " + text, name
    assert _update(lib_mod, lib, dict(S=1 << 31)) == INVALID
    assert lib.saev_last_error(None).decode() == "saev_latent_topk_update: size above 2^31 - 1"


def test_an_empty_batch_is_accepted_and_touches_nothing():
    lib_mod, lib = _lib()
    st = _state(lib_mod)
    assert lib.saev_latent_topk_update(None, None, None, 8, None, None, None, 0, None, 0, 512, 0, C.byref(st), None, 0, None) == 0
    # rows without a single slot, and no latents, have nothing to launch either
    ws, nb = C.c_void_p(1 << 20), 1 << 20
    assert lib.saev_latent_topk_update(_fake(3), _fake(4), None, 0, None, None, None, 0, None, 100, 512, 0, C.byref(st), ws, nb, None) == 0
    assert lib.saev_latent_topk_update(_fake(3), _fake(4), None, 8, None, None, None, 0, None, 100, 0, 0, C.byref(st), ws, nb, None) == 0


def test_python_entries_refuse_bad_arguments():
    _lib()
    from saev_amd import helpers
    from saev_amd.engine import LatentTopK
    from saev_amd.framework import inference

    for k in (0, 65, -1):
        with pytest.raises(ValueError, match="unsupported k"):
            LatentTopK(64, k, "cuda")
    with pytest.raises(ValueError, match="unsupported d_sae"):
        LatentTopK(0, 4, "cuda")
    with pytest.raises(RuntimeError, match="no CPU path"):
        LatentTopK(64, 4, "cpu")
    arr = scipy.sparse.csr_array(np.eye(4, dtype=np.float32))
    with pytest.raises(ValueError, match="axis 0 .per column. or 1 .per row."):
        helpers.csr_topk(arr, k=2, axis=2)
    with pytest.raises(TypeError, match="CSR"):
        helpers.csr_topk(np.eye(4), k=2, axis=1)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU path"):
            helpers.csr_topk(arr, k=2, axis=0)
    with pytest.raises(ValueError, match="top_k_tokens"):
        inference.worker_fn(inference.Config(), top_k_tokens=65)


@pytest.mark.parametrize("shape,axis,k", [((17,), None, 5), ((17,), 0, 17), ((6, 9), 0, 3), ((6, 9), 1, 4), ((6, 9), -1, 1),
                                          ((6, 9), None, 7), ((4, 5, 6), 1, 2), ((4, 5, 6), -3, 4), ((4, 5, 6), 2, 6)])
def test_np_topk_matches_torch_topk(shape, axis, k):
    from saev_amd import helpers

    arr = np.random.default_rng(3).permutation(int(np.prod(shape))).astype(np.float32).reshape(shape) - 20  # distinct values
    got = helpers.np_topk(arr, k, axis=axis)
    t = torch.from_numpy(arr)
    want = torch.topk(t.flatten() if axis is None else t, k, dim=0 if axis is None else axis)
    assert isinstance(got, helpers.NumpyTopK) and got._fields == ("values", "indices")
    np.testing.assert_array_equal(got.values, want.values.numpy())
    np.testing.assert_array_equal(got.indices, want.indices.numpy())


def test_np_topk_puts_the_lower_index_first_among_equal_values():
    from saev_amd import helpers

    got = helpers.np_topk(np.array([1.0, 3.0, 3.0, 2.0, 3.0]), 4)
    np.testing.assert_array_equal(got.values, [3.0, 3.0, 3.0, 2.0])
    np.testing.assert_array_equal(got.indices, [1, 2, 4, 3])


@pytest.mark.parametrize("dtype", [np.uint8, np.bool_, np.int8, np.int64, np.float64])
def test_np_topk_orders_every_dtype_as_torch_does(dtype):
    """Unsigned and boolean arrays and the most negative integer (which have no negation) order as torch.topk orders them."""
    from saev_amd import helpers

    info = None if dtype in (np.bool_, np.float64) else np.iinfo(dtype)
    base = {np.bool_: [True, False, True, False, False, True], np.float64: [0.5, -np.inf, np.inf, -0.0, 3.0, 0.5]}.get(
        dtype, None if info is None else [info.min, info.max, 0, info.max // 2, info.min, 1])
    arr = np.array(base, dtype=dtype)
    got = helpers.np_topk(arr, 4)
    want = torch.topk(torch.from_numpy(arr.astype(np.int16) if dtype in (np.uint8, np.bool_) else arr), 4)
    np.testing.assert_array_equal(got.values.astype(np.float64), want.values.numpy().astype(np.float64))
    assert got.values.dtype == arr.dtype
    np.testing.assert_array_equal(np.sort(arr[got.indices])[::-1], got.values)  # the indices point at the values
    assert [int(i) for i in got.indices] == sorted(range(arr.size), key=lambda i: (-float(arr[i]), i))[:4]


def test_csr_topk_axis1_matches_np_topk_on_the_dense_form():
    from saev_amd import helpers

    rng = np.random.default_rng(5)
    n_rows, n_cols, k = 40, 23, 6
    dense = np.zeros((n_rows, n_cols), dtype=np.float32)
    on = rng.random((n_rows, n_cols)) < 0.4
    vals = (rng.permutation(int(on.sum())) + 1).astype(np.float32) / 8
    dense[on] = vals * np.where(rng.random(vals.size) < 0.3, -1, 1)
    dense[0] = 0                                      # an empty row
    dense[1] = 0
    dense[1, [2, 7]] = [0.5, 4.0]                     # fewer than k nonzeros, all positive
    dense[2] = 0
    dense[2, [1, 4, 9]] = [-1.0, 2.0, -3.0]           # negatives that lose to the implicit zeros
    dense[3] = -np.arange(1, n_cols + 1)              # a full row of negatives: no implicit zero to win
    dense[4] = 0
    dense[4, :k + 2] = -np.arange(1, k + 3)           # k + 2 negatives: the implicit zeros take every place
    got = helpers.csr_topk(scipy.sparse.csr_array(dense), k=k, axis=1)
    want = helpers.np_topk(dense, k, axis=1)
    assert got.values.shape == (n_rows, k) and got.values.dtype == np.float32 and got.indices.dtype == np.int64
    np.testing.assert_array_equal(got.values, want.values)
    stored = got.values != 0                          # an implicit zero carries index 0, as the reference has it
    np.testing.assert_array_equal(got.indices[stored], want.indices[stored])
    assert (got.indices[~stored] == 0).all()
    assert (got.values[0] == 0).all() and (got.values[2] == [2.0, 0, 0, 0, 0, 0]).all() and (got.values[4] == 0).all()
    np.testing.assert_array_equal(got.values[3], -np.arange(1, k + 1))


def test_fixture_g21_equals_the_restatement():
    """The checker of the GPU tests against the reference's recorded outputs: value descending, row ascending, zero padding."""
    with np.load(GOLDEN / "g21_csr_topk.npz") as z:
        g = {name: z[name] for name in z.files}
    assert g["ks"].tolist() == [1, 5, 20]
    for case in ("a", "b", "ties"):
        n_cols = int(g[f"{case}_shape"][1])
        per = np.bincount(g[f"{case}_indices"], minlength=n_cols)
        assert per.min() == 0 and (per > 20).any()
        assert (g[f"{case}_data"] < 0).any() and (g[f"{case}_data"] != 0).all()
        for k in g["ks"].tolist():
            values, indices, counts = restate_csr(g[f"{case}_indptr"], g[f"{case}_indices"], g[f"{case}_data"], n_cols, k)
            np.testing.assert_array_equal(g[f"{case}_k{k}_values"], values)
            np.testing.assert_array_equal(counts, np.minimum(per, k))
            if case == "ties":
                assert f"{case}_k{k}_indices" not in g
            else:
                np.testing.assert_array_equal(g[f"{case}_k{k}_indices"], indices)
    assert np.unique(g["a_data"]).size == g["a_data"].size and np.unique(g["ties_data"]).size == 4
    assert (np.bincount(g["a_indices"], minlength=40) == 1).any()  # a column with one entry
