"""CPU-only tests of POOL CSR (include/saev_amd.h): the entries are declared, exported and bound with the header's
types; every argument check refuses a call before anything touches a device, in the order the header states; the workspace has its
documented size; the numpy restatement the GPU tests lean on (tests/pool_csr_restatement.py) agrees with a brute-force dense matrix
and with examples counted by hand; every case of tests/pool_csr_cases.py holds what it is said to hold; and ``engine.pool_csr``
refuses bad arguments on the host.

Tolerances: none."""

import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import pool_csr_cases as K
import pool_csr_restatement as R
from conftest import ROOT
from saev_amd.engine import pool_csr  # noqa: F401  (without the feature nothing here can run)

CTYPES = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double, "float": C.c_float}
INVALID, UNSUPPORTED = -1, -3


def _lib():
    subprocess.run(["make", "-C", str(ROOT)], check=True, capture_output=True)
    from saev_amd import _lib

    return _lib, _lib.load()


def test_the_entries_are_declared_exported_and_bound_with_the_headers_types():
    lib_mod, lib = _lib()
    raw = (ROOT / "include" / "saev_amd.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name, n_args in (("saev_pool_csr_range", 0), ("saev_pool_csr_workspace_bytes", 4), ("saev_pool_csr_count", 14), ("saev_pool_csr_fill", 18)):
        m = re.search(r"(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, f"{name} is not declared"
        args = []
        for a in (m.group(2).split(",") if m.group(2).strip() != "void" else []):
            decl = re.sub(r"\w+\s*$", "", a.strip()).replace("const", "").strip()
            args.append(C.c_void_p if "*" in decl else CTYPES[decl.split()[0]])
        want_res, want_args = lib_mod._SIGNATURES[name]
        assert want_res is CTYPES[m.group(1)] and list(want_args) == args and len(args) == n_args, name
        assert hasattr(lib, name) and name in lib_mod.EXPORTED_SYMBOLS
    assert lib.saev_abi_version() == 12 and lib_mod.ABI_VERSION == 12  # additive entries: the version stays
    codes = {k: int(v) for k, v in re.findall(r"#define\s+(SAEV_POOL_CSR_ERR_\w+)\s+(\d+)\b", text)}
    assert codes == {"SAEV_POOL_CSR_ERR_COLUMN": R.ERR_COLUMN, "SAEV_POOL_CSR_ERR_VALUE": R.ERR_VALUE, "SAEV_POOL_CSR_ERR_INDPTR": R.ERR_INDPTR,
                     "SAEV_POOL_CSR_ERR_THRESHOLD": R.ERR_THRESHOLD}
    assert "POOL CSR" in raw and "DESIGN.md 3.30" in raw and "poolcsr.hip" in (ROOT / "Makefile").read_text()
    assert lib.saev_pool_csr_range() == K.RANGE and K.RANGE % 64 == 0


def _fake(i):
    return C.c_void_p((1 << 21) + 4096 * i)


SHAPE = dict(nnz=800, n_images=10, T=12, S=64, thr=0.0)
TOO_SMALL = "workspace smaller than saev_pool_csr_workspace_bytes(n_images, tokens_per_image, n_latents, nnz)"
ZERO = "n_images, tokens_per_image and n_latents must be at least 1"
BELOW = "n_images * tokens_per_image and n_latents must stay below 2^31"
UNITS = "n_images * ceil(n_latents / 4096) must stay below 2^31"
SCALAR = "a scalar threshold must be finite and at least 0"
SPARSE = "indices and data come with nnz > 0"
OUT = {"count": "out_indptr and err must not be NULL", "fill": "out_indptr, out_indices, out_data and err must not be NULL"}
# the fake device pointers are never dereferenced: a launch on them would fault, and this machine has no device to launch on.  Status
# and saev_last_error(NULL) word for word, then the FIRST refusal of two bad arguments at once, in the header's order
BAD = [
    ("negative_images", dict(n_images=-1), INVALID, "negative size"), ("negative_tokens", dict(T=-1), INVALID, "negative size"),
    ("negative_latents", dict(S=-1), INVALID, "negative size"), ("negative_nnz", dict(nnz=-1), INVALID, "negative size"),
    ("zero_images", dict(n_images=0), INVALID, ZERO), ("zero_tokens", dict(T=0), INVALID, ZERO), ("zero_latents", dict(S=0), INVALID, ZERO),
    ("images_2_31", dict(n_images=1 << 31, T=1), UNSUPPORTED, BELOW), ("rows_2_31", dict(n_images=1 << 19, T=4096), UNSUPPORTED, BELOW),
    ("latents_2_31", dict(S=1 << 31), UNSUPPORTED, BELOW),
    ("units_2_31", dict(n_images=1 << 30, T=1, S=2 * 4096 + 1), UNSUPPORTED, UNITS),
    ("thr_negative", dict(thr=-0.5), INVALID, SCALAR), ("thr_nan", dict(thr=float("nan")), INVALID, SCALAR), ("thr_inf", dict(thr=float("inf")), INVALID, SCALAR),
    ("null_indptr", dict(indptr=None), INVALID, "indptr is NULL"), ("null_indices", dict(indices=None), INVALID, SPARSE), ("null_data", dict(data=None), INVALID, SPARSE),
    ("null_out_indptr", dict(out_indptr=None), INVALID, OUT), ("null_err", dict(err=None), INVALID, OUT),
    ("workspace_null", dict(ws=None), INVALID, TOO_SMALL), ("workspace_too_small", dict(ws_short=1), INVALID, TOO_SMALL),
    ("workspace_misaligned", dict(ws=C.c_void_p((1 << 20) + 8)), INVALID, "workspace must be 256-byte aligned"),
    ("negative_before_zero", dict(nnz=-1, S=0), INVALID, "negative size"), ("zero_before_2_31", dict(T=0, S=1 << 31), INVALID, ZERO),
    ("below_before_units", dict(S=1 << 31, n_images=1 << 30, T=1), UNSUPPORTED, BELOW), ("units_before_thr", dict(n_images=1 << 30, T=1, S=8193, thr=-1.0), UNSUPPORTED, UNITS),
    ("thr_before_pointers", dict(thr=-1.0, indptr=None), INVALID, SCALAR), ("indptr_before_indices", dict(indptr=None, data=None), INVALID, "indptr is NULL"),
    ("input_before_output", dict(indices=None, err=None), INVALID, SPARSE), ("outputs_before_workspace", dict(out_indptr=None, ws_short=1), INVALID, OUT),
    ("size_before_alignment", dict(ws=C.c_void_p((1 << 20) + 8), ws_short=1), INVALID, TOO_SMALL),
]
FILL_ONLY = [("null_out_indices", dict(out_indices=None), INVALID, OUT), ("null_out_data", dict(out_data=None), INVALID, OUT)]


def _call(lib, entry, over):
    a = dict(SHAPE, indptr=_fake(0), indices=_fake(1), data=_fake(2), thr_vec=None, out_indptr=_fake(3), out_indices=_fake(4), out_data=_fake(5),
             out_patch=_fake(6), out_count=_fake(7), err=_fake(8), ws=C.c_void_p(1 << 20), ws_short=0)
    a.update(over)
    need = lib.saev_pool_csr_workspace_bytes(SHAPE["n_images"], SHAPE["T"], SHAPE["S"], SHAPE["nnz"])
    head = (a["indptr"], a["indices"], a["data"], a["nnz"], a["n_images"], a["T"], a["S"], a["thr"], a["thr_vec"])
    if entry == "count":
        return lib.saev_pool_csr_count(*head, a["out_indptr"], a["ws"], need - a["ws_short"], a["err"], None)
    return lib.saev_pool_csr_fill(*head, a["out_indptr"], a["out_indices"], a["out_data"], a["out_patch"], a["out_count"], a["ws"], need - a["ws_short"],
                                  a["err"], None)


@pytest.mark.parametrize("entry", ["count", "fill"])
@pytest.mark.parametrize("case", BAD + FILL_ONLY, ids=[c[0] for c in BAD + FILL_ONLY])
def test_the_calls_refuse_bad_arguments_without_a_device_in_order(case, entry):
    _, lib = _lib()
    _, over, status, text = case
    if case in FILL_ONLY and entry == "count":
        status, text = INVALID, TOO_SMALL  # the count pass takes no such pointer: make it fail at the last check instead
        over = dict(over, ws=None)
    rc = _call(lib, entry, over)
    assert rc == status, (rc, lib.saev_last_error(None))
    assert lib.saev_last_error(None).decode() == f"saev_pool_csr_{entry}: " + (text[entry] if isinstance(text, dict) else text)


def test_what_is_allowed_gets_as_far_as_the_workspace_check():
    """nnz = 0 needs no indices; a threshold vector makes the scalar irrelevant; the detail arrays may be NULL; the limits themselves pass."""
    _, lib = _lib()
    for over in (dict(nnz=0, indices=None, data=None), dict(thr=-1.0, thr_vec=_fake(9)), dict(thr=float("nan"), thr_vec=_fake(9)), dict(out_patch=None, out_count=None),
                 dict(out_patch=None), dict(n_images=(1 << 31) - 1, T=1, S=4096), dict(n_images=1, T=1, S=(1 << 31) - 1), dict(thr=float(np.finfo(np.float32).max))):
        for entry in ("count", "fill"):
            assert _call(lib, entry, dict(over, ws=None)) == INVALID and lib.saev_last_error(None).decode() == f"saev_pool_csr_{entry}: " + TOO_SMALL


def test_workspace_size():
    _, lib = _lib()
    size = lib.saev_pool_csr_workspace_bytes
    for n, t, s, nnz in ((10, 12, 64, 800), (1, 1, 1, 0), (16_384, 16, 16_384, 1 << 23), (200_000, 1, 70_001, 400_000), (3, 5, K.RANGE, 7), (3, 5, K.RANGE + 1, 7),
                         (70_000, 1, 48, 140_000), ((1 << 31) - 1, 1, 1, 0)):
        want = R.workspace_bytes(n, s, K.RANGE)
        assert size(n, t, s, nnz) == want and want % 256 == 0, (n, t, s, nnz)
    assert size(300, 5, K.RANGE + 1, 7) > size(300, 5, K.RANGE, 7) == size(300, 5, 1, 10**12)  # sized by units, not by nnz
    for bad in ((0, 1, 1, 0), (1, 0, 1, 0), (1, 1, 0, 0), (-1, 1, 1, 0), (1, 1, 1, -1), (1 << 31, 1, 1, 0), (1 << 19, 4096, 1, 0), (1, 1, 1 << 31, 0), (1 << 30, 1, 2 * K.RANGE + 1, 0)):
        assert size(*bad) == -1, bad


def test_python_surface_refuses_host_tensors_and_bad_arguments():
    import torch
    from saev_amd import engine

    z, i, v = torch.zeros(5, dtype=torch.int64), torch.zeros(0, dtype=torch.int32), torch.zeros(0)
    ok = dict(n_images=1, tokens_per_image=4, n_latents=3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        engine.pool_csr(z, i, v, **ok)
    for over, match in ((dict(n_images=0), "n_images"), (dict(tokens_per_image=0), "tokens_per_image"), (dict(n_latents=0), "n_latents"), (dict(n_latents=1 << 31), "n_latents"),
                        (dict(n_images=1 << 29), "below 2\\^31"), (dict(threshold=-1.0), "scalar threshold"), (dict(threshold=float("nan")), "scalar threshold"),
                        (dict(threshold=float("inf")), "scalar threshold"), (dict(threshold=torch.zeros(4)), "threshold vector"),
                        (dict(threshold=np.zeros(3)), "threshold vector"), (dict(threshold=torch.zeros(3, dtype=torch.float64)), "threshold vector")):
        with pytest.raises(ValueError, match=match):
            engine.pool_csr(z, i, v, **dict(ok, **over))
    assert engine.PoolCsrResult._ERRORS == {1: "a column index lies outside [0, n_latents)", 2: "a stored value is not finite",
                                            3: "indptr is not a non-decreasing sequence of positions into indices", 4: "an entry of the threshold vector is negative"}


# ---------------------------------------------------------------- the restatement ---------------------------------------------------------

def _brute_force(c):
    """Zeros, the elementwise maximum of every stored value that passes, then nonzero -- and, for the details, a second dense walk."""
    n, t, s = c["n_images"], c["t"], c["s"]
    rows = np.repeat(np.arange(n * t), np.diff(c["indptr"]))
    thr = np.broadcast_to(np.asarray(c["thr"], dtype=np.float32), (s,))
    with np.errstate(invalid="ignore"):
        ok = c["data"] > thr[c["indices"]]
    img, lat, val, patch = rows[ok] // t, c["indices"][ok], c["data"][ok], rows[ok] % t
    fires = np.zeros((n, s), dtype=bool)
    fires[img, lat] = True
    dense = np.full((n, s), -np.inf, dtype=np.float32)
    np.maximum.at(dense, (img, lat), val)
    count = np.zeros((n, s), dtype=np.int32)
    np.add.at(count, (img, lat), 1)
    first = np.full((n, s), t, dtype=np.int32)
    at = val == dense[img, lat]
    np.minimum.at(first, (img[at], lat[at]), patch[at].astype(np.int32))
    indptr = np.zeros(n + 1, dtype=np.int64)
    indptr[1:] = np.cumsum(fires.sum(axis=1))
    return dict(indptr=indptr, indices=np.nonzero(fires)[1].astype(np.int32), data=dense[fires], patch=first[fires], count=count[fires])


@pytest.fixture(scope="module")
def restated():
    return {name: R.restate(**make()) for name, make in K.SMALL.items()}


@pytest.mark.parametrize("name", [n for n, make in K.SMALL.items() if K.densifiable(make())])
def test_restatement_equals_a_brute_force_dense_matrix(name, restated):
    c = K.SMALL[name]()
    want = _brute_force(c)
    for key in R.ARRAYS:
        assert restated[name][key].dtype == want[key].dtype and np.array_equal(R.bits(restated[name][key]), R.bits(want[key])), key
    if np.ndim(c["thr"]) == 0 and c["thr"] == 0:  # the parent's path on the host: zeros, the maximum of every stored value, != 0
        rows = np.repeat(np.arange(c["n_images"] * c["t"]), np.diff(c["indptr"]))
        dense = np.zeros((c["n_images"], c["s"]), dtype=np.float32)
        np.maximum.at(dense, (rows // c["t"], c["indices"]), c["data"])
        assert np.array_equal(np.nonzero(dense)[1], want["indices"]) and np.array_equal(R.bits(dense[dense != 0]), R.bits(want["data"]))


def test_restatement_on_an_example_counted_by_hand():
    ev = [(0, 0, 2, 1.0), (0, 1, 2, 3.0), (0, 2, 2, 3.0), (0, 1, 0, 0.5), (0, 2, 1, -1.0), (1, 0, 1, 0.0), (2, 2, 1, 2.0), (2, 0, 1, 2.0), (2, 1, 0, 4.0)]
    out = R.restate(**K.build(ev, 3, 3, 3))
    assert out["indptr"].tolist() == [0, 2, 2, 4] and out["indices"].tolist() == [0, 2, 0, 1] and out["data"].tolist() == [0.5, 3.0, 4.0, 2.0]
    assert out["patch"].tolist() == [1, 1, 1, 0] and out["count"].tolist() == [1, 3, 1, 2]
    out = R.restate(**K.build(ev, 3, 3, 3, thr=1.0))  # 1.0 itself no longer passes
    assert out["indptr"].tolist() == [0, 1, 1, 3] and out["data"].tolist() == [3.0, 4.0, 2.0] and out["count"].tolist() == [2, 1, 2]


def test_cases_hold_what_they_are_said_to_hold(restated):
    case = {name: make() for name, make in K.SMALL.items()}
    for name, c in case.items():
        assert R.error_word(c["indptr"], c["indices"], c["data"], c["s"], c["thr"]) == 0, name
    assert case["one_image"]["n_images"] == 1 and restated["one_image"]["indptr"][-1] > 0
    assert [case[f"tokens_{t}"]["t"] for t in (1, 5, 16, 257)] == [1, 5, 16, 257]
    sizes = {"s_1": 1, "s_64": 64, "s_65": 65, "s_range_minus_1": K.RANGE - 1, "s_range": K.RANGE, "s_range_plus_1": K.RANGE + 1, "s_70001": 70_001}
    for name, s in sizes.items():
        c = case[name]
        assert c["s"] == s and c["indices"].max() == s - 1 and restated[name]["indices"].max() == s - 1, name  # the last latent is stored and fires
        assert s == 1 or any((np.diff(c["indices"][a:b]) < 0).any() for a, b in zip(c["indptr"][:-1], c["indptr"][1:])), name  # unsorted rows
    c = case["spans"]
    assert tuple(int(c["indptr"][(i + 1) * 5] - c["indptr"][i * 5]) for i in range(7)) == K.SPAN_LENGTHS and np.diff(restated["spans"]["indptr"]).tolist() == list(K.SPAN_LENGTHS)
    c = case["long_span"]
    assert c["t"] == 257 and c["indptr"][257] == K.LONG_SPAN == 70_000 and len(c["data"]) == K.LONG_SPAN + 2 and np.diff(restated["long_span"]["indptr"])[0] == c["s"]
    assert restated["long_span"]["count"].max() > 64 and restated["long_span"]["patch"].max() > 200
    assert len(case["no_entries"]["data"]) == 0 and restated["no_entries"]["indptr"].tolist() == [0, 0, 0, 0]
    full = restated["full_row"]
    assert K.FULL_S == 8193 > K.RANGE
    assert np.diff(full["indptr"]).tolist() == [K.FULL_S, 0] and np.array_equal(full["indices"], np.arange(K.FULL_S)) and len(case["full_row"]["data"]) == 2 * K.FULL_S
    many = case["many_images"]
    assert many["n_images"] == K.MANY == 70_000 > 65_536 and (np.diff(many["indptr"]) == 2).all() and (many["indices"][0::2] != many["indices"][1::2]).all()
    assert set(np.diff(restated["many_images"]["indptr"]).tolist()) == {0, 1, 2}
    v0, vh = restated["values_thr_0"], restated["values_thr_half"]
    assert v0["indices"].tolist() == [1, 6, 8] * 2 and vh["indices"].tolist() == [1, 8] * 2  # thr itself, the zeros, the negatives and latent 10 are out
    assert v0["data"][1] == np.float32(1e-45) > 0 and v0["data"][2] == K.FLT_MAX and vh["data"][0] == np.nextafter(np.float32(0.5), np.float32(1)) and v0["data"][0] == np.float32(1e-45)
    d = case["values_thr_0"]["data"]
    assert (d == 0).sum() == 4 + 2 and np.signbit(d[d == 0]).sum() == 2 and (d[case["values_thr_0"]["indices"] == 10] < 0).all() and (case["values_thr_0"]["indices"] == 10).sum() == 6
    p = restated["patches"]
    assert p["patch"].tolist() == [0, 5, 2, 0, 5, 0] and p["count"].tolist() == [3, 3, 4, 6, 6, 6] and p["data"].tolist() == [9.0, 7.0, 4.0, 2.5, 6.0, 9.0]
    col = restated["columns"]
    assert col["indices"].tolist() == [1, 3, 6, 7, 0, 2, 3] and col["data"].tolist() == [2.0, 5.0, 1.0, 1.0, 1.0, 1.0, 4.0] and col["count"].tolist() == [1, 3, 1, 1, 1, 1, 2]
    assert col["patch"].tolist() == [0, 1, 1, 0, 1, 1, 0]
    vt = restated["vector_thresholds"]
    assert np.diff(vt["indptr"]).tolist() == [2, 3, 5] and vt["indices"].tolist() == [0, 6, 0, 1, 6, 0, 1, 2, 6, 7]  # 2.0 under 2.0 is out
    assert not np.isin(vt["indices"], [3, 4, 5]).any()  # +Inf, NaN and FLT_MAX under FLT_MAX
    thr = case["vector_random"]["thr"]
    assert np.isnan(thr).sum() > 100 and np.isposinf(thr).sum() > 100 and (thr == 0).sum() > 300 and case["vector_random"]["s"] > K.RANGE
    assert not np.isin(restated["vector_random"]["indices"], np.flatnonzero(np.isnan(thr) | np.isinf(thr))).any() and restated["vector_random"]["indices"].max() >= K.RANGE
    for kind in K.BROKEN:
        c, code = K.broken(kind)
        assert R.error_word(c["indptr"], c["indices"], c["data"], c["s"], c["thr"]) == code, kind
    assert {K.broken(k)[1] for k in K.BROKEN} == {1, 2, 3, 4}
    c, _ = K.broken("indptr_decreasing")
    assert c["indptr"].min() >= 0 and c["indptr"].max() <= len(c["data"])  # only the order is wrong
    base = case["tokens_16"]
    alone = R.restate(**K.one_image_of(base, 3))
    lo, hi = restated["tokens_16"]["indptr"][3:5]
    perm = np.asarray([4, 0, 6, 2, 1, 5, 3])
    moved = R.restate(**K.permuted(base, perm))
    for key in R.ARRAYS[1:]:
        assert np.array_equal(R.bits(alone[key]), R.bits(restated["tokens_16"][key][lo:hi])), key
    assert np.array_equal(np.diff(moved["indptr"]), np.diff(restated["tokens_16"]["indptr"])[perm])
