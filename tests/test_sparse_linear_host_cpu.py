"""CPU-only tests of SPARSE LINEAR (include/saev_amd.h): the entries are declared, exported and bound with the header's
types; the layout mirrors what gcc makes of the header; the workspace arithmetic; every argument check refuses a call before anything
touches a device; the numpy restatement the GPU tests lean on (tests/sparse_linear_restatement.py) is held against fixture G27,
recorded from the reference and scikit-learn; and the Python surface (grouping, defaults, checkpoint, refusals).

Tolerances (derived, not tuned).  Pooling is exact (np.array_equal).  For two points a, b of the convex objective F and any
subgradient s of F at a,  F(a) - F(b) <= <s, a - b> <= ||s||_inf (||W_a - W_b||_1 + ||b_a - b_b||_1); the KKT residual eps_a is the
smallest such ||s||_inf, recomputed here in float64 from the coefficients alone.  The bound is applied in both directions."""

import ctypes as C
import dataclasses
import enum
import json
import logging
import pathlib
import pickle
import re
import subprocess

import numpy as np
import pytest

import sparse_linear_restatement as R
from conftest import GOLDEN, ROOT
from sparse_linear_cases import N_CLS, closed_form_intercepts, cls_design, golden

ENTRIES = ("saev_pool_images_range", "saev_pool_images", "saev_l1_logistic_workspace_bytes", "saev_l1_logistic_layout_of", "saev_l1_logistic_init",
           "saev_l1_logistic_iterate", "saev_l1_logistic_result")
CTYPES = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double}
INVALID, UNSUPPORTED = -1, -3


def _lib():
    subprocess.run(["make", "-C", str(ROOT)], check=True, capture_output=True)
    from saev_amd import _lib

    return _lib, _lib.load()


def _ctype(decl: str, lib_mod):
    decl = decl.replace("const", "").strip()
    if "saev_l1_logistic_layout" in decl:
        return C.POINTER(lib_mod.SaevL1LogisticLayout)
    if "*" in decl:
        return C.c_void_p
    return CTYPES[decl.split()[0]]


def test_entries_are_declared_exported_and_bound_with_the_headers_types():
    lib_mod, lib = _lib()
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "saev_amd.h").read_text(), flags=re.S)
    for name in ENTRIES:
        m = re.search(r"(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, f"{name} is not declared"
        decls = [a.strip() for a in m.group(2).split(",")]
        args = [] if decls == ["void"] else [_ctype(re.sub(r"\w+\s*$", "", a), lib_mod) for a in decls]
        want_res, want_args = lib_mod._SIGNATURES[name]
        assert want_res is CTYPES[m.group(1)], name
        assert list(want_args) == args, name
        assert hasattr(lib, name) and name in lib_mod.EXPORTED_SYMBOLS
    assert lib.saev_abi_version() == 12 and lib_mod.ABI_VERSION == 12  # additive entries: the version stays
    for name in ("SAEV_POOL_MAX 0", "SAEV_POOL_MEAN 1", "SAEV_POOL_ERR_COLUMN 1", "SAEV_POOL_ERR_VALUE 2", "SAEV_L1_ERR_VALUE 1", "SAEV_L1_STATE_DONE 8"):
        assert re.search(r"#define\s+" + name.replace(" ", r"\s+") + r"\b", text)
    assert "sparselinear.hip" in (ROOT / "Makefile").read_text()


def test_layout_mirror_matches_the_header(tmp_path):
    lib_mod, _ = _lib()
    cls = lib_mod.SaevL1LogisticLayout
    fields = [f for f, _ in cls._fields_]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "saev_amd.h"', "int main(void) {", 'printf("size %zu\\n", sizeof(saev_l1_logistic_layout));']
    src += [f'printf("{f} %zu\\n", offsetof(saev_l1_logistic_layout, {f}));' for f in fields]
    src.append("return 0; }")
    (tmp_path / "layout.c").write_text("\n".join(src))
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True)
    want = dict(line.split() for line in subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.splitlines())
    assert C.sizeof(cls) == int(want["size"])
    for f in fields:
        assert getattr(cls, f).offset == int(want[f]), f


def test_workspace_and_layout():
    lib_mod, lib = _lib()
    assert lib.saev_pool_images_range() == 8192  # an fp32 accumulator and an int32 count per latent: 64 KB of LDS
    for n, s, k in [(1, 1, 2), (2, 1, 2), (96, 40, 3), (1025, 4097, 64), (16384, 16384, 10), (2049, 255, 7), ((1 << 31) - 1, 1, 2)]:
        L = lib_mod.SaevL1LogisticLayout()
        assert lib.saev_l1_logistic_layout_of(n, s, k, C.byref(L)) == 0
        kc = 1 if k == 2 else k
        assert L.struct_size == C.sizeof(L) and L.coef_rows == kc
        assert L.total_bytes == lib.saev_l1_logistic_workspace_bytes(n, s, k) and L.total_bytes % 256 == 0
        assert L.chunk_rows % 64 == 0 and 1 <= L.n_chunks <= 32 and (L.n_chunks - 1) * L.chunk_rows < n <= L.n_chunks * L.chunk_rows
        assert L.col_blocks == -(-(s + 1) // 256)
        offs = sorted((getattr(L, f), f) for f, _ in lib_mod.SaevL1LogisticLayout._fields_ if f.startswith("off_"))
        assert all(o % 256 == 0 for o, _ in offs) and len({o for o, _ in offs}) == len(offs)
        r256 = lambda b: -(-b // 256) * 256  # noqa: E731
        sizes = {"off_err": 4, "off_state": 128, "off_w": 3 * r256(8 * kc * (s + 1)), "off_z": 3 * r256(8 * kc * n), "off_g": 8 * kc * (s + 1),
                 "off_part": 8 * L.n_chunks * kc * (s + 1), "off_r": 8 * kc * n, "off_loss": 2 * r256(8 * n), "off_bp": 64 * L.col_blocks}
        for (o, f), (o_next, _) in zip(offs, offs[1:] + [(L.total_bytes, "")]):
            assert o_next - o >= sizes[f], f
    # the bench shape: X is 1.07 GB; the workspace is the 32 partial gradients (42 MB) and a few n x K and K x S arrays
    assert lib.saev_l1_logistic_workspace_bytes(16384, 16384, 10) < 64 * 2**20
    for bad in [(0, 4, 3), (4, 0, 3), (4, 4, 1), (4, 4, 0), (4, 4, 65), (1 << 31, 4, 3), (4, (1 << 30) + 1, 3), (-1, 4, 3)]:
        assert lib.saev_l1_logistic_workspace_bytes(*bad) == -1, bad
        assert lib.saev_l1_logistic_layout_of(*bad, C.byref(lib_mod.SaevL1LogisticLayout())) == UNSUPPORTED
        assert b"saev_l1_logistic_layout_of" in lib.saev_last_error(None)
    assert lib.saev_l1_logistic_layout_of(4, 4, 3, None) == INVALID


def _fake(i):
    return C.c_void_p((1 << 21) + 4096 * i)


# the fake device pointers are never dereferenced: a launch on them would fault, and this machine has no device to launch on
POOL_BAD = [
    ("negative_images", dict(n_images=-1), INVALID), ("zero_images", dict(n_images=0), INVALID), ("zero_tpi", dict(tpi=0), INVALID),
    ("zero_latents", dict(S=0), INVALID), ("negative_nnz", dict(nnz=-1), INVALID), ("rows_2_31", dict(n_images=1 << 16, tpi=1 << 15), UNSUPPORTED),
    ("latents_2_31", dict(S=1 << 31), UNSUPPORTED), ("too_many_ranges", dict(S=8192 * 65535 + 1), UNSUPPORTED), ("bad_agg", dict(agg=2), INVALID),
    ("null_indptr", dict(indptr=None), INVALID), ("null_indices", dict(indices=None), INVALID), ("null_data", dict(data=None), INVALID),
    ("null_out", dict(out=None), INVALID), ("null_err", dict(err=None), INVALID),
]


@pytest.mark.parametrize("case", POOL_BAD, ids=[c[0] for c in POOL_BAD])
def test_pool_images_refuses_bad_arguments_without_a_device(case):
    _, lib = _lib()
    _, over, status = case
    a = dict(indptr=_fake(0), indices=_fake(1), data=_fake(2), nnz=800, n_images=10, tpi=4, S=64, agg=0, out=_fake(3), err=_fake(4))
    a.update(over)
    rc = lib.saev_pool_images(a["indptr"], a["indices"], a["data"], a["nnz"], a["n_images"], a["tpi"], a["S"], a["agg"], a["out"], a["err"], None)
    assert rc == status, (rc, lib.saev_last_error(None))
    assert lib.saev_last_error(None).startswith(b"saev_pool_images:")


L1_BAD = [
    ("negative_n", dict(n=-1), INVALID), ("zero_rows", dict(n=0), UNSUPPORTED), ("zero_columns", dict(S=0), UNSUPPORTED), ("one_class", dict(K=1), INVALID),
    ("too_many_classes", dict(K=65), UNSUPPORTED), ("rows_2_31", dict(n=1 << 31), UNSUPPORTED), ("zero_C", dict(C=0.0), INVALID),
    ("negative_C", dict(C=-1.0), INVALID), ("nan_C", dict(C=float("nan")), INVALID), ("infinite_C", dict(C=float("inf")), INVALID),
    ("negative_tol", dict(tol=-1e-4), INVALID), ("null_X", dict(X=None), INVALID), ("null_y", dict(y=None), INVALID),
    ("workspace_null", dict(ws=None), INVALID), ("workspace_too_small", dict(ws_short=1), INVALID), ("workspace_misaligned", dict(ws=C.c_void_p((1 << 20) + 8)), INVALID),
]


@pytest.mark.parametrize("entry", ["init", "iterate", "result"])
@pytest.mark.parametrize("case", L1_BAD, ids=[c[0] for c in L1_BAD])
def test_l1_logistic_refuses_bad_arguments_without_a_device(case, entry):
    _, lib = _lib()
    _, over, status = case
    a = dict(X=_fake(0), y=_fake(1), n=100, S=64, K=3, C=0.01, tol=1e-4, ws=C.c_void_p(1 << 20), ws_short=0)
    a.update(over)
    need = lib.saev_l1_logistic_workspace_bytes(100, 64, 3)
    common = (a["X"], a["y"], a["n"], a["S"], a["K"], a["C"], a["tol"])
    tail = (a["ws"], need - a["ws_short"], None)
    if entry == "init":
        rc = lib.saev_l1_logistic_init(*common, *tail)
    elif entry == "iterate":
        rc = lib.saev_l1_logistic_iterate(*common, 1, *tail)
    else:
        rc = lib.saev_l1_logistic_result(*common, _fake(2), _fake(3), _fake(4), *tail)
    assert rc == status, (rc, lib.saev_last_error(None))
    assert lib.saev_last_error(None).startswith(b"saev_l1_logistic_" + entry.encode() + b":")


# status and saev_last_error(NULL) word for word, as the library gave them when each entry formatted its own message
L1_EXACT = {
    "negative_n": "negative size", "one_class": "fewer than two classes", "too_many_classes": "1 <= n < 2^31, 1 <= S <= 2^30, 2 <= K <= 64",
    "rows_2_31": "1 <= n < 2^31, 1 <= S <= 2^30, 2 <= K <= 64", "nan_C": "C must be positive and finite", "negative_tol": "kkt_tol must not be negative",
    "null_y": "X and y must not be NULL", "workspace_null": "workspace smaller than saev_l1_logistic_workspace_bytes(n, S, K)",
    "workspace_too_small": "workspace smaller than saev_l1_logistic_workspace_bytes(n, S, K)", "workspace_misaligned": "workspace must be 256-byte aligned",
}
POOL_EXACT = {
    "negative_images": "negative size", "zero_tpi": "n_images, tokens_per_image and n_latents must be at least 1",
    "rows_2_31": "n_images * tokens_per_image and n_latents must stay below 2^31", "too_many_ranges": "more than 65535 latent ranges",
    "bad_agg": "agg is SAEV_POOL_MAX or SAEV_POOL_MEAN", "negative_nnz": "negative nnz", "null_indptr": "indptr, out and err must not be NULL",
    "null_data": "indices and data come with nnz > 0",
}


def test_refusals_keep_their_status_and_their_text():
    _, lib = _lib()
    need = lib.saev_l1_logistic_workspace_bytes(100, 64, 3)
    cases = {name: (over, status) for name, over, status in L1_BAD}
    for name, text in L1_EXACT.items():
        over, status = cases[name]
        a = dict(X=_fake(0), y=_fake(1), n=100, S=64, K=3, C=0.01, tol=1e-4, ws=C.c_void_p(1 << 20), ws_short=0)
        a.update(over)
        common = (a["X"], a["y"], a["n"], a["S"], a["K"], a["C"], a["tol"])
        tail = (a["ws"], need - a["ws_short"], None)
        for entry, call in (("init", lambda: lib.saev_l1_logistic_init(*common, *tail)), ("iterate", lambda: lib.saev_l1_logistic_iterate(*common, -1, *tail)),
                            ("result", lambda: lib.saev_l1_logistic_result(*common, None, None, None, *tail))):
            assert call() == status, (name, entry)
            assert lib.saev_last_error(None).decode() == f"saev_l1_logistic_{entry}: {text}", (name, entry)
    common = (_fake(0), _fake(1), 100, 64, 3, 0.01, 1e-4)
    assert lib.saev_l1_logistic_iterate(*common, -1, C.c_void_p(1 << 20), need, None) == INVALID
    assert lib.saev_last_error(None).decode() == "saev_l1_logistic_iterate: negative n_iters"
    assert lib.saev_l1_logistic_result(*common, _fake(2), None, _fake(4), C.c_void_p(1 << 20), need, None) == INVALID
    assert lib.saev_last_error(None).decode() == "saev_l1_logistic_result: coef, intercept and scalars must not be NULL"
    cases = {name: (over, status) for name, over, status in POOL_BAD}
    for name, text in POOL_EXACT.items():
        over, status = cases[name]
        a = dict(indptr=_fake(0), indices=_fake(1), data=_fake(2), nnz=800, n_images=10, tpi=4, S=64, agg=0, out=_fake(3), err=_fake(4))
        a.update(over)
        rc = lib.saev_pool_images(a["indptr"], a["indices"], a["data"], a["nnz"], a["n_images"], a["tpi"], a["S"], a["agg"], a["out"], a["err"], None)
        assert rc == status, name
        assert lib.saev_last_error(None).decode() == "saev_pool_images: " + text, name


def test_iterate_and_result_refuse_their_own_arguments():
    _, lib = _lib()
    need = lib.saev_l1_logistic_workspace_bytes(100, 64, 3)
    common = (_fake(0), _fake(1), 100, 64, 3, 0.01, 1e-4)
    assert lib.saev_l1_logistic_iterate(*common, -1, C.c_void_p(1 << 20), need, None) == INVALID
    for missing in range(3):
        outs = [_fake(2), _fake(3), _fake(4)]
        outs[missing] = None
        assert lib.saev_l1_logistic_result(*common, *outs, C.c_void_p(1 << 20), need, None) == INVALID


def test_python_surface_refuses_before_a_device_and_without_one():
    import torch
    from saev_amd import classification as cl
    from saev_amd import engine

    z = torch.zeros(2, dtype=torch.int64)
    e32, f32 = torch.zeros(0, dtype=torch.int32), torch.zeros(0)
    with pytest.raises(ValueError, match="agg"):
        engine.pool_images(z, e32, f32, 1, 1, 1, "sum")
    with pytest.raises(ValueError, match="n_latents"):
        engine.pool_images(z, e32, f32, 1, 1, 0)
    with pytest.raises(ValueError, match="tokens_per_image"):
        engine.pool_images(z, e32, f32, 1 << 16, 1 << 15, 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        engine.pool_images(z, e32, f32, 1, 1, 1)
    x, y = torch.zeros(4, 3), torch.tensor([0, 1, 0, 1])
    with pytest.raises(ValueError, match="C must be positive"):
        engine.l1_logistic(x, y, 0.0)
    with pytest.raises(ValueError, match="C must be positive"):
        engine.l1_logistic(x, y, float("nan"))
    with pytest.raises(ValueError, match="float32"):
        engine.l1_logistic(x.double(), y, 1.0)
    with pytest.raises(ValueError, match="X must be"):
        engine.l1_logistic(x, y[:3], 1.0)
    with pytest.raises(ValueError, match="check_every"):
        engine.l1_logistic(x, y, 1.0, check_every=0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        engine.l1_logistic(x, y, 1.0)
    if not torch.cuda.is_available():
        import scipy.sparse

        with pytest.raises(RuntimeError, match="no CPU path"):
            cl.aggregate_to_images(scipy.sparse.csr_matrix(np.ones((4, 3), dtype=np.float32)), 2, 2, cl.PatchAgg.MAX)
        with pytest.raises(RuntimeError, match="no CPU path"):
            cl.SparseLinearClassifier.fit(np.ones((4, 3), dtype=np.float32), np.array([0, 1, 0, 1]))


# ---------------------------------------------------------------- the restatement against G27 ------------------------------------------

def test_fixture_holds_what_it_is_said_to_hold():
    g = golden()
    assert (GOLDEN / "g27_sparse_linear.npz").stat().st_size < 300_000
    n_img, tpi, s = (int(v) for v in g["pool0_shape"])
    data, indptr = g["pool0_data"], g["pool0_indptr"]
    assert np.diff(indptr).min() == 0 and (np.diff(indptr).reshape(n_img, tpi).sum(axis=1) == 0).any()  # empty patches, an empty image
    zeros = data[data == 0]
    assert len(zeros) == 2 and np.signbit(zeros).sum() == 1  # explicit zeros of both signs
    mx, mn = g["pool0_max"], g["pool0_mean"]
    assert mx[0, 0] < 0 and mx[0, 1] == 0 and mn[0, 1] < 0  # stored in all tpi patches / in tpi - 1, negative values only
    assert mn[0, 2] == np.float32(0.25)  # 1e8, 1, -1e8, 1 in float32 patch order; a float64 sum gives 0.5
    assert [tuple(int(v) for v in g[f"cls{i}_shape"][[0, 2, 3]]) for i in range(N_CLS)] == [(96, 40, 2), (96, 40, 3), (200, 300, 5), (64, 1000, 3)]
    for i in range(N_CLS):
        assert g[f"cls{i}_sparse_ref_coef"].dtype == np.float32 and g[f"cls{i}_sparse_opt_coef"].dtype == np.float64
        assert 5 <= int((g[f"cls{i}_sparse_opt_coef"] != 0).any(axis=0).sum()) <= 15
        assert not g[f"cls{i}_zero_opt_coef"].any() and not g[f"cls{i}_zero_ref_coef"].any()
        assert g[f"cls{i}_sparse_opt_coef"].shape[0] == (1 if int(g[f"cls{i}_shape"][3]) == 2 else int(g[f"cls{i}_shape"][3]))


@pytest.mark.parametrize("i", range(4))
def test_restated_pooling_equals_the_references(i):
    g = golden()
    n_img, tpi, s = (int(v) for v in g[f"pool{i}_shape"])
    for agg in ("max", "mean"):
        got = R.pool_images(g[f"pool{i}_indptr"], g[f"pool{i}_indices"], g[f"pool{i}_data"], n_img, tpi, s, agg)
        assert got.dtype == np.float32 and np.array_equal(got, g[f"pool{i}_{agg}"]), agg


@pytest.mark.parametrize("i", range(N_CLS))
def test_restated_solver_against_the_recorded_fits(i):
    g = golden()
    x, y, k = cls_design(g, i)
    _, yi = R.class_indices(y)
    centre = (lambda b: b - b.mean()) if k > 2 else (lambda b: b)
    for tag in ("sparse", "zero"):
        c = float(g[f"cls{i}_{tag}_C"])
        wo, bo = g[f"cls{i}_{tag}_opt_coef"], centre(g[f"cls{i}_{tag}_opt_intercept"])
        wr, br = g[f"cls{i}_{tag}_ref_coef"].astype(np.float64), g[f"cls{i}_{tag}_ref_intercept"].astype(np.float64)
        own = R.fista(x, y, c)
        assert own["converged"] and own["kkt"] <= 1e-4 + R.gradient_rounding(x, len(y), k, c)
        eps_o = R.kkt_residual(x, yi, k, wo, bo, c)
        f_own, f_o, f_r = own["objective"], R.objective(x, yi, k, wo, bo, c), R.objective(x, yi, k, wr, br, c)
        dist = float(np.abs(own["coef"] - wo).sum() + np.abs(own["intercept"] - bo).sum())
        print(f"cls{i} {tag}: C {c:.4g}, {own['n_iter']} iterations, kkt own {own['kkt']:.3g} recorded {eps_o:.3g}, F own - recorded {f_own - f_o:.3g} "
              f"(bound {own['kkt'] * dist:.3g}), recorded - own {f_o - f_own:.3g} (bound {eps_o * dist:.3g}), default - own {f_r - f_own:.3g}")
        # (at the W = 0 value of C saga leaves the intercept unconverged -- tools/gen_golden_sparse_linear.py; the bounds hold whatever eps is)
        assert eps_o <= 1e-5 or tag == "zero"
        assert f_own - f_o <= own["kkt"] * dist and f_o - f_own <= eps_o * dist
        assert f_own <= f_r  # at least as good as where the reference's own setting stops
        assert np.array_equal(R.ranked_support(own["coef"]), R.ranked_support(wo))
        if tag == "zero":
            assert not own["coef"].any()
            closed, curv = closed_form_intercepts(y)
            assert len(set(np.bincount(yi).tolist())) > 1 and np.abs(own["intercept"] - closed).max() <= 2 * own["kkt"] / (c * len(yi) * curv)


# ---------------------------------------------------------------- the Python module ----------------------------------------------------

def _plain(obj):
    if dataclasses.is_dataclass(obj) and not isinstance(obj, type):
        return {f.name: _plain(getattr(obj, f.name)) for f in dataclasses.fields(obj)}
    if isinstance(obj, pathlib.PurePath):
        return str(obj)
    if isinstance(obj, enum.Enum):
        return obj.value
    if isinstance(obj, (tuple, list)):
        return [_plain(v) for v in obj]
    if isinstance(obj, dict):
        return {k: _plain(v) for k, v in obj.items()}
    return obj


def test_apply_grouping_and_config_defaults_are_the_references():
    from saev_amd import classification as cl

    g = golden()
    for name in ("plain", "grouped", "unlisted"):
        case = json.loads(str(g[f"grouping_{name}"]))
        targets, names, mask = cl.apply_grouping(case["labels"], cl.LabelGrouping(name=name, source_col="habitat", groups=case["groups"]))
        assert targets.dtype == np.int32 and mask.dtype == bool
        assert targets.tolist() == case["targets"] and names == case["class_names"] and mask.tolist() == case["mask"]
    assert not all(json.loads(str(g["grouping_unlisted"]))["mask"])
    with pytest.raises(AssertionError, match="in multiple groups"):
        cl.apply_grouping(["a"], cl.LabelGrouping(name="t", source_col="c", groups={"x": ["a"], "y": ["a"]}))
    assert _plain(cl.TrainConfig()) | {"cls": None} == json.loads(str(g["train_config_defaults"])) | {"cls": None}
    own, want = _plain(cl.SparseLinear()), json.loads(str(g["sparse_linear_defaults"]))
    assert {k: own[k] for k in want} == want and own["C"] == 0.01 and own["max_iter"] == 90  # the reference's fields and defaults
    assert {k: own[k] for k in own if k not in want} == {"kkt_tol": 1e-4, "solver_iters": 5000}  # and this solver's two
    assert _plain(cl.TrainConfig().cls) == own and _plain(cl.DecisionTree()) == {"key": "decision-tree", "max_depth": -1}
    assert [m.value for m in cl.PatchAgg] == ["mean", "max"]


def test_classifier_predicts_as_sklearn_and_its_checkpoint_loads(tmp_path):
    from saev_amd import classification as cl

    rng = np.random.default_rng(3)
    x = rng.standard_normal((9, 5))
    multi = cl.SparseLinearClassifier(np.array([[0.0, -2.0, 1.0, 0.0, 1.0], [0.5, 1.0, -2.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0, 0.25]]), [0.1, -0.1, 0.0], [3, 5, 9])
    scores = x @ multi.coef_.T + multi.intercept_
    assert np.array_equal(multi.decision_function(x), scores) and np.array_equal(multi.predict(x), np.array([3, 5, 9])[scores.argmax(axis=1)])
    binary = cl.SparseLinearClassifier(np.array([[0.0, 1.0, 0.0, -1.0, 0.0]]), [0.2], [0, 1])
    z = x @ binary.coef_[0] + 0.2
    assert binary.decision_function(x).shape == (9,) and np.array_equal(binary.predict(x), (z > 0).astype(int))

    path = tmp_path / "cls.pkl"
    cfg = cl.TrainConfig(cls=cl.SparseLinear(C=0.02))
    with open(path, "wb") as fd:
        fd.write(json.dumps({"cfg": cl._jsonable(dataclasses.asdict(cfg)), "test_acc": 0.5, "n_classes": 3, "class_names": ["a", "b", "c"]}).encode() + b"\n")
        pickle.dump({"classifier": multi, "test_pred": multi.predict(x), "test_y": multi.predict(x)}, fd)
    loaded, cls_type, ranked, imp = cl.load_classifier_checkpoint(path, logging.getLogger("t"))
    assert cls_type == "sparse-linear" and isinstance(loaded, cl.SparseLinearClassifier)
    assert imp.tolist() == [0.5, 3.0, 3.0, 0.0, 1.25] and ranked.tolist() == [1, 2, 4, 0, 3]
    assert np.array_equal(loaded.coef_, multi.coef_) and loaded.classes_.tolist() == [3, 5, 9]
    header = json.loads(path.read_bytes().split(b"\n", 1)[0])
    assert header["cfg"]["cls"] == {"key": "sparse-linear", "C": 0.02, "max_iter": 90, "kkt_tol": 1e-4, "solver_iters": 5000}
    assert header["cfg"]["patch_agg"] == "max" and header["cfg"]["run"] == "runs/abcdefg"


def test_decision_tree_is_refused_by_name_and_labels_are_read_from_csv(tmp_path):
    from saev_amd import classification as cl
    from saev_amd.data import write_shards

    with pytest.raises(NotImplementedError, match="DecisionTree"):
        cl.train_worker_fn(cl.TrainConfig(cls=cl.DecisionTree()))
    shards = write_shards(tmp_path / "s0", np.zeros((3, 1, 2, 4), dtype=np.float32))
    with pytest.raises(FileNotFoundError, match="image_labels.csv"):
        cl.load_image_labels(shards)
    (shards / "image_labels.csv").write_text('stem,habitat,"water, kind"\nimg0,pelagic,salt\nimg1,"reef-associated",fresh\nimg2,demersal,salt\n')
    cols, labels = cl.load_image_labels(shards)
    assert cols == ["habitat", "water, kind"] and labels == {"habitat": ["pelagic", "reef-associated", "demersal"], "water, kind": ["salt", "fresh", "salt"]}
    (shards / "image_labels.csv").write_text("stem,habitat\nimg0,pelagic\n")
    with pytest.raises(ValueError, match="1 rows, the shards hold 3"):
        cl.load_image_labels(shards)
    (shards / "image_labels.csv").write_text("name,habitat\na,b\nc,d\ne,f\n")
    with pytest.raises(ValueError, match="header"):
        cl.load_image_labels(shards)


def test_the_module_imports_neither_sklearn_nor_cloudpickle():
    src = (ROOT / "saev_amd" / "classification.py").read_text()
    assert not re.search(r"^\s*(import|from)\s+(sklearn|cloudpickle)", src, flags=re.M)
    for tool in ("train_audit_classifier.py", "bench_sparse_linear.py"):
        assert not re.search(r"^\s*(import|from)\s+(sklearn|cloudpickle)", (ROOT / "tools" / tool).read_text(), flags=re.M)
