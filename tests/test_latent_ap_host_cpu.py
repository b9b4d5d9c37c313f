"""CPU-only tests of the latent AP (include/saev_amd.h: LATENT AP): the entries are declared, exported and bound with
the header's types; the layout mirrors what gcc makes of the header; every argument check refuses a call before anything touches a
device; and the numpy restatement the GPU tests lean on (tests/latent_ap_restatement.py) is held against fixture G26, recorded from
the reference, and against the high-precision evaluation of every small design of tests/latent_ap_cases.py.

Tolerances (derived, not tuned): in AP units every piece of a term is at most 1, a pair has n_{j,c} + 1 terms and a term at most about
16 roundings of 2^-53, so |ap - exact| <= (n_{j,c} + 2) 2^-49; both the reference's float64 sum and the contract's are far inside half
a float32 ulp of the exact value, so rounded to float32 they are equal or neighbours (<= 1 ulp)."""

import ctypes as C
import json
import pathlib
import re
import subprocess
import types

import numpy as np
import pytest

import latent_ap_cases as K
import latent_ap_restatement as R
from conftest import GOLDEN, ROOT

ENTRIES = ("saev_latent_ap_workspace_bytes", "saev_latent_ap_layout_of", "saev_latent_ap")
CTYPES = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double}
INVALID, UNSUPPORTED = -1, -3


def _lib():
    subprocess.run(["make", "-C", str(ROOT)], check=True, capture_output=True)
    from saev_amd import _lib

    return _lib, _lib.load()


def _golden():
    with np.load(GOLDEN / "g26_latent_ap.npz") as z:
        return {k: z[k] for k in z.files}


def _ctype(decl: str, lib_mod):
    decl = decl.replace("const", "").strip()
    if "saev_latent_ap_layout" in decl:
        return C.POINTER(lib_mod.SaevLatentAPLayout)
    if "*" in decl:
        return C.c_void_p
    return CTYPES[decl.split()[0]]


def test_entries_are_declared_exported_and_bound_with_the_headers_types():
    lib_mod, lib = _lib()
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "saev_amd.h").read_text(), flags=re.S)
    for name in ENTRIES:
        m = re.search(r"(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, f"{name} is not declared"
        args = [_ctype(re.sub(r"\w+\s*$", "", a.strip()), lib_mod) for a in m.group(2).split(",")]
        want_res, want_args = lib_mod._SIGNATURES[name]
        assert want_res is CTYPES[m.group(1)], name
        assert list(want_args) == args, name
        assert hasattr(lib, name) and name in lib_mod.EXPORTED_SYMBOLS
    assert lib.saev_abi_version() == 12 and lib_mod.ABI_VERSION == 12  # additive entries: the version stays
    for name in ("SAEV_LATENT_AP_ERR_CLASS 1", "SAEV_LATENT_AP_ERR_LATENT 2"):
        assert re.search(r"#define\s+" + name.replace(" ", r"\s+") + r"\b", text)


def test_layout_mirror_matches_the_header(tmp_path):
    lib_mod, _ = _lib()
    cls = lib_mod.SaevLatentAPLayout
    fields = [f for f, _ in cls._fields_]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "saev_amd.h"', "int main(void) {", 'printf("size %zu\\n", sizeof(saev_latent_ap_layout));']
    src += [f'printf("{f} %zu\\n", offsetof(saev_latent_ap_layout, {f}));' for f in fields]
    src.append("return 0; }")
    (tmp_path / "layout.c").write_text("\n".join(src))
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True)
    want = dict(line.split() for line in subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.splitlines())
    assert C.sizeof(cls) == int(want["size"])
    for f in fields:
        assert getattr(cls, f).offset == int(want[f]), f


def test_workspace_and_layout():
    lib_mod, lib = _lib()
    for shape in [(1, 1, 1, 0), (1, 1, 1, 1), (600, 24, 9, 4682), (5000, 1031, 64, 40000), (1 << 20, 16384, 150, 1 << 25), (300, 1 << 24, 4096, 77)]:
        L = lib_mod.SaevLatentAPLayout()
        assert lib.saev_latent_ap_layout_of(*shape, C.byref(L)) == 0
        n, s, c, nnz = shape
        assert L.struct_size == C.sizeof(L)
        assert L.total_bytes == lib.saev_latent_ap_workspace_bytes(*shape) and L.total_bytes % 256 == 0
        assert L.direct_max == K.DIRECT_MAX == R.DIRECT_MAX
        assert L.passes == 4 + (1 if s < 256 else 2 if s < 65536 else 3 if s < (1 << 24) else 4)
        assert 1 <= L.parts and L.parts * L.part_len >= nnz and L.part_len % 64 == 0
        offs = sorted((getattr(L, f), f) for f, _ in lib_mod.SaevLatentAPLayout._fields_ if f.startswith("off_"))
        assert all(o % 256 == 0 for o, _ in offs) and len({o for o, _ in offs}) == len(offs)
        sizes = {"off_err": 4, "off_starts": 8 * (s + 1), "off_hist": 4 * 256 * (L.parts + 1), **{f"off_{k}{i}": 4 * nnz for k in ("key", "latent", "row") for i in ("", "2")}}
        for (o, f), (o_next, _) in zip(offs, offs[1:] + [(L.total_bytes, "")]):
            assert o_next - o >= sizes[f], f
        # sized by nnz and S alone: neither N nor C moves it
        assert lib.saev_latent_ap_workspace_bytes(max(n // 2, 1), s, 1, nnz) == L.total_bytes
    # the bench shape: 24 bytes per stored entry -- an nnz x C array would be 2^25 x 150 x 8 bytes = 40 GB, N x S of fp32 64 GB
    assert lib.saev_latent_ap_workspace_bytes(1 << 20, 16384, 150, 1 << 25) < 2**30
    for bad in [(0, 4, 4, 0), (4, 0, 4, 0), (4, 4, 0, 0), (4, 4, 4097, 0), (1 << 31, 4, 4, 0), (4, 1 << 31, 4, 0), (4, 4, 4, 1 << 31), (4, 4, 4, -1)]:
        assert lib.saev_latent_ap_workspace_bytes(*bad) == -1, bad
        assert lib.saev_latent_ap_layout_of(*bad, C.byref(lib_mod.SaevLatentAPLayout())) == UNSUPPORTED
        assert b"saev_latent_ap_layout_of" in lib.saev_last_error(None)
    assert lib.saev_latent_ap_workspace_bytes(4, 4, 4096, 4) > 0 and lib.saev_latent_ap_workspace_bytes((1 << 31) - 1, (1 << 31) - 1, 1, 0) > 0


def _fake(i):
    return C.c_void_p((1 << 21) + 4096 * i)


SHAPE = dict(N=100, S=64, C=11, nnz=800)
# the fake device pointers are never dereferenced: a launch on them would fault, and this machine has no device to launch on
BAD = [
    ("negative_n", dict(N=-1), INVALID), ("zero_rows", dict(N=0), INVALID), ("zero_latents", dict(S=0), INVALID),
    ("rows_2_31", dict(N=1 << 31), UNSUPPORTED), ("nnz_2_31", dict(nnz=1 << 31), UNSUPPORTED), ("latents_2_31", dict(S=1 << 31), UNSUPPORTED),
    ("no_classes", dict(C=0), UNSUPPORTED), ("too_many_classes", dict(C=4097), UNSUPPORTED),
    ("null_row_ptr", dict(row_ptr=None), INVALID), ("null_indices", dict(indices=None), INVALID), ("null_data", dict(data=None), INVALID),
    ("no_label_form", dict(u8=None), INVALID), ("both_label_forms", dict(i32=_fake(8)), INVALID), ("remap_without_bytes", dict(u8=None, i32=_fake(8), remap=_fake(9)), INVALID),
    ("null_ap", dict(ap=None), INVALID), ("null_pos", dict(pos=None), INVALID),
    ("workspace_null", dict(ws=None), INVALID), ("workspace_too_small", dict(ws_short=1), INVALID),
    ("workspace_misaligned", dict(ws=C.c_void_p((1 << 20) + 8)), INVALID),
]


def _call(lib, over):
    a = dict(SHAPE, row_ptr=_fake(0), indices=_fake(1), data=_fake(2), u8=_fake(3), remap=None, i32=None, ap=_fake(4), pos=_fake(5), best_ap=_fake(6),
             best_class=_fake(7), ws=C.c_void_p(1 << 20), ws_short=0)
    a.update(over)
    need = lib.saev_latent_ap_workspace_bytes(100, 64, 11, 800)
    return lib.saev_latent_ap(a["row_ptr"], a["indices"], a["data"], a["nnz"], a["N"], a["S"], a["C"], a["u8"], a["remap"], a["i32"], a["ap"], a["pos"],
                              a["best_ap"], a["best_class"], a["ws"], need - a["ws_short"], None)


@pytest.mark.parametrize("case", BAD, ids=[c[0] for c in BAD])
def test_the_call_refuses_bad_arguments_without_a_device(case):
    _, lib = _lib()
    _, over, status = case
    rc = _call(lib, over)
    assert rc == status, (rc, lib.saev_last_error(None))
    assert lib.saev_last_error(None).startswith(b"saev_latent_ap:")


# status and saev_last_error(NULL) of the refusals this entry shares with saev_probe_ap and the saev_probe1d_* entries, word for word as
# the library gave them when every entry made these checks itself; the last three are the FIRST refusal of two bad arguments at once
EXACT = [
    ("negative_n", dict(N=-1), INVALID, "negative size"),
    ("latents_2_31", dict(S=1 << 31), UNSUPPORTED, "N, S and nnz must stay below 2^31"),
    ("zero_rows", dict(N=0), INVALID, "N and S must be at least 1"),
    ("too_many_classes", dict(C=4097), UNSUPPORTED, "the number of classes must lie in [1, 4096]"),
    ("null_row_ptr", dict(row_ptr=None), INVALID, "row_ptr is NULL"),
    ("null_data", dict(data=None), INVALID, "indices and data come with nnz > 0"),
    ("both_label_forms", dict(i32=_fake(8)), INVALID, "give the classes as class_u8 (with an optional remap) or as class_i32, one of the two"),
    ("remap_without_bytes", dict(u8=None, i32=_fake(8), remap=_fake(9)), INVALID, "remap goes with class_u8"),
    ("null_ap", dict(ap=None), INVALID, "ap and pos must not be NULL"),
    ("workspace_null", dict(ws=None), INVALID, "workspace smaller than saev_latent_ap_workspace_bytes(N, S, C, nnz)"),
    ("workspace_too_small", dict(ws_short=1), INVALID, "workspace smaller than saev_latent_ap_workspace_bytes(N, S, C, nnz)"),
    ("workspace_misaligned", dict(ws=C.c_void_p((1 << 20) + 8)), INVALID, "workspace must be 256-byte aligned"),
    ("size_before_pointers", dict(C=4097, row_ptr=None, ws=None), UNSUPPORTED, "the number of classes must lie in [1, 4096]"),
    ("labels_before_outputs", dict(i32=_fake(8), ap=None), INVALID, "give the classes as class_u8 (with an optional remap) or as class_i32, one of the two"),
    ("outputs_before_workspace", dict(pos=None, ws_short=1), INVALID, "ap and pos must not be NULL"),
]


@pytest.mark.parametrize("case", EXACT, ids=[c[0] for c in EXACT])
def test_shared_refusals_keep_their_status_and_their_text(case):
    _, lib = _lib()
    _, over, status, text = case
    assert _call(lib, over) == status
    assert lib.saev_last_error(None).decode() == "saev_latent_ap: " + text


def test_python_surface_refuses_host_tensors_and_bad_labels():
    import torch
    from saev_amd import classification, engine

    z = torch.zeros(2, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU path"):
        engine.latent_ap(z, torch.zeros(0, dtype=torch.int32), torch.zeros(0), 1, 1, 1, labels=torch.zeros(1, dtype=torch.int32))
    with pytest.raises(ValueError, match="n_classes"):
        engine.latent_ap(z, torch.zeros(0, dtype=torch.int32), torch.zeros(0), 1, 1, 4097, labels=torch.zeros(1, dtype=torch.int32))
    y = np.eye(3, dtype=np.float32)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU path"):
            classification.compute_ap_for_latent(np.arange(3, dtype=np.float32), y, y.sum(axis=0))
    y[0, 1] = 1.0
    with pytest.raises(ValueError, match="at most one 1"):
        classification.compute_ap_batched(np.zeros((3, 2), dtype=np.float32), y, y.sum(axis=0))


# ---------------------------------------------------------------- the restatement ---------------------------------------------------------

def test_restatement_against_the_references_recorded_values():
    g = _golden()
    n, s, c = int(g["n_rows"]), int(g["n_latents"]), int(g["n_classes"])
    assert (n, s, c) == (600, 24, 9) and (GOLDEN / "g26_latent_ap.npz").stat().st_size < 40_000  # within the size of the G23 files
    ap, pos, n_ev = R.latent_ap(g["indptr"], g["indices"], g["data"], n, s, g["labels"], c)
    assert g["ref_ap"].dtype == np.float32 and g["ref_ap"].shape == (s, c)
    assert R.ulps32(ap.astype(np.float32), g["ref_ap"]).max() <= 1
    assert (np.abs(ap - g["exact_ap"]) <= R.bound(n_ev)).all() and (n_ev == g["n_events"]).all()
    # the design holds what it is said to hold
    assert pos[c - 1] == 0 and (ap[:, c - 1] == 0).all() and 0.05 < (g["labels"] < 0).mean() < 0.15
    starts, _, val, _ = R.sorted_events(g["indptr"], g["indices"], g["data"], s)
    m = np.diff(starts)
    assert m.min() >= 1 and m[0] == 1 and m[1] == n == m[2]
    assert len(np.unique(val[starts[1]:starts[2]])) == n and len(np.unique(val[starts[2]:starts[3]])) == 1
    stored_zeros = g["data"][g["data"] == 0]
    assert len(stored_zeros) == 2 and np.signbit(stored_zeros).sum() == 1 and m.sum() == len(g["data"]) - 2
    assert any((val[starts[j]:starts[j + 1]] < 0).any() for j in range(s))


def test_without_ties_the_tie_aware_value_is_the_references_batched_value():
    g = _golden()
    j = int(g["no_ties_latent"])
    ap, _, _ = R.latent_ap(g["indptr"], g["indices"], g["data"], int(g["n_rows"]), int(g["n_latents"]), g["labels"], int(g["n_classes"]))
    assert R.ulps32(ap[j].astype(np.float32), g["ref_batched_row"]).max() <= 1


@pytest.mark.parametrize("name", list(K.SMALL))
def test_restatement_against_the_exact_evaluation(name):
    d = K.SMALL[name]()
    args = (d["indptr"], d["indices"], d["data"], d["n"], d["s"], d["cls"], d["c"])
    ap, pos, n_ev = R.latent_ap(*args)
    exact, pos_x, n_ev_x = R.exact_ap(*args)
    assert (pos == pos_x).all() and (n_ev == n_ev_x).all() and (pos == np.bincount(d["cls"][d["cls"] >= 0], minlength=d["c"])).all()
    miss = np.abs(ap - exact) / R.bound(n_ev)
    print(f"{name}: largest |restatement - exact| / bound = {miss.max():.3g}")
    assert (miss <= 1.0).all()
    assert ((ap >= 0) & (ap <= 1 + 2.0 ** -40)).all()


def test_harmonic_differences_are_accurate_relative_to_themselves():
    import decimal

    ctx = decimal.Context(prec=60)
    cases = [(t, n) for t in (0, 1, 5, 31, 32, 33, 63, 64, 1000, 65_000, 4_000_000) for n in (1, 3, 9, 31, 32, 33, 1000, 70_000)]
    worst = 0.0
    for t, n in cases:
        exact = sum((ctx.divide(1, decimal.Decimal(p)) for p in range(t + 1, t + n + 1)), decimal.Decimal(0))
        got = decimal.Decimal(R.dh(t, n))
        worst = max(worst, float(abs(got - exact) / exact) / 2.0 ** -53)
    print(f"largest relative error of H(t+n) - H(t): {worst:.3g} x 2^-53")
    assert worst <= 4.0  # "a few ulps relative to the difference itself"


def test_design_tables_hold_what_they_are_said_to_hold():
    d = K.tie_groups(K.DIRECT_MAX + 1)
    starts, lat, val, rows = R.sorted_events(d["indptr"], d["indices"], d["data"], d["s"])
    assert d["s"] == len(K.GROUP_T) * 2 * 5
    seen = set()
    for j in range(d["s"]):
        v = val[starts[j]:starts[j + 1]]
        size = int((np.abs(v) == 0.5).sum())
        assert size == K.DIRECT_MAX + 1
        neg = bool((v == -0.5).any())
        t = int((v > 0.5).sum()) + (d["n"] - len(v) if neg else 0)
        seen.add((t, neg))
    assert seen == {(t if t != "last" else d["n"] - K.DIRECT_MAX - 1, neg) for t in K.GROUP_T for neg in (False, True)}
    z = K.zero_groups()
    assert sorted(set((z["n"] - np.diff(R.sorted_events(z["indptr"], z["indices"], z["data"], z["s"])[0])).tolist())) == \
        [0, 1, K.DIRECT_MAX - 1, K.DIRECT_MAX + 1, z["n"] - 1]
    v = K.value_images()
    keys = R.value_key(v["data"][v["data"] != 0])
    assert all(len(np.unique((keys >> s) & 255)) > 100 for s in (0, 8, 16, 24)) and np.isinf(v["data"]).sum() >= 2
    assert ((np.abs(v["data"]) < 1e-38) & (v["data"] != 0)).sum() >= 10


# ---------------------------------------------------------------- the Python module -------------------------------------------------------

def test_eval_config_defaults_are_the_references():
    from saev_amd import classification

    want = json.loads(str(_golden()["eval_config_defaults"]))
    cfg = classification.EvalConfig()
    got = {}
    for f in __import__("dataclasses").fields(cfg):
        v = getattr(cfg, f.name)
        got[f.name] = str(v) if isinstance(v, pathlib.PurePath) else [str(x) if isinstance(x, pathlib.PurePath) else x for x in v] if isinstance(v, tuple) else v
    assert got == want


def test_feature_ranking_and_yield_arithmetic_on_hand_made_arrays(tmp_path):
    import logging
    import pickle

    from saev_amd import classification as cl

    linear = types.SimpleNamespace(coef_=np.array([[0.0, -2.0, 1.0, 0.0, 1.0], [0.5, 1.0, -2.0, 0.0, 0.0]]))
    ranked, imp = cl.extract_feature_ranking(linear, "sparse-linear")
    assert imp.tolist() == [0.5, 3.0, 3.0, 0.0, 1.0] and ranked.tolist() == [1, 2, 4, 0, 3]  # the tie 1, 2 keeps its order
    tree = types.SimpleNamespace(feature_importances_=np.array([0.1, 0.0, 0.6, 0.3, 0.0]))
    ranked_t, _ = cl.extract_feature_ranking(tree, "decision-tree")
    assert ranked_t.tolist() == [2, 3, 0, 1, 4]
    with pytest.raises(ValueError, match="Unknown classifier type"):
        cl.extract_feature_ranking(tree, "forest")

    best = np.array([0.31, 0.30, np.nan, 0.1, 0.9], dtype=np.float32)
    y, auc = cl.yield_at_budgets(ranked, best, (1, 2, 4), 0.3)
    # ranked = 1, 2, 4, 0: float32(0.30) = 0.3000000119 >= 0.3 is grounded, the NaN (outside the union) is not, 0.9 and 0.31 are
    want = {1: 1 / 1, 2: 1 / 2, 4: 3 / 4}
    assert y == want and auc == (1 / 1 + 1 / 2 + 3 / 4) / 3

    path = tmp_path / "cls.pkl"
    with open(path, "wb") as fd:
        fd.write(json.dumps({"cfg": {"cls": {"key": "decision-tree"}}}).encode() + b"\n")
        pickle.dump({"classifier": types.SimpleNamespace(feature_importances_=tree.feature_importances_)}, fd)
    _, cls_type, ranked_l, imp_l = cl.load_classifier_checkpoint(path, logging.getLogger("t"))
    assert cls_type == "decision-tree" and ranked_l.tolist() == [2, 3, 0, 1, 4] and imp_l.tolist() == tree.feature_importances_.tolist()
    src = (ROOT / "saev_amd" / "classification.py").read_text()
    assert not re.search(r"^\s*(import|from)\s+(sklearn|cloudpickle)", src, flags=re.M)
