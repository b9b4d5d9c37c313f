"""CPU-only tests of the latent operating points (include/saev_amd.h: LATENT OPERATING POINTS): the entry is declared,
exported and bound with the header's types and sizes its workspace as LATENT AUROC does; every argument check refuses a call before
anything touches a device, in the header's order; the numpy restatement the GPU tests lean on
(tests/latent_operating_restatement.py) equals the definition -- every subset of the rows as the predicted set -- on tiny inputs and
``sklearn.metrics.roc_curve`` on random ones; every design of tests/latent_operating_cases.py holds what it is said to hold; and the
parts of ``saev_amd.operating`` that need no device (``thresholds``, ``scorecard``, the file's keys) do what they say.

Everything is compared on integers, ``fractions.Fraction`` or float bits: there is no tolerance in this file."""

import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import latent_operating_cases as OK
import latent_operating_restatement as OR
from conftest import ROOT

CTYPES = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double}
INVALID, UNSUPPORTED = -1, -3


def _lib():
    subprocess.run(["make", "-C", str(ROOT)], check=True, capture_output=True)
    from saev_amd import _lib

    return _lib, _lib.load()


def _restate(d):
    return OR.operating(d["indptr"], d["indices"], d["data"], d["n"], d["s"], d["cls"], d["roles"])


def _dense(d):
    dense = np.zeros((d["n"], d["s"]), dtype=np.float32)
    rows = np.repeat(np.arange(d["n"]), np.diff(d["indptr"]))
    dense[rows, d["indices"]] = d["data"]
    return dense + np.float32(0)


# ---------------------------------------------------------------- the ABI ----------------------------------------------------------------

def test_the_entry_is_declared_exported_and_bound_with_the_headers_types():
    lib_mod, lib = _lib()
    raw = (ROOT / "include" / "saev_amd.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name, n_args in (("saev_latent_operating", 28), ("saev_latent_operating_workspace_bytes", 5)):
        m = re.search(r"(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, f"{name} is not declared"
        args = []
        for a in m.group(2).split(","):
            decl = re.sub(r"\w+\s*$", "", a.strip()).replace("const", "").strip()
            args.append(C.c_void_p if "*" in decl else CTYPES[decl.split()[0]])
        want_res, want_args = lib_mod._SIGNATURES[name]
        assert want_res is CTYPES[m.group(1)] and list(want_args) == args and len(args) == n_args
        assert hasattr(lib, name) and name in lib_mod.EXPORTED_SYMBOLS
    assert lib.saev_abi_version() == 12 and lib_mod.ABI_VERSION == 12  # an additive entry: the version stays
    assert re.search(r"#define\s+SAEV_OPERATING_SORTED\s+1\b", text) and lib_mod.OPERATING_SORTED == 1
    assert "LATENT OPERATING POINTS" in raw and "DESIGN.md 3.29" in raw


def test_workspace_is_latent_aurocs():
    _, lib = _lib()
    for shape in ((100, 64, 11, 7, 800), (1, 1, 1, 1, 0), (70_000, 48, 5, 3, 2_240_000), (300, 5, 4096, 4096, 600), (300, 5, 300, 65, 600)):
        assert lib.saev_latent_operating_workspace_bytes(*shape) == lib.saev_latent_auroc_workspace_bytes(*shape) > 0
    for bad in ((0, 64, 11, 7, 800), (100, 64, 4097, 7, 800), (100, 64, 11, 0, 800), (100, 64, 11, 4097, 800), (100, 64, 11, 7, 1 << 31)):
        assert lib.saev_latent_operating_workspace_bytes(*bad) == -1


def _fake(i):
    return C.c_void_p((1 << 21) + 4096 * i)


SHAPE = dict(N=100, S=64, C=11, T=7, nnz=800, flags=0)
PAIRS = ("f1", "f1_thr", "f1_tp", "f1_fp", "j2", "youden", "j_thr", "j_tp", "j_fp")
COUNTS = ("n_pos", "n_neg", "pos")
SHARED = "give the classes as class_u8 (with an optional remap) or as class_i32, one of the two"
NULL_OUT = "f1, f1_thr, f1_tp, f1_fp, j2, youden, j_thr, j_tp and j_fp must not be NULL"
NULL_COUNTS = "n_pos, n_neg and pos must not be NULL"
NULL_INPUTS = "with SAEV_OPERATING_SORTED n_pos, n_neg and pos are inputs and must not be NULL"
BAD_FLAG = "flags holds a bit other than SAEV_OPERATING_SORTED"
TOO_SMALL = "workspace smaller than saev_latent_operating_workspace_bytes(N, S, C, T, nnz)"
# the fake device pointers are never dereferenced: a launch on them would fault, and this machine has no device to launch on.  Status
# and saev_last_error(NULL) word for word; the refusals shared with saev_latent_auroc where they sit there, this entry's own among them,
# with the flag set and without it, and the FIRST refusal of two bad arguments at once
BAD = [
    ("negative_n", dict(N=-1), INVALID, "negative size"), ("zero_latents", dict(S=0), INVALID, "N and S must be at least 1"),
    ("nnz_2_31", dict(nnz=1 << 31), UNSUPPORTED, "N, S and nnz must stay below 2^31"),
    ("too_many_classes", dict(C=4097), UNSUPPORTED, "the number of classes must lie in [1, 4096]"),
    ("no_tasks", dict(T=0), UNSUPPORTED, "the number of tasks must lie in [1, 4096]"),
    ("too_many_tasks", dict(T=4097), UNSUPPORTED, "the number of tasks must lie in [1, 4096]"),
    ("too_many_tasks_sorted", dict(T=4097, flags=1), UNSUPPORTED, "the number of tasks must lie in [1, 4096]"),
    ("null_row_ptr", dict(row_ptr=None), INVALID, "row_ptr is NULL"), ("null_data", dict(data=None), INVALID, "indices and data come with nnz > 0"),
    ("no_label_form", dict(u8=None), INVALID, SHARED), ("both_label_forms", dict(i32=_fake(8)), INVALID, SHARED),
    ("no_label_form_sorted", dict(u8=None, flags=1), INVALID, SHARED),
    ("remap_without_bytes", dict(u8=None, i32=_fake(8), remap=_fake(9)), INVALID, "remap goes with class_u8"),
    ("null_role", dict(role=None), INVALID, "role must not be NULL"),
    *[(f"null_{name}", {name: None}, INVALID, NULL_OUT) for name in PAIRS],
    ("unknown_flag_bit", dict(flags=2), INVALID, BAD_FLAG), ("unknown_flag_bit_beside_the_known", dict(flags=5), INVALID, BAD_FLAG),
    ("negative_flags", dict(flags=-1), INVALID, BAD_FLAG),
    *[(f"null_{name}", {name: None}, INVALID, NULL_COUNTS) for name in COUNTS],
    *[(f"sorted_with_null_{name}", {name: None, "flags": 1}, INVALID, NULL_INPUTS) for name in COUNTS],
    ("workspace_null", dict(ws=None), INVALID, TOO_SMALL), ("workspace_too_small", dict(ws_short=1), INVALID, TOO_SMALL),
    ("workspace_too_small_sorted", dict(ws_short=1, flags=1), INVALID, TOO_SMALL),
    ("workspace_of_latent_ap", dict(ws_latent_ap=True), INVALID, TOO_SMALL),
    ("workspace_misaligned", dict(ws=C.c_void_p((1 << 20) + 8)), INVALID, "workspace must be 256-byte aligned"),
    ("workspace_misaligned_sorted", dict(ws=C.c_void_p((1 << 20) + 8), flags=1), INVALID, "workspace must be 256-byte aligned"),
    ("classes_before_tasks", dict(C=4097, T=4097), UNSUPPORTED, "the number of classes must lie in [1, 4096]"),
    ("tasks_before_pointers", dict(T=4097, row_ptr=None), UNSUPPORTED, "the number of tasks must lie in [1, 4096]"),
    ("labels_before_role", dict(u8=None, role=None), INVALID, SHARED),
    ("role_before_outputs", dict(role=None, j2=None), INVALID, "role must not be NULL"),
    ("outputs_before_flags", dict(j_fp=None, flags=2), INVALID, NULL_OUT),
    ("flags_before_counts", dict(flags=3, n_pos=None), INVALID, BAD_FLAG),
    ("counts_before_workspace", dict(pos=None, ws_short=1), INVALID, NULL_COUNTS),
    ("size_before_alignment", dict(ws=C.c_void_p((1 << 20) + 8), ws_short=1), INVALID, TOO_SMALL),
]


def _call(lib, over):
    a = dict(SHAPE, row_ptr=_fake(0), indices=_fake(1), data=_fake(2), u8=_fake(3), remap=None, i32=None, role=_fake(10), ws=C.c_void_p(1 << 20), ws_short=0,
             ws_latent_ap=False, **{name: _fake(20 + i) for i, name in enumerate(PAIRS + COUNTS)})
    a.update(over)
    need = lib.saev_latent_operating_workspace_bytes(100, 64, 11, 7, 800)
    if a["ws_latent_ap"]:
        need = lib.saev_latent_ap_workspace_bytes(100, 64, 11, 800)
    return lib.saev_latent_operating(a["row_ptr"], a["indices"], a["data"], a["nnz"], a["N"], a["S"], a["C"], a["u8"], a["remap"], a["i32"], a["role"], a["T"],
                                     a["flags"], *[a[name] for name in PAIRS + COUNTS], a["ws"], need - a["ws_short"], None)


@pytest.mark.parametrize("case", BAD, ids=[c[0] for c in BAD])
def test_the_call_refuses_bad_arguments_without_a_device_in_order(case):
    _, lib = _lib()
    _, over, status, text = case
    rc = _call(lib, over)
    assert rc == status, (rc, lib.saev_last_error(None))
    assert lib.saev_last_error(None).decode() == "saev_latent_operating: " + text


def test_python_surface_refuses_host_tensors_and_bad_arguments():
    import torch
    from saev_amd import _lib as lib_mod
    from saev_amd import engine

    z, i, v = torch.zeros(2, dtype=torch.int64), torch.zeros(0, dtype=torch.int32), torch.zeros(0)
    lab, roles = torch.zeros(1, dtype=torch.int32), torch.ones(1, 1, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        engine.latent_operating(z, i, v, 1, 1, 1, labels=lab, roles=roles)
    with pytest.raises(ValueError, match="n_classes"):
        engine.latent_operating(z, i, v, 1, 1, 4097, labels=lab, roles=roles)
    with pytest.raises(ValueError, match="roles must be"):
        engine.latent_operating(z, i, v, 1, 1, 1, labels=lab, roles=roles.to(torch.int32))
    with pytest.raises(ValueError, match="n_tasks"):
        engine.latent_operating(z, i, v, 1, 1, 1, labels=lab, roles=torch.ones(4097, 1, dtype=torch.uint8))
    assert engine.LatentOperatingResult._ERRORS == engine.LatentAUROCResult._ERRORS and engine.LatentOperatingResult._WHO == "latent_operating"
    assert engine.LatentOperatingResult.PAIRS == PAIRS
    # reuse= is checked against the call's shapes before any device work: here there is no device, and the mismatch is what is reported
    with pytest.raises(ValueError, match="reuse takes"):
        engine.latent_operating(z, i, v, 1, 1, 1, labels=lab, roles=roles, reuse=object())
    layout = lib_mod.SaevLatentAPLayout()
    for shape, n_tasks in (((2, 1, 1, 0), 1), ((1, 2, 1, 0), 1), ((1, 1, 2, 0), 1), ((1, 1, 1, 3), 1), ((1, 1, 1, 0), 2)):
        out = dict(n_pos=torch.zeros(n_tasks, dtype=torch.int64))
        for cls in (engine.LatentAUROCResult, engine.LatentOperatingResult):
            with pytest.raises(ValueError, match="the result to reuse has"):
                engine.latent_operating(z, i, v, 1, 1, 1, labels=lab, roles=roles, reuse=cls(out, torch.zeros(256, dtype=torch.uint8), layout, shape))
    same = engine.LatentAUROCResult(dict(n_pos=torch.zeros(1, dtype=torch.int64)), torch.zeros(256, dtype=torch.uint8), layout, (1, 1, 1, 0))
    with pytest.raises(RuntimeError, match="no CPU path"):  # the shapes agree: the call goes on to the device it does not have
        engine.latent_operating(z, i, v, 1, 1, 1, labels=lab, roles=roles, reuse=same)


# ---------------------------------------------------------------- the restatement ---------------------------------------------------------

def _random_pair(rng, n, signed=True, both=True):
    levels = rng.integers(2, 6)
    values = (rng.integers(-levels if signed else 0, levels + 1, size=n) / 2).astype(np.float32)
    values[rng.random(n) < 0.3] = 0  # a zero block
    is_pos = rng.random(n) < rng.uniform(0.2, 0.8)
    if both:
        is_pos[0], is_pos[1] = True, False
    return values, is_pos


def test_restatement_against_every_subset_as_the_predicted_set():
    rng = np.random.default_rng(0)
    seen_tie = 0
    for trial in range(120):
        n = int(rng.integers(1, 10))
        values, is_pos = _random_pair(rng, n, both=False)
        n_pos, n_neg = int(is_pos.sum()), int((~is_pos).sum())
        got = OR.best_points(values, is_pos, n_pos, n_neg)
        want = OR.by_subsets(values, is_pos)
        assert got == want, (values, is_pos, got, want)
        seen_tie += got[0][2] != got[1][3]
    assert seen_tie > 10  # the two objectives do not always agree: both are exercised


def test_restatement_against_sklearns_roc_curve():
    pytest.importorskip("sklearn")
    rng = np.random.default_rng(1)
    for trial in range(300):
        n = int(rng.integers(2, 60))
        values, is_pos = _random_pair(rng, n, signed=trial % 3 > 0)
        got = OR.best_points(values, is_pos, int(is_pos.sum()), int((~is_pos).sum()))
        assert got == OR.by_roc_curve(values, is_pos), (values, is_pos)


def test_outputs_are_formed_with_the_contracts_expressions():
    d = OK.SMALL["kinds"]()
    w = _restate(d)
    for j in range(d["s"]):
        for t in range(d["roles"].shape[0]):
            tp, fp, n_pos, n_neg = int(w["f1_tp"][j, t]), int(w["f1_fp"][j, t]), int(w["n_pos"][t]), int(w["n_neg"][t])
            if n_pos == 0:
                assert np.isnan(w["f1"][j, t]) and tp == 0 and w["f1_thr"][j, t] == np.inf
            else:
                assert w["f1"][j, t] == (2.0 * tp) / float(tp + fp + n_pos)
            assert w["j2"][j, t] == int(w["j_tp"][j, t]) * n_neg - int(w["j_fp"][j, t]) * n_pos >= 0
            if n_pos == 0 or n_neg == 0:
                assert np.isnan(w["youden"][j, t]) and w["j2"][j, t] == 0 and w["j_thr"][j, t] == np.inf
            else:
                assert w["youden"][j, t] == float(w["j2"][j, t]) / (float(n_pos) * float(n_neg))
    assert w["f1"].dtype == np.float64 and w["f1_thr"].dtype == np.float32 and w["j2"].dtype == np.int64


# ---------------------------------------------------------------- the designs ------------------------------------------------------------

def test_planted_ties_go_to_the_higher_threshold():
    d = OK.planted()
    w = _restate(d)
    assert w["n_pos"].tolist() == [2, 3, 2] and w["n_neg"].tolist() == [2, 2, 2]
    for j, (name, (_, which, (tp, fp, thr))) in enumerate(OK.PLANTED.items()):
        if which in ("f1", "both"):
            assert (w["f1_tp"][j, 0], w["f1_fp"][j, 0], w["f1_thr"][j, 0]) == (tp, fp, thr), name
        if which in ("j", "both"):
            assert (w["j_tp"][j, 0], w["j_fp"][j, 0], w["j_thr"][j, 0]) == (tp, fp, thr), name
        for key in OR.PAIRS_INT + OR.PAIRS_F32:
            assert w[key][j, 0] == w[key][j, 2]  # the same task twice
    # the ties are ties: the loser's score equals the winner's, as fractions
    dense, role = _dense(d), np.array([2, 2, 1, 1, 0, 0])
    for j, (name, (_, which, (tp, fp, thr))) in enumerate(OK.PLANTED.items()):
        if which == "both":
            continue
        lower = sorted({v for v in dense[role > 0, j].tolist() if v < thr})[-1]
        tp2, fp2 = int((dense[role == 2, j] >= lower).sum()), int((dense[role == 1, j] >= lower).sum())
        if which == "f1":
            assert (tp, fp, tp2, fp2) == (1, 0, 2, 2) and tp * (tp2 + fp2 + 2) == tp2 * (tp + fp + 2), name
        else:
            assert (tp, fp, tp2, fp2) == (1, 0, 2, 1) and tp * 2 - fp * 2 == tp2 * 2 - fp2 * 2, name
    # rows outside the task sit inside the tie groups, below and above 0, and the walk's two sides are both planted
    assert (d["cls"][4], d["roles"][0, d["cls"][5]]) == (-1, 0) and (dense[4] != 0).sum() >= 6 and (dense[5] != 0).sum() >= 6
    signs = {name: (min(col.values()) < 0, max(col.values()) > 0) for name, (col, _, _) in OK.PLANTED.items()}
    assert signs["f1_down"] == signs["j_down"] == (False, True) and signs["f1_up"] == signs["j_up"] == (True, False)
    assert signs["f1_across"] == signs["j_across"] == (True, True)


def test_designs_hold_what_they_are_said_to_hold():
    w = _restate(OK.single())
    assert w["f1_thr"].tolist() == [[2.0, np.inf, np.inf], [-2.0, np.inf, np.inf], [0.0, np.inf, np.inf]] and w["f1"][:, 0].tolist() == [1.0, 1.0, 1.0]
    assert np.isnan(w["f1"][:, 1:]).all() and np.isnan(w["youden"]).all() and (w["j2"] == 0).all() and np.isinf(w["j_thr"]).all()

    d = OK.marks_negatives()
    w = _restate(d)
    dense = _dense(d)
    for j in range(2):  # every candidate but "everything" has J2 < 0 in task 0; swapped, the latent wins
        for v in np.unique(dense[:, j]):
            tp, fp = int((dense[:10, j] >= v).sum()), int((dense[10:, j] >= v).sum())
            assert tp * 10 - fp * 10 < 0 or (tp, fp) == (10, 10)
        assert (w["j2"][j, 0], w["j_tp"][j, 0], w["j_fp"][j, 0], w["j_thr"][j, 0]) == (0, 0, 0, np.inf) and w["youden"][j, 0] == 0.0
        assert w["j2"][j, 1] > 0 and np.isfinite(w["j_thr"][j, 1])
    assert (d["data"] == 0).sum() == 1 and (w["j_tp"][0, 1], w["j_fp"][0, 1], w["j_thr"][0, 1]) == (9, 0, 1.0)
    assert (w["j_tp"][1, 1], w["j_fp"][1, 1], w["j_thr"][1, 1]) == (10, 2, 0.0)  # the zero block wins: two rows of class 0 sit in it

    d = OK.zero_block_lanes()
    dense, cls = _dense(d), d["cls"]
    silent = dense[:, 0] == 0
    assert not silent[cls <= 1].any() and silent[cls >= 2].all() and (dense[:, 0] < 0).any() and (dense[:, 1] >= 0).all()
    w = _restate(d)
    # by hand: task 0 has (1, 0), (2, 1), (3, 2) at 2, 1, -1: 2/4 < 4/6 < 6/8; task 1 has its zero block alone; task 2 has (2, 0) at 1: 4/5
    assert w["f1_thr"][0].tolist() == [-1.0, 0.0, 1.0] and w["f1_tp"][0].tolist() == [3, 3, 2] and w["f1_fp"][0].tolist() == [2, 3, 0]

    d = OK.specials()
    w = _restate(d)
    assert (w["f1_thr"][0, 0], w["f1_tp"][0, 0], w["f1_fp"][0, 0], w["j_thr"][0, 0], w["j_tp"][0, 0]) == (np.inf, 2, 0, np.inf, 2)  # +Inf wins, and predicts
    assert (w["f1_thr"][1, 1], w["f1_tp"][1, 1], w["f1"][1, 1]) == (-np.inf, 4, 1.0) and np.isnan(w["youden"][:, 1]).all()   # -Inf predicts everything
    assert w["f1_thr"][1, 0] == 1.0 and w["f1_fp"][1, 0] == 0
    tiny = np.float32(1e-45)  # by hand: F1 climbs 2/5, 4/7, 6/10 (the zero block), 6/11, 8/12 down to -2 tiny; J2 ties at 4 and stays at 2 tiny
    assert tiny > 0 and tiny.view(np.uint32) == 1 and (w["f1_thr"][2, 0], w["f1_tp"][2, 0], w["f1_fp"][2, 0]) == (-2 * tiny, 4, 4)
    assert (w["j_thr"][2, 0], w["j_tp"][2, 0], w["j_fp"][2, 0], w["j2"][2, 0]) == (2 * tiny, 1, 0, 4)
    assert OK.ABOVE_ONE.view(np.uint32) - OK.ONE.view(np.uint32) == 1 and (w["f1_thr"][3, 0], w["f1_tp"][3, 0], w["f1_fp"][3, 0]) == (OK.ABOVE_ONE, 2, 0)
    assert (w["f1_thr"][4, 0], w["f1_tp"][4, 0], w["f1_fp"][4, 0]) == (-np.inf, 4, 4) and (w["j_thr"][4, 0], w["j2"][4, 0]) == (np.inf, 0)

    c = OK.SMALL["chunks"]()
    assert set(OK.AK.CHUNK_GROUPS) >= {1, 2, 63, 64, 65, 130} and np.cumsum(OK.AK.CHUNK_GROUPS)[1] == 64  # (the AUROC tests pin the rest of it)
    assert sum(OK.AK.CHUNK_GROUPS[:2]) % 8 == 0 and OK.AK.CHUNK_GROUPS[0] % 8 == 7 and c["s"] == 5
    k = _restate(OK.SMALL["kinds"]())
    assert (k["n_pos"] == 0).any() and ((k["n_neg"] == 0) & (k["n_pos"] > 0)).any()
    shapes = [OK.AK.GRID[g] for g in OK.AK.GRID]
    assert {s[3] for s in shapes} >= {1, 64, 65, 130} and {s[2] for s in shapes} >= {255, 256, 4096}

    d = OK.many_latents()
    n_events = np.bincount(d["indices"], minlength=d["s"])
    assert d["s"] == 70_001 and n_events[0] > 0 and n_events[-1] > 0 and n_events[65_536] > 0 and (n_events > 0).sum() < 300 and (d["data"] < 0).any()

    d = OK.wide_products()
    w = _restate(d)
    assert d["n"] == 150_000 and len(np.unique(d["data"][0::2])) == d["n"] and (d["data"][1::2] < 0).sum() == d["n"] // 3 and (d["data"] != 0).all()
    assert (w["j2"][:, 0] > 1 << 32).all() and (w["f1_tp"][:, 0] * (w["f1_tp"][:, 0] + w["f1_fp"][:, 0] + w["n_pos"][0]) > 1 << 32).all()
    assert (w["j2"][:, 1] == 0).all() and (w["f1_thr"][:, 1] == d["data"].reshape(-1, 2).min(axis=0)).all()  # swapped: nothing for J, everything for F1
    for key in OR.PAIRS_INT:
        assert (w[key][0] == w[key][1]).all()  # the signed copy has the same order, so the same counts

    d = OK.big_group()
    vals, counts = np.unique(d["data"], return_counts=True)
    assert counts.max() == 70_000 and vals[counts.argmax()] == 1.0 and d["n"] - len(d["data"]) == 20 and (vals < 0).sum() == 10 and (vals > 1).sum() == 20


@pytest.mark.parametrize("name", ["kinds", "chunks", "grid_5x11x130", "planted", "specials", "zero_block_lanes"])
def test_restatement_on_the_designs_against_the_definition_by_comparison(name):
    """The winners of every pair recounted from the dense column with ``a >= theta``, and no candidate strictly better than them."""
    d = OK.SMALL[name]()
    w = _restate(d)
    dense = _dense(d)
    table = np.concatenate([np.zeros((d["roles"].shape[0], 1), dtype=np.uint8), d["roles"]], axis=1)[:, d["cls"] + 1]
    for t in range(min(d["roles"].shape[0], 12)):
        pos, neg = table[t] == 2, table[t] == 1
        n_pos, n_neg = int(pos.sum()), int(neg.sum())
        for j in range(d["s"]):
            col = dense[:, j]
            for which, tp_key, fp_key in (("f1_thr", "f1_tp", "f1_fp"), ("j_thr", "j_tp", "j_fp")):
                thr = w[which][j, t]
                if thr == np.inf and w[tp_key][j, t] + w[fp_key][j, t] == 0:
                    continue  # "predict nothing": +Inf stands for no threshold at all (a row AT +Inf would meet it)
                assert (int((col[pos] >= thr).sum()), int((col[neg] >= thr).sum())) == (w[tp_key][j, t], w[fp_key][j, t])
            ftp, ffp, j2 = int(w["f1_tp"][j, t]), int(w["f1_fp"][j, t]), int(w["j2"][j, t])
            for v in np.unique(col[pos | neg]):
                tp, fp = int((col[pos] >= v).sum()), int((col[neg] >= v).sum())
                lhs, rhs = tp * (ftp + ffp + n_pos), ftp * (tp + fp + n_pos)
                assert lhs < rhs or (lhs == rhs and v <= w["f1_thr"][j, t])
                assert tp * n_neg - fp * n_pos < j2 or (tp * n_neg - fp * n_pos == j2 and v <= w["j_thr"][j, t])


# ---------------------------------------------------------------- saev_amd.operating ------------------------------------------------------

def _file_of(d, names):
    """The arrays of ``latent_operating.npz`` from the restatement of a design (what ``operating.compute`` leaves, without a device)."""
    from saev_amd import operating

    w = _restate(d)
    dense = _dense(d)
    table = np.concatenate([np.zeros((d["roles"].shape[0], 1), dtype=np.uint8), d["roles"]], axis=1)[:, d["cls"] + 1]
    z = {k: np.ascontiguousarray(w[k].T) for k in operating.PAIRS}
    z.update(n_pos=w["n_pos"], n_neg=w["n_neg"], level=np.asarray("image"), task=np.asarray(names, dtype=str),
             fire_pos=np.stack([(dense[table[t] == 2] > 0).sum(axis=0) for t in range(len(names))]).astype(np.int64),
             fire_neg=np.stack([(dense[table[t] == 1] > 0).sum(axis=0) for t in range(len(names))]).astype(np.int64),
             auroc=np.full((len(names), d["s"]), 0.5))
    assert set(z) == set(operating.KEYS)
    return z, dense, table


def test_thresholds_are_the_strict_form_the_consumers_compare_with(tmp_path):
    from saev_amd import operating

    assert operating.KEYS == ("level", "task", "n_pos", "n_neg", "f1", "f1_thr", "f1_tp", "f1_fp", "j2", "youden", "j_thr", "j_tp", "j_fp", "auroc",
                              "fire_pos", "fire_neg") and operating.NPZ_FNAME == "latent_operating.npz"
    for make, names in ((OK.SMALL["kinds"], [f"t{i}" for i in range(7)]), (OK.specials, ["a", "b"]), (OK.planted, ["p", "q", "r"])):
        d = make()
        z, dense, table = _file_of(d, names)
        np.savez(tmp_path / operating.NPZ_FNAME, **z)
        for t, name in enumerate(names):
            for which in ("f1", "j"):
                thr = operating.thresholds(tmp_path / operating.NPZ_FNAME, name, which)
                assert thr.dtype == np.float32 and thr.shape == (d["s"],) and np.array_equal(thr, operating.thresholds(z, t, which), equal_nan=True)
                theta = z[f"{which}_thr"][t]
                finite = np.isfinite(theta)
                assert (thr[finite] < theta[finite]).all() and (np.nextafter(thr[finite], np.float32(np.inf)) == theta[finite]).all()
                assert (thr[np.isposinf(theta)] == np.inf).all() and (thr[np.isneginf(theta)] == -np.inf).all()
                fires = dense > thr[None, :]  # what ClassFireCounts and coactivation_match do with it
                # (+-Inf as a winning VALUE has no strict form; +Inf as "predict nothing" has: it predicts nothing)
                ok = np.isfinite(theta) | (np.isposinf(theta) & (z[f"{which}_tp"][t] + z[f"{which}_fp"][t] == 0))
                assert np.array_equal(fires[table[t] == 2].sum(axis=0)[ok], z[f"{which}_tp"][t][ok])
                assert np.array_equal(fires[table[t] == 1].sum(axis=0)[ok], z[f"{which}_fp"][t][ok])
    assert operating.strict(np.float32(0.0)) < 0 and operating.strict(np.float32(0.0)) == -np.float32(1e-45)
    with pytest.raises(ValueError, match="which must be"):
        operating.thresholds(z, 0, "f2")
    with pytest.raises(ValueError, match="is not in the file"):
        operating.thresholds(z, "nope")


def test_scorecard_on_a_hand_made_file(tmp_path):
    from saev_amd import operating

    z = dict(level=np.asarray("image"), task=np.asarray(["a_v_vs_b_v", "c_v_vs_d_v"]), n_pos=np.array([4, 10]), n_neg=np.array([6, 0]),
             f1=np.array([[1.0, 0.5, 0.0], [0.9, np.nan, 0.8]]), f1_thr=np.array([[2.0, 0.0, np.inf], [1.0, 1.0, 1.0]], dtype=np.float32),
             f1_tp=np.array([[4, 4, 0], [9, 0, 8]]), f1_fp=np.array([[0, 6, 0], [0, 0, 2]]), j2=np.array([[24, 0, 0], [0, 0, 0]]),
             youden=np.array([[1.0, 0.0, 0.0], [np.nan] * 3]), j_thr=np.array([[2.0, np.inf, np.inf], [np.inf] * 3], dtype=np.float32),
             j_tp=np.array([[4, 0, 0], [0, 0, 0]]), j_fp=np.zeros((2, 3), dtype=np.int64), auroc=np.array([[1.0, 0.5, 0.4], [np.nan] * 3]),
             fire_pos=np.array([[4, 4, 0], [10, 0, 5]]), fire_neg=np.array([[3, 6, 0], [0, 0, 0]]))
    np.savez(tmp_path / "latent_operating.npz", **z)
    card = operating.scorecard(tmp_path / "latent_operating.npz", min_auroc=0.8, min_f1=0.8, min_consistency=0.5)
    assert card["task"].tolist() == ["a_v_vs_b_v"] * 3 + ["c_v_vs_d_v"] * 3 and card["feature_id"].tolist() == [0, 1, 2, 0, 1, 2]
    np.testing.assert_array_equal(card["precision"], [1.0, 0.4, np.nan, 1.0, np.nan, 0.8])
    np.testing.assert_array_equal(card["recall"], [1.0, 1.0, 0.0, 0.9, 0.0, 0.8])
    np.testing.assert_array_equal(card["tpr"], [1.0, 0.0, 0.0, 0.0, 0.0, 0.0])
    np.testing.assert_array_equal(card["fpr"], [0.0, 0.0, 0.0, np.nan, np.nan, np.nan])
    np.testing.assert_array_equal(card["fire_rate_pos"], [1.0, 1.0, 0.0, 1.0, 0.0, 0.5])
    np.testing.assert_array_equal(card["fire_rate_neg"], [0.5, 1.0, 0.0, np.nan, np.nan, np.nan])
    assert card["pass_discriminative"].tolist() == [True, False, False, False, False, False]
    assert card["pass_operating"].tolist() == [True, False, False, True, False, True] and card["pass_all"].tolist() == [True] + [False] * 5
    assert "pass_spatial" not in card and "position_consistency" not in card
    for key in ("f1", "f1_thr", "youden", "j_thr", "auroc"):
        np.testing.assert_array_equal(card[key], z[key].reshape(-1).astype(card[key].dtype))
    # an AUROC of one's own, and the spatial scores: the latent's largest over the groups, NaN where it fires in none
    sp = dict(position_consistency=np.array([[0.2, 0.6], [np.nan, np.nan], [0.9, np.nan]]), clustering=np.array([[1.0, 3.0], [np.nan, np.nan], [2.0, 0.5]]))
    np.savez(tmp_path / "latent_spatial.npz", **sp)
    card = operating.scorecard(z, auroc=np.full((2, 3), 0.95), spatial_file=tmp_path / "latent_spatial.npz", min_auroc=0.8, min_f1=0.8, min_consistency=0.5)
    np.testing.assert_array_equal(card["position_consistency"], [0.6, np.nan, 0.9] * 2)
    np.testing.assert_array_equal(card["clustering"], [3.0, np.nan, 2.0] * 2)
    assert card["pass_spatial"].tolist() == [True, False, True] * 2 and card["pass_all"].tolist() == [True, False, False, True, False, True]
    # the AUROC of mimics.score_run's file, task-major as it is written
    mim = dict(task=np.repeat(z["task"], 3), auroc=np.arange(6, dtype=np.float32) / 8)
    np.savez(tmp_path / "cambridge-mimics.npz", **mim)
    np.testing.assert_array_equal(operating.scorecard(z, auroc=tmp_path / "cambridge-mimics.npz")["auroc"], np.arange(6) / 8)
    with pytest.raises(ValueError, match="the AUROC file scores the tasks"):
        operating.scorecard(z, auroc=dict(mim, task=mim["task"][::-1]))
    with pytest.raises(ValueError, match="auroc must be"):
        operating.scorecard(z, auroc=np.zeros((3, 2)))
