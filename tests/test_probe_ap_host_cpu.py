"""CPU-only tests of the probe AP (include/saev_amd.h: PROBE AP): the entry is declared, exported and bound with the
header's types; every argument check refuses a call before anything touches a device; the numpy restatement the GPU tests lean on
(tests/probe_ap_restatement.py) is held against fixture G28, recorded from the reference, against the 80-digit evaluation of every
small design of tests/probe_ap_cases.py, and -- on designs of at most 7 rows -- against the definition itself: the mean of the AP
over every order of the tied rows, in rationals; and ``probe_metrics.worker_fn`` makes the reference's file checks.

Tolerances (derived, not tuned): |ap - exact| <= (n_{j,c} + 2) 2^-49 as for LATENT AP (a pair has at most n_{j,c} + 1 non-zero terms);
against the reference's float32 ``ap``: (2 N + 4) 2^-24, the bound the generator of G28 asserts for the reference itself."""

import ctypes as C
import fractions
import itertools
import re
import subprocess

import numpy as np
import pytest

import probe_ap_cases as PK
import probe_ap_restatement as PR
from conftest import GOLDEN, ROOT

CTYPES = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double}
INVALID, UNSUPPORTED = -1, -3


def _lib():
    subprocess.run(["make", "-C", str(ROOT)], check=True, capture_output=True)
    from saev_amd import _lib

    return _lib, _lib.load()


def _golden():
    with np.load(GOLDEN / "g28_probe_metrics.npz") as z:
        return {k: z[k] for k in z.files}


def _args(d, dtype):
    return (d["indptr"], d["indices"], d["data"], d["n"], d["s"], d["cls"], d["c"], d["w"].astype(dtype), d["b"].astype(dtype))


def test_the_entry_is_declared_exported_and_bound_with_the_headers_types():
    lib_mod, lib = _lib()
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "saev_amd.h").read_text(), flags=re.S)
    m = re.search(r"(\w+)\s+saev_probe_ap\s*\(([^)]*)\)\s*;", text)
    assert m, "saev_probe_ap is not declared"
    args = []
    for a in m.group(2).split(","):
        decl = re.sub(r"\w+\s*$", "", a.strip()).replace("const", "").strip()
        args.append(C.c_void_p if "*" in decl else CTYPES[decl.split()[0]])
    want_res, want_args = lib_mod._SIGNATURES["saev_probe_ap"]
    assert want_res is CTYPES[m.group(1)] and list(want_args) == args and len(args) == 22
    assert hasattr(lib, "saev_probe_ap") and "saev_probe_ap" in lib_mod.EXPORTED_SYMBOLS
    assert lib.saev_abi_version() == 12 and lib_mod.ABI_VERSION == 12  # an additive entry: the version stays
    assert re.search(r"#define\s+SAEV_PROBE_AP_ERR_VALUE\s+3\b", text)
    assert "PROBE AP" in (ROOT / "include" / "saev_amd.h").read_text()


def _fake(i):
    return C.c_void_p((1 << 21) + 4096 * i)


SHAPE = dict(N=100, S=64, C=11, nnz=800)
# the fake device pointers are never dereferenced: a launch on them would fault, and this machine has no device to launch on
BAD = [
    ("negative_n", dict(N=-1), INVALID), ("zero_rows", dict(N=0), INVALID), ("zero_latents", dict(S=0), INVALID),
    ("rows_2_31", dict(N=1 << 31), UNSUPPORTED), ("nnz_2_31", dict(nnz=1 << 31), UNSUPPORTED), ("no_classes", dict(C=0), UNSUPPORTED),
    ("too_many_classes", dict(C=4097), UNSUPPORTED),
    ("null_row_ptr", dict(row_ptr=None), INVALID), ("null_indices", dict(indices=None), INVALID), ("null_data", dict(data=None), INVALID),
    ("no_label_form", dict(u8=None), INVALID), ("both_label_forms", dict(i32=_fake(8)), INVALID),
    ("remap_without_bytes", dict(u8=None, i32=_fake(8), remap=_fake(9)), INVALID),
    ("null_w", dict(w=None), INVALID), ("null_b", dict(b=None), INVALID),
    ("score_dtype_2", dict(score_dtype=2), INVALID), ("score_dtype_negative", dict(score_dtype=-1), INVALID),
    ("null_ap", dict(ap=None), INVALID), ("null_pos", dict(pos=None), INVALID), ("null_tp", dict(tp=None), INVALID),
    ("null_pred_pos", dict(pred_pos=None), INVALID),
    ("top_k_negative", dict(top_k=-1), INVALID), ("top_k_above_n", dict(top_k=101), INVALID), ("top_k_without_top_row", dict(top_k=5, top_row=None), INVALID),
    ("workspace_null", dict(ws=None), INVALID), ("workspace_too_small", dict(ws_short=1), INVALID),
    ("workspace_misaligned", dict(ws=C.c_void_p((1 << 20) + 8)), INVALID),
]


def _call(lib, over):
    a = dict(SHAPE, row_ptr=_fake(0), indices=_fake(1), data=_fake(2), u8=_fake(3), remap=None, i32=None, w=_fake(10), b=_fake(11), score_dtype=0,
             ap=_fake(4), pos=_fake(5), tp=_fake(6), pred_pos=_fake(7), top_k=0, top_row=_fake(12), ws=C.c_void_p(1 << 20), ws_short=0)
    a.update(over)
    need = lib.saev_latent_ap_workspace_bytes(100, 64, 11, 800)
    return lib.saev_probe_ap(a["row_ptr"], a["indices"], a["data"], a["nnz"], a["N"], a["S"], a["C"], a["u8"], a["remap"], a["i32"], a["w"], a["b"],
                             a["score_dtype"], a["ap"], a["pos"], a["tp"], a["pred_pos"], a["top_k"], a["top_row"], a["ws"], need - a["ws_short"], None)


@pytest.mark.parametrize("case", BAD, ids=[c[0] for c in BAD])
def test_the_call_refuses_bad_arguments_without_a_device(case):
    _, lib = _lib()
    _, over, status = case
    rc = _call(lib, over)
    assert rc == status, (rc, lib.saev_last_error(None))
    assert lib.saev_last_error(None).startswith(b"saev_probe_ap:")


# status and saev_last_error(NULL), word for word as the library gave them when this entry made every check itself: the refusals it
# shares with saev_latent_ap, its own where they sit among those, and the FIRST refusal of two bad arguments at once
EXACT = [
    ("negative_nnz", dict(nnz=-1), INVALID, "negative size"),
    ("latents_2_31", dict(S=1 << 31), UNSUPPORTED, "N, S and nnz must stay below 2^31"),
    ("zero_latents", dict(S=0), INVALID, "N and S must be at least 1"),
    ("too_many_classes", dict(C=4097), UNSUPPORTED, "the number of classes must lie in [1, 4096]"),
    ("null_row_ptr", dict(row_ptr=None), INVALID, "row_ptr is NULL"),
    ("null_indices", dict(indices=None), INVALID, "indices and data come with nnz > 0"),
    ("both_label_forms", dict(i32=_fake(8)), INVALID, "give the classes as class_u8 (with an optional remap) or as class_i32, one of the two"),
    ("remap_without_bytes", dict(u8=None, i32=_fake(8), remap=_fake(9)), INVALID, "remap goes with class_u8"),
    ("null_w", dict(w=None), INVALID, "w and b must not be NULL"),
    ("score_dtype_2", dict(score_dtype=2), INVALID, "score_dtype is 0 (fp32) or 1 (fp64)"),
    ("null_tp", dict(tp=None), INVALID, "ap, pos, tp and pred_pos must not be NULL"),
    ("top_k_above_n", dict(top_k=101), INVALID, "top_k must lie in [0, N]"),
    ("top_k_without_top_row", dict(top_k=5, top_row=None), INVALID, "top_row comes with top_k > 0"),
    ("workspace_null", dict(ws=None), INVALID, "workspace smaller than saev_latent_ap_workspace_bytes(N, S, C, nnz)"),
    ("workspace_too_small", dict(ws_short=1), INVALID, "workspace smaller than saev_latent_ap_workspace_bytes(N, S, C, nnz)"),
    ("workspace_misaligned", dict(ws=C.c_void_p((1 << 20) + 8)), INVALID, "workspace must be 256-byte aligned"),
    ("size_before_top_k", dict(N=0, top_k=5), INVALID, "N and S must be at least 1"),
    ("labels_before_weights", dict(u8=None, w=None), INVALID, "give the classes as class_u8 (with an optional remap) or as class_i32, one of the two"),
    ("weights_before_dtype", dict(b=None, score_dtype=2), INVALID, "w and b must not be NULL"),
    ("dtype_before_outputs", dict(score_dtype=-1, ap=None), INVALID, "score_dtype is 0 (fp32) or 1 (fp64)"),
    ("top_k_before_workspace", dict(top_k=-1, ws_short=1), INVALID, "top_k must lie in [0, N]"),
]


@pytest.mark.parametrize("case", EXACT, ids=[c[0] for c in EXACT])
def test_refusals_keep_their_status_their_text_and_their_order(case):
    _, lib = _lib()
    _, over, status, text = case
    assert _call(lib, over) == status
    assert lib.saev_last_error(None).decode() == "saev_probe_ap: " + text


def test_python_surface_refuses_host_tensors_and_bad_arguments():
    import torch
    from saev_amd import engine

    z, i, v = torch.zeros(2, dtype=torch.int64), torch.zeros(0, dtype=torch.int32), torch.zeros(0)
    lab, w = torch.zeros(1, dtype=torch.int32), torch.zeros(1, 1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        engine.probe_ap(z, i, v, 1, 1, 1, labels=lab, weights=w, biases=w)
    with pytest.raises(ValueError, match="n_classes"):
        engine.probe_ap(z, i, v, 1, 1, 4097, labels=lab, weights=w, biases=w)
    with pytest.raises(ValueError, match="top_k"):
        engine.probe_ap(z, i, v, 1, 1, 1, labels=lab, weights=w, biases=w, top_k=2)


# ---------------------------------------------------------------- the restatement ---------------------------------------------------------

def test_restatement_against_the_references_recorded_values():
    g = _golden()
    n, s, c = int(g["n_examples"]) * int(g["tokens_per_example"]), int(g["n_latents"]), int(g["n_classes"])
    assert (n, s, c) == (320, 8, 4) and int(g["max_k"]) == 96 > 64 and (GOLDEN / "g28_probe_metrics.npz").stat().st_size < 40_000
    assert g["weights"].dtype == g["biases"].dtype == np.float32
    got = PR.probe_ap(g["indptr"], g["indices"], g["data"], n, s, g["labels"].astype(np.int32), c, g["weights"], g["biases"])
    x = PR.exact_ap(g["indptr"], g["indices"], g["data"], n, s, g["labels"].astype(np.int32), c, g["weights"], g["biases"])
    j_c, cols = np.argmin(g["loss"], axis=0), np.arange(c)
    assert j_c.tolist() == [0, 1, 2, 2] and (np.sign(g["weights"][j_c, cols]) == [1, -1, 1, -1]).all()  # both signs, a shared latent
    assert (np.abs(got["ap"] - x["ap"]) <= PR.bound(got["n_ev"])).all()
    # the tie-aware value of a selected pair is the plain AP: no positive row is in a tie
    assert (np.abs(x["ap"][j_c, cols] - g["exact_ap"]) <= 2.0 ** -52).all()
    assert [fractions.Fraction(t) for t in g["exact_ap_fraction"].tolist()] == [fractions.Fraction(*map(int, t.split("/"))) for t in g["exact_ap_fraction"].tolist()]
    assert (np.abs([float(fractions.Fraction(t)) for t in g["exact_ap_fraction"].tolist()] - g["exact_ap"]) == 0).all()
    bound = (2 * n + 4) * 2.0 ** -24
    assert g["ref_ap"].dtype == np.float32 and (np.abs(got["ap"][j_c, cols] - g["ref_ap"].astype(np.float64)) <= bound).all()
    assert (g["ref_ap_distance"] <= bound).all()
    for key, mine in (("tp", got["tp"][j_c, cols]), ("pred_pos", got["pred_pos"][j_c, cols]), ("pos", got["pos"])):
        np.testing.assert_array_equal(mine, g[key])
    top = PR.top_rows(g["indptr"], g["indices"], g["data"], s, 96)
    np.testing.assert_array_equal(g["labels"][top], g["ref_top_labels"])
    assert (np.diff(PR.sorted_events(g["indptr"], g["indices"], g["data"], s)[0]) < 96).any()  # a latent with fewer than max_k events


def test_scores_from_counts_and_purity_reproduce_the_reference():
    from saev_amd import probe_metrics

    g = _golden()
    for mine, key in zip(probe_metrics.scores_from_counts(g["tp"], g["pred_pos"], g["pos"]), ("ref_precision", "ref_recall", "ref_f1")):
        assert mine.dtype == np.float32 and np.array_equal(mine, g[key])
    rng = np.random.default_rng(0)
    top = rng.integers(0, 5, size=(37, 64)).astype(np.uint8)
    top[3] = 200
    for k in (16, 64):
        want = np.empty(37, dtype=np.float32)
        for i in range(37):  # the reference's loop
            want[i] = np.unique(top[i, :k], return_counts=True)[1].max() / k
        assert probe_metrics.purity_stats(top, k) == (want.mean().item(), want.min().item(), want.max().item())
    cfg = probe_metrics.Config()
    assert (cfg.max_k, cfg.debug, cfg.mem_gb, cfg.slurm_acct, cfg.slurm_partition, cfg.n_hours) == (256, False, 80, "", "", 6.0)
    assert [str(p) for p in (cfg.run, cfg.train_shards, cfg.test_shards, cfg.log_to)] == ["runs/abcdefg", "shards/01234567", "shards/abcdef01", "logs"]


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("name", list(PK.SMALL))
def test_restatement_against_the_exact_evaluation(name, dtype):
    d = PK.SMALL[name]()
    got, x = PR.probe_ap(*_args(d, dtype)), PR.exact_ap(*_args(d, dtype))
    for key in ("pos", "n_ev", "tp", "pred_pos"):
        np.testing.assert_array_equal(got[key], x[key])
    miss = np.abs(got["ap"] - x["ap"]) / PR.bound(got["n_ev"])
    print(f"{name}: largest |restatement - exact| / bound = {miss.max():.3g}")
    assert (miss <= 1.0).all() and ((got["ap"] >= 0) & (got["ap"] <= 1 + 2.0 ** -40)).all()
    assert (got["ap"][:, got["pos"] == 0] == 0).all()
    assert (got["tp"] <= got["pred_pos"]).all() and (got["tp"] <= got["pos"][None, :]).all() and (got["pred_pos"] <= d["n"]).all()


def test_void_pairs_in_the_restatement():
    d = PK.middle()
    w, b = d["w"].copy(), d["b"].copy()
    w[0, 0], b[1, 1], w[2, 2] = np.nan, np.inf, -np.inf
    got = PR.probe_ap(*_args(dict(d, w=w, b=b), np.float64))
    base = PR.probe_ap(*_args(d, np.float64))
    void = np.zeros(w.shape, dtype=bool)
    void[0, 0] = void[1, 1] = void[2, 2] = True
    assert np.isnan(got["ap"][void]).all() and (got["tp"][void] == 0).all() and (got["pred_pos"][void] == 0).all()
    np.testing.assert_array_equal(got["ap"][~void], base["ap"][~void])


def _brute_force(scores, is_c):
    """The mean over every order of the tied rows of the AP of the ranking by descending score, in rationals."""
    n, pos = len(scores), int(is_c.sum())
    if pos == 0:
        return fractions.Fraction(0)
    levels = sorted(set(scores.tolist()), reverse=True)
    blocks = [[i for i in range(n) if scores[i] == v] for v in levels]
    total, count = fractions.Fraction(0), 0
    for perm in itertools.product(*(itertools.permutations(b) for b in blocks)):
        hits, ap = 0, fractions.Fraction(0)
        for rank, row in enumerate(itertools.chain.from_iterable(perm), start=1):
            if is_c[row]:
                hits += 1
                ap += fractions.Fraction(hits, rank)
        total += ap / pos
        count += 1
    return total / count


def test_tie_aware_expectation_against_every_order_of_the_tied_rows():
    seen_ties = 0
    for seed in range(60):
        d = PK.tiny(seed)
        assert d["n"] <= 7
        for dtype in (np.float32, np.float64):
            got = PR.exact_ap(*_args(d, dtype))
            dense = np.zeros((d["n"], d["s"]), dtype=np.float32)
            for r in range(d["n"]):
                for p in range(d["indptr"][r], d["indptr"][r + 1]):
                    dense[r, d["indices"][p]] = d["data"][p]
            for j in range(d["s"]):
                for c in range(d["c"]):
                    s = PR.score(d["w"][j, c], dense[:, j], d["b"][j, c], dtype)
                    seen_ties += len(set(s.tolist())) < d["n"]
                    want = _brute_force(s, d["cls"] == c)
                    assert abs(got["ap"][j, c] - float(want)) <= 2.0 ** -50, (seed, j, c)
                    assert got["pred_pos"][j, c] == int((s > 0).sum()) and got["tp"][j, c] == int(((s > 0) & (d["cls"] == c)).sum())
    assert seen_ties > 100


def test_designs_hold_what_they_are_said_to_hold():
    reach = {(name, dt.__name__): PR.probe_ap(*_args(PK.SMALL[name](), dt))["reach"] for name in ("kinds", "middle", "created", "chunks") for dt in (np.float32, np.float64)}
    assert reach["kinds", "float32"]["inf_ties"] > 0 and reach["kinds", "float32"]["collapsed"] > reach["kinds", "float64"]["collapsed"] > 0
    for dt in ("float32", "float64"):
        assert reach["middle", dt]["merged"] == 6 and reach["middle", dt]["zero_inside"] == 16
    assert reach["created", "float32"]["merged"] > 0 and reach["created", "float64"]["zero_first"] > 0
    d = PK.chunks()
    assert np.diff(PR.sorted_events(d["indptr"], d["indices"], d["data"], d["s"])[0]).tolist() == [63, 64, 65, 129] and (d["w"][:, [0, 2]] < 0).all()
    d = PK.created()
    starts, _, val, rows = PR.sorted_events(d["indptr"], d["indices"], d["data"], d["s"])
    for col, dtype in ((0, np.float32), (1, np.float64), (2, np.float32), (3, np.float64)):
        ranks = []
        for j in (0, 1):  # (one of the two has its zero block of 52 rows first)
            groups, _, _ = PR.pair_groups(val[starts[j]:starts[j + 1]], d["cls"][rows[starts[j]:starts[j + 1]]] == col, d["n"], int((d["cls"] == col).sum()),
                                          d["w"][j, col], d["b"][j, col], dtype)
            made = [(t, n) for t, n, _, _, z in groups if n > 1 and not z]
            sizes = sorted(n for _, n in made)
            assert sizes == sorted(2 * [PK.DIRECT_MAX - 1, PK.DIRECT_MAX, PK.DIRECT_MAX + 1]), (col, j, made)
            ranks += [t for t, _ in made]
        assert min(ranks) == 0 and sorted(ranks)[2] < 32 < max(ranks)
    s = PK.silent()
    ev = PR.probe_ap(*_args(s, np.float32))
    assert (ev["n_ev"].diagonal() < ev["pos"]).all() and (ev["n_ev"].diagonal() > 0).all()  # positive rows in the zero block


# ---------------------------------------------------------------- the Python module -------------------------------------------------------

@pytest.mark.parametrize("leave_out, message", [("train_acts", "Train SAE acts missing: '"), ("test_acts", "Validation SAE acts missing: '"),
                                                ("probe", "Probe metrics missing: '"), ("labels", "Validation labels missing: '")])
def test_worker_fn_makes_the_references_file_checks(tmp_path, leave_out, message):
    from saev_amd import probe_metrics

    run_dir, train_shards, test_shards = PK.g28_run(tmp_path, _golden(), leave_out=(leave_out,))
    with pytest.raises(AssertionError, match=re.escape(message)):
        probe_metrics.worker_fn(probe_metrics.Config(run=run_dir, train_shards=train_shards, test_shards=test_shards, max_k=96))


def test_worker_fn_checks_shapes_before_it_needs_a_device(tmp_path):
    from saev_amd import probe_metrics

    g = _golden()
    run_dir, train_shards, test_shards = PK.g28_run(tmp_path, dict(g, biases=g["biases"][:, :3]))
    with pytest.raises(AssertionError, match="Probe metric shapes are inconsistent: loss"):
        probe_metrics.worker_fn(probe_metrics.Config(run=run_dir, train_shards=train_shards, test_shards=test_shards, max_k=96))
    run_dir, train_shards, test_shards = PK.g28_run(tmp_path / "b", g)
    with pytest.raises(AssertionError, match=r"max_k \(321\) exceeds validation samples \(320\)"):
        probe_metrics.worker_fn(probe_metrics.Config(run=run_dir, train_shards=train_shards, test_shards=test_shards, max_k=321))
    with pytest.raises(AssertionError, match="max_k must be positive; got 0"):
        probe_metrics.worker_fn(probe_metrics.Config(run=run_dir, train_shards=train_shards, test_shards=test_shards, max_k=0))
