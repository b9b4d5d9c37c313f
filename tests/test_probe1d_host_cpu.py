"""CPU-only tests of the per-latent logistic probes (include/saev_amd.h: PROBE1D): the entries are declared,
exported and bound with the header's types; the struct mirrors match what gcc makes of the header; every argument check refuses a
call before anything touches a device; the Python surface refuses what the reference refuses; worker_fn returns 1 on every missing
input; and the numpy restatement the GPU tests compare against (tests/probe1d_restatement.py) is held against fixtures G23 and G25,
recorded from the reference, under the rules the GPU end-to-end test applies to the kernels."""

import ctypes as C
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse
import torch

import probe1d_cases as K
import probe1d_restatement as R
from conftest import GOLDEN, ROOT

ENTRIES = ("saev_probe1d_workspace_bytes", "saev_probe1d_layout_of", "saev_probe1d_prepare", "saev_probe1d_stats", "saev_probe1d_init",
           "saev_probe1d_update", "saev_probe1d_fit", "saev_probe1d_evaluate")
CTYPES = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double}
INVALID, UNSUPPORTED = -1, -3
FIXTURES = ("plain", "absent", "groups", "wide")


def _lib():
    subprocess.run(["make", "-C", str(ROOT)], check=True, capture_output=True)
    from saev_amd import _lib

    return _lib, _lib.load()


def _ctype(decl: str, lib_mod):
    decl = decl.replace("const", "").strip()
    if "saev_probe1d_cfg" in decl:
        return C.POINTER(lib_mod.SaevProbe1DCfg)
    if "saev_probe1d_layout" in decl:
        return C.POINTER(lib_mod.SaevProbe1DLayout)
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
    assert re.search(r"#define\s+SAEV_AMD_ABI_VERSION\s+12\b", text)


@pytest.mark.parametrize("struct,cls_name", [("saev_probe1d_cfg", "SaevProbe1DCfg"), ("saev_probe1d_layout", "SaevProbe1DLayout")])
def test_struct_mirrors_match_the_header(tmp_path, struct, cls_name):
    lib_mod, _ = _lib()
    cls = getattr(lib_mod, cls_name)
    fields = [f for f, _ in cls._fields_]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "saev_amd.h"', "int main(void) {", f'printf("size %zu\\n", sizeof({struct}));']
    src += [f'printf("{f} %zu\\n", offsetof({struct}, {f}));' for f in fields]
    src.append("return 0; }")
    (tmp_path / "layout.c").write_text("\n".join(src))
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True)
    want = dict(line.split() for line in subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.splitlines())
    assert C.sizeof(cls) == int(want["size"])
    for f in fields:
        assert getattr(cls, f).offset == int(want[f]), f


def test_workspace_and_layout():
    lib_mod, lib = _lib()
    from saev_amd.engine import Probe1D

    for shape in [(1, 1, 1, 0), (600, 48, 11, 6363), (5000, 1031, 256, 40000), (1 << 20, 16384, 151, 1 << 25)]:
        L = lib_mod.SaevProbe1DLayout()
        assert lib.saev_probe1d_layout_of(*shape, C.byref(L)) == 0
        n, s, c, nnz = shape
        assert L.total_bytes == lib.saev_probe1d_workspace_bytes(*shape) and L.total_bytes % 256 == 0
        assert L.chunk == Probe1D.CHUNK == 512 and L.words == (c + 31) // 32
        assert L.max_chunks >= sum(-(-k // L.chunk) for k in (nnz,)) and L.max_chunks >= s  # one chunk per latent and per 512 events
        offs = sorted((getattr(L, f), f) for f, _ in lib_mod.SaevProbe1DLayout._fields_ if f.startswith("off_"))
        assert all(o % 256 == 0 for o, _ in offs) and len({o for o, _ in offs}) == len(offs)
        sizes = {"off_starts": 8 * (s + 1), "off_row": 4 * nnz, "off_val": 4 * nnz, "off_qx": 8 * s, "off_ybits": 4 * n * L.words, "off_pos": 8 * c,
                 "off_b": 8 * s * c, "off_sums": 56 * s * c, "off_part": 56 * c * L.max_chunks, "off_cnt": 4 * L.parts * s}
        for (o, f), (o_next, _) in zip(offs, offs[1:] + [(L.total_bytes, "")]):
            assert o_next - o >= sizes.get(f, 0), f
    # the issue's 5 M-token split: a few GB, no (nnz, C) array (that would be 1.6e8 x 151 x 8 bytes = 193 GB)
    assert lib.saev_probe1d_workspace_bytes(5_000_000, 16384, 151, 160_000_000) < 12 * 2**30
    for bad in [(0, 4, 4, 0), (4, 0, 4, 0), (4, 4, 0, 0), (4, 4, 4097, 0), (1 << 31, 4, 4, 0), (4, 1 << 31, 4, 0), (4, 4, 4, 1 << 31), (4, 4, 4, -1)]:
        assert lib.saev_probe1d_workspace_bytes(*bad) == -1, bad
    assert lib.saev_probe1d_workspace_bytes(100, 16, 256, 50) > 0  # labels.bin is uint8: 256 classes are in range


def _fake(i):
    return C.c_void_p((1 << 21) + 4096 * i)


def _cfg(lib_mod, **over):
    a = dict(struct_size=C.sizeof(lib_mod.SaevProbe1DCfg), max_iter=30, class_slab_size=8, poll_every=0, out_dtype=0, ridge=1e-8, tol=1e-6,
             lam_init=1e-3, lam_shrink=0.1, lam_grow=10.0, delta_logit=6.0)
    a.update(over)
    return lib_mod.SaevProbe1DCfg(**a)


SHAPE = dict(N=100, S=64, C=11, nnz=800)
# the fake device pointers are never dereferenced: a launch on them would fault, and this machine has no device to launch on
BAD_PREPARE = [
    ("negative_n", dict(N=-1), INVALID), ("zero_rows", dict(N=0), INVALID), ("zero_latents", dict(S=0), INVALID),
    ("rows_2_31", dict(N=1 << 31), UNSUPPORTED), ("nnz_2_31", dict(nnz=1 << 31), UNSUPPORTED), ("latents_2_31", dict(S=1 << 31), UNSUPPORTED),
    ("no_classes", dict(C=0), UNSUPPORTED), ("too_many_classes", dict(C=4097), UNSUPPORTED),
    ("null_row_ptr", dict(row_ptr=None), INVALID), ("null_indices", dict(indices=None), INVALID), ("null_data", dict(data=None), INVALID),
    ("no_labels", dict(u8=None), INVALID), ("two_label_forms", dict(i32=_fake(8)), INVALID), ("ids_and_matrix", dict(mat=_fake(9)), INVALID),
    ("uint8_ids_for_300_classes", dict(C=300), INVALID),
    ("workspace_null", dict(ws=None), INVALID), ("workspace_too_small", dict(ws_short=1), INVALID),
    ("workspace_misaligned", dict(ws=C.c_void_p((1 << 20) + 8)), INVALID),
]


@pytest.mark.parametrize("case", BAD_PREPARE, ids=[c[0] for c in BAD_PREPARE])
def test_prepare_refuses_bad_arguments_without_a_device(case):
    _, lib = _lib()
    _, over, status = case
    a = dict(SHAPE, row_ptr=_fake(0), indices=_fake(1), data=_fake(2), u8=_fake(3), i32=None, mat=None, ws=C.c_void_p(1 << 20), ws_short=0)
    a.update(over)
    need = max(lib.saev_probe1d_workspace_bytes(a["N"], a["S"], a["C"], a["nnz"]), 256)
    rc = lib.saev_probe1d_prepare(a["row_ptr"], a["indices"], a["data"], a["nnz"], a["N"], a["S"], a["C"], a["u8"], a["i32"], a["mat"], a["ws"],
                                  need - a["ws_short"], None)
    assert rc == status, case[0]
    assert lib.saev_last_error(None).decode().startswith("saev_probe1d_prepare:")


BAD_CFG = [("no_cfg", None), ("max_iter", dict(max_iter=-1)), ("slab", dict(class_slab_size=0)), ("poll", dict(poll_every=-1)),
           ("dtype", dict(out_dtype=2)), ("shrink_0", dict(lam_shrink=0.0)), ("shrink_1", dict(lam_shrink=1.0)), ("grow", dict(lam_grow=1.0)),
           ("delta", dict(delta_logit=0.0)), ("ridge", dict(ridge=-1.0)), ("lam_init", dict(lam_init=0.0)), ("struct_size", dict(struct_size=0))]


@pytest.mark.parametrize("case", BAD_CFG, ids=[c[0] for c in BAD_CFG])
def test_solver_entries_refuse_a_bad_cfg_without_a_device(case):
    lib_mod, lib = _lib()
    cfg = None if case[1] is None else C.byref(_cfg(lib_mod, **case[1]))
    shape = tuple(SHAPE.values())
    ws, nb = C.c_void_p(1 << 20), lib.saev_probe1d_workspace_bytes(*shape)
    assert lib.saev_probe1d_fit(*shape, cfg, _fake(0), _fake(1), _fake(2), ws, nb, None) == INVALID
    assert lib.saev_last_error(None).decode().startswith("saev_probe1d_fit:")
    assert lib.saev_probe1d_update(*shape, cfg, None, None, None, ws, nb, None) == INVALID
    assert lib.saev_probe1d_init(*shape, cfg, ws, nb, None) == INVALID


def test_stats_and_evaluate_refuse_bad_arguments_without_a_device():
    lib_mod, lib = _lib()
    shape = tuple(SHAPE.values())
    ws, nb = C.c_void_p(1 << 20), lib.saev_probe1d_workspace_bytes(*shape)
    assert lib.saev_probe1d_stats(*shape, None, _fake(1), _fake(2), ws, nb, None) == INVALID
    assert lib.saev_probe1d_stats(*shape, _fake(0), _fake(1), None, ws, nb, None) == INVALID
    assert lib.saev_probe1d_stats(*shape, _fake(0), _fake(1), _fake(2), ws, nb - 1, None) == INVALID
    out = [_fake(i) for i in range(3, 8)]
    for thr in (0.0, 1.0, -0.5, float("nan")):
        assert lib.saev_probe1d_evaluate(*shape, _fake(0), _fake(1), thr, 0, *out, ws, nb, None) == INVALID
    assert lib.saev_probe1d_evaluate(*shape, _fake(0), _fake(1), 0.5, 7, *out, ws, nb, None) == INVALID
    assert lib.saev_probe1d_evaluate(*shape, None, _fake(1), 0.5, 0, *out, ws, nb, None) == INVALID
    assert lib.saev_last_error(None).decode().startswith("saev_probe1d_evaluate:")
    assert lib.saev_probe1d_layout_of(*shape, None) == INVALID
    assert lib.saev_probe1d_layout_of(4, 4, 4097, 0, C.byref(lib_mod.SaevProbe1DLayout())) == UNSUPPORTED


# status and saev_last_error(NULL) word for word, as the library gave them when p1_open and p1_cfg formatted their own messages
P1_EXACT = [
    (dict(N=-1), INVALID, "negative size"),
    (dict(S=1 << 31), UNSUPPORTED, "N, S and nnz must stay below 2^31"),
    (dict(N=0), INVALID, "N and S must be at least 1"),
    (dict(C=4097), UNSUPPORTED, "the number of classes must lie in [1, 4096]"),
    (dict(ws=None), INVALID, "workspace smaller than saev_probe1d_workspace_bytes(N, S, C, nnz)"),
    (dict(ws_short=1), INVALID, "workspace smaller than saev_probe1d_workspace_bytes(N, S, C, nnz)"),
    (dict(ws=C.c_void_p((1 << 20) + 8)), INVALID, "workspace must be 256-byte aligned"),
]
P1_ENTRIES = ("prepare", "stats", "init", "update", "fit", "evaluate")


@pytest.mark.parametrize("entry", P1_ENTRIES)
def test_every_entry_keeps_the_status_and_the_text_of_the_shared_refusals(entry):
    lib_mod, lib = _lib()
    cfg = C.byref(_cfg(lib_mod))
    for over, status, text in P1_EXACT:
        a = dict(SHAPE, ws=C.c_void_p(1 << 20), ws_short=0)
        a.update(over)
        shape = (a["N"], a["S"], a["C"], a["nnz"])
        tail = (a["ws"], lib.saev_probe1d_workspace_bytes(*SHAPE.values()) - a["ws_short"], None)
        if entry == "prepare":  # (its own arguments are all bad: the shared checks come first)
            rc = lib.saev_probe1d_prepare(None, None, None, a["nnz"], a["N"], a["S"], a["C"], None, None, None, *tail)
        elif entry == "stats":
            rc = lib.saev_probe1d_stats(*shape, None, None, None, *tail)
        elif entry == "init":
            rc = lib.saev_probe1d_init(*shape, None, *tail)
        elif entry == "update":
            rc = lib.saev_probe1d_update(*shape, None, None, None, None, *tail)
        elif entry == "fit":
            rc = lib.saev_probe1d_fit(*shape, cfg, _fake(0), _fake(1), _fake(2), *tail)
        else:
            rc = lib.saev_probe1d_evaluate(*shape, None, None, 2.0, 7, None, None, None, None, None, *tail)
        assert rc == status, (entry, over)
        assert lib.saev_last_error(None).decode() == f"saev_probe1d_{entry}: {text}", (entry, over)


def test_prepare_and_cfg_refusals_keep_their_text():
    lib_mod, lib = _lib()
    shape = tuple(SHAPE.values())
    ws, nb = C.c_void_p(1 << 20), lib.saev_probe1d_workspace_bytes(*shape)
    n, s, c, nnz = shape
    for args, text in [
        ((None, _fake(1), _fake(2), nnz, n, s, c, _fake(3), None, None), "row_ptr is NULL"),
        ((_fake(0), None, _fake(2), nnz, n, s, c, _fake(3), None, None), "indices and data come with nnz > 0"),
        ((_fake(0), _fake(1), _fake(2), nnz, n, s, c, _fake(3), _fake(8), None),
         "give the labels as class ids (uint8 or int32) or as an N x C 0/1 matrix, one of the three"),
        ((_fake(0), _fake(1), _fake(2), nnz, n, s, 300, _fake(3), None, None), "uint8 class ids cannot name more than 256 classes"),
    ]:
        need = lib.saev_probe1d_workspace_bytes(*args[4:7], nnz)
        assert lib.saev_probe1d_prepare(*args, ws, need, None) == INVALID
        assert lib.saev_last_error(None).decode() == "saev_probe1d_prepare: " + text
    for over, text in [(None, "no saev_probe1d_cfg (or its struct_size is unset)"), (dict(max_iter=-1), "max_iter must be >= 0"),
                       (dict(out_dtype=2), "out_dtype must be SAEV_PROBE1D_F32 or SAEV_PROBE1D_F64"), (dict(lam_shrink=1.0), "lam_shrink must lie in (0, 1)"),
                       (dict(lam_init=0.0), "ridge and tol must be >= 0 and lam_init > 0")]:
        cfg = None if over is None else C.byref(_cfg(lib_mod, **over))
        assert lib.saev_probe1d_init(*shape, cfg, ws, nb, None) == INVALID
        assert lib.saev_last_error(None).decode() == "saev_probe1d_init: " + text
        assert lib.saev_probe1d_update(*shape, cfg, None, None, None, ws, nb, None) == INVALID
        assert lib.saev_last_error(None).decode() == "saev_probe1d_update: " + text
        assert lib.saev_probe1d_fit(*shape, cfg, _fake(0), _fake(1), _fake(2), ws, nb, None) == INVALID
        assert lib.saev_last_error(None).decode() == "saev_probe1d_fit: " + text
    assert lib.saev_probe1d_layout_of(4, 4, 4097, 0, C.byref(lib_mod.SaevProbe1DLayout())) == UNSUPPORTED
    assert lib.saev_last_error(None).decode() == "saev_probe1d_layout_of: 1 <= N, S < 2^31, 1 <= C <= 4096, 0 <= nnz < 2^31"


def test_python_entries_refuse_bad_arguments():
    _lib()
    from saev_amd import probe1d
    from saev_amd.engine import Probe1D

    for kw, msg in ((dict(lam_shrink=0.0), "lam_shrink"), (dict(lam_shrink=1.0), "lam_shrink"), (dict(lam_grow=1.0), "lam_grow"),
                    (dict(delta_logit=0.0), "delta_logit"), (dict(dtype=torch.float16), "dtype"), (dict(n_classes=0), "n_classes"),
                    (dict(n_classes=4097), "n_classes"), (dict(class_slab_size=0), "class_slab_size")):
        with pytest.raises(ValueError, match=msg):
            probe1d.Sparse1DProbe(**{**dict(n_latents=8, n_classes=3), **kw})
    probe = probe1d.Sparse1DProbe(n_latents=8, n_classes=3, row_batch_size=77)  # accepted, ignored
    x = scipy.sparse.csr_matrix(np.eye(8, dtype=np.float32))
    y = np.zeros((8, 3), dtype=np.float32)
    with pytest.raises(TypeError, match="CSR"):
        probe.fit(x.tocsc(), y)
    with pytest.raises(TypeError, match="CSR"):
        probe.fit(torch.eye(8), y)
    with pytest.raises(ValueError, match="9 latents"):
        probe.fit(scipy.sparse.csr_matrix(np.ones((8, 9), dtype=np.float32)), y)
    with pytest.raises(ValueError, match="shape"):
        probe.fit(x, np.zeros((8, 4), dtype=np.float32))
    with pytest.raises(ValueError, match="7 class ids"):
        probe.fit(x, np.zeros(7, dtype=np.uint8))
    with pytest.raises(ValueError, match="class ids must be"):
        probe.fit(x, np.zeros(8, dtype=np.float32))
    bad = y.copy()
    bad[3, 1] = 0.5
    with pytest.raises(ValueError, match="only 0 and 1"):
        probe.fit(x, bad)
    with pytest.raises(RuntimeError, match="not fitted"):
        probe.loss_matrix(x, y)
    for shape, msg in (((0, 4, 4, 0), "n_rows"), ((4, 0, 4, 0), "n_latents"), ((4, 4, 0, 0), "n_classes"), ((4, 4, 4097, 0), "n_classes"),
                       ((4, 4, 4, -1), "nnz"), ((4, 4, 4, 1 << 31), "nnz")):
        with pytest.raises(ValueError, match=msg):
            Probe1D(*shape, "cuda")
    with pytest.raises(RuntimeError, match="no CPU path"):
        Probe1D(4, 4, 4, 0, "cpu")
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU path"):
            probe.fit(x, y)


def test_the_package_imports_none_of_the_references_extras():
    text = (ROOT / "saev_amd" / "probe1d.py").read_text()
    assert not re.search(r"^\s*(import|from)\s+(sklearn|beartype|cloudpickle|jaxtyping|tyro)\b", text, flags=re.M)


def _run_dirs(tmp_path, *, labels=True, inference=True, acts=True):
    from saev_amd import disk
    from saev_amd.data import write_shards

    rng = np.random.default_rng(0)
    shards = []
    for i in range(2):
        x = rng.standard_normal((3 + i, 1, 4, 8)).astype(np.float32)  # 12 and 16 tokens
        shards.append(write_shards(tmp_path / f"s{i}", x, labels=rng.integers(0, 3, size=(3 + i, 4)).astype(np.uint8) if labels else None))
    run = disk.Run.new("probe0001", train_shards_dir=shards[0], val_shards_dir=shards[1], runs_root=tmp_path / "saev" / "runs")
    for i, sh in enumerate(shards):
        if inference:
            (run.inference / sh.name).mkdir()
            if acts:
                scipy.sparse.save_npz(run.inference / sh.name / "token_acts.npz",
                                      scipy.sparse.random(12 + 4 * i, 6, density=0.4, format="csr", dtype=np.float32))
    return run, shards


@pytest.mark.parametrize("missing", ["train_dir", "test_dir", "labels", "inference", "acts", "rows"])
def test_worker_fn_returns_1_on_every_missing_input_without_a_device(tmp_path, monkeypatch, missing):
    _lib()
    from saev_amd import engine, probe1d

    run, shards = _run_dirs(tmp_path, labels=missing != "labels", inference=missing != "inference", acts=missing != "acts")
    cfg = probe1d.Config(run=run.run_dir, train_shards=shards[0], test_shards=shards[1])
    if missing == "train_dir":
        cfg = dataclasses_replace(cfg, train_shards=tmp_path / "nowhere")
    if missing == "test_dir":
        cfg = dataclasses_replace(cfg, test_shards=tmp_path / "nowhere")
    if missing == "rows":
        scipy.sparse.save_npz(run.inference / shards[1].name / "token_acts.npz", scipy.sparse.random(13, 6, density=0.4, format="csr", dtype=np.float32))

    def no_device(*a, **k):
        raise AssertionError("the device object was built although an input is missing")

    monkeypatch.setattr(engine.Probe1D, "__init__", no_device)
    assert probe1d.worker_fn(cfg) == 1


def dataclasses_replace(cfg, **kw):
    import dataclasses

    return dataclasses.replace(cfg, **kw)


def _g23(tag):
    with np.load(GOLDEN / f"{'g25' if tag in ('groups', 'wide') else 'g23'}_probe1d_{tag}.npz") as z:
        return {k: z[k] for k in z.files}


def _hyper(g):
    return R.Hyper(**{k: type(getattr(R.Hyper(), k))(g[k]) for k in ("ridge", "tol", "max_iter", "lam_init", "lam_shrink", "lam_grow", "delta_logit",
                                                                    "class_slab_size")})


def test_fixture_g23_holds_the_designs_the_tests_rely_on():
    g = _g23("plain")
    per = np.bincount(g["indices"], minlength=48)
    assert (per == 0).sum() == 2 and (per == 1).sum() == 1 and (per == 600).sum() == 1
    assert (g["data"] < 0).any() and (g["data"] == 0).sum() == 1 and int(g["class_slab_size"]) == 8 and int(g["n_classes"]) == 11
    j = 7
    rows = np.repeat(np.arange(600), np.diff(g["indptr"]))[g["indices"] == j]
    assert set(rows) == set(np.flatnonzero(g["labels"] == 2))  # a latent that separates a class
    a = _g23("absent")
    assert not np.isin(a["labels"], (4, 5, 6, 7)).any() and int(a["class_slab_size"]) == 4
    assert a["r64_n_iter"][4:8].tolist() == [1] * 4 and a["r64_n_iter"].max() > 1  # that slab stops at once, the others run on
    for f in (g, a):
        assert f["min_gap"] >= 1e-9 and f["r64_coef"].dtype == np.float64 and f["r32_coef"].dtype == np.float32 and int(f["max_iter"]) == 30


def test_fixture_g25_holds_the_designs_the_tests_rely_on():
    g, w = _g23("groups"), _g23("wide")
    assert (int(g["n_rows"]), int(g["n_classes"]), int(g["class_slab_size"])) == (600, 70, 32) and g["labels"].max() == 61
    assert g["r64_n_iter"][64:].tolist() == [1] * 6 and g["r64_n_iter"][:64].min() > 1  # the last slab is absent and stops at once
    assert (int(w["n_rows"]), int(w["n_classes"]), int(w["class_slab_size"])) == (600, 151, 8) and not np.isin(w["labels"], range(64, 72)).any()
    assert w["r64_n_iter"][64:72].tolist() == [1] * 8 and np.delete(w["r64_n_iter"], range(64, 72)).min() > 1 and w["labels"].max() == 150
    biggest = max((GOLDEN / f"g23_probe1d_{t}.npz").stat().st_size for t in ("plain", "absent"))
    for f, name in ((g, "groups"), (w, "wide")):
        assert f["min_gap"] >= 1e-9 and f["well_posed"].any() and f["r64_coef"].dtype == np.float64 and int(f["max_iter"]) == 30
        assert (GOLDEN / f"g25_probe1d_{name}.npz").stat().st_size <= biggest


@pytest.mark.parametrize("tag", FIXTURES)
def test_the_restatement_reproduces_g23_under_the_end_to_end_rules(tag):
    """The numpy restatement of the contract against the reference's recorded results, under the rules of the GPU end-to-end test:
    n_iter equal; every loss within loss_band of R64; coefficients and intercepts of every well-posed pair within coef_band, at most
    1 % of all pairs outside; counts equal at R64's coefficients; qx to 1e-14."""
    g = _g23(tag)
    s, c, n = int(g["n_latents"]), int(g["n_classes"]), int(g["n_rows"])
    b, w, n_iter, qx = R.fit(g["indptr"], g["indices"], g["data"], s, g["labels"], c, _hyper(g))
    np.testing.assert_array_equal(n_iter, g["r64_n_iter"])
    np.testing.assert_allclose(qx, g["r64_qx"], rtol=1e-14)
    dist = np.maximum(np.abs(w - g["r64_coef"]) / (1 + np.abs(g["r64_coef"])), np.abs(b - g["r64_intercept"]) / (1 + np.abs(g["r64_intercept"])))
    print(f"{tag}: largest distance {dist.max():.3g} (well-posed {dist[g['well_posed']].max():.3g}), coef_band {float(g['coef_band']):.3g}")
    assert (dist[g["well_posed"]] <= g["coef_band"]).all()
    assert (dist > g["coef_band"]).mean() <= 0.01
    loss, tp, fp, tn, fn, _ = R.evaluate(g["indptr"], g["indices"], g["data"], s, g["labels"], c, b, w)
    print(f"{tag}: largest loss difference {np.abs(loss - g['r64_loss']).max():.3g}, loss_band {float(g['loss_band']):.3g}")
    assert (np.abs(loss - g["r64_loss"]) <= g["loss_band"]).all()
    np.testing.assert_array_equal(tp + fp + tn + fn, n)
    np.testing.assert_array_equal(tp + fn, np.broadcast_to(np.bincount(g["labels"], minlength=c), (s, c)))
    at = R.evaluate(g["indptr"], g["indices"], g["data"], s, g["labels"], c, g["r64_intercept"], g["r64_coef"])
    for name, got in zip(("tp", "fp", "tn", "fn"), at[1:5]):
        np.testing.assert_array_equal(got, g[f"r64_{name}"], err_msg=name)
    assert (np.abs(at[0] - g["r64_loss"]) <= 1e-12 * at[5] + 2.0 ** -24 * np.abs(g["r64_loss"])).all()  # (R64's loss is stored as float32)


def test_both_label_forms_restate_to_the_same_bits():
    rng = np.random.default_rng(4)
    for c in (1, 11, 32, 33, 65, 256):
        ids = rng.integers(0, c, size=97)
        a, b = R.labels_matrix(ids, c), R.labels_matrix(np.eye(c, dtype=np.uint8)[ids], c)
        np.testing.assert_array_equal(R.pack_bits(a), R.pack_bits(b))
        assert R.pack_bits(a).shape == (97, (c + 31) // 32)
        assert all((R.pack_bits(a)[i, ids[i] // 32] >> np.uint32(ids[i] % 32)) & 1 for i in range(97))


# ---- the conditions the tests of test_gpu_probe1d_geometry.py rely on, checked on the very same arrays ---------------------------------------

@pytest.mark.parametrize("name", list(K.PLACEMENT))
def test_placement_designs_have_the_groups_per_part_they_are_named_for(name):
    """From the library's own part count and lm_part_len restated here: a change of LM_PARTS or of the rule cannot quietly turn these
    designs into ones with a single group of 64 per part."""
    lib_mod, lib = _lib()
    fn, groups, parts, ragged = K.PLACEMENT[name]
    d = fn()
    L = lib_mod.SaevProbe1DLayout()
    assert lib.saev_probe1d_layout_of(d.n, d.s, d.c, d.nnz, C.byref(L)) == 0
    per_part = -(-d.nnz // L.parts)
    part_len = max(64, -(-per_part // 64) * 64)  # lm_part_len
    assert L.parts == parts and part_len == 64 * groups and (L.parts, part_len) == K.parts_of(d.s, d.nnz)
    assert -(-d.nnz // part_len) >= 2 and (not ragged or d.nnz % part_len != 0)
    assert d.indptr[0] == 0 and d.indptr[-1] == d.nnz == d.indices.size and d.indptr.size == d.n + 1 and (d.data < 0).any()
    per, row_len = np.bincount(d.indices, minlength=d.s), np.diff(d.indptr)
    e = np.arange(d.nnz)
    key = (e // part_len) * d.s + d.indices  # (part, latent)
    in_first, in_later = key[e % part_len < 64], key[e % part_len >= 64]
    if name != "long_rows":  # (there a part holds 128 different latents, each once)
        assert np.intersect1d(in_first, in_later).size > 0  # a latent's cursor is advanced by one group and read by a later one
    if name == "two_groups":
        assert (d.n, d.s, d.c) == (2100, 300, 11) and 65537 <= d.nnz <= 70000 and set(row_len) == {31, 32}
    if name == "four_groups":
        stored = row_len > 0
        assert (d.n, d.s, d.c) == (5000, 1031, 33) and 190000 <= d.nnz <= 210000
        assert per[0] == stored.sum() and -(-per[0] // K.CHUNK) == 10 and per[1] == (stored & (np.arange(d.n) % 2 == 0)).sum() and per[2] == 0
        assert not stored[0] and not stored[-1] and not stored[3::17].any() and stored.sum() == d.n - 2 - len(range(3, d.n, 17))
        o = K.four_groups_other()
        assert (o.n, o.s, o.c, o.nnz) == (d.n, d.s, d.c, d.nnz) and not np.array_equal(o.indices, d.indices) and not np.array_equal(o.ids, d.ids)
    if name == "many_latents":
        assert (d.n, d.s, d.c) == (3000, 131072, 1) and L.parts == (1 << 26) // d.s < -(-d.nnz // 64) and 95000 <= d.nnz <= 105000
        assert (per == 0).mean() > 0.5 and per[-1] == 0 and d.s // 1024 == 128
    if name == "one_latent_rows":
        assert (d.n, d.s, d.c) == (70000, 5, 1) and d.nnz == d.n and (d.indices == 3).all() and (row_len == 1).all()
    if name == "long_rows":
        assert (d.n, d.s) == (40, 2048) and d.nnz == 81920 and (row_len == d.s).all() and (d.indices.reshape(d.n, d.s) == np.arange(d.s)).all()
        assert d.s // 64 == 32 and part_len < d.s


@pytest.mark.parametrize("c", K.LABEL_CLASSES)
def test_label_designs_hold_the_classes_the_tests_name(c):
    d = K.label_design(c)
    assert (d.n, d.s) == (5000, 8) and d.ids.dtype == np.int64 and d.ids.min() == 0 and d.ids.max() == c - 1 and not (d.ids == c - 3).any()
    assert np.bincount(d.indices, minlength=d.s).tolist() == list(K.LABEL_COUNTS) and d.nnz * c * 8 < 100 << 20  # (a term of the numpy sums)
    assert all(d.ymat[:, k].sum() >= 30 for k in K.ALONE_CLASSES if k < c)
    assert c <= 4096 and K.LABEL_CLASSES[-1] == 4096  # 4 097 is refused: test_python_entries_refuse_bad_arguments


@pytest.mark.parametrize("pair", list(K.FIT_PAIRS), ids=[f"c{c}_slab{s}" for c, s in K.FIT_PAIRS])
def test_fit_designs_stop_slab_by_slab_ten_times_clear_of_tol(pair):
    """What test_gpu_probe1d_geometry.py takes for granted of a fit design, by the restatement: slabs stop at different iterations
    (in C = 151 and 130 a whole 64-class group before another), one is still running at max_iter, and at every decision the slab's
    largest scaled gradient is 10 x away from tol -- below it at the stopping iteration, above it at every one before and, for a
    slab left running, through max_iter.  The factor is a condition on these inputs, not a tolerance on any kernel."""
    c, slab = pair
    d, hp = K.fit_design(c, slab), K.fit_hyper(c, slab)
    b, w, n_iter, gmax, done = K.fit_trace(d, hp)
    rb, rw, rn, _ = R.fit(*d.csr, d.s, d.ymat, d.c, hp)  # the trace is the restatement's fit
    np.testing.assert_array_equal(b.view(np.uint64), rb.view(np.uint64))
    np.testing.assert_array_equal(w.view(np.uint64), rw.view(np.uint64))
    np.testing.assert_array_equal(n_iter, rn)
    per = np.bincount(d.indices, minlength=d.s)
    assert (d.n, d.s) == (600, 24) and per[0] == 0 and per[1] == d.n > K.CHUNK and per[2:].min() >= 30 and (d.data < 0).any()
    slabs = K.slabs_of(c, slab)
    stops = []
    for i, (c0, c1) in enumerate(slabs):
        assert (n_iter[c0:c1] == n_iter[c0]).all()
        k = int(n_iter[c0])
        stops.append(k if done[i] else None)
        ran = gmax[:k, i]
        assert np.isfinite(ran).all() and np.isnan(gmax[k:, i]).all()
        if done[i]:
            assert ran[-1] <= hp.tol / 10 and (ran[:-1] >= 10 * hp.tol).all(), (i, ran)
        else:
            assert k == hp.max_iter and (ran >= 10 * hp.tol).all(), (i, ran)
    print(pair, "stopping iterations per slab (None: running at max_iter):", stops)
    stopped = {k for k in stops if k is not None}
    if len(slabs) == 1:
        assert stops == ([None] if c == 8 else [hp.max_iter])
    else:
        assert len(stopped) >= 2 and None in stops and stops[1] == 1 and max(stopped) > 1
    if pair in ((151, 8), (130, 64)):
        group = [[k for k, (c0, c1) in zip(stops, slabs) if c0 < 64 * g + 64 and c1 > 64 * g] for g in range(-(-c // 64))]
        ends = [None if None in ks else max(ks) for ks in group]
        assert ends[1] == 1 and ends[0] is not None and ends[0] > 1 and ends[2] is None  # the second group's waves return early from iteration 2 on
    if pair in K.POLLED:
        assert hp.max_iter % 3 != 0 and hp.max_iter > 3


def test_evaluate_inputs_keep_every_probability_off_the_thresholds():
    """The counts of evaluate can only be compared exactly when no event's and no zero row's probability sits on a threshold:
    at least 1e-9 away for every (case, threshold) of test_gpu_probe1d_geometry.py, as the fixtures' min_gap."""
    gaps = {}
    for i in range(len(K.CASES)):
        d = K.case_design(i)
        gaps[K.CASE_IDS[i]] = K.threshold_gap(d, *K.coefficients(d.s, d.c, K.EVAL_SEED + i))
    d = K.four_groups()
    gaps["four_groups"] = K.threshold_gap(d, *K.coefficients(d.s, d.c, K.EVAL_SEED - 1))
    print(gaps)
    assert all(g >= 1e-9 for g in gaps.values()), gaps
    assert K.THRESHOLDS == (0.2, 0.5, 0.9)
