"""CPU-only tests of the latent AUROC (include/saev_amd.h: LATENT AUROC): the entry is declared, exported and bound
with the header's types; every argument check refuses a call before anything touches a device; the numpy restatement the GPU tests
lean on (tests/latent_auroc_restatement.py) equals the pair-counting definition on the integers for every small design of
tests/latent_auroc_cases.py and reproduces fixture G29, recorded from the reference's ``mimics.scoring``; and the pieces of
``saev_amd.mimics`` that need no device reproduce the reference's task specs and defaults.

Tolerances (derived, not tuned): ``auroc`` and the supports on the float32 bits (the statistic is an integer, and both sides make
one fp64 division and one cast); a mean within (n + 2) 2^-24 (sum |a|) / n of the reference's, which sums n float32 values in
float32 -- the bound holds for any order of summation."""

import ctypes as C
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse

import latent_auroc_cases as AK
import latent_auroc_restatement as AR
from conftest import GOLDEN, ROOT

CTYPES = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double}
INVALID, UNSUPPORTED = -1, -3


def _lib():
    subprocess.run(["make", "-C", str(ROOT)], check=True, capture_output=True)
    from saev_amd import _lib

    return _lib, _lib.load()


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN / "g29_latent_auroc.npz") as z:
        return {k: z[k] for k in z.files}


def test_the_entry_is_declared_exported_and_bound_with_the_headers_types():
    lib_mod, lib = _lib()
    raw = (ROOT / "include" / "saev_amd.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name, n_args in (("saev_latent_auroc", 24), ("saev_latent_auroc_workspace_bytes", 5)):
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
    codes = {k: int(v) for k, v in re.findall(r"#define\s+(SAEV_(?:LATENT_AP|PROBE_AP|LATENT_AUROC)_ERR_\w+)\s+(\d+)\b", text)}
    assert codes["SAEV_LATENT_AUROC_ERR_ROLE"] == 4 and len(set(codes.values())) == len(codes) == 4
    assert "LATENT AUROC" in raw and "DESIGN.md 3.23" in raw


def _fake(i):
    return C.c_void_p((1 << 21) + 4096 * i)


SHAPE = dict(N=100, S=64, C=11, T=7, nnz=800)
OUTPUTS = ("auroc", "u2", "n_pos", "n_neg", "fire_pos", "fire_neg", "sum_pos", "sum_neg", "pos")
SHARED = "give the classes as class_u8 (with an optional remap) or as class_i32, one of the two"
NULL_OUT = "auroc, u2, n_pos, n_neg, fire_pos, fire_neg, sum_pos, sum_neg and pos must not be NULL"
TOO_SMALL = "workspace smaller than saev_latent_auroc_workspace_bytes(N, S, C, T, nnz)"
# the fake device pointers are never dereferenced: a launch on them would fault, and this machine has no device to launch on.
# Status and saev_last_error(NULL) word for word, the refusals shared with saev_latent_ap where they sit there, this entry's own among
# them, and the FIRST refusal of two bad arguments at once
BAD = [
    ("negative_n", dict(N=-1), INVALID, "negative size"), ("negative_nnz", dict(nnz=-1), INVALID, "negative size"),
    ("zero_rows", dict(N=0), INVALID, "N and S must be at least 1"), ("zero_latents", dict(S=0), INVALID, "N and S must be at least 1"),
    ("rows_2_31", dict(N=1 << 31), UNSUPPORTED, "N, S and nnz must stay below 2^31"), ("nnz_2_31", dict(nnz=1 << 31), UNSUPPORTED, "N, S and nnz must stay below 2^31"),
    ("no_classes", dict(C=0), UNSUPPORTED, "the number of classes must lie in [1, 4096]"),
    ("too_many_classes", dict(C=4097), UNSUPPORTED, "the number of classes must lie in [1, 4096]"),
    ("no_tasks", dict(T=0), UNSUPPORTED, "the number of tasks must lie in [1, 4096]"),
    ("negative_tasks", dict(T=-3), UNSUPPORTED, "the number of tasks must lie in [1, 4096]"),
    ("too_many_tasks", dict(T=4097), UNSUPPORTED, "the number of tasks must lie in [1, 4096]"),
    ("null_row_ptr", dict(row_ptr=None), INVALID, "row_ptr is NULL"), ("null_indices", dict(indices=None), INVALID, "indices and data come with nnz > 0"),
    ("null_data", dict(data=None), INVALID, "indices and data come with nnz > 0"),
    ("no_label_form", dict(u8=None), INVALID, SHARED), ("both_label_forms", dict(i32=_fake(8)), INVALID, SHARED),
    ("remap_without_bytes", dict(u8=None, i32=_fake(8), remap=_fake(9)), INVALID, "remap goes with class_u8"),
    ("null_role", dict(role=None), INVALID, "role must not be NULL"),
    *[(f"null_{name}", {name: None}, INVALID, NULL_OUT) for name in OUTPUTS],
    ("workspace_null", dict(ws=None), INVALID, TOO_SMALL), ("workspace_too_small", dict(ws_short=1), INVALID, TOO_SMALL),
    ("workspace_of_latent_ap", dict(ws_latent_ap=True), INVALID, TOO_SMALL),
    ("workspace_misaligned", dict(ws=C.c_void_p((1 << 20) + 8)), INVALID, "workspace must be 256-byte aligned"),
    ("size_before_tasks", dict(N=0, T=0), INVALID, "N and S must be at least 1"),
    ("classes_before_tasks", dict(C=4097, T=4097), UNSUPPORTED, "the number of classes must lie in [1, 4096]"),
    ("tasks_before_pointers", dict(T=4097, row_ptr=None), UNSUPPORTED, "the number of tasks must lie in [1, 4096]"),
    ("labels_before_role", dict(u8=None, role=None), INVALID, SHARED),
    ("role_before_outputs", dict(role=None, u2=None), INVALID, "role must not be NULL"),
    ("outputs_before_workspace", dict(sum_neg=None, ws_short=1), INVALID, NULL_OUT),
    ("size_before_alignment", dict(ws=C.c_void_p((1 << 20) + 8), ws_short=1), INVALID, TOO_SMALL),
]


def _call(lib, over):
    a = dict(SHAPE, row_ptr=_fake(0), indices=_fake(1), data=_fake(2), u8=_fake(3), remap=None, i32=None, role=_fake(10), ws=C.c_void_p(1 << 20), ws_short=0,
             ws_latent_ap=False, **{name: _fake(20 + i) for i, name in enumerate(OUTPUTS)})
    a.update(over)
    need = lib.saev_latent_auroc_workspace_bytes(100, 64, 11, 7, 800)
    if a["ws_latent_ap"]:
        need = lib.saev_latent_ap_workspace_bytes(100, 64, 11, 800)
    return lib.saev_latent_auroc(a["row_ptr"], a["indices"], a["data"], a["nnz"], a["N"], a["S"], a["C"], a["u8"], a["remap"], a["i32"], a["role"], a["T"],
                                 *[a[name] for name in OUTPUTS], a["ws"], need - a["ws_short"], None)


@pytest.mark.parametrize("case", BAD, ids=[c[0] for c in BAD])
def test_the_call_refuses_bad_arguments_without_a_device_in_order(case):
    _, lib = _lib()
    _, over, status, text = case
    rc = _call(lib, over)
    assert rc == status, (rc, lib.saev_last_error(None))
    assert lib.saev_last_error(None).decode() == "saev_latent_auroc: " + text


def test_workspace_begins_with_latent_aps_and_adds_the_role_table():
    lib_mod, lib = _lib()
    for n, s, c, t, nnz in ((100, 64, 11, 7, 800), (1, 1, 1, 1, 0), (70_000, 48, 5, 3, 2_240_000), (300, 5, 4096, 4096, 600), (300, 5, 300, 65, 600)):
        ap, own = lib.saev_latent_ap_workspace_bytes(n, s, c, nnz), lib.saev_latent_auroc_workspace_bytes(n, s, c, t, nnz)
        L = lib_mod.SaevLatentAPLayout()
        assert lib.saev_latent_ap_layout_of(n, s, c, nnz, C.byref(L)) == 0 and L.total_bytes == ap
        table = (c + 1) * (-(-t // 64) * 64)
        assert own == ap + -(-table // 256) * 256 and own >= ap and own % 256 == 0
    for bad in ((0, 64, 11, 7, 800), (100, 64, 4097, 7, 800), (100, 64, 11, 0, 800), (100, 64, 11, 4097, 800), (100, 64, 11, 7, 1 << 31)):
        assert lib.saev_latent_auroc_workspace_bytes(*bad) == -1


def test_python_surface_refuses_host_tensors_and_bad_arguments():
    import torch
    from saev_amd import engine

    z, i, v = torch.zeros(2, dtype=torch.int64), torch.zeros(0, dtype=torch.int32), torch.zeros(0)
    lab, roles = torch.zeros(1, dtype=torch.int32), torch.ones(1, 1, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        engine.latent_auroc(z, i, v, 1, 1, 1, labels=lab, roles=roles)
    with pytest.raises(ValueError, match="n_classes"):
        engine.latent_auroc(z, i, v, 1, 1, 4097, labels=lab, roles=roles)
    with pytest.raises(ValueError, match="roles must be"):
        engine.latent_auroc(z, i, v, 1, 1, 1, labels=lab, roles=roles.to(torch.int32))
    with pytest.raises(ValueError, match="roles must be"):
        engine.latent_auroc(z, i, v, 1, 1, 1, labels=lab, roles=roles[0])
    with pytest.raises(ValueError, match="n_tasks"):
        engine.latent_auroc(z, i, v, 1, 1, 1, labels=lab, roles=torch.ones(4097, 1, dtype=torch.uint8))
    with pytest.raises(ValueError, match="n_tasks"):
        engine.latent_auroc(z, i, v, 1, 1, 1, labels=lab, roles=torch.ones(0, 1, dtype=torch.uint8))
    assert engine.LatentAUROCResult._ERRORS[4] == "a role byte is above 2" and set(engine.LatentAUROCResult._ERRORS) == {1, 2, 4}


# ---------------------------------------------------------------- the restatement ---------------------------------------------------------

def _args(d):
    return d["indptr"], d["indices"], d["data"], d["n"], d["s"], d["cls"], d["roles"]


@pytest.mark.parametrize("name", list(AK.SMALL))
def test_restatement_equals_the_pair_counting_definition(name):
    d = AK.SMALL[name]()
    got = AR.one_walk(*_args(d))
    np.testing.assert_array_equal(got["u2"], AR.by_pairs(*_args(d)))
    ranks = AR.by_ranks(*_args(d))
    for key in ("u2", "n_pos", "n_neg", "fire_pos", "fire_neg"):
        np.testing.assert_array_equal(got[key], ranks[key])
    assert np.array_equal(got["sum_pos"].view(np.int64), ranks["sum_pos"].view(np.int64))
    void = (got["n_pos"] == 0) | (got["n_neg"] == 0)
    assert np.isnan(got["auroc"][:, void]).all() and (got["u2"][:, void] == 0).all()
    ok = got["auroc"][:, ~void]
    assert ((ok >= 0) & (ok <= 1)).all()
    n_events = np.bincount(d["indices"][d["data"] != 0], minlength=d["s"])
    assert (ok[n_events == 0] == 0.5).all()


def test_designs_hold_what_they_are_said_to_hold():
    from latent_ap_restatement import sorted_events

    d = AK.kinds()
    got = AR.one_walk(*_args(d))
    n_events = np.bincount(d["indices"][d["data"] != 0], minlength=d["s"])
    neg = np.bincount(d["indices"][d["data"] < 0], minlength=d["s"])
    assert (n_events == 0).any() and (n_events == d["n"]).sum() >= 3 and ((neg > 0) & (neg < n_events)).any() and (neg == n_events)[n_events > 0].any()
    assert np.isinf(d["data"]).sum() == 4 and (d["data"] == 0).sum() == 2 and (d["cls"] == -1).any()
    assert got["n_pos"][3] == 0 and got["n_neg"][3] > 0 and got["n_neg"][4] == 0 and got["n_pos"][4] > 0 and got["n_pos"][6] == got["n_neg"][6] == 0
    assert d["roles"][1, 0] == 0 and d["roles"][0, 0] == 2 and d["roles"][0, 1] == 1 and d["roles"][1, 1] == 2
    assert np.isnan(got["sum_pos"]).any() or np.isnan(got["sum_neg"]).any()  # +Inf and -Inf met in one sum
    c = AK.chunks()
    starts, _, val, _ = sorted_events(c["indptr"], c["indices"], c["data"], c["s"])
    v0 = val[starts[0]:starts[1]]
    assert tuple(np.diff(np.flatnonzero(np.concatenate([[True], v0[1:] != v0[:-1], [True]])))) == AK.CHUNK_GROUPS
    assert set(AK.CHUNK_GROUPS) >= {1, 2, 63, 64, 65, 130} and np.cumsum(AK.CHUNK_GROUPS)[1] == 64 and np.cumsum(AK.CHUNK_GROUPS)[2] == 128
    assert np.diff(starts).tolist() == [sum(AK.CHUNK_GROUPS), 130, c["n"], 0, 140] and len(np.unique(val[starts[2]:starts[3]])) == 1
    shapes = [AK.GRID[k] for k in AK.GRID]
    assert {s[3] for s in shapes} >= {1, 64, 65, 130} and {s[2] for s in shapes} >= {1, 255, 256, 300, 4096} and {s[1] for s in shapes} == {1, 5}
    labels, remap = AK.as_bytes(d)
    assert (remap == -1).sum() == 256 - d["c"] and np.array_equal(remap[labels], d["cls"])
    one = AK.one_latent(d, 7)
    assert one["s"] == 1 and len(one["data"]) == d["n"] and np.array_equal(AR.one_walk(*_args(one))["u2"][0], got["u2"][7])


# ---------------------------------------------------------------- fixture G29 ------------------------------------------------------------

def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).reshape(-1).view(np.uint32)


def test_restatement_against_the_references_recorded_values(golden):
    from saev_amd import mimics

    assert (GOLDEN / "g29_latent_auroc.npz").stat().st_size < 100_000
    designs = AK.g29_designs(golden)
    assert len(designs) == 3
    for d in designs:
        assert (d["data"] < 0).any() and (d["data"] == 0).any() and np.signbit(d["data"][d["data"] == 0]).any()
        assert d["pooled"].dtype == np.float32 and (d["pooled"] >= 0).all() and (d["pooled"][1] == 0).all()
        specs = mimics.build_task_specs(d["sv"], pair_specs=d["pair_specs"], views=d["views"], min_samples=d["min_samples"])
        cls, roles = mimics.task_classes(specs, d["n_images"])
        assert roles.shape == (4, 8) and (cls == -1).any() and set(cls.tolist()) == set(range(-1, 8))
        p = scipy.sparse.csr_matrix(d["pooled"])
        own = AR.one_walk(p.indptr, p.indices, p.data, d["n_images"], d["s"], cls, roles)
        np.testing.assert_array_equal(own["n_pos"], d["n_pos"])
        np.testing.assert_array_equal(own["n_neg"], d["n_neg"])
        assert d["col_auroc"].dtype == np.float32 and np.array_equal(_bits(own["auroc"].T), d["col_auroc"].view(np.uint32))
        assert len(np.unique(d["col_auroc"])) > 50 and (d["col_auroc"] == 0.5).any()
        for role, side, n in (("neg", "erato", own["n_neg"]), ("pos", "melpomene", own["n_pos"])):
            nf = n[:, None].astype(np.float64)
            assert np.array_equal(_bits(own[f"fire_{role}"].T / nf), d[f"col_support_{side}"].view(np.uint32))
            miss = np.abs((own[f"sum_{role}"].T / nf).reshape(-1) - d[f"col_mean_act_{side}"].astype(np.float64))
            assert (miss <= AR.mean_bound(nf, own[f"abs_{role}"].T).reshape(-1)).all()
        assert d["col_feature_id"].dtype == np.int32 and np.array_equal(d["col_feature_id"], np.tile(np.arange(d["s"], dtype=np.int32), 4))
        assert d["col_task"].tolist() == np.repeat(d["task_names"], d["s"]).tolist() and set(d["col_run_id"].tolist()) == {"run0"}


def test_build_task_specs_names_and_counts_against_the_reference(golden):
    from saev_amd import mimics

    for d in AK.g29_designs(golden):
        specs = mimics.build_task_specs(d["sv"], pair_specs=d["pair_specs"], views=d["views"], min_samples=d["min_samples"])
        assert [s.name for s in specs] == d["task_names"].tolist() and len(specs) == 4 < len(d["pair_specs"]) * len(d["views"])  # a pair is dropped
        assert [s.n_pos for s in specs] == d["n_pos"].tolist() and [s.n_neg for s in specs] == d["n_neg"].tolist()
        for s in specs:
            assert s.include.dtype == bool and s.include.sum() == s.n_pos + s.n_neg and s.binary.dtype == np.int8
            assert np.array_equal(s.binary.astype(bool), s.melp_mask) and not (s.melp_mask & s.erato_mask).any()
        assert any(lbl.startswith("notabilis") for lbl in d["sv"]) and not any("notabilis" in s.name for s in specs)
        keep_all = mimics.build_task_specs(d["sv"], pair_specs=d["pair_specs"], views=d["views"], min_samples=0)
        assert len(keep_all) == 6


def test_max_pool_csr_restated_against_the_references_pooled_values(golden):
    """The clamp at 0 that ``mimics.max_pool_csr`` applies to ``engine.pool_images(..., "max")``, on the pooling's restatement."""
    import sparse_linear_restatement as SR

    for d in AK.g29_designs(golden):
        raw = SR.pool_images(d["indptr"], d["indices"], d["data"], d["n_images"], d["tpi"], d["s"], "max")
        assert (raw < 0).any()  # a latent stored in every patch of an image with negative values only
        assert np.array_equal(np.maximum(raw, 0) + np.float32(0), d["pooled"])


def test_task_names_groupings_and_defaults(tmp_path):
    import dataclasses

    from saev_amd import mimics
    from saev_amd.data import write_shards

    assert mimics.parse_pair_spec(" lativitta : malleti ") == ("lativitta", "malleti")
    for bad in ("lativitta", ":malleti", "lativitta:"):
        with pytest.raises(AssertionError, match="Pair spec"):
            mimics.parse_pair_spec(bad)
    name = mimics.get_task_name("cyrbia", "cythera", "ventral")
    assert name == "cyrbia_ventral_vs_cythera_ventral" and mimics.parse_task_name(name) == ("cyrbia", "cythera", "ventral")
    with pytest.raises(AssertionError, match="mismatched views"):
        mimics.parse_task_name("cyrbia_ventral_vs_cythera_dorsal")
    with pytest.raises(AssertionError, match="Task must match"):
        mimics.parse_task_name("cyrbia-ventral")
    g = mimics.make_label_grouping(name)
    assert (g.name, g.source_col, g.groups) == (name, "subspecies_view", {"erato": ["cyrbia_ventral"], "melpomene": ["cythera_ventral"]})
    assert mimics.DEFAULT_PAIR_SPECS == ["lativitta:malleti", "cyrbia:cythera", "notabilis:plesseni", "hydara:melpomene", "venus:vulcanus", "demophoon:rosina",
                                         "phyllis:nanna", "erato:thelxiopeia"] and mimics.DEFAULT_VIEWS == ["dorsal", "ventral"]
    cfg = mimics.Config()
    assert (cfg.min_samples, cfg.feature_chunk, cfg.force_recompute, cfg.slurm_acct, cfg.slurm_partition, cfg.n_hours, cfg.mem_gb, cfg.log_to) == \
        (10, 1024, False, "", "", 4.0, 80, "logs")
    assert cfg.run_ids == [] and cfg.views == ["dorsal", "ventral"] and cfg.pair_specs == [tuple(p.split(":")) for p in mimics.DEFAULT_PAIR_SPECS[:5]]
    assert [f.name for f in dataclasses.fields(cfg)] == ["run_root_dpath", "shards_dpath", "run_ids", "pair_specs", "views", "min_samples", "feature_chunk",
                                                         "force_recompute", "slurm_acct", "slurm_partition", "n_hours", "mem_gb", "log_to"]
    assert mimics.get_scores_fpath(tmp_path, run_id="r", shard_id="s") == tmp_path / "r" / "inference" / "s" / "cambridge-mimics.parquet"

    sv = ["a_dorsal"] * 3 + ["b_dorsal"] * 2 + ["a_ventral"] * 4 + ["b_ventral"] * 4 + ["c_dorsal"]
    shards = write_shards(tmp_path / "s", np.zeros((len(sv), 1, 2, 4), dtype=np.float32))
    (shards / "image_labels.csv").write_text("stem,subspecies_view\n" + "".join(f"i{k},{lbl}\n" for k, lbl in enumerate(sv)))
    dcfg = mimics.DecideTaskSpecsConfig(shards_dpath=shards, pair_specs=["a:b", "c:d", "a:b"], min_samples_per_class=3)
    specs, rows = mimics.decide_task_specs(dcfg)
    assert [s.task_name for s in specs] == ["a_ventral_vs_b_ventral"] and specs[0].keep and (specs[0].n_erato, specs[0].n_melpomene, specs[0].n_total) == (4, 4, 8)
    # the reference's sort: keep descending, n_total descending, task_name ascending
    assert [r["task_name"] for r in rows] == ["a_ventral_vs_b_ventral", "a_dorsal_vs_b_dorsal", "c_dorsal_vs_d_dorsal", "c_ventral_vs_d_ventral"]
    assert list(rows[0]) == ["task_name", "n_erato", "n_melpomene", "n_total", "keep", "source_col", "erato_label", "melpomene_label"]
    assert rows[1] == {"task_name": "a_dorsal_vs_b_dorsal", "n_erato": 3, "n_melpomene": 2, "n_total": 5, "keep": False, "source_col": "subspecies_view",
                       "erato_label": "a_dorsal", "melpomene_label": "b_dorsal"}
    assert len(mimics.decide_task_specs(dataclasses.replace(dcfg, include_filtered=True))[0]) == 4
    # score_run without the codes: None, as the reference
    assert mimics.score_run("nope", run_root_dpath=tmp_path, shard_id=shards.name, task_specs=[], n_images=len(sv)) is None
