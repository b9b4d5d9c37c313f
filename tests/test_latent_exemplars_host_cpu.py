"""CPU-only tests of LATENT EXEMPLARS (include/saev_amd.h): the entries are declared, exported and bound with the
header's types and the out struct has the header's layout; every argument check refuses a call before anything touches a device,
in the order the header states; the workspace has the size of its layout; the numpy restatement the GPU tests lean on
(tests/latent_exemplars_restatement.py) agrees with a brute-force sort of the dense pooled matrix and with examples counted by hand;
every case of tests/latent_exemplars_cases.py holds what it is said to hold; and the host pieces of ``saev_amd.exemplars`` are right.

Tolerances: none."""

import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import latent_exemplars_cases as K
import latent_exemplars_restatement as R
from conftest import ROOT
from saev_amd.engine import latent_exemplars, latent_patch_rows  # noqa: F401  (without the feature nothing here can run)

CTYPES = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double, "float": C.c_float}
INVALID, UNSUPPORTED = -1, -3


def _lib():
    subprocess.run(["make", "-C", str(ROOT)], check=True, capture_output=True)
    from saev_amd import _lib

    return _lib, _lib.load()


def test_the_entries_are_declared_exported_and_bound_with_the_headers_types():
    from saev_amd import engine

    assert callable(engine.latent_exemplars) and callable(engine.latent_patch_rows)
    lib_mod, lib = _lib()
    raw = (ROOT / "include" / "saev_amd.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name, n_args in (("saev_latent_exemplars", 15), ("saev_latent_exemplars_workspace_bytes", 4), ("saev_latent_patch_rows", 13)):
        m = re.search(r"(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, f"{name} is not declared"
        args = []
        for a in m.group(2).split(","):
            decl = re.sub(r"\w+\s*$", "", a.strip()).replace("const", "").strip()
            args.append(C.c_void_p if "*" in decl else CTYPES[decl.split()[0]])
        want_res, want_args = lib_mod._SIGNATURES[name]
        bound = [C.c_void_p if a is C.POINTER(lib_mod.SaevLatentExemplarsOut) else a for a in want_args]
        assert want_res is CTYPES[m.group(1)] and bound == args and len(args) == n_args
        assert hasattr(lib, name) and name in lib_mod.EXPORTED_SYMBOLS
    assert lib.saev_abi_version() == 12 and lib_mod.ABI_VERSION == 12  # additive entries: the version stays
    codes = {k: int(v) for k, v in re.findall(r"#define\s+(SAEV_LATENT_EXEMPLARS_ERR_\w+)\s+(\d+)\b", text)}
    assert codes == {"SAEV_LATENT_EXEMPLARS_ERR_GROUP": R.ERR_GROUP, "SAEV_LATENT_EXEMPLARS_ERR_LATENT": R.ERR_LATENT, "SAEV_LATENT_EXEMPLARS_ERR_IMAGE": R.ERR_IMAGE}
    assert "LATENT EXEMPLARS" in raw and "DESIGN.md 3.28" in raw
    assert "exemplars.hip" in (ROOT / "Makefile").read_text()


def test_the_out_struct_has_the_headers_layout():
    lib_mod, _ = _lib()
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "saev_amd.h").read_text(), flags=re.S)
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*saev_latent_exemplars_out\s*;", text)
    assert m, "saev_latent_exemplars_out is not declared"
    fields = [(re.search(r"(\w+)\s*$", f).group(1), "*" in f, f.split()[0]) for f in (f.strip() for f in m.group(1).split(";")) if f]
    struct = lib_mod.SaevLatentExemplarsOut
    assert [n for n, _, _ in fields] == [n for n, _ in struct._fields_] == ["struct_size", "reserved", *R.ARRAYS]
    for (name, pointer, ctype), (_, bound) in zip(fields, struct._fields_):
        assert bound is (C.c_void_p if pointer else CTYPES[ctype]), name
    assert C.sizeof(struct) == 8 + 8 * len(R.ARRAYS) and struct.n_group_images.offset == 8 and struct.silent_img.offset == 8 * len(R.ARRAYS)
    assert struct.OUTPUTS == R.ARRAYS


def _fake(i):
    return C.c_void_p((1 << 21) + 4096 * i)


SHAPE = dict(nnz=800, n_images=10, T=12, S=64, G=5, k=8, thr=0.0)
WHO = "saev_latent_exemplars: "
TOO_SMALL = "workspace smaller than saev_latent_exemplars_workspace_bytes(nnz, S, n_images, G)"
BELOW = "N, S and nnz must stay below 2^31"
ZERO = "N and S must be at least 1"
GROUPS = "the number of groups must lie in [1, 64]"
LISTS_K = "k must lie in [1, 32]"
TOKENS = "T must lie in [1, 4096]"
ROWS = "n_images * T must stay below 2^31"
SLOTS = "S * G * k must stay below 2^31"
NO_OUT = "no saev_latent_exemplars_out (or its struct_size is unset)"
NULL_OUT = "every output of saev_latent_exemplars_out must be set"
# the fake device pointers are never dereferenced: a launch on them would fault, and this machine has no device to launch on.  Status
# and saev_last_error(NULL) word for word, then the FIRST refusal of two bad arguments at once, in the header's order
BAD = [
    ("negative_images", dict(n_images=-1), INVALID, "negative size"), ("negative_latents", dict(S=-1), INVALID, "negative size"),
    ("negative_nnz", dict(nnz=-1), INVALID, "negative size"),
    ("images_2_31", dict(n_images=1 << 31), UNSUPPORTED, BELOW), ("latents_2_31", dict(S=1 << 31), UNSUPPORTED, BELOW), ("nnz_2_31", dict(nnz=1 << 31), UNSUPPORTED, BELOW),
    ("zero_images", dict(n_images=0), INVALID, ZERO), ("zero_latents", dict(S=0), INVALID, ZERO),
    ("no_groups", dict(G=0), UNSUPPORTED, GROUPS), ("negative_groups", dict(G=-1), UNSUPPORTED, GROUPS), ("too_many_groups", dict(G=65), UNSUPPORTED, GROUPS),
    ("k_0", dict(k=0), UNSUPPORTED, LISTS_K), ("k_33", dict(k=33), UNSUPPORTED, LISTS_K), ("k_negative", dict(k=-8), UNSUPPORTED, LISTS_K),
    ("t_0", dict(T=0), UNSUPPORTED, TOKENS), ("t_4097", dict(T=4097), UNSUPPORTED, TOKENS),
    ("rows_2_31", dict(n_images=1 << 19, T=4096), UNSUPPORTED, ROWS),
    ("slots_2_31", dict(S=1 << 20, G=64, k=32), UNSUPPORTED, SLOTS),
    ("thr_negative", dict(thr=-0.5), INVALID, "thr must be at least 0"), ("thr_nan", dict(thr=float("nan")), INVALID, "thr must be at least 0"),
    ("null_row_ptr", dict(row_ptr=None), INVALID, "row_ptr is NULL"), ("null_indices", dict(indices=None), INVALID, "indices and data come with nnz > 0"),
    ("null_data", dict(data=None), INVALID, "indices and data come with nnz > 0"),
    ("null_groups", dict(group=None), INVALID, "group_i32 must not be NULL"),
    ("no_out", dict(out=None), INVALID, NO_OUT), ("out_size_unset", dict(struct_size=0), INVALID, NO_OUT),
    ("out_cut_short", dict(struct_size=8 + 8 * 5), INVALID, NULL_OUT),
    *[(f"null_{name}", {name: None}, INVALID, NULL_OUT) for name in R.ARRAYS],
    ("workspace_null", dict(ws=None), INVALID, TOO_SMALL), ("workspace_too_small", dict(ws_short=1), INVALID, TOO_SMALL),
    ("workspace_misaligned", dict(ws=C.c_void_p((1 << 20) + 8)), INVALID, "workspace must be 256-byte aligned"),
    ("negative_before_2_31", dict(nnz=-1, S=1 << 31), INVALID, "negative size"),
    ("below_2_31_before_zero", dict(n_images=0, nnz=1 << 31), UNSUPPORTED, BELOW),
    ("zero_before_groups", dict(S=0, G=65), INVALID, ZERO),
    ("groups_before_k", dict(G=65, k=0), UNSUPPORTED, GROUPS),
    ("k_before_t", dict(k=33, T=0), UNSUPPORTED, LISTS_K),
    ("t_before_rows", dict(T=4097, n_images=1 << 20), UNSUPPORTED, TOKENS),
    ("rows_before_slots", dict(n_images=1 << 19, T=4096, S=1 << 20, G=64, k=32), UNSUPPORTED, ROWS),
    ("slots_before_thr", dict(S=1 << 20, G=64, k=32, thr=-1.0), UNSUPPORTED, SLOTS),
    ("thr_before_pointers", dict(thr=-1.0, row_ptr=None), INVALID, "thr must be at least 0"),
    ("row_ptr_before_groups", dict(row_ptr=None, group=None), INVALID, "row_ptr is NULL"),
    ("groups_before_out", dict(group=None, out=None), INVALID, "group_i32 must not be NULL"),
    ("outputs_before_workspace", dict(bot_val=None, ws_short=1), INVALID, NULL_OUT),
    ("size_before_alignment", dict(ws=C.c_void_p((1 << 20) + 8), ws_short=1), INVALID, TOO_SMALL),
]


def _call(lib_mod, lib, over):
    a = dict(SHAPE, row_ptr=_fake(0), indices=_fake(1), data=_fake(2), group=_fake(3), ws=C.c_void_p(1 << 20), ws_short=0, out=True,
             struct_size=C.sizeof(lib_mod.SaevLatentExemplarsOut), **{name: _fake(20 + i) for i, name in enumerate(R.ARRAYS)})
    a.update(over)
    struct = lib_mod.SaevLatentExemplarsOut(struct_size=a["struct_size"], **{name: a[name] for name in R.ARRAYS})
    need = lib.saev_latent_exemplars_workspace_bytes(800, 64, 10, 5)
    return lib.saev_latent_exemplars(a["row_ptr"], a["indices"], a["data"], a["nnz"], a["group"], a["n_images"], a["T"], a["S"], a["G"], a["k"], a["thr"],
                                     C.byref(struct) if a["out"] else None, a["ws"], need - a["ws_short"], None)


@pytest.mark.parametrize("case", BAD, ids=[c[0] for c in BAD])
def test_the_call_refuses_bad_arguments_without_a_device_in_order(case):
    lib_mod, lib = _lib()
    _, over, status, text = case
    rc = _call(lib_mod, lib, over)
    assert rc == status, (rc, lib.saev_last_error(None))
    assert lib.saev_last_error(None).decode() == WHO + text


def test_no_entries_and_the_limits_themselves_are_not_refused_by_the_checks():
    """nnz = 0 needs no indices, and G = 64, k = 32, T = 4096 are inside the limits: the calls get as far as the workspace check."""
    lib_mod, lib = _lib()
    for over in (dict(nnz=0, indices=None, data=None, ws=None), dict(G=64, k=32, T=4096, ws=None), dict(S=(1 << 20) - 1, G=64, k=32, ws=None),
                 dict(n_images=(1 << 19) - 1, T=4096, ws=None)):
        assert _call(lib_mod, lib, over) == INVALID and lib.saev_last_error(None).decode() == WHO + TOO_SMALL


ROWS_WHO = "saev_latent_patch_rows: "
ROWS_SHAPE = dict(nnz=800, n_images=10, T=12, S=64, Q=5)
ROWS_BAD = [
    ("negative_images", dict(n_images=-1), INVALID, "negative size"), ("latents_2_31", dict(S=1 << 31), UNSUPPORTED, BELOW),
    ("zero_latents", dict(S=0), INVALID, ZERO), ("t_0", dict(T=0), UNSUPPORTED, TOKENS), ("t_4097", dict(T=4097), UNSUPPORTED, TOKENS),
    ("rows_2_31", dict(n_images=1 << 19, T=4096), UNSUPPORTED, ROWS), ("negative_queries", dict(Q=-1), INVALID, "negative size"),
    ("values_2_31", dict(Q=1 << 28), UNSUPPORTED, "Q * T must stay below 2^31"),
    ("null_row_ptr", dict(row_ptr=None), INVALID, "row_ptr is NULL"), ("null_data", dict(data=None), INVALID, "indices and data come with nnz > 0"),
    *[(f"null_{name}", {name: None}, INVALID, "q_latent, q_image, out and err must not be NULL") for name in ("q_latent", "q_image", "out", "err")],
    ("zero_before_t", dict(n_images=0, T=0), INVALID, ZERO), ("t_before_queries", dict(T=4097, Q=-1), UNSUPPORTED, TOKENS),
    ("queries_before_pointers", dict(Q=-1, row_ptr=None), INVALID, "negative size"), ("row_ptr_before_out", dict(row_ptr=None, out=None), INVALID, "row_ptr is NULL"),
]


def _call_rows(lib, over):
    a = dict(ROWS_SHAPE, row_ptr=_fake(0), indices=_fake(1), data=_fake(2), q_latent=_fake(3), q_image=_fake(4), out=_fake(5), err=_fake(6))
    a.update(over)
    return lib.saev_latent_patch_rows(a["row_ptr"], a["indices"], a["data"], a["nnz"], a["n_images"], a["T"], a["S"], a["q_latent"], a["q_image"], a["Q"],
                                      a["out"], a["err"], None)


@pytest.mark.parametrize("case", ROWS_BAD, ids=[c[0] for c in ROWS_BAD])
def test_patch_rows_refuses_bad_arguments_without_a_device_in_order(case):
    _, lib = _lib()
    _, over, status, text = case
    rc = _call_rows(lib, over)
    assert rc == status, (rc, lib.saev_last_error(None))
    assert lib.saev_last_error(None).decode() == ROWS_WHO + text


def test_patch_rows_without_queries_returns_ok_and_touches_nothing():
    _, lib = _lib()
    assert _call_rows(lib, dict(Q=0)) == 0 and _call_rows(lib, dict(Q=0, row_ptr=None, q_latent=None, out=None, err=None)) == 0
    assert _call_rows(lib, dict(Q=0, T=0)) == UNSUPPORTED  # the shape is checked all the same


def test_workspace_size():
    _, lib = _lib()
    size = lib.saev_latent_exemplars_workspace_bytes
    r256 = lambda b: -(-max(b, 1) // 256) * 256  # noqa: E731
    for nnz, s, n_images, g in ((800, 64, 10, 5), (0, 1, 1, 1), (1 << 25, 16384, 4096, 16), (600, 1000, 300, 64), (5, 70_001, 2, 1), (100, 3, 100_000, 2)):
        parts = max(1, min(1024, -(-nnz // 64), max(1, (1 << 26) // s)))
        want = 256 + r256(8 * (s + 1)) + r256(4 * s) + r256(4 * parts * s) + 3 * r256(4 * nnz) + 2 * r256(4 * n_images) + r256(4 * 65)
        assert size(nnz, s, n_images, g) == want and want % 256 == 0
    for bad in ((-1, 64, 10, 5), (1 << 31, 64, 10, 5), (800, 0, 10, 5), (800, 1 << 31, 10, 5), (800, 64, 0, 5), (800, 64, 1 << 31, 5), (800, 64, 10, 0),
                (800, 64, 10, 65), (800, 64, 10, -1)):
        assert size(*bad) == -1, bad
    assert size(800, 64, 10, 64) > 0 and size((1 << 31) - 1, 64, 10, 5) > 0


def test_python_surface_refuses_host_tensors_and_bad_arguments():
    import torch
    from saev_amd import engine

    z, i, v = torch.zeros(5, dtype=torch.int64), torch.zeros(0, dtype=torch.int32), torch.zeros(0)
    ok = dict(n_images=1, tokens_per_image=4, n_latents=3, groups=torch.zeros(1, dtype=torch.int32), n_groups=1, k=8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        engine.latent_exemplars(z, i, v, **ok)
    for over, match in ((dict(tokens_per_image=0), "tokens_per_image"), (dict(tokens_per_image=4097), "tokens_per_image"), (dict(n_groups=65), "n_groups"),
                        (dict(n_groups=0), "n_groups"), (dict(k=0), "unsupported k"), (dict(k=33), "unsupported k"), (dict(n_latents=0), "n_latents"),
                        (dict(n_images=0), "n_images"), (dict(n_images=1 << 29), "n_images"), (dict(n_latents=1 << 28), "below 2\\^31"),
                        (dict(threshold=-1.0), "threshold"), (dict(threshold=float("nan")), "threshold")):
        with pytest.raises(ValueError, match=match):
            engine.latent_exemplars(z, i, v, **dict(ok, **over))
    assert engine.LatentExemplarsResult._ERRORS == {1: "a group id lies outside [-1, n_groups)", 2: "a column index lies outside [0, n_latents)"}
    assert engine.LatentExemplarsResult.ARRAYS == R.ARRAYS
    q = torch.zeros(2, dtype=torch.int32)
    rows = dict(n_images=1, tokens_per_image=4, n_latents=3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        engine.latent_patch_rows(z, i, v, q, q, **rows)
    for args, over, match in (((q, q[:1]), {}, "one shape"), ((q.float(), q), {}, "int32 or int64"), ((q, q), dict(tokens_per_image=0), "tokens_per_image"),
                              ((q, q), dict(n_latents=0), "n_latents"), ((q, q), dict(n_images=1 << 29), "n_images")):
        with pytest.raises(ValueError, match=match):
            engine.latent_patch_rows(z, i, v, *args, **dict(rows, **over))


# ---------------------------------------------------------------- the restatement ---------------------------------------------------------

def _brute_force(c):
    """From the dense pooled (n_images, S) matrix by sorting (key, image) tuples in Python: the lists, the counts, the silent images."""
    n, t, s, g, k = c["n_images"], c["t"], c["s"], c["g"], c["k"]
    rows, lats, vals = R.events(c["indptr"], c["indices"], c["data"], t, s, c["groups"], c["thr"])
    pooled = np.full((n, s), -np.inf, dtype=np.float32)
    np.maximum.at(pooled, (rows // t, lats), vals)
    patch = np.full((n, s), -1, dtype=np.int64)
    for r, j, v in sorted(zip(rows.tolist(), lats.tolist(), vals.tolist()), reverse=True):  # descending rows: the lowest patch is written last
        if v == pooled[r // t, j]:
            patch[r // t, j] = r % t
    fires = np.zeros((n, s), dtype=bool)
    fires[rows // t, lats] = True
    out = R.restate(c["indptr"][:1].repeat(len(c["indptr"])), c["indices"][:0], c["data"][:0], n_images=n, t=t, s=s, groups=c["groups"], g=g, k=k)
    for j in range(s):
        for q in range(g):
            mem = [i for i in range(n) if c["groups"][i] == q]
            f = [i for i in mem if fires[i, j]]
            out["n_fire"][j, q] = len(f)
            for end, sign in (("top", -1.0), ("bot", 1.0)):
                for slot, i in enumerate(sorted(f, key=lambda i: (sign * float(pooled[i, j]), i))[:k]):
                    out[end + "_val"][j, q, slot], out[end + "_img"][j, q, slot], out[end + "_patch"][j, q, slot] = pooled[i, j], i, patch[i, j]
            silent = [i for i in mem if not fires[i, j]][:k]
            out["silent_img"][j, q] = silent + [-1] * (k - len(silent))
    return out


@pytest.mark.parametrize("name", [n for n in K.SMALL if n != "wide"])
def test_restatement_equals_a_brute_force_sort_of_the_pooled_matrix(name):
    c = K.SMALL[name]()
    got, want = R.restate(**c), _brute_force(c)
    for key in R.ARRAYS:
        assert got[key].dtype == want[key].dtype and np.array_equal(R.bits(got[key]), R.bits(want[key])), key
    # what holds of every result: the lists are as long as they can be, the padding is 0.0 / -1 / -1
    n_g = got["n_group_images"][None, :]
    held = lambda a: (a >= 0).sum(axis=2)  # noqa: E731
    assert (held(got["top_img"]) == np.minimum(c["k"], got["n_fire"])).all() and (held(got["bot_img"]) == held(got["top_img"])).all()
    assert (held(got["silent_img"]) == np.minimum(c["k"], n_g - got["n_fire"])).all() and (got["n_fire"] <= n_g).all()
    for end in ("top", "bot"):
        pad = got[end + "_img"] < 0
        assert (got[end + "_val"][pad] == 0).all() and (got[end + "_patch"][pad] == -1).all() and (got[end + "_patch"][~pad] >= 0).all()
        assert (got[end + "_patch"] < c["t"]).all() and (c["groups"][got[end + "_img"][~pad]] >= 0).all()


def test_restatement_on_examples_counted_by_hand():
    """Five images of 3 patches in one group, image 3 left out.  Latent 0: image 0 holds 2, 5, 5 (M = 5 at patch 1, the lower of the
    two), image 1 holds 7 at patch 2, image 2 holds 5 at patch 0, image 3 (group -1) holds 9, image 4 nothing above thr."""
    ev = [(0, 0, 0, 2.0), (0, 1, 0, 5.0), (0, 2, 0, 5.0), (1, 2, 0, 7.0), (2, 0, 0, 5.0), (3, 1, 0, 9.0), (4, 1, 0, 0.0), (4, 2, 0, -1.0), (4, 0, 1, 1.0)]
    out = R.restate(**K.build(ev, n_images=5, t=3, s=2, groups=[0, 0, 0, -1, 0], g=1, k=2))
    assert out["n_group_images"].tolist() == [4] and out["n_fire"].tolist() == [[3], [1]]
    assert (out["top_img"][0, 0].tolist(), out["top_val"][0, 0].tolist(), out["top_patch"][0, 0].tolist()) == ([1, 0], [7.0, 5.0], [2, 1])
    assert (out["bot_img"][0, 0].tolist(), out["bot_val"][0, 0].tolist(), out["bot_patch"][0, 0].tolist()) == ([0, 2], [5.0, 5.0], [1, 0])
    assert out["silent_img"][0, 0].tolist() == [4, -1] and out["silent_img"][1, 0].tolist() == [0, 1]
    assert (out["top_img"][1, 0].tolist(), out["bot_img"][1, 0].tolist(), out["top_val"][1, 0].tolist(), out["top_patch"][1, 0].tolist()) == ([4, -1], [4, -1], [1.0, 0.0], [0, -1])
    wider = R.restate(**K.build(ev, n_images=5, t=3, s=2, groups=[0, 0, 0, -1, 0], g=1, k=2, thr=5.0))  # 5 is no longer an event
    assert wider["n_fire"].tolist() == [[1], [0]] and wider["top_img"][0, 0].tolist() == [1, -1] and wider["silent_img"][0, 0].tolist() == [0, 2]
    rows = R.patch_rows(*(K.build(ev, n_images=5, t=3, s=2, groups=[0] * 5, g=1, k=2)[key] for key in ("indptr", "indices", "data")), 3, [[0, 0], [1, 0]], [[0, 4], [4, -1]])
    assert rows.tolist() == [[[2.0, 5.0, 5.0], [0.0, 0.0, -1.0]], [[1.0, 0.0, 0.0], [0.0, 0.0, 0.0]]]


def _events_of(c, j):
    rows, lats, vals = R.events(c["indptr"], c["indices"], c["data"], c["t"], c["s"], c["groups"], c["thr"])
    return rows[lats == j], vals[lats == j]


def test_cases_hold_what_they_are_said_to_hold():
    got = {name: R.restate(**K.ALL[name]()) for name in K.SMALL}
    case = {name: K.ALL[name]() for name in K.SMALL}
    assert case["one_image"]["n_images"] == 1 and got["one_image"]["top_patch"][0, 0, 0] == 1 and got["one_image"]["silent_img"][1, 0, 0] == 0
    assert case["single_latent"]["s"] == 1 and case["wide"]["s"] == 70_001 and got["wide"]["n_fire"][70_000, 0] == 2 and got["wide"]["top_patch"][70_000, 0].tolist() == [1, 3]
    assert [case[f"tokens_{t}"]["t"] for t in (1, 5, 16, 257)] == [1, 5, 16, 257]
    for t in (1, 5, 16, 257):  # unsorted rows, free images that fire, and (for T > 1) images with several events of a latent
        c = case[f"tokens_{t}"]
        rows, lats, vals = R.events(c["indptr"], c["indices"], c["data"], t, c["s"], np.zeros(c["n_images"], np.int32), 0.0)
        assert (c["groups"][rows // t] == -1).any() and (t == 1 or len(np.unique((rows // t) * 8 + lats)) < len(rows))
        assert t == 1 or any((np.diff(c["indices"][a:b]) < 0).any() for a, b in zip(c["indptr"][:-1], c["indptr"][1:]))
    assert len(case["empty"]["indices"]) == 0 and got["empty"]["silent_img"][2].tolist() == [[0, 3, 4, 6], [-1] * 4, [1, 5, -1, -1]] and got["empty"]["n_fire"].sum() == 0
    for k in K.LENGTH_KS:
        assert case[f"lengths_k{k}"]["k"] == k and got[f"lengths_k{k}"]["n_fire"][:, 0].tolist() == [0, k - 1, k, k + 1, 2 * k + 1]
        assert (got[f"lengths_k{k}"]["n_fire"][:, 1] == 3).all()
    c = case["lists"]
    assert tuple(len(_events_of(c, q)[0]) for q in range(3)) == K.LIST_LENGTHS == (63, 64, 65)
    c = case["straddle"]
    for q, peaks in enumerate(K.STRADDLE_PEAKS):  # the run really crosses events 64 and 128, and its maximum lies where it is said to
        rows, vals = _events_of(c, q)
        for border, image in ((K.CHUNK, 4), (2 * K.CHUNK, 8)):
            assert rows[border - 1] // 16 == rows[border] // 16 == image and rows[border] % 16 == 6
            run = rows // 16 == image
            assert tuple(rows[run][vals[run] == vals[run].max()] % 16) == peaks
        assert got["straddle"]["top_img"][q, 0, :2].tolist() == [8, 4] and got["straddle"]["top_patch"][q, 0, :2].tolist() == [peaks[0]] * 2
    assert (K.STRADDLE_PEAKS[0][0] < 6 <= K.STRADDLE_PEAKS[1][0]) and K.STRADDLE_PEAKS[2][0] < 6 <= K.STRADDLE_PEAKS[2][1]
    c = case["long_run"]
    assert c["t"] == 200 > 3 * K.CHUNK and len(c["indices"]) == 4 * 200 and (c["data"] > 0).all()
    assert got["long_run"]["top_img"][0, 0, :4].tolist() == [2, 1, 0, 3] and got["long_run"]["top_patch"][0, 0, :4].tolist() == [10, 0, 199, 0]
    ties = got["ties"]  # values really tie, at both ends and inside an image
    assert ties["top_val"][0, 0].tolist() == [3.0, 3.0, 2.0, 2.0] and ties["top_img"][0, 0].tolist() == [6, 18, 0, 4]
    assert ties["bot_val"][0, 0].tolist() == [1.0, 1.0, 1.0, 1.0] and ties["bot_img"][0, 0].tolist() == [2, 10, 14, 22] and ties["n_fire"][0, 0] == 12
    assert (ties["top_val"][1] == 1.5).all() and ties["top_img"][1].tolist() == [[0, 2, 4, 6], [1, 3, 5, 7]] and ties["bot_img"][1].tolist() == ties["top_img"][1].tolist()
    assert (ties["top_patch"][2, 0] == 1).all() and (ties["bot_patch"][2, 0] == 1).all()
    inf = got["inf_two"]
    assert inf["top_img"][0, 0].tolist() == [2, 5, 4] and np.isposinf(inf["top_val"][0, 0, :2]).all() and inf["top_patch"][0, 0].tolist() == [1, 2, 1]
    assert case["one_group"]["g"] == 1 and case["groups_64"]["g"] == 64 and (got["groups_64"]["n_fire"].sum(axis=0) > 0).all()
    for g in (64, 32):
        c = case[f"limits_g{g}_k32"]
        assert (c["g"], c["k"]) == (g, 32) and c["g"] * c["k"] * 24 * (2 if g == 32 else 1) == 48 * 1024 and (got[f"limits_g{g}_k32"]["n_fire"].sum(axis=0) > 0).all()
    mixed, n_g = got["groups_mixed"], got["groups_mixed"]["n_group_images"]
    assert n_g.tolist() == [14, 6, 0, 2, 4] and (K.MIXED_GROUPS == -1).sum() == 4 and n_g[3] < K.MIXED_K
    assert mixed["n_fire"][0].tolist() == [5, 6, 0, 2, 0] and (mixed["silent_img"][0, 1] == -1).all() and mixed["silent_img"][0, 4].tolist() == [2, 7, 17, 24]
    c = case["groups_mixed"]
    assert (c["groups"][R.events(c["indptr"], c["indices"], c["data"], 3, 2, np.zeros(30, np.int32), 0.0)[0] // 3] == -1).sum() >= 4  # the free images fire
    gaps = got["gaps"]
    assert gaps["n_group_images"].tolist() == [40] and gaps["n_fire"][:, 0].tolist() == [2, 5, 1, 2] and case["gaps"]["k"] == 3 < 7
    mem = np.flatnonzero(case["gaps"]["groups"] == 0)
    assert gaps["silent_img"][:, 0].tolist() == [mem[[1, 2, 3]].tolist(), mem[[1, 2, 3]].tolist(), mem[[0, 1, 2]].tolist(), mem[[0, 1, 2]].tolist()]
    one = R.restate(**dict(case["gaps"], k=40))["silent_img"][:, 0]  # with room for all: the cursor passes every gap and the tail
    assert [int((row >= 0).sum()) for row in one] == [38, 35, 39, 38] and one[1, 6] == mem[9] and one[2, 38] == mem[38] and one[0, 37] == mem[38]
    d = K.value_kinds(0.0)["data"]
    assert np.isnan(d).sum() == 3 and np.isposinf(d).sum() == 1 and np.isneginf(d).sum() == 2 and (d == 0).sum() == 6 and np.signbit(d[d == 0]).sum() == 3
    assert ((d > 0) & (d < np.finfo(np.float32).tiny)).sum() == 4 and (d == np.float32(K.KINDS_THR)).sum() == 2 and (d < 0).sum() == 5
    v0, vh = got["values_thr_0"], got["values_thr_half"]
    assert v0["n_fire"].tolist() == [[4, 3], [1, 0], [1, 0]] and vh["n_fire"].tolist() == [[2, 1], [1, 0], [1, 0]]
    assert v0["top_val"][1, 0, 0] == 3.0 and v0["top_patch"][1, 0, 0] == 9 and v0["bot_val"][0, 0, 0] == np.float32(1e-45) > 0
    assert 13 in v0["silent_img"][2, 1] and 13 in vh["silent_img"][2, 1] and v0["top_img"][2, 0].tolist()[:2] == [14, -1] and v0["top_patch"][2, 0, 0] == 1
    assert 8 in vh["silent_img"][0, 0] and 8 not in v0["silent_img"][0, 0]  # the image that holds exactly thr
    c = K.every_row()
    n_ev = np.bincount(c["indices"], minlength=3)
    assert n_ev[1] == 300 * 256 == 76_800 == 1200 * K.CHUNK and (c["groups"] >= 0).all() and 0 < n_ev[0] < 64 and 0 < n_ev[2] < 64
    for name in K.UNTIED:
        assert len(np.unique(case[name]["data"])) == len(case[name]["data"])
    for kind in K.BROKEN:
        c, code = K.broken(kind)
        assert R.error_word(c["indices"], c["s"], c["groups"], c["g"]) == code
        assert (c["indices"][-1] == c["s"]) == (code == 2) and (c["groups"][-1] == c["g"]) == (kind != "latent_s")
        assert ((c["indices"][:-1] >= 0) & (c["indices"][:-1] < c["s"])).all() and (c["groups"][:-1] < c["g"]).all()
    base = case["tokens_16"]
    alone = R.restate(**K.one_latent(base, 3))
    apart = R.restate(**K.one_group_of(base, 1))
    for key in R.ARRAYS[1:]:
        assert np.array_equal(R.bits(alone[key][0]), R.bits(got["tokens_16"][key][3])) and np.array_equal(R.bits(apart[key][:, 1]), R.bits(got["tokens_16"][key][:, 1])), key


# ---------------------------------------------------------------- the module's host pieces ------------------------------------------------

def test_config_keys_path_and_the_choice_of_patch_latents():
    import dataclasses

    from saev_amd import exemplars

    assert [f.name for f in dataclasses.fields(exemplars.Config)] == ["run", "shards", "group_col", "grouping", "k", "threshold", "patch_latents", "min_images"]
    cfg = exemplars.Config()
    assert (cfg.group_col, cfg.grouping, cfg.k, cfg.threshold, cfg.patch_latents, cfg.min_images) == (None, None, 8, 0.0, 256, 8)
    assert exemplars.KEYS == ("group_names", "n_group_images", "n_fire", "top_val", "top_img", "top_patch", "bot_val", "bot_img", "bot_patch", "silent_img",
                              "patch_latents", "patch_top", "patch_bot")
    assert exemplars.exemplars_fpath(exemplars.Config(run="runs/r", shards="/data/shards/abc")).as_posix() == "runs/r/inference/abc/latent_exemplars.npz"
    #          latent 0: 9 / 10 against 1 / 20 (too few: counts as 0) -> 0.9; 1: 0.8 - 0.5 = 0.3; 2: nothing fires often enough; 3: 0.9 - 0 = 0.9 (a tie
    #          with 0); 4: 1.0 - 0.4 = 0.6
    nf = np.array([[9, 1], [8, 10], [7, 7], [0, 18], [10, 8]])
    ng = np.array([10, 20])
    assert exemplars.choose_patch_latents(nf, ng, 2, 8).tolist() == [0, 3] and exemplars.choose_patch_latents(nf, ng, 3, 8).tolist() == [0, 3, 4]
    assert exemplars.choose_patch_latents(nf, ng, 1, 8).tolist() == [0] and exemplars.choose_patch_latents(nf, ng, 10, 8).tolist() == [0, 1, 3, 4]
    assert exemplars.choose_patch_latents(nf, ng, 0, 8).tolist() == [] and exemplars.choose_patch_latents(nf, ng, 5, 100).tolist() == []
    # one group: the latents that fire in the most images, ties to the lower
    assert exemplars.choose_patch_latents(np.array([[9], [12], [3], [12], [8]]), np.array([20]), 3, 8).tolist() == [0, 1, 3]
    assert exemplars.choose_patch_latents(np.array([[9], [12], [3], [12], [8]]), np.array([20]), 1, 8).tolist() == [1]
    assert exemplars.choose_patch_latents(np.array([[9, 0], [12, 0]]), np.array([20, 0]), 1, 8).tolist() == [1]  # an empty group does not count


def test_strips_and_counter_examples():
    from saev_amd import exemplars

    c = K.groups_mixed()
    res = R.restate(**c)
    s = exemplars.strips(res, 0, 0)
    assert [r["image"] for r in s["top"]] == res["top_img"][0, 0].tolist() and len(s["bottom"]) == 4 and set(s["top"][0]) == {"image", "value", "patch"}
    assert s["top"][0]["value"] == float(res["top_val"][0, 0, 0]) and s["bottom"][0]["patch"] == int(res["bot_patch"][0, 0, 0])
    assert exemplars.strips(res, 0, 2) == dict(top=[], bottom=[]) and len(exemplars.strips(res, 0, 3)["top"]) == 2
    ce = exemplars.counter_examples(res, 0, pos_group=0, neg_group=1)  # latent 0 read as a detector of group 0: it misses 9 of 14 and fires on all of group 1
    assert ce["n_false_negatives"] == 9 and ce["false_negatives"] == res["silent_img"][0, 0].tolist() and len(ce["false_negatives"]) == 4
    assert ce["n_false_positives"] == 6 and [r["image"] for r in ce["false_positives"]] == res["top_img"][0, 1].tolist()
    ce = exemplars.counter_examples(res, 0, pos_group=1, neg_group=4)
    assert ce == dict(false_positives=[], n_false_positives=0, false_negatives=[], n_false_negatives=0)


def test_for_tasks_groups_the_images_by_their_roles():
    from saev_amd import exemplars, mimics

    #                  image  0  1  2  3  4  5  6  7
    include_a = np.array([1, 1, 1, 1, 0, 0, 1, 0], dtype=bool)  # task a: erato 0, 1; melpomene 2, 3, 6
    include_b = np.array([1, 1, 0, 0, 1, 1, 0, 0], dtype=bool)  # task b: erato 0, 1; melpomene 4, 5
    a = mimics.TaskSpec(name="a", include=include_a, erato_mask=np.array([1, 1, 0, 0, 0], bool), melp_mask=np.array([0, 0, 1, 1, 1], bool),
                        binary=np.array([0, 0, 1, 1, 1], np.int8), n_pos=3, n_neg=2)
    b = mimics.TaskSpec(name="b", include=include_b, erato_mask=np.array([1, 1, 0, 0], bool), melp_mask=np.array([0, 0, 1, 1], bool),
                        binary=np.array([0, 0, 1, 1], np.int8), n_pos=2, n_neg=2)
    groups, n_groups, sides = exemplars.for_tasks([a, b], 8)
    assert groups.dtype == np.int32 and n_groups == 3 and groups[7] == -1 and groups[0] == groups[1] and groups[2] == groups[3] == groups[6] and groups[4] == groups[5]
    assert len({groups[0], groups[2], groups[4]}) == 3
    assert sides == {"a": ([int(groups[0])], [int(groups[2])]), "b": ([int(groups[0])], [int(groups[4])])}
    groups, n_groups, sides = exemplars.for_tasks([a], 8)
    assert n_groups == 2 and (groups[[4, 5, 7]] == -1).all() and sides["a"] == ([int(groups[0])], [int(groups[2])])
