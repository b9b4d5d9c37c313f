"""CPU-only tests of LATENT SPATIAL (include/saev_amd.h): the entry is declared, exported and bound with the header's
types; every argument check refuses a call before anything touches a device, in the order the header states; the numpy restatement
the GPU tests lean on (tests/latent_spatial_restatement.py) agrees with an independent count (shifted ANDs of the dense firing
arrays for the pairs, ``np.bincount`` for the maps); every case of tests/latent_spatial_cases.py holds what it is said to hold; and
the derived scores of ``saev_amd.spatial`` are right on examples counted by hand.

Tolerances: none on the integers; the scores are single float64 expressions of small integers, compared with 1e-12 where the hand
value is not a float64 itself."""

import ctypes as C
import itertools
import re
import subprocess

import numpy as np
import pytest

import latent_spatial_cases as K
import latent_spatial_restatement as R
from conftest import ROOT

CTYPES = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double, "float": C.c_float}
INVALID, UNSUPPORTED = -1, -3


def _lib():
    subprocess.run(["make", "-C", str(ROOT)], check=True, capture_output=True)
    from saev_amd import _lib

    return _lib, _lib.load()


def test_the_entry_is_declared_exported_and_bound_with_the_headers_types():
    lib_mod, lib = _lib()
    raw = (ROOT / "include" / "saev_amd.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name, n_args in (("saev_latent_spatial", 25), ("saev_latent_spatial_workspace_bytes", 5)):
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
    codes = {k: int(v) for k, v in re.findall(r"#define\s+(SAEV_LATENT_SPATIAL_ERR_\w+)\s+(\d+)\b", text)}
    assert codes == {"SAEV_LATENT_SPATIAL_ERR_GROUP": R.ERR_GROUP, "SAEV_LATENT_SPATIAL_ERR_LATENT": R.ERR_LATENT}
    assert "LATENT SPATIAL" in raw and "DESIGN.md 3.27" in raw
    assert "spatial.hip" in (ROOT / "Makefile").read_text()


def _fake(i):
    return C.c_void_p((1 << 21) + 4096 * i)


SHAPE = dict(nnz=800, N=120, n_images=10, gh=3, gw=4, S=64, G=5, thr=0.0)
OUTPUTS = ("n_group_images", "n_events", "n_images_fire", "pairs_h", "pairs_v", "sum_m2", "overlap", "moments", "count_map", "sum_map")
NULL_OUT = "n_group_images, n_events, n_images_fire, pairs_h, pairs_v, sum_m2, overlap, moments and count_map must not be NULL"
TOO_SMALL = "workspace smaller than saev_latent_spatial_workspace_bytes(n_images, T, S, G, nnz)"
BELOW = "N, S and nnz must stay below 2^31"
GROUPS = "the number of groups must lie in [1, 64]"
GRID = "the grid must have gh, gw >= 1 and at most 4096 positions"
ROWS = "N must equal n_images * gh * gw"
CELLS = "S * G * gh * gw must stay below 2^31"
# the fake device pointers are never dereferenced: a launch on them would fault, and this machine has no device to launch on.  Status
# and saev_last_error(NULL) word for word, then the FIRST refusal of two bad arguments at once, in the header's order
BAD = [
    ("negative_n", dict(N=-1), INVALID, "negative size"), ("negative_nnz", dict(nnz=-1), INVALID, "negative size"),
    ("negative_images", dict(n_images=-10), INVALID, "negative size"), ("negative_gh", dict(gh=-3), INVALID, "negative size"),
    ("negative_groups", dict(G=-1), INVALID, "negative size"),
    ("rows_2_31", dict(N=1 << 31), UNSUPPORTED, BELOW), ("latents_2_31", dict(S=1 << 31), UNSUPPORTED, BELOW), ("nnz_2_31", dict(nnz=1 << 31), UNSUPPORTED, BELOW),
    ("zero_rows", dict(N=0), INVALID, "N and S must be at least 1"), ("zero_latents", dict(S=0), INVALID, "N and S must be at least 1"),
    ("no_groups", dict(G=0), UNSUPPORTED, GROUPS), ("too_many_groups", dict(G=65), UNSUPPORTED, GROUPS),
    ("zero_gw", dict(gw=0), UNSUPPORTED, GRID), ("grid_4097", dict(gh=1, gw=4097, N=40970), UNSUPPORTED, GRID),
    ("grid_65x64", dict(gh=65, gw=64, N=41600), UNSUPPORTED, GRID), ("grid_huge", dict(gh=1 << 40, gw=1 << 40), UNSUPPORTED, GRID),
    ("rows_not_images", dict(N=121), INVALID, ROWS), ("grid_of_15_for_12_rows", dict(gh=5, gw=3), INVALID, ROWS),
    ("images_2_31", dict(n_images=1 << 31), INVALID, ROWS),
    ("cells_2_31", dict(S=1 << 19, G=64, gh=8, gw=8, N=640), UNSUPPORTED, CELLS),
    ("thr_negative", dict(thr=-0.5), INVALID, "thr must be at least 0"), ("thr_nan", dict(thr=float("nan")), INVALID, "thr must be at least 0"),
    ("null_row_ptr", dict(row_ptr=None), INVALID, "row_ptr is NULL"), ("null_indices", dict(indices=None), INVALID, "indices and data come with nnz > 0"),
    ("null_data", dict(data=None), INVALID, "indices and data come with nnz > 0"),
    ("null_groups", dict(group=None), INVALID, "group_i32 must not be NULL"),
    *[(f"null_{name}", {name: None}, INVALID, NULL_OUT) for name in OUTPUTS[:-1]],
    ("workspace_null", dict(ws=None), INVALID, TOO_SMALL), ("workspace_too_small", dict(ws_short=1), INVALID, TOO_SMALL),
    ("workspace_misaligned", dict(ws=C.c_void_p((1 << 20) + 8)), INVALID, "workspace must be 256-byte aligned"),
    ("negative_before_2_31", dict(G=-1, S=1 << 31), INVALID, "negative size"),
    ("below_2_31_before_zero", dict(N=0, nnz=1 << 31), UNSUPPORTED, BELOW),
    ("zero_before_groups", dict(S=0, G=65), INVALID, "N and S must be at least 1"),
    ("groups_before_grid", dict(G=65, gw=0), UNSUPPORTED, GROUPS),
    ("grid_before_rows", dict(gh=1, gw=4097), UNSUPPORTED, GRID),
    ("rows_before_cells", dict(S=1 << 19, G=64, gh=8, gw=8), INVALID, ROWS),
    ("cells_before_thr", dict(S=1 << 19, G=64, gh=8, gw=8, N=640, thr=-1.0), UNSUPPORTED, CELLS),
    ("thr_before_pointers", dict(thr=-1.0, row_ptr=None), INVALID, "thr must be at least 0"),
    ("row_ptr_before_groups", dict(row_ptr=None, group=None), INVALID, "row_ptr is NULL"),
    ("groups_before_outputs", dict(group=None, overlap=None), INVALID, "group_i32 must not be NULL"),
    ("outputs_before_workspace", dict(moments=None, ws_short=1), INVALID, NULL_OUT),
    ("size_before_alignment", dict(ws=C.c_void_p((1 << 20) + 8), ws_short=1), INVALID, TOO_SMALL),
]


def _call(lib, over):
    a = dict(SHAPE, row_ptr=_fake(0), indices=_fake(1), data=_fake(2), group=_fake(3), ws=C.c_void_p(1 << 20), ws_short=0,
             **{name: _fake(20 + i) for i, name in enumerate(OUTPUTS)})
    a.update(over)
    need = lib.saev_latent_spatial_workspace_bytes(10, 12, 64, 5, 800)
    return lib.saev_latent_spatial(a["row_ptr"], a["indices"], a["data"], a["nnz"], a["N"], a["n_images"], a["gh"], a["gw"], a["S"], a["group"], a["G"],
                                   a["thr"], *[a[name] for name in OUTPUTS], a["ws"], need - a["ws_short"], None)


@pytest.mark.parametrize("case", BAD, ids=[c[0] for c in BAD])
def test_the_call_refuses_bad_arguments_without_a_device_in_order(case):
    _, lib = _lib()
    _, over, status, text = case
    rc = _call(lib, over)
    assert rc == status, (rc, lib.saev_last_error(None))
    assert lib.saev_last_error(None).decode() == "saev_latent_spatial: " + text


def test_a_null_sum_map_and_no_entries_are_not_refused_by_the_checks():
    """sum_map may be NULL and nnz = 0 needs no indices: both calls get as far as the workspace check."""
    _, lib = _lib()
    for over in (dict(sum_map=None, ws_short=1), dict(nnz=0, indices=None, data=None, ws=None)):
        assert _call(lib, over) == INVALID and lib.saev_last_error(None).decode() == "saev_latent_spatial: " + TOO_SMALL


def test_workspace_size():
    _, lib = _lib()
    size = lib.saev_latent_spatial_workspace_bytes
    r256 = lambda b: -(-max(b, 1) // 256) * 256  # noqa: E731
    for n_images, T, s, g, nnz in ((10, 12, 64, 5, 800), (1, 1, 1, 1, 0), (4096, 256, 16384, 16, 1 << 25), (300, 1369, 1000, 64, 600), (2, 4, 70_001, 1, 5)):
        parts = max(1, min(1024, -(-nnz // 64), max(1, (1 << 26) // s)))
        want = 256 + r256(8 * (s + 1)) + r256(4 * s) + r256(4 * parts * s) + 3 * r256(4 * nnz)
        assert size(n_images, T, s, g, nnz) == want and want % 256 == 0
    for bad in ((0, 12, 64, 5, 800), (10, 0, 64, 5, 800), (10, 4097, 64, 5, 800), (10, 12, 0, 5, 800), (10, 12, 64, 0, 800), (10, 12, 64, 65, 800),
                (10, 12, 64, 5, -1), (10, 12, 64, 5, 1 << 31), (10, 12, 1 << 31, 1, 800), (1 << 31, 1, 64, 5, 800), (1 << 20, 4096, 64, 5, 800),
                (10, 64, 1 << 19, 64, 800)):
        assert size(*bad) == -1, bad
    assert size(10, 64, (1 << 19) - 1, 64, 800) > 0


def test_python_surface_refuses_host_tensors_and_bad_arguments():
    import torch
    from saev_amd import engine

    z, i, v = torch.zeros(5, dtype=torch.int64), torch.zeros(0, dtype=torch.int32), torch.zeros(0)
    ok = dict(n_images=1, grid=(2, 2), n_latents=3, groups=torch.zeros(1, dtype=torch.int32), n_groups=1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        engine.latent_spatial(z, i, v, **ok)
    for over, match in ((dict(grid=(65, 64)), "unsupported grid"), (dict(grid=(0, 4)), "unsupported grid"), (dict(n_groups=65), "n_groups"),
                        (dict(n_groups=0), "n_groups"), (dict(n_latents=0), "n_latents"), (dict(n_images=0), "n_images"),
                        (dict(n_latents=1 << 29), "below 2\\^31"), (dict(threshold=-1.0), "threshold"), (dict(threshold=float("nan")), "threshold")):
        with pytest.raises(ValueError, match=match):
            engine.latent_spatial(z, i, v, **dict(ok, **over))
    assert engine.LatentSpatialResult._ERRORS == {1: "a group id lies outside [-1, n_groups)", 2: "a column index lies outside [0, n_latents)"}


# ---------------------------------------------------------------- the restatement ---------------------------------------------------------

def _dense(c):
    """(n_images, gh, gw, S) firing array and values, the images of group -1 silent."""
    fire = np.zeros((c["n_images"] * c["gh"] * c["gw"], c["s"]), dtype=bool)
    val = np.zeros(fire.shape, dtype=np.float64)
    rows = np.repeat(np.arange(len(c["indptr"]) - 1), np.diff(c["indptr"]))
    with np.errstate(invalid="ignore"):
        hit = c["data"] > np.float32(c["thr"])
    fire[rows[hit], c["indices"][hit]] = True
    val[rows[hit], c["indices"][hit]] = c["data"][hit]
    shape = (c["n_images"], c["gh"], c["gw"], c["s"])
    fire, val = fire.reshape(shape), val.reshape(shape)
    fire[c["groups"] < 0] = False
    return fire, val


def _independent(c):
    """The integer outputs by whole-array operations: shifted ANDs for the pairs, bincount for the maps."""
    fire, _ = _dense(c)
    g, s, T = c["g"], c["s"], c["gh"] * c["gw"]
    grp = np.maximum(c["groups"], 0)
    per_image = lambda x: np.stack([np.bincount(grp, weights=x[:, j], minlength=g) for j in range(s)]).astype(np.int64)  # noqa: E731
    m = fire.sum(axis=(1, 2))
    out = dict(n_events=per_image(m), n_images_fire=per_image(m > 0), sum_m2=per_image(m * m),
               pairs_h=per_image((fire[:, :, :-1] & fire[:, :, 1:]).sum(axis=(1, 2))), pairs_v=per_image((fire[:, :-1] & fire[:, 1:]).sum(axis=(1, 2))))
    i, r, col, j = np.nonzero(fire)
    flat = (j * g + c["groups"][i]) * T + r * c["gw"] + col
    out["count_map"] = np.bincount(flat, minlength=s * g * T).reshape(s, g, T).astype(np.int32)
    out["overlap"] = (out["count_map"].astype(np.int64) ** 2).sum(axis=2)
    return out


@pytest.mark.parametrize("name", [n for n in K.SMALL if n != "wide"])
def test_restatement_equals_an_independent_count(name):
    c = K.SMALL[name]()
    got, want = R.restate(**c), _independent(c)
    for k in R.INTEGERS + ("count_map",):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    fire, val = _dense(c)
    # the sums against pairwise numpy sums: equal up to rounding (all terms are positive or the sum is not finite)
    for g in range(c["g"]):
        sel = c["groups"] == g
        with np.errstate(invalid="ignore"):
            total = np.where(fire[sel], val[sel], 0.0).sum(axis=(0, 1, 2))
        np.testing.assert_allclose(got["moments"][:, g, 0], total, rtol=1e-12, equal_nan=True)
        np.testing.assert_allclose(got["sum_map"][:, g].sum(axis=1), total, rtol=1e-12, equal_nan=True)
    assert (got["pairs_h"] + got["pairs_v"] <= got["n_images_fire"] * (c["gh"] * (c["gw"] - 1) + c["gw"] * (c["gh"] - 1))).all()
    np.testing.assert_array_equal(got["count_map"].sum(axis=2), got["n_events"])


def test_cases_hold_what_they_are_said_to_hold():
    got = {name: R.restate(**K.ALL[name]()) for name in K.SMALL}
    assert got["grid_1x1"]["pairs_h"].sum() == got["grid_1x1"]["pairs_v"].sum() == 0 and got["grid_1x1"]["n_events"].sum() > 0
    assert got["grid_1x5"]["pairs_v"].sum() == 0 < got["grid_1x5"]["pairs_h"].sum() and got["grid_5x1"]["pairs_h"].sum() == 0 < got["grid_5x1"]["pairs_v"].sum()
    c = K.ALL["grid_3x5"]()
    swapped = R.restate(**dict(c, gh=5, gw=3))
    assert not np.array_equal(swapped["pairs_h"], got["grid_3x5"]["pairs_h"]) and not np.array_equal(swapped["pairs_v"], got["grid_3x5"]["pairs_v"])
    assert (c["groups"] == -1).any() and got["grid_3x5"]["n_events"].sum() < (c["data"] > 0).sum()
    assert K.ALL["grid_37x37"]()["gh"] * K.ALL["grid_37x37"]()["gw"] == 1369 and 1369 % 64 != 0
    # consecutive rows that are no neighbours; rows gw apart that are no neighbours
    c = K.row_end()
    rows = np.repeat(np.arange(len(c["indptr"]) - 1), np.diff(c["indptr"]))
    assert np.diff(rows).tolist() == [1, 19, 1] and got["row_end"]["pairs_h"].sum() == got["row_end"]["pairs_v"].sum() == 0
    c = K.image_border()
    rows = np.repeat(np.arange(len(c["indptr"]) - 1), np.diff(c["indptr"]))
    assert (np.isin(rows + c["gw"], rows).sum(), got["image_border"]["pairs_v"].sum(), got["image_border"]["pairs_h"].sum()) == (4, 0, 0)
    full = got["full_image"]
    assert (full["pairs_h"][2, 0], full["pairs_v"][2, 0], full["n_events"][2, 0], full["sum_m2"][2, 0]) == (12, 10, 15, 225) and full["n_events"].sum() == 15
    assert got["silent"]["n_events"].tolist() == [[0, 0], [0, 0], [0, 1]] and (got["silent"]["moments"][:2] == 0).all()
    assert tuple(got["lists"]["n_events"].sum(axis=1)) == K.LIST_LENGTHS == (63, 64, 65)
    c = K.straddle()
    image_of_event = np.repeat(np.arange(len(c["indptr"]) - 1), np.diff(c["indptr"]))[c["indices"] == 0] // 16
    for border in (K.CHUNK, 2 * K.CHUNK):
        assert image_of_event[border - 1] == image_of_event[border] and 0 < (image_of_event[:border] == image_of_event[border]).sum() < 16
    same = got["same_cell"]
    assert same["count_map"][0].max() == 100 and (same["count_map"][0] > 0).sum() == 2 and (same["overlap"][0] == 100 * 100).all()
    free = K.groups_free()
    assert (free["groups"] == -1).sum() == 3 and (got["groups_free"]["n_events"][:, 1] == 0).all() and got["groups_free"]["n_group_images"].tolist() == [4, 0, 3]
    assert got["groups_free"]["n_events"].sum() < (free["data"] > 0).sum()
    assert K.one_group()["g"] == 1 and K.groups_64()["g"] == 64 and (got["groups_64"]["n_events"].sum(axis=0) > 0).all()
    d = K.value_kinds(0.0)["data"]
    assert np.isnan(d).sum() == 1 and np.isposinf(d).sum() == 2 and np.isneginf(d).sum() == 1 and (d == 0).sum() == 2 and np.signbit(d[d == 0]).sum() == 1
    assert ((d > 0) & (d < np.finfo(np.float32).tiny)).sum() == 2 and (d == np.float32(K.KINDS_THR)).sum() == 1 and (d < 0).sum() == 2
    v0, vh = got["values_thr_0"], got["values_thr_half"]
    assert v0["n_events"].sum() == (d > 0).sum() == 13 and vh["n_events"].sum() == (d > np.float32(0.5)).sum() == 9
    assert np.isnan(v0["moments"][1, 0, 1]) and np.isposinf(v0["moments"][1, 0, 0])  # +Inf at r = 0: Inf * 0 in sum v r
    wide = K.wide()
    assert wide["s"] == 70_001 and got["wide"]["n_events"][70_000, 0] == 3 and got["wide"]["pairs_h"][70_000, 0] == 1
    c = K.every_row()
    n_ev = np.bincount(c["indices"], minlength=3)
    assert n_ev[1] == 300 * 256 == 76_800 and (c["groups"] >= 0).all() and 0 < n_ev[0] < 64 and 0 < n_ev[2] < 64
    for kind in K.BROKEN:
        c, code = K.broken(kind)
        assert R.error_word(c["indices"], c["s"], c["groups"], c["g"]) == code
    base = K.ALL["grid_3x5"]()
    perm = np.arange(base["n_images"])[::-1]
    moved = R.restate(**K.permute_images(base, perm))
    for k in R.INTEGERS + ("count_map",):
        np.testing.assert_array_equal(moved[k], got["grid_3x5"][k])
    alone = R.restate(**K.one_latent(base, 3))
    assert np.array_equal(R.bits(alone["moments"][0]), R.bits(got["grid_3x5"]["moments"][3])) and np.array_equal(alone["count_map"][0], got["grid_3x5"]["count_map"][3])


# ---------------------------------------------------------------- the derived scores ------------------------------------------------------

def _scores(c):
    from saev_amd import spatial

    out = R.restate(**c)
    return out, spatial.scores_of(out, out["moments"], (c["gh"], c["gw"]))


def test_scores_on_a_2x2_example_counted_by_hand():
    """Image A fires at (0, 0), (0, 1); image B at (0, 0), (1, 0), (1, 1); unit activations.  5 events, 2 + 1 pairs, sum m^2 = 13, the
    cell counts 2, 1, 1, 1.  Of the 5 firing patches, the two at (0, 0) meet the other image there: consistency 2 / 5."""
    ev = [(0, 0, 0, 0, 1.0), (0, 0, 1, 0, 1.0), (1, 0, 0, 0, 1.0), (1, 1, 0, 0, 1.0), (1, 1, 1, 0, 1.0)]
    out, sc = _scores(K.build(ev, n_images=2, gh=2, gw=2, s=1, groups=[0, 0], g=1))
    assert [int(out[k][0, 0]) for k in R.INTEGERS] == [5, 2, 2, 1, 13, 7]
    assert sc["adjacency"][0, 0] == 2 * 3 / 5 and abs(sc["clustering"][0, 0] - 3 / (4 * 8 / 12)) < 1e-12 and sc["position_consistency"][0, 0] == 2 / 5
    assert sc["centroid"][0, 0].tolist() == [2 / 5, 2 / 5] and abs(sc["spread"][0, 0] - np.sqrt(2 * (0.4 - 0.16))) < 1e-12


def test_scores_on_3x5_examples_counted_by_hand():
    from saev_amd import spatial

    out, sc = _scores(K.full_image())
    # a full image: all 22 edges are pairs, which is what 15 patches thrown on 15 cells must give: clustering exactly 1
    assert spatial.n_grid_edges((3, 5)) == 22 and sc["adjacency"][2, 0] == 2 * 22 / 15 and abs(sc["clustering"][2, 0] - 1.0) < 1e-12
    assert np.isnan(sc["position_consistency"][2, 0]) and np.isnan(sc["adjacency"][0, 0]) and np.isnan(sc["clustering"][2, 1]) and np.isnan(sc["centroid"][0, 0]).all()
    # a horizontal bar (1, 1..3) in three images and a lone patch in a fourth; weights 1, 2, 3 along the bar
    ev = [(i, 1, c, 0, float(c)) for i in range(3) for c in (1, 2, 3)] + [(3, 2, 4, 0, 6.0)]
    out, sc = _scores(K.build(ev, n_images=4, gh=3, gw=5, s=1, groups=[0, 0, 0, 0], g=1))
    assert [int(out[k][0, 0]) for k in R.INTEGERS] == [10, 4, 6, 0, 28, 28]
    assert sc["adjacency"][0, 0] == 12 / 10 and abs(sc["clustering"][0, 0] - 6 / (22 * 18 / 210)) < 1e-12
    assert abs(sc["position_consistency"][0, 0] - (28 - 10) / (10 * 3)) < 1e-12  # nine patches meet 2 of 3 others, one meets none
    assert abs(sc["centroid"][0, 0, 0] - (18 * 1 + 6 * 2) / 24) < 1e-12 and abs(sc["centroid"][0, 0, 1] - (3 * (1 + 4 + 9) + 24) / 24) < 1e-12
    var_r = (18 + 24) / 24 - (30 / 24) ** 2
    var_c = (3 * (1 + 8 + 27) + 6 * 16) / 24 - (66 / 24) ** 2
    assert abs(sc["spread"][0, 0] - np.sqrt(var_r + var_c)) < 1e-12
    rate = spatial.rate_map(out["count_map"].reshape(1, 1, 3, 5), out["n_group_images"])
    mean = spatial.mean_map(out["sum_map"].reshape(1, 1, 3, 5), out["n_group_images"])
    assert rate[0, 0, 1].tolist() == [0, 0.75, 0.75, 0.75, 0] and mean[0, 0, 1].tolist() == [0, 0.75, 1.5, 2.25, 0] and mean[0, 0, 2, 4] == 1.5


def test_clustering_is_1_over_all_placements_of_two_patches_on_a_2x3_grid():
    """Every one of the 15 placements once: the pairs counted are exactly the expectation under uniform placement."""
    ev = []
    for i, (p, q) in enumerate(itertools.combinations(range(6), 2)):
        ev += [(i, p // 3, p % 3, 0, 1.0), (i, q // 3, q % 3, 0, 1.0)]
    out, sc = _scores(K.build(ev, n_images=15, gh=2, gw=3, s=1, groups=[0] * 15, g=1))
    assert out["pairs_h"][0, 0] + out["pairs_v"][0, 0] == 7 and abs(sc["clustering"][0, 0] - 1.0) < 1e-12
    assert abs(sc["position_consistency"][0, 0] - (15 * 2 * 4) / (30 * 14)) < 1e-12  # each patch meets 4 of the 14 other images at its cell


def test_difference_map_and_position_consistency_bounds():
    from saev_amd import spatial

    c = K.ALL["groups_64"]()
    out, sc = _scores(c)
    pc = sc["position_consistency"]
    assert ((pc[~np.isnan(pc)] >= 0) & (pc[~np.isnan(pc)] <= 1)).all() and (~np.isnan(pc)).any()
    mean = spatial.mean_map(out["sum_map"].reshape(c["s"], c["g"], c["gh"], c["gw"]), out["n_group_images"])
    diff = spatial.difference_map({"mean_map": mean}, 1, 3, 5)
    assert diff.shape == (2, 3) and np.array_equal(diff, mean[1, 3] - mean[1, 5]) and np.array_equal(-diff, spatial.difference_map({"mean_map": mean}, 1, 5, 3))


# ---------------------------------------------------------------- the module's host pieces ------------------------------------------------

def test_grid_inference_keys_config_and_map_latents_choice():
    import dataclasses

    from saev_amd import spatial

    assert spatial.infer_grid(256) == (16, 16) and spatial.infer_grid(1) == (1, 1) and spatial.infer_grid(1369) == (37, 37)
    assert spatial.infer_grid(15, (3, 5)) == (3, 5) and spatial.infer_grid(15, [5, 3]) == (5, 3)
    for t, grid, match in ((15, None, "not a square grid"), (200, None, "not a square grid"), (15, (4, 4), "does not hold"), (16, (0, 16), "does not hold")):
        with pytest.raises(ValueError, match=match):
            spatial.infer_grid(t, grid)
    assert [f.name for f in dataclasses.fields(spatial.Config)] == ["run", "shards", "grid", "group_col", "grouping", "threshold", "map_latents", "min_images"]
    cfg = spatial.Config()
    assert (cfg.grid, cfg.group_col, cfg.grouping, cfg.threshold, cfg.map_latents, cfg.min_images) == (None, None, None, 0.0, 256, 8)
    assert spatial.KEYS == ("n_events", "n_images_fire", "pairs_h", "pairs_v", "sum_m2", "overlap", "moments", "adjacency", "clustering",
                            "position_consistency", "centroid", "spread", "group_names", "n_group_images", "grid", "map_latents", "count_map", "mean_map")
    assert spatial.spatial_fpath(spatial.Config(run="runs/r", shards="/data/shards/abc")).as_posix() == "runs/r/inference/abc/latent_spatial.npz"
    assert spatial.image_groups(spatial.Config(), 5)[0].tolist() == [0] * 5 and spatial.image_groups(spatial.Config(), 5)[1] == ["all"]
    #          latent 0: best 0.9 but in too few images; 1: 0.5; 2: never defined; 3: 0.8 in its second group; 4: 0.5 (a tie with 1)
    pc = np.array([[0.9, 0.1], [0.5, np.nan], [np.nan, np.nan], [0.2, 0.8], [0.5, 0.3]])
    nf = np.array([[3, 9], [8, 1], [0, 1], [20, 8], [9, 9]])
    assert spatial.choose_map_latents(pc, nf, 2, 8).tolist() == [1, 3] and spatial.choose_map_latents(pc, nf, 3, 8).tolist() == [1, 3, 4]
    assert spatial.choose_map_latents(pc, nf, 10, 8).tolist() == [0, 1, 3, 4] and spatial.choose_map_latents(pc, nf, 1, 2).tolist() == [0]
    assert spatial.choose_map_latents(pc, nf, 0, 8).tolist() == [] and spatial.choose_map_latents(pc, nf, 5, 100).tolist() == []
