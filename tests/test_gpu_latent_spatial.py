"""GPU tests of LATENT SPATIAL (include/saev_amd.h): engine.latent_spatial on every case of
tests/latent_spatial_cases.py against the numpy restatement (tests/latent_spatial_restatement.py), the error word, determinism and
independence of other latents, other groups and the order of the images, and saev_amd.spatial / tools/latent_spatial.py end to end
on a run directory the test writes.

No tolerance anywhere: the integer outputs and count_map must EQUAL the restatement; moments and sum_map must equal it ON THE BITS
(each product is exact in float64 and each sum takes its terms one at a time in ascending row order on both sides).

The one-line errors the cases catch:
  the row-end wrap      (r, gw - 1) and (r + 1, 0) taken for neighbours: ``row_end`` (pairs_h must be 0), every ``grid_*`` with gw > 1
  the image-border wrap (gh - 1, c) of image i and (0, c) of image i + 1 taken for neighbours: ``image_border`` (pairs_v must be 0),
                        ``straddle``, ``every_row`` (300 x 240 pairs each way and no more)
  ``>=`` for ``>``      ``values_thr_half`` stores values equal to thr, ``values_thr_0`` stored zeros of both signs
  group -1 counted      ``groups_free`` (firing images of group -1), every ``grid_*`` (a fifth of the images are free)
  gh for gw             ``grid_3x5``, ``grid_1x5`` against ``grid_5x1``, ``row_end``, ``image_border``, ``full_image`` (pairs_h 12, pairs_v 10)
  a trip's border       ``lists`` (63 / 64 / 65 events), ``straddle`` (an image across events 64 and 128), ``every_row`` (1 200 trips)
  two events, one cell  ``same_cell`` (every event of a trip updates one map cell: the order of the float64 sum)"""

import functools
import importlib.util

import numpy as np
import pytest
import scipy.sparse
import torch

import latent_spatial_cases as K
import latent_spatial_restatement as R
from conftest import ROOT

pytestmark = [pytest.mark.gpu, pytest.mark.encoder_modes("f32")]
DEV = "cuda"
FLOATS = ("moments", "sum_map")


@functools.lru_cache(maxsize=None)
def _case(name):
    return K.ALL[name]()


@functools.lru_cache(maxsize=None)
def _expected(name):
    return R.restate(**_case(name))


def _run(c, sum_map=True):
    from saev_amd import engine

    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    return engine.latent_spatial(t(c["indptr"]), t(c["indices"]), t(c["data"]), n_images=c["n_images"], grid=(c["gh"], c["gw"]), n_latents=c["s"],
                                 groups=t(c["groups"]), n_groups=c["g"], threshold=c["thr"], sum_map=sum_map)


def _host(res):
    out = {k: getattr(res, k).cpu().numpy() for k in R.INTEGERS + ("moments", "n_group_images")}
    out["count_map"] = res.count_map.cpu().numpy().reshape(*out["n_events"].shape, -1)
    out["sum_map"] = None if res.sum_map is None else res.sum_map.cpu().numpy().reshape(*out["n_events"].shape, -1)
    return out


def _assert_equal(got, want, floats=FLOATS, sel=slice(None), gsel=slice(None)):
    for k in R.INTEGERS + ("count_map",):
        assert got[k].dtype == want[k].dtype, k
        bad = np.argwhere(got[k] != want[k][sel][:, gsel])
        assert bad.size == 0, (k, bad[:5].tolist(), got[k][tuple(bad[0])], want[k][sel][:, gsel][tuple(bad[0])])
    for k in floats:
        bad = np.argwhere(R.bits(got[k]) != R.bits(want[k][sel][:, gsel]))
        assert bad.size == 0, (k, bad[:5].tolist(), got[k][tuple(bad[0])], want[k][sel][:, gsel][tuple(bad[0])])


@pytest.mark.parametrize("name", list(K.ALL))
def test_equals_the_restatement(name):
    c = _case(name)
    res = _run(c)
    got = _host(res)
    _assert_equal(got, _expected(name))
    np.testing.assert_array_equal(got["n_group_images"], _expected(name)["n_group_images"])
    assert res.count_map.shape == (c["s"], c["g"], c["gh"], c["gw"]) and res.grid == (c["gh"], c["gw"])


@pytest.mark.parametrize("name", ["grid_3x5", "grid_37x37", "same_cell", "straddle", "values_thr_0", "every_row"])
def test_two_calls_give_the_same_bits_and_sum_map_is_optional(name):
    c = _case(name)
    first, second, lean = _host(_run(c)), _host(_run(c)), _run(c, sum_map=False)
    assert lean.sum_map is None
    for k in R.INTEGERS + ("count_map",) + FLOATS:
        assert np.array_equal(first[k].view(np.int64 if first[k].dtype == np.float64 else first[k].dtype),
                              second[k].view(np.int64 if second[k].dtype == np.float64 else second[k].dtype)), k
    _assert_equal(_host(lean), _expected(name), floats=("moments",))


@pytest.mark.parametrize("name,j", [("grid_3x5", 3), ("grid_37x37", 0), ("every_row", 1), ("values_thr_0", 1), ("wide", 70_000)])
def test_a_latent_alone_gives_the_bits_it_has_among_others(name, j):
    got = _host(_run(K.one_latent(_case(name), j)))
    _assert_equal(got, _expected(name), sel=slice(j, j + 1))


@pytest.mark.parametrize("name,g", [("grid_3x5", 1), ("groups_64", 63), ("every_row", 2), ("same_cell", 0)])
def test_a_group_alone_gives_the_bits_it_has_among_others(name, g):
    """The other groups' images set to -1, and G cut down to g + 1: the outputs of (j, g) do not depend on G beyond g."""
    c = _case(name)
    alone = dict(c, groups=np.where(c["groups"] == g, c["groups"], -1).astype(np.int32), g=g + 1)
    got = _host(_run(alone))
    _assert_equal({k: v[:, g:g + 1] for k, v in got.items() if k != "n_group_images"}, _expected(name), gsel=slice(g, g + 1))
    assert (got["n_events"][:, :g] == 0).all() and (got["count_map"][:, :g] == 0).all()


@pytest.mark.parametrize("name", ["grid_3x5", "groups_free", "straddle", "same_cell", "grid_37x37"])
def test_permuting_the_images_leaves_every_integer_unchanged(name):
    c = _case(name)
    perm = np.random.default_rng(3).permutation(c["n_images"])
    got = _host(_run(K.permute_images(c, perm)))
    _assert_equal(got, _expected(name), floats=())


@pytest.mark.parametrize("kind", K.BROKEN)
def test_error_word(kind):
    """Bad input is reported, never followed out of bounds; the outputs are void, the call returns, and the next call is right."""
    c, code = K.broken(kind)
    assert R.error_word(c["indices"], c["s"], c["groups"], c["g"]) == code
    res = _run(c)
    assert int(res._err.item()) == code
    with pytest.raises(ValueError, match="found on the device"):
        res.n_events
    with pytest.raises(ValueError):
        res.count_map
    _assert_equal(_host(_run(_case("grid_3x5"))), _expected("grid_3x5"))


def test_c_entry_with_an_exact_workspace_and_poisoned_outputs():
    """The C entry itself: a workspace exactly as large as the size function says, outputs the call must overwrite wholly, and an
    indptr that does not start at 0 (a block cut out of a longer CSR)."""
    from saev_amd import _lib
    from saev_amd.engine import _ptr, _stream

    lib = _lib.load()
    c = _case("grid_3x5")
    n, T, s, g = c["n_images"], c["gh"] * c["gw"], c["s"], c["g"]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    pad = 37
    indptr, indices, data = t(c["indptr"] + pad), t(np.concatenate([np.full(pad, 99, np.int32), c["indices"]])), t(np.concatenate([np.full(pad, 9, np.float32), c["data"]]))
    nnz = len(c["indices"])
    need = lib.saev_latent_spatial_workspace_bytes(n, T, s, g, nnz)
    ws = torch.full((need,), 0xAB, device=DEV, dtype=torch.uint8)
    i64 = lambda *shape: torch.full(shape, -77, device=DEV, dtype=torch.int64)  # noqa: E731
    outs = [i64(g)] + [i64(s, g) for _ in range(6)] + [torch.full((s, g, 5), -7.0, device=DEV, dtype=torch.float64),
                                                        torch.full((s, g, T), -77, device=DEV, dtype=torch.int32),
                                                        torch.full((s, g, T), -7.0, device=DEV, dtype=torch.float64)]
    groups = t(c["groups"])
    args = (_ptr(indptr), _ptr(indices), _ptr(data), nnz, n * T, n, c["gh"], c["gw"], s, _ptr(groups), g, c["thr"], *map(_ptr, outs), _ptr(ws))
    assert lib.saev_latent_spatial(*args, need, _stream()) == 0, lib.saev_last_error(None)
    want = _expected("grid_3x5")
    got = dict(zip(("n_group_images",) + R.INTEGERS + ("moments", "count_map", "sum_map"), (o.cpu().numpy() for o in outs)))
    _assert_equal(got, want)
    np.testing.assert_array_equal(got["n_group_images"], want["n_group_images"])
    assert ws[:4].view(torch.int32).item() == 0
    assert lib.saev_latent_spatial(*args, need - 1, _stream()) == -1


# ---------------------------------------------------------------- the module and the tool -------------------------------------------------

N_IMG, GH, GW, S = 48, 3, 4, 40
LABELS = ["erato", "melpomene", "other"]


@pytest.fixture(scope="module")
def run_dir(tmp_path_factory):
    """A run directory with token_acts.npz of 48 images x (3 x 4) tokens and shards with image_labels.csv: latent 0 fires at (1, 2) of
    every image (position consistency 1), latent 1 in a 2 x 2 block of the erato images only, the others at random."""
    from saev_amd.data import write_shards

    root = tmp_path_factory.mktemp("spatial")
    rng = np.random.default_rng(41)
    T = GH * GW
    dense = np.where(rng.random((N_IMG, GH, GW, S)) < 0.15, rng.random((N_IMG, GH, GW, S)) + 0.1, 0.0).astype(np.float32)
    labels = [LABELS[i % 3] for i in range(N_IMG)]
    dense[..., 0] = 0
    dense[:, 1, 2, 0] = 1.0 + rng.random(N_IMG)
    dense[..., 1] = 0
    dense[0::3, 0:2, 1:3, 1] = 2.0
    ta = scipy.sparse.csr_matrix(dense.reshape(N_IMG * T, S))
    shards = write_shards(root / "shards" / "abc", np.zeros((N_IMG, 1, T, 4), dtype=np.float32))
    (shards / "image_labels.csv").write_text("stem,species\n" + "".join(f"i{k},{lbl}\n" for k, lbl in enumerate(labels)))
    d = root / "run0" / "inference" / shards.name
    d.mkdir(parents=True)
    scipy.sparse.save_npz(str(d / "token_acts.npz"), ta)
    groups = np.array([i % 3 for i in range(N_IMG)], dtype=np.int32)
    return root / "run0", shards, ta, groups


def test_worker_fn_writes_the_scores_and_the_maps(run_dir):
    from saev_amd import spatial

    run, shards, ta, groups = run_dir
    fpath = spatial.worker_fn(spatial.Config(run=run, shards=shards, grid=(GH, GW), group_col="species", map_latents=5, min_images=8))
    assert fpath == run / "inference" / shards.name / "latent_spatial.npz"
    want = R.restate(ta.indptr.astype(np.int64), ta.indices, ta.data, n_images=N_IMG, gh=GH, gw=GW, s=S, groups=groups, g=3)
    with np.load(fpath) as z:
        assert tuple(z.files) == spatial.KEYS and z["group_names"].tolist() == LABELS and z["grid"].tolist() == [GH, GW]
        for k in R.INTEGERS:
            np.testing.assert_array_equal(z[k], want[k])
        assert np.array_equal(R.bits(z["moments"]), R.bits(want["moments"]))
        scores = spatial.scores_of(want, want["moments"], (GH, GW))
        for k in spatial.SCORES:
            assert np.array_equal(z[k], scores[k], equal_nan=True), k
        assert (z["position_consistency"][0] == 1.0).all() and z["adjacency"][1, 0] == 2.0 and np.isnan(z["adjacency"][1, 1])
        chosen = z["map_latents"]
        assert np.array_equal(chosen, spatial.choose_map_latents(scores["position_consistency"], want["n_images_fire"], 5, 8)) and 0 in chosen
        np.testing.assert_array_equal(z["count_map"].reshape(len(chosen), 3, -1), want["count_map"][chosen])
        mean = want["sum_map"][chosen] / want["n_group_images"].astype(np.float64)[None, :, None]
        assert np.array_equal(R.bits(z["mean_map"].reshape(len(chosen), 3, -1)), R.bits(mean))
        k0 = int(np.flatnonzero(chosen == 0)[0])
        diff = spatial.difference_map({"mean_map": z["mean_map"]}, k0, 0, 1)
        assert diff.shape == (GH, GW) and (diff[np.arange(GH) != 1] == 0).all()
    # a given list of latents, no grouping: one group of all images
    fpath = spatial.worker_fn(spatial.Config(run=run, shards=shards, grid=(GH, GW), map_latents=(1, 7)))
    with np.load(fpath) as z:
        assert z["map_latents"].tolist() == [1, 7] and z["group_names"].tolist() == ["all"] and z["n_group_images"].tolist() == [N_IMG]
        one = R.restate(ta.indptr.astype(np.int64), ta.indices, ta.data, n_images=N_IMG, gh=GH, gw=GW, s=S, groups=np.zeros(N_IMG, np.int32), g=1)
        np.testing.assert_array_equal(z["count_map"].reshape(2, 1, -1), one["count_map"][[1, 7]])
        np.testing.assert_array_equal(z["overlap"], one["overlap"])
    with pytest.raises(ValueError, match="does not hold"):
        spatial.worker_fn(spatial.Config(run=run, shards=shards, grid=(5, 2)))
    with pytest.raises(ValueError, match="not a square grid"):
        spatial.worker_fn(spatial.Config(run=run, shards=shards))


def test_tool_main(run_dir, capsys):
    run, shards, ta, groups = run_dir
    spec = importlib.util.spec_from_file_location("latent_spatial_tool", ROOT / "tools" / "latent_spatial.py")
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    out = tool.main(["--run", str(run), "--shards", str(shards), "--group-col", "species", "--grid", str(GH), str(GW)])
    text = capsys.readouterr().out
    assert out["n_latents"] == S and out["groups"] == LABELS and 0.0 <= out["clustered_fraction"] <= 1.0
    assert len(out["position_consistency_quantiles"]) == 7 and out["most_coherent"][0][0] == 0 and "clustering > 2" in text
    out = tool.main(["--run", str(run), "--shards", str(shards), "--group-col", "species", "--grid", str(GH), str(GW), "--latent", "1", "--pair", "erato",
                     "melpomene"])
    text = capsys.readouterr().out
    assert out["latent"] == 1 and out["pair"] == ["erato", "melpomene"]
    assert np.array(out["difference_map"]).shape == (GH, GW) and np.array(out["difference_map"])[0, 1] == 2.0 and "rate map" in text
