"""GPU tests of LATENT EXEMPLARS (include/saev_amd.h): engine.latent_exemplars on every case of
tests/latent_exemplars_cases.py against the numpy restatement (tests/latent_exemplars_restatement.py), the error word, determinism
and independence of other latents and other groups, engine.latent_patch_rows against scipy's slices, the tie to the reference's
``csr_topk(...).indices // T``, and saev_amd.exemplars / tools/latent_exemplars.py end to end on a run directory the test writes.

No tolerance anywhere: every output must EQUAL the restatement, floats compared on the bits.

The one-line errors the cases catch:
  a token list for an image list   an image with several strong patches fills several slots: ``tokens_5``, ``tokens_16``, ``long_run``
  the higher patch on equal values ``>=`` for ``>`` in the fold or the carry: ``ties`` (latent 2), ``straddle`` (latent 2), ``long_run`` (image 2)
  a run cut at the trip's border   an image counted twice, or its earlier half forgotten: ``straddle``, ``lists``, ``long_run``, ``every_row``
  the later image on equal M       an insertion in front of equal values: ``ties`` (latents 0, 1), ``inf_two``, ``lengths_k*``
  a full list not updated          the k-th value not refreshed after an insertion: ``lengths_k*`` (k + 1 and 2 k + 1 firing images)
  ``>=`` for ``>`` in the event    ``values_thr_half`` stores values equal to thr, ``values_thr_0`` stored zeros of both signs
  group -1 listed                  ``groups_mixed``, ``gaps``, every ``tokens_*`` (a fifth of the images are free, and they fire)
  the silent cursor                a member before the first, between two or behind the last firing one dropped, or a stranger listed:
                                   ``gaps``, ``groups_mixed`` (a group that all fire, one that never fires, an empty one), ``empty``
  a slot left as it was            the outputs are poisoned before the C entry runs: padding must be 0.0 / -1 / -1"""

import functools
import importlib.util

import numpy as np
import pytest
import scipy.sparse
import torch

import latent_exemplars_cases as K
import latent_exemplars_restatement as R
from conftest import ROOT
from saev_amd.engine import latent_exemplars, latent_patch_rows  # noqa: F401  (without the feature nothing here can run)

pytestmark = [pytest.mark.gpu, pytest.mark.encoder_modes("f32")]
DEV = "cuda"


@functools.lru_cache(maxsize=None)
def _case(name):
    return K.ALL[name]()


@functools.lru_cache(maxsize=None)
def _expected(name):
    return R.restate(**_case(name))


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _run(c):
    from saev_amd import engine

    return engine.latent_exemplars(_t(c["indptr"]), _t(c["indices"]), _t(c["data"]), n_images=c["n_images"], tokens_per_image=c["t"], n_latents=c["s"],
                                   groups=_t(c["groups"]), n_groups=c["g"], k=c["k"], threshold=c["thr"])


def _host(res):
    return {name: getattr(res, name).cpu().numpy() for name in R.ARRAYS}


def _assert_equal(got, want, sel=slice(None), gsel=slice(None)):
    for name in R.ARRAYS[1:]:
        w = want[name][sel][:, gsel]
        assert got[name].dtype == w.dtype and got[name].shape == w.shape, (name, got[name].dtype, got[name].shape, w.shape)
        bad = np.argwhere(R.bits(got[name]) != R.bits(w))
        assert bad.size == 0, (name, bad[:5].tolist(), got[name][tuple(bad[0])], w[tuple(bad[0])])


@pytest.mark.parametrize("name", list(K.ALL))
def test_equals_the_restatement(name):
    c = _case(name)
    res = _run(c)
    got = _host(res)
    _assert_equal(got, _expected(name))
    np.testing.assert_array_equal(got["n_group_images"], _expected(name)["n_group_images"])
    assert got["n_group_images"].dtype == np.int64 and res.top_val.shape == (c["s"], c["g"], c["k"]) and res.k == c["k"]


@pytest.mark.parametrize("name", ["tokens_16", "ties", "straddle", "groups_mixed", "values_thr_0", "every_row"])
def test_two_calls_give_the_same_bits(name):
    first, second = _host(_run(_case(name))), _host(_run(_case(name)))
    for key in R.ARRAYS:
        assert np.array_equal(R.bits(first[key]), R.bits(second[key])), key


@pytest.mark.parametrize("name,j", [("tokens_16", 3), ("straddle", 2), ("every_row", 1), ("ties", 0), ("wide", 70_000), ("lengths_k8", 4)])
def test_a_latent_alone_gives_the_bits_it_has_among_others(name, j):
    got = _host(_run(K.one_latent(_case(name), j)))
    _assert_equal(got, _expected(name), sel=slice(j, j + 1))


@pytest.mark.parametrize("name,g", [("tokens_16", 1), ("groups_64", 63), ("every_row", 2), ("groups_mixed", 3), ("groups_mixed", 0)])
def test_a_group_alone_gives_the_bits_it_has_among_others(name, g):
    """The other groups' images set to -1, and G cut down to g + 1: the outputs of (j, g) do not depend on the other groups."""
    got = _host(_run(K.one_group_of(_case(name), g)))
    _assert_equal({key: v[:, g:g + 1] for key, v in got.items() if key != "n_group_images"}, _expected(name), gsel=slice(g, g + 1))
    assert got["n_group_images"][g] == _expected(name)["n_group_images"][g]
    assert (got["n_fire"][:, :g] == 0).all() and (got["top_img"][:, :g] == -1).all() and (got["silent_img"][:, :g] == -1).all()


@pytest.mark.parametrize("kind", K.BROKEN)
def test_error_word(kind):
    """Bad input is reported, never followed out of bounds; the outputs are void, the call returns, and the next call is right."""
    c, code = K.broken(kind)
    assert R.error_word(c["indices"], c["s"], c["groups"], c["g"]) == code
    res = _run(c)
    assert int(res._err.item()) == code
    with pytest.raises(ValueError, match="found on the device"):
        res.n_fire
    with pytest.raises(ValueError):
        res.top_img
    _assert_equal(_host(_run(_case("tokens_5"))), _expected("tokens_5"))


def test_c_entry_with_an_exact_workspace_and_poisoned_outputs():
    """The C entry itself: a workspace exactly as large as the size function says, outputs the call must overwrite wholly, and an
    indptr that does not start at 0 (a block cut out of a longer CSR)."""
    import ctypes as C

    from saev_amd import _lib
    from saev_amd.engine import _ptr, _stream

    lib = _lib.load()
    c = _case("groups_mixed")
    n, T, s, g, k = c["n_images"], c["t"], c["s"], c["g"], c["k"]
    pad = 37
    indptr, indices = _t(c["indptr"] + pad), _t(np.concatenate([np.full(pad, 99, np.int32), c["indices"]]))
    data, groups = _t(np.concatenate([np.full(pad, 9, np.float32), c["data"]])), _t(c["groups"])
    nnz = len(c["indices"])
    need = lib.saev_latent_exemplars_workspace_bytes(nnz, s, n, g)
    ws = torch.full((need,), 0xAB, device=DEV, dtype=torch.uint8)
    outs = dict(n_group_images=torch.full((g,), -77, device=DEV, dtype=torch.int64), n_fire=torch.full((s, g), -77, device=DEV, dtype=torch.int32))
    for name in R.LISTS:
        outs[name] = torch.full((s, g, k), -7, device=DEV, dtype=torch.float32 if name.endswith("val") else torch.int32)
    struct = _lib.SaevLatentExemplarsOut(struct_size=C.sizeof(_lib.SaevLatentExemplarsOut), **{name: _ptr(v) for name, v in outs.items()})
    args = (_ptr(indptr), _ptr(indices), _ptr(data), nnz, _ptr(groups), n, T, s, g, k, c["thr"], C.byref(struct), _ptr(ws))
    assert lib.saev_latent_exemplars(*args, need, _stream()) == 0, lib.saev_last_error(None)
    got = {name: v.cpu().numpy() for name, v in outs.items()}
    _assert_equal(got, _expected("groups_mixed"))
    np.testing.assert_array_equal(got["n_group_images"], _expected("groups_mixed")["n_group_images"])
    assert ws[:4].view(torch.int32).item() == 0
    assert lib.saev_latent_exemplars(*args, need - 1, _stream()) == -1


# ---------------------------------------------------------------- patch rows --------------------------------------------------------------

def _rows(c, latents, images):
    from saev_amd import engine

    return engine.latent_patch_rows(_t(c["indptr"]), _t(c["indices"]), _t(c["data"]), _t(np.asarray(latents)), _t(np.asarray(images)),
                                    n_images=c["n_images"], tokens_per_image=c["t"], n_latents=c["s"]).cpu().numpy()


def _scipy_rows(c, latents, images):
    """``ta[rows][:, j].toarray()`` per query, as the reference slices its patch values; an image of -1 gives zeros."""
    ta = K.scipy_csr(c)
    latents, images = np.asarray(latents), np.asarray(images)
    out = np.zeros(latents.shape + (c["t"],), dtype=np.float32)
    for at in np.ndindex(latents.shape):
        if images[at] >= 0:
            rows = np.arange(images[at] * c["t"], (images[at] + 1) * c["t"])
            out[at] = ta[rows][:, [int(latents[at])]].toarray()[:, 0]
    return out


@pytest.mark.parametrize("name", ["tokens_16", "groups_mixed", "ties", "values_thr_0"])
def test_patch_rows_of_the_lists_equal_scipys_slices(name):
    """The lists of a case passed straight in, padding slots included.  ``values_thr_0`` stores NaN, -0.0 and negatives: they come
    back on the bits (scipy's ``toarray`` ADDS the stored values to zeros and so turns -0.0 into +0.0; that case is held against
    the loop of the restatement alone)."""
    c, want = _case(name), _expected(name)
    latents = np.broadcast_to(np.arange(c["s"], dtype=np.int32)[:, None, None], want["top_img"].shape)
    for end in ("top_img", "bot_img", "silent_img"):
        got = _rows(c, latents, want[end])
        assert got.shape == want[end].shape + (c["t"],) and got.dtype == np.float32
        if name != "values_thr_0":
            assert np.array_equal(R.bits(got), R.bits(_scipy_rows(c, latents, want[end]))), end
        assert np.array_equal(R.bits(got), R.bits(R.patch_rows(c["indptr"], c["indices"], c["data"], c["t"], latents, want[end]))), end
    if name == "tokens_16":  # the patch of the maximum is where the patch vector has it
        got = _rows(c, latents, want["top_img"])
        held = want["top_img"] >= 0
        assert held.any() and (np.take_along_axis(got, np.maximum(want["top_patch"], 0)[..., None], axis=-1)[..., 0][held] == want["top_val"][held]).all()


def test_patch_rows_on_hand_made_queries():
    """Rows unsorted by column: the latent first and last in its row, absent from the image, image -1, Q = 0, Q = 1, T = 1 and 257,
    int64 queries, and more queries than one grid of workgroups."""
    ev = [(0, 0, 5, 1.5), (0, 0, 2, -2.0), (0, 0, 7, 3.0), (0, 2, 7, -0.0), (1, 1, 2, np.nan), (1, 1, 5, 4.0), (2, 0, 0, 8.0)]
    c = K.build(ev, n_images=3, t=3, s=8, groups=[0, 0, 0], g=1, k=2, shuffle_rows=1)
    c["indices"][:3], c["data"][:3] = [5, 2, 7], [1.5, -2.0, 3.0]  # row 0 as written: 5 first, 7 last, 2 between them
    lat, img = [5, 7, 2, 3, 7, 2, 0], [0, 0, 0, 0, -1, 1, 2]
    got = _rows(c, lat, img)
    want = np.zeros((7, 3), dtype=np.float32)
    want[0, 0], want[1, 0], want[1, 2], want[2, 0], want[5, 1], want[6, 0] = 1.5, 3.0, -0.0, -2.0, np.nan, 8.0
    assert np.array_equal(R.bits(got), R.bits(want)) and np.signbit(got[1, 2]) and np.isnan(got[5, 1])
    assert np.array_equal(R.bits(_rows(c, np.array(lat, dtype=np.int64).reshape(7, 1), np.array(img, dtype=np.int64).reshape(7, 1))), R.bits(want.reshape(7, 1, 3)))
    assert _rows(c, np.zeros((0, 4), np.int32), np.zeros((0, 4), np.int32)).shape == (0, 4, 3)
    assert np.array_equal(R.bits(_rows(c, [7], [0])), R.bits(want[1:2]))
    for name in ("tokens_1", "tokens_257"):
        c = _case(name)
        rng = np.random.default_rng(2)
        lat, img = rng.integers(0, c["s"], 50).astype(np.int32), rng.integers(-1, c["n_images"], 50).astype(np.int32)
        assert np.array_equal(R.bits(_rows(c, lat, img)), R.bits(_scipy_rows(c, lat, img))), name
    c = _case("tokens_1")  # 70 000 queries: past one grid of 65 536 workgroups
    q = 70_000
    lat, img = (np.arange(q) % c["s"]).astype(np.int32), (np.arange(q) % (c["n_images"] + 1) - 1).astype(np.int32)
    dense = np.concatenate([np.zeros((1, c["s"]), np.float32), K.scipy_csr(c).toarray()])
    assert np.array_equal(R.bits(_rows(c, lat, img)[:, 0]), R.bits(dense[img + 1, lat]))


@pytest.mark.parametrize("lat,img,match", [(8, 0, "latent"), (-1, 0, "latent"), (0, 3, "image"), (0, -2, "image")])
def test_patch_rows_error_word(lat, img, match):
    from saev_amd import engine

    c = K.build([(0, 0, 5, 1.5)], n_images=3, t=3, s=8, groups=[0, 0, 0], g=1, k=2)
    args = (_t(c["indptr"]), _t(c["indices"]), _t(c["data"]))
    with pytest.raises(ValueError, match=match + ".*found on the device"):
        engine.latent_patch_rows(*args, _t(np.array([5, lat], np.int32)), _t(np.array([0, img], np.int32)), n_images=3, tokens_per_image=3, n_latents=8)
    assert engine.latent_patch_rows(*args, _t(np.array([5], np.int32)), _t(np.array([0], np.int32)), n_images=3, tokens_per_image=3,
                                    n_latents=8).cpu().numpy().tolist() == [[1.5, 0.0, 0.0]]


# ---------------------------------------------------------------- the reference's surface -------------------------------------------------

@pytest.mark.parametrize("name", K.UNTIED)
def test_the_deduplicated_top_tokens_are_a_prefix_of_the_top_images(name):
    """``csr_topk(token_acts, k, axis=0).indices // T`` of the reference's visuals.py lists the top TOKENS; without its repeats it is
    the head of the top-image list (the values of the case are all different, so neither order has a tie to break)."""
    from saev_amd import exemplars, helpers

    c = _case(name)
    ta, top_k = K.scipy_csr(c), 8
    tokens = helpers.csr_topk(ta, k=top_k, axis=0)
    img, val, patch = exemplars.top_images(ta, c["t"], top_k)
    one = R.restate(**dict(c, groups=np.zeros(c["n_images"], np.int32), g=1, k=top_k))
    assert np.array_equal(img, one["top_img"][:, 0]) and np.array_equal(R.bits(val), R.bits(one["top_val"][:, 0])) and np.array_equal(patch, one["top_patch"][:, 0])
    shorter = 0
    for j in range(c["s"]):
        rows = tokens.indices[:, j][tokens.values[:, j] > 0]
        images = rows // c["t"]
        distinct = images[np.sort(np.unique(images, return_index=True)[1])]
        shorter += len(distinct) < len(images)
        assert len(distinct) > 0 and img[j, :len(distinct)].tolist() == distinct.tolist(), j
        first = np.sort(np.unique(images, return_index=True)[1])
        assert patch[j, :len(distinct)].tolist() == (rows[first] % c["t"]).tolist() and val[j, :len(distinct)].tolist() == tokens.values[:, j][first].tolist()
    assert shorter > 0 or c["t"] == 1  # the reference's gallery really comes out short of k images


# ---------------------------------------------------------------- the module and the tool -------------------------------------------------

N_IMG, T, S = 48, 12, 40
LABELS = ["erato", "melpomene", "other"]


@pytest.fixture(scope="module")
def run_dir(tmp_path_factory):
    """A run directory with token_acts.npz of 48 images x 12 tokens and shards with image_labels.csv: latent 0 fires in every erato
    image and in two melpomene ones, latent 1 in every image, the others at random."""
    from saev_amd.data import write_shards

    root = tmp_path_factory.mktemp("exemplars")
    rng = np.random.default_rng(41)
    dense = np.where(rng.random((N_IMG, T, S)) < 0.04, rng.random((N_IMG, T, S)) + 0.1, 0.0).astype(np.float32)
    labels = [LABELS[i % 3] for i in range(N_IMG)]
    dense[..., 0] = 0
    dense[0::3, 5, 0] = 1.0 + rng.random(N_IMG // 3)
    dense[[1, 7], 2, 0] = [9.0, 0.5]
    dense[..., 1] = 0
    dense[:, 3, 1] = 2.0
    ta = scipy.sparse.csr_matrix(dense.reshape(N_IMG * T, S))
    shards = write_shards(root / "shards" / "abc", np.zeros((N_IMG, 1, T, 4), dtype=np.float32))
    (shards / "image_labels.csv").write_text("stem,species\n" + "".join(f"i{k},{lbl}\n" for k, lbl in enumerate(labels)))
    d = root / "run0" / "inference" / shards.name
    d.mkdir(parents=True)
    scipy.sparse.save_npz(str(d / "token_acts.npz"), ta)
    groups = np.array([i % 3 for i in range(N_IMG)], dtype=np.int32)
    return root / "run0", shards, ta, groups


def test_worker_fn_writes_the_lists_and_the_patch_vectors(run_dir):
    from saev_amd import exemplars

    run, shards, ta, groups = run_dir
    k = 4
    fpath = exemplars.worker_fn(exemplars.Config(run=run, shards=shards, group_col="species", k=k, patch_latents=5, min_images=8))
    assert fpath == run / "inference" / shards.name / "latent_exemplars.npz"
    c = dict(indptr=ta.indptr.astype(np.int64), indices=ta.indices, data=ta.data, n_images=N_IMG, t=T, s=S, groups=groups, g=3, k=k)
    want = R.restate(**c)
    with np.load(fpath) as z:
        assert tuple(z.files) == exemplars.KEYS and z["group_names"].tolist() == LABELS and z["n_group_images"].tolist() == [16, 16, 16]
        for name in R.ARRAYS:
            assert z[name].dtype == want[name].dtype and np.array_equal(R.bits(z[name]), R.bits(want[name])), name
        chosen = z["patch_latents"]
        assert chosen.dtype == np.int64 and np.array_equal(chosen, exemplars.choose_patch_latents(want["n_fire"], want["n_group_images"], 5, 8))
        assert len(chosen) == 5 and chosen[0] == 0  # latent 0: rate 1 on erato against 2 / 16 (too few to count) and 0: the largest spread there is
        lat = np.broadcast_to(chosen[:, None, None], (5, 3, k))
        for end in ("top", "bot"):
            assert z["patch_" + end].dtype == np.float32 and z["patch_" + end].shape == (5, 3, k, T)
            assert np.array_equal(R.bits(z["patch_" + end]), R.bits(R.patch_rows(c["indptr"], c["indices"], c["data"], T, lat, want[end + "_img"][chosen])))
        assert z["top_img"][0, 1].tolist() == [1, 7, -1, -1] and z["top_val"][0, 1].tolist() == [9.0, 0.5, 0.0, 0.0] and z["top_patch"][0, 1, 0] == 2
        assert z["patch_top"][0, 1, 0].tolist() == [0, 0, 9.0] + [0] * 9 and (z["patch_top"][0, 1, 2:] == 0).all()
        ce = exemplars.counter_examples({key: z[key] for key in z.files}, 0, 0, 1)
        assert ce["n_false_negatives"] == 0 and ce["false_negatives"] == [] and ce["n_false_positives"] == 2
        assert [r["image"] for r in ce["false_positives"]] == [1, 7] and ce["false_positives"][0] == dict(image=1, value=9.0, patch=2)
    # a given list of latents, no grouping: one group of all images
    fpath = exemplars.worker_fn(exemplars.Config(run=run, shards=shards, k=2, patch_latents=(1, 7)))
    with np.load(fpath) as z:
        assert z["patch_latents"].tolist() == [1, 7] and z["group_names"].tolist() == ["all"] and z["n_group_images"].tolist() == [N_IMG]
        one = R.restate(**dict(c, groups=np.zeros(N_IMG, np.int32), g=1, k=2))
        for name in R.ARRAYS:
            assert np.array_equal(R.bits(z[name]), R.bits(one[name])), name
        assert z["top_img"][1, 0].tolist() == [0, 1] and z["patch_top"].shape == (2, 1, 2, T) and z["patch_top"][0, 0, 0, 3] == 2.0
    with pytest.raises(ValueError, match="k = 33"):
        exemplars.worker_fn(exemplars.Config(run=run, shards=shards, k=33))


def test_tool_main(run_dir, capsys):
    run, shards, ta, groups = run_dir
    spec = importlib.util.spec_from_file_location("latent_exemplars_tool", ROOT / "tools" / "latent_exemplars.py")
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    out = tool.main(["--run", str(run), "--shards", str(shards), "--group-col", "species", "-k", "4"])
    text = capsys.readouterr().out
    assert out["n_latents"] == S and out["groups"] == LABELS and 0.0 < out["short_fraction"] < 1.0 and "fewer than k firing images" in text
    out = tool.main(["--run", str(run), "--shards", str(shards), "--group-col", "species", "-k", "4", "--latent", "0", "--pos", "erato", "--neg", "melpomene"])
    text = capsys.readouterr().out
    assert out["latent"] == 0 and out["strips"]["melpomene"]["top"][0] == dict(image=1, value=9.0, patch=2) and out["strips"]["erato"]["n_fire"] == 16
    assert out["strips"]["other"]["silent"] == [2, 5, 8, 11] and out["top_image"] == 1 and out["top_image_group"] == "melpomene"
    assert out["top_image_patches"][2] == 9.0 and out["counter_examples"]["n_false_positives"] == 2 and out["counter_examples"]["false_negatives"] == []
    assert "1:9@2 7:0.5@2" in text and "false positives (2 images of 'melpomene' fire)" in text and ". . 9" in text
