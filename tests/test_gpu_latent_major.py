"""GPU tests of the latent-major regroup (saev_amd/csrc/latent_major.h) as latent_spatial and latent_exemplars leave it
in their workspace: ``starts``, and ``row`` and ``val`` up to ``starts[S]``, against the numpy restatement of
tests/latent_major_cases.py.  No tolerance: integers equal, floats equal on the bits; what lies past ``starts[S]`` is unspecified
and is not looked at.  (probe1d.hip sorts with kernels of its own; test_gpu_probe1d_geometry.py, section A, checks those the same way.)

The cases are those of tests/latent_major_cases.py -- three trips a part with a ragged last part, the part count capped by S, a trip
of one latent and a trip of 64 latents, every kind of entry that is no event, no entry, fewer entries than a trip, an indptr of
absolute positions -- and tests/test_latent_major_host_cpu.py checks on the CPU that they are."""

import functools

import numpy as np
import pytest
import torch

import latent_major_cases as K

pytestmark = [pytest.mark.gpu, pytest.mark.encoder_modes("f32")]
DEV = "cuda"
ENTRIES = ("latent_spatial", "latent_exemplars")


@functools.lru_cache(maxsize=None)
def _case(name):
    return K.ALL[name]()


@functools.lru_cache(maxsize=None)
def _expected(name):
    return K.restate(_case(name))


def _run(entry, c, nnz=None):
    from saev_amd import engine

    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    common = dict(n_images=c["n_images"], n_latents=c["s"], groups=t(c["groups"]), n_groups=c["g"], threshold=c["thr"], nnz=nnz)
    if entry == "latent_spatial":
        return engine.latent_spatial(t(c["indptr"]), t(c["indices"]), t(c["data"]), grid=(c["gh"], c["gw"]), sum_map=False, **common)
    return engine.latent_exemplars(t(c["indptr"]), t(c["indices"]), t(c["data"]), tokens_per_image=c["gh"] * c["gw"], k=1, **common)


def _left_by_prepare(res, s, nnz):
    """(starts, row[:starts[S]], val[:starts[S]] by its bits) out of the result's retained workspace."""
    res.check()
    off = K.offsets(s, nnz)
    assert res._ws.numel() >= off["end"]
    part = lambda at, n, dtype: res._ws[at:at + n].cpu().numpy().view(dtype)  # noqa: E731  (the count table stays on the device)
    starts = part(off["starts"], 8 * (s + 1), np.int64)
    total = int(starts[s])
    assert 0 <= total <= nnz
    return starts, part(off["row"], 4 * total, np.int32), part(off["val"], 4 * total, np.uint32)


def _assert_same(got, want):
    starts, row, val = want
    np.testing.assert_array_equal(got[0], starts, err_msg="starts")
    np.testing.assert_array_equal(got[1], row, err_msg="row")  # ascending inside every latent: the stable order
    np.testing.assert_array_equal(got[2], val.view(np.uint32), err_msg="val")


@pytest.mark.parametrize("name", list(K.ALL))
def test_both_entries_leave_the_restated_lists(name):
    c = _case(name)
    nnz = int(c["indices"].size)
    left = [_left_by_prepare(_run(entry, c), c["s"], nnz) for entry in ENTRIES]
    for got in left:
        _assert_same(got, _expected(name))
    for a, b in zip(*left):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("entry", ENTRIES)
def test_indptr_holds_absolute_positions(entry):
    """indices and data are read from their base pointers at indptr's positions; the SHIFT entries in front (an index out of range,
    a NaN value) are never looked at, and the error word stays 0."""
    c, nnz = K.shifted(_case("no_events"))
    _assert_same(_left_by_prepare(_run(entry, c, nnz=nnz), c["s"], nnz), _expected("no_events"))
