"""CPU checks of the inputs of tests/test_gpu_latent_major.py (tests/latent_major_cases.py): from the library's own workspace sizing
and the formulas restated there, every case does what it is named for -- a change of LM_PARTS or of the part rule cannot quietly turn
the cases into ones that reach no branch -- and the restatement equals a count written another way."""

import subprocess

import numpy as np
import pytest

import latent_major_cases as K
from conftest import ROOT


@pytest.fixture(scope="module")
def lib():
    subprocess.run(["make", "-C", str(ROOT)], check=True, capture_output=True)
    from saev_amd import _lib

    return _lib.load()


@pytest.fixture(scope="module")
def cases():
    return {name: make() for name, make in K.ALL.items()}


def _nnz(c):
    return int(c["indices"].size)


def _laid_out(lib, c):
    """The parts the library lays out for the case, from the size of its count table inside saev_latent_spatial_workspace_bytes."""
    nnz, s = _nnz(c), c["s"]
    size = lib.saev_latent_spatial_workspace_bytes(c["n_images"], K.T, s, c["g"], nnz)
    cnt = size - 256 - K._r256(8 * (s + 1)) - K._r256(4 * s) - 3 * K._r256(4 * nnz)
    parts, part_len = K.parts_of(s, nnz)
    assert cnt == K._r256(4 * parts * s) and (parts == 1 or K._r256(4 * (parts - 1) * s) < cnt)
    return parts, part_len


def _trips(c):
    """The latents of the events of every trip of the place pass (-1: no event, or past the part's end)."""
    nnz = _nnz(c)
    _, part_len = K.parts_of(c["s"], nnz)
    ev, _ = K.is_event(c)
    col = np.where(ev, c["indices"], -1)
    out = []
    for first in range(0, nnz, part_len):
        last = min(first + part_len, nnz)
        for g in range(first, last, K.TRIP):
            out.append(np.concatenate([col[g:min(g + K.TRIP, last)], np.full(max(0, g + K.TRIP - last), -1)]))
    return np.array(out).reshape(-1, K.TRIP)


@pytest.mark.parametrize("name", list(K.ALL))
def test_both_entries_keep_the_regroup_at_the_restated_offsets(lib, cases, name):
    c = cases[name]
    nnz, s = _nnz(c), c["s"]
    off = K.offsets(s, nnz)
    assert lib.saev_latent_spatial_workspace_bytes(c["n_images"], K.T, s, c["g"], nnz) == off["end"]
    assert lib.saev_latent_exemplars_workspace_bytes(nnz, s, c["n_images"], c["g"]) == off["end"] + 2 * K._r256(4 * c["n_images"]) + K._r256(4 * 65)
    assert all(v % 256 == 0 for v in off.values()) and off["starts"] < off["row"] < off["val"] < off["end"]
    assert c["indptr"][0] == 0 and c["indptr"][-1] == nnz and c["indptr"].size == c["n_images"] * K.T + 1
    assert c["s"] * c["g"] * K.T < 2**31


def test_three_trips_a_part_fewer_parts_used_than_laid_out_and_a_ragged_tail(lib, cases):
    c = cases["three_trips"]
    parts, part_len = _laid_out(lib, c)
    nnz = _nnz(c)
    used = -(-nnz // part_len)
    assert 140_000 < nnz < 160_000 and parts == K.LM_PARTS and part_len == 3 * K.TRIP
    assert 1 < used < parts and 0 < nnz % part_len and nnz % K.TRIP != 0
    assert K.is_event(c)[0].all()


def test_cap_binds_the_parts_at_512(lib, cases):
    c = cases["cap"]
    parts, part_len = _laid_out(lib, c)
    nnz = _nnz(c)
    assert c["s"] == 131072 and 95_000 < nnz < 105_000
    assert parts == K.LM_CNT_ENTRIES // c["s"] == 512 < min(K.LM_PARTS, -(-nnz // 64)) and part_len == 4 * K.TRIP
    starts, _, _ = K.restate(c)
    counts = np.diff(starts)
    assert (counts == 0).sum() > 100_000 and counts[-1] == 0 and counts.max() > 1 and c["s"] / 1024 == 128


def test_one_latent_64_times_in_a_trip_and_64_distinct_latents_in_another(lib, cases):
    c = cases["one_and_distinct"]
    _, part_len = _laid_out(lib, c)
    trips = _trips(c)
    distinct = np.array([np.unique(t).size for t in trips])
    assert part_len == K.TRIP and K.is_event(c)[0].all() and (trips >= 0).all()
    assert (trips[:4] == 0).all() and (distinct[:4] == 1).all()
    assert (distinct[4:] == K.TRIP).all() and distinct.size > 8 and (trips[4::2, 0] == 0).all()


def test_no_events_holds_every_kind_of_entry_that_is_none(cases):
    c = cases["no_events"]
    ev, rows = K.is_event(c)
    grp = c["groups"][rows // K.T]
    thr = np.float32(c["thr"])
    assert c["thr"] == 0.5 and ((grp < 0) & (c["data"] > thr)).sum() > 50 and (grp >= 0).sum() > 1000
    assert (c["data"][grp >= 0] == thr).sum() > 50 and (c["data"][grp >= 0] < thr).sum() > 50 and np.isnan(c["data"]).sum() == 1
    assert grp[np.isnan(c["data"])][0] >= 0
    stored = np.bincount(c["indices"], minlength=c["s"])
    fired = np.bincount(c["indices"][ev], minlength=c["s"])
    assert (stored[:5] == 0).all() and (stored[5:11] > 0).all() and (fired[:11] == 0).all() and (fired[11:] > 0).all()
    assert 0 < ev.sum() < ev.size


def test_the_smallest_cases(lib, cases):
    assert _nnz(cases["empty"]) == 0 and _laid_out(lib, cases["empty"]) == (1, 64)
    assert K.restate(cases["empty"])[0].tolist() == [0] * (cases["empty"]["s"] + 1)
    c = cases["under_a_trip"]
    assert 0 < _nnz(c) < K.TRIP and _laid_out(lib, c) == (1, 64) and 0 < K.is_event(c)[0].sum() < _nnz(c)


def test_the_shifted_case_reads_nothing_in_front_of_its_rows(cases):
    c, nnz = K.shifted(cases["no_events"])
    assert c["indptr"][0] == K.SHIFT and c["indptr"][-1] == K.SHIFT + nnz == c["indices"].size
    assert (c["indices"][:K.SHIFT] == c["s"]).all() and np.isnan(c["data"][:K.SHIFT]).all()
    np.testing.assert_array_equal(c["indices"][K.SHIFT:], cases["no_events"]["indices"])


@pytest.mark.parametrize("name", ["no_events", "under_a_trip", "one_and_distinct"])
def test_restatement_equals_a_walk_latent_by_latent(cases, name):
    """The same lists by a loop over the latents and the rows, without a sort."""
    c = cases[name]
    thr = np.float32(c["thr"])
    lists = [[] for _ in range(c["s"])]
    for row in range(c["indptr"].size - 1):
        if c["groups"][row // K.T] < 0:
            continue
        for p in range(c["indptr"][row], c["indptr"][row + 1]):
            if c["data"][p] > thr:
                lists[c["indices"][p]].append((row, p))
    starts, rows, vals = K.restate(c)
    assert starts[-1] == rows.size == vals.size == sum(map(len, lists))
    for j, events in enumerate(lists):
        assert starts[j + 1] - starts[j] == len(events)
        assert rows[starts[j]:starts[j + 1]].tolist() == [r for r, _ in events]
        np.testing.assert_array_equal(vals[starts[j]:starts[j + 1]].view(np.uint32), c["data"][[p for _, p in events]].view(np.uint32))
        assert np.all(np.diff(rows[starts[j]:starts[j + 1]]) > 0)
