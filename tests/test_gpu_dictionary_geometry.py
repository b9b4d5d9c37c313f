"""The two dictionary filters on pairs their fp16 images misorder (needs -m gpu): saev_dictionary_match and
saev_dictionary_coherence on the inputs of dictionary_cases.py, whose image argmax is wrong by more than 8 tol(D) for a quarter to
two thirds of the rows while fp64 decides every asserted index by more than 4 tol(D) (test_dictionary_cases_host_cpu.py proves both
on the CPU for the same bits).  Only a filter whose bound E >= |c~ - c| holds keeps the true maximiser among its candidates there,
so here index EQUALITY with the planted answer is the assertion, and the number of candidates and of revisited tiles must lie inside
the bracket the restated rule derives (dictionary_restatement.py) -- a bound too loose overflows, a bound too tight drops pairs, and
either moves the count.

Values use test_gpu_dictionary_match's and test_gpu_coherence's tol(D) and checks; nothing is measured into a tolerance here.
The largest input is 4 800 x 16 floats (2 400 x 64 at D = 64)."""

import functools
import struct

import pytest
import torch

import dictionary_cases as K
import dictionary_restatement as R
import test_gpu_coherence as COH
import test_gpu_dictionary_match as DM

pytestmark = [pytest.mark.gpu, pytest.mark.encoder_modes("f32")]

DEV = DM.DEV
PLANTED = ["decoys", "decoys_absolute", "decoys_d64", "decoys_overflow", "decoys_self"]


@functools.lru_cache(maxsize=None)
def match_case(name):
    """The case, its tensors on the device, the fp64 reference (best, second, argmax per row) and, from the restated rule on the CPU
    tensors, the brackets of candidates and tiles.  Computed once per case and left unchanged."""
    c = K.MATCH_CASES[name]()
    A, B = c.A.to(DEV), None if c.B is None else c.B.to(DEV)
    kw = dict(absolute=c.absolute, self_mode=c.self_mode)
    return c, A, B, DM.fp64_rows(A, B, c.absolute), R.match_bracket(c.A, c.B, **kw), R.match_tile_bracket(c.A, c.B, **kw)


@functools.lru_cache(maxsize=None)
def coherence_case(D):
    W, pair = K.planted_pairs(D)
    return W.to(DEV), pair, R.coherence_bracket(W), R.coherence_tile_bracket(W)


def check_rows(name, r):
    """Values and pairs against fp64, index equality where fp64 decides it -- for the planted rows that is every row, and the index
    is the planted one."""
    c, A, B, ref, _, _ = match_case(name)
    if c.planted is None or c.self_mode:
        DM.check(A, B, r, c.absolute, ref=ref)
    else:
        DM.check(A, B, r, c.absolute, every_index=True, ref=ref)
    if c.planted is not None:
        n = c.planted.numel()
        best, second, _ = ref
        assert (best[:n] - second[:n] > 4 * DM.tol(c.D)).all()
        wrong = r.indices[:n].long() != c.planted.to(DEV)
        assert not wrong.any(), (int(wrong.sum()), wrong.nonzero()[:5].flatten().tolist())


def in_bracket(label, got, bracket):
    sure, maybe = bracket
    print(f"{label}: {got} in [{sure}, {maybe}]")
    assert sure <= got <= maybe, (label, got, bracket)


@pytest.mark.parametrize("name", sorted(K.MATCH_FILTER_CASES))
def test_the_filter_keeps_the_maximiser_the_images_misorder(name):
    c, A, B, _, cand, tiles = match_case(name)
    r = DM.match(A, B, absolute=c.absolute)
    assert r.route == "filter" and not r.overflow and r.capacity == R.match_capacity(*c.shape, c.self_mode), r
    check_rows(name, r)
    in_bracket(f"{name} candidates", r.candidates, cand)
    in_bracket(f"{name} tiles", r.tiles_refiltered, tiles)
    r2 = DM.match(A, B, absolute=c.absolute)
    assert DM.same_bits(r, r2) and (r2.candidates, r2.tiles_refiltered) == (r.candidates, r.tiles_refiltered)


@pytest.mark.parametrize("name", sorted(K.MATCH_FILTER_CASES))
def test_the_exact_route_gives_the_same_indices(name):
    c, A, B, ref, _, _ = match_case(name)
    auto, exact = DM.match(A, B, absolute=c.absolute), DM.match(A, B, absolute=c.absolute, route="exact")
    assert auto.route == "filter" and exact.route == "exact" and not exact.overflow and exact.candidates == 0, (auto, exact)
    check_rows(name, exact)
    assert (auto.values.double() - exact.values.double()).abs().max().item() <= 2 * DM.tol(c.D)
    clear = ref[0] - ref[1] > 4 * DM.tol(c.D)
    assert torch.equal(auto.indices[clear], exact.indices[clear])


@pytest.mark.parametrize("name", sorted(K.MATCH_OVERFLOW_CASES))
def test_more_candidates_than_the_list_holds_take_the_exact_route(name):
    c, A, B, _, cand, _ = match_case(name)
    r = DM.match(A, B, absolute=c.absolute)
    assert r.route == "exact" and r.overflow and r.candidates > r.capacity == R.match_capacity(*c.shape) == 4096, r
    in_bracket(f"{name} candidates", r.candidates, cand)  # (the count goes on past the capacity)
    check_rows(name, r)
    e = DM.match(A, B, absolute=c.absolute, route="exact")
    assert e.route == "exact" and not e.overflow and e.candidates == 0, e
    assert DM.same_bits(r, e)


@pytest.mark.parametrize("D", K.COHERENCE_DS)
def test_coherence_finds_the_planted_pair_the_images_misorder(D):
    W, pair, cand, tiles = coherence_case(D)
    want = COH.fp64_max(W)
    assert abs(COH.fp64_pair(W, *pair) - want) <= 1e-12  # (the planted pair is the fp64 maximiser: proved on the CPU)
    r = COH.coherence(W)
    assert r.route == "filter" and not r.overflow and r.capacity == R.coherence_capacity(W.shape[0]), r
    assert (r.i, r.j) == pair, (r, pair)
    COH.check(W, r, want=want)
    in_bracket(f"planted pairs D={D} candidates", r.candidates, cand)
    in_bracket(f"planted pairs D={D} tiles", r.tiles_refiltered, tiles)
    r2 = COH.coherence(W)
    assert struct.pack("f", r.value) == struct.pack("f", r2.value) and (r2.i, r2.j, r2.candidates) == (r.i, r.j, r.candidates)
    e = COH.coherence(W, route="exact")
    assert e.route == "exact" and not e.overflow and (e.i, e.j) == pair, (e, pair)
    COH.check(W, e, want=want)
    assert abs(e.value - r.value) <= 2 * COH.tol(D)


def test_coherence_is_the_largest_absolute_self_match_on_the_decoys():
    """decoys_self: the two entries refine different candidate sets in different kernels and must name the same pair (fp64 decides it
    by hundreds of tol: test_dictionary_cases_host_cpu.py)."""
    c, W, _, _, _, _ = match_case("decoys_self")
    m, r = DM.match(W, absolute=True), COH.coherence(W)
    assert m.route == "filter" and r.route == "filter" and not m.overflow and not r.overflow, (m, r)
    in_bracket("decoys_self absolute candidates", m.candidates, R.match_bracket(c.A, None, absolute=True, self_mode=True))
    in_bracket("decoys_self coherence candidates", r.candidates, R.coherence_bracket(c.A))
    COH.check(W, r)
    top = m.values.max().item()
    assert abs(top - r.value) <= COH.tol(c.D), (top, r)
    i = int(m.values.argmax())
    assert i in (r.i, r.j) and int(m.indices[i]) in (r.i, r.j) and int(m.indices[i]) != i, (i, int(m.indices[i]), r)
    assert int(m.indices[r.i]) == r.j and int(m.indices[r.j]) == r.i
    DM.check(W, None, m, True)
