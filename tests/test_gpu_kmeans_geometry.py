"""GPU tests of the k-means kernels where they change behaviour (kmeans.hip): more tiles than persistent workgroups,
the API's largest n and k (the refinement and the exact route stride, the scan gives a thread 1 024 centres), exact ties in
different 128-wide tiles, centred rows without a unit image, rows of mixed norms and inputs rescaled by powers of two, and the
group's switch between its two sort paths with entries outside [0, k).

The rules are test_gpu_kmeans.py's: check_assign (both routes against fp64), same_bits (auto == exact), and check_filter wherever
the filter is expected to answer -- route == "filter", no overflow, and the device's candidate count inside the bracket of the
restated rule computed on the same device tensors.  The inputs come from kmeans_cases; test_kmeans_host_cpu.py checks on the CPU
that they meet the conditions asserted here.  Every shape is the smallest that reaches its loop."""

import pytest
import torch

import kmeans_cases as K
import kmeans_restatement as R
from test_gpu_kmeans import DEV, check_assign, check_filter, check_group, check_group_and_update, d2_64, same_bits, tol

pytestmark = [pytest.mark.gpu, pytest.mark.encoder_modes("f32")]


def both_routes(X, C, farthest, label, bracket=None):
    """auto and exact against fp64 and against each other; with a bracket, the filter answered inside it."""
    from saev_amd.engine import kmeans_assign

    auto = kmeans_assign(X, C, farthest=farthest)
    exact = kmeans_assign(X, C, farthest=farthest, route="exact")
    assert exact.route == "exact" and not exact.overflow
    check_assign(auto, X, C, farthest, label)
    check_assign(exact, X, C, farthest, label + " (exact)")
    assert same_bits(auto, exact), "both routes return the same bits"
    if bracket is not None:
        check_filter(auto, bracket, f"{label} farthest={farthest}")
    return auto


def more_tiles_than_workgroups(n, k):
    """The persistent filter runs 2 x (compute units) workgroups: the shape must leave every one of them a second tile."""
    tiles = -(-n // 128) * -(-k // 128)
    groups = 2 * torch.cuda.get_device_properties(0).multi_processor_count
    print(f"{tiles} tiles of 128 x 128 for {groups} persistent workgroups")
    assert tiles > groups, "this shape no longer reaches the second trip of the tile loop on this part"


def test_assign_with_more_tiles_than_persistent_workgroups():
    n, k, D = K.GRID
    more_tiles_than_workgroups(n, k)
    X, C = (t.to(DEV) for t in K.gaussian(n, k, D))
    brackets = R.candidate_brackets(X, C)
    for farthest in (False, True):
        both_routes(X, C, farthest, f"grid {K.GRID}", brackets[farthest])


def test_collapsed_with_more_tiles_than_persistent_workgroups():
    from saev_amd.engine import kmeans_collapsed

    k, D = K.GRID[1:]
    more_tiles_than_workgroups(k, k)
    C, counts = K.collapsed_case(k, D)
    tol_ = K.COLLAPSED_TOL
    want = torch.from_numpy(R.collapsed(C.numpy(), counts.numpy(), tol_))
    assert int(want.sum()) == 6, "the planted losers and no others"
    C, counts = C.to(DEV), counts.to(DEV)
    p2 = d2_64(C, C)[tuple(torch.triu_indices(k, k, 1).to(DEV))]
    gap = ((p2 - tol_ * tol_).abs() / torch.maximum(p2, torch.tensor(tol_ * tol_, device=DEV))).min().item()
    print(f"collapsed ({k}, {D}): smallest relative gap to tol^2 {gap:.3g} against 4 tol(D) = {4 * tol(D):.3g}")
    assert gap > 4 * tol(D), "the gap: fp64 decides every pair"
    auto, exact = kmeans_collapsed(C, counts, tol_), kmeans_collapsed(C, counts, tol_, route="exact")
    assert exact.route == "exact" and not exact.overflow
    assert torch.equal(auto.losers.cpu(), want) and torch.equal(exact.losers.cpu(), want)
    check_filter(auto, R.collapsed_bracket(C, tol_), f"collapsed ({k}, {D})")


def test_assign_and_group_at_the_largest_n():
    """n = 2^20 against three centres at D = 4: 8 192 filter tiles, more candidates than the refinement has threads (4 096 x 256),
    16 384 exact-route tiles for 8 192 workgroups; then the group of n rows into three segments, each far past the LDS sort."""
    n = 2 ** 20
    X, C = (t.to(DEV) for t in K.three_centres(n))
    brackets = R.candidate_brackets(X, C)
    d = d2_64(X[:2000], C)
    for farthest in (False, True):
        res = both_routes(X, C, farthest, "three centres, n = 2^20", brackets[farthest])
        assert res.candidates > 4096 * 256, "the refinement strides"
        idx = res.indices[:2000].long()
        if not farthest:  # the tied rows: centre 0 before centre 1 wherever centre 2 is not nearer by the gap rule
            tie, other = d[:, 0], d[:, 2]
            assert int(((idx == 1)).sum()) == 0
            zero_wins = tie < other * (1 - 4 * tol(4))
            assert int(zero_wins.sum()) > 1000 and bool((idx[zero_wins] == 0).all())
        else:  # farthest: centre 2 or the tie; the tie goes to centre 0
            assert int((idx == 1).sum()) == 0
        check_group(res.indices.cpu(), 3)


def test_assign_at_the_largest_k():
    """Three rows against k = 2^20 centres at D = 4: one row tile against 8 192 centre tiles, so L_i is raised by 8 192 workgroups,
    and the column sums of the centring vector take 16 384 rows per chunk."""
    X, C = (t.to(DEV) for t in K.many_centres())
    brackets = R.candidate_brackets(X, C)
    for farthest in (False, True):
        both_routes(X, C, farthest, "k = 2^20", brackets[farthest])


@pytest.mark.parametrize("kind", ["permutation", "randint"])
def test_group_at_the_largest_n_and_k(kind):
    g = torch.Generator().manual_seed(71)
    n = k = 2 ** 20
    idx = (torch.randperm(n, generator=g) if kind == "permutation" else torch.randint(0, k, (n,), generator=g)).to(torch.int32)
    check_group(idx, k)


def test_assign_ties_in_different_tiles():
    X, C = (t.to(DEV) for t in K.tied_tiles())
    brackets = R.candidate_brackets(X, C)
    for farthest in (False, True):
        res = both_routes(X, C, farthest, "tied tiles", brackets[farthest])
        assert int(res.indices.max()) < 500, "of two exact copies the one with the smaller index"
        assert res.candidates >= 2 * X.shape[0]


def test_assign_a_row_without_a_unit_image_takes_the_exact_route():
    from saev_amd.engine import kmeans_assign

    for name, (X, C) in (("a row of X", K.no_image_row_of_x()), ("a centre", K.no_image_centre())):
        X, C = X.to(DEV), C.to(DEV)
        for farthest in (False, True):
            res = kmeans_assign(X, C, farthest=farthest)
            print(f"no unit image, {name}: route {res.route}, overflow {res.overflow}, candidates {res.candidates}")
            assert res.overflow and res.route == "exact" and res.candidates == 0
            exact = kmeans_assign(X, C, farthest=farthest, route="exact")
            assert exact.route == "exact" and not exact.overflow and same_bits(res, exact)
            check_assign(res, X, C, farthest, f"no unit image, {name}")


def test_collapsed_a_centre_without_a_unit_image_takes_the_exact_route():
    from saev_amd.engine import kmeans_collapsed

    C = K.no_image_centre()[1]
    counts = torch.ones(65)
    tol_ = 18.5  # (between the mean's distances to the integer centres, about 19.6, and far from every squared distance: the gap below)
    want = torch.from_numpy(R.collapsed(C.numpy(), counts.numpy(), tol_))
    p2 = d2_64(C.to(DEV), C.to(DEV))[tuple(torch.triu_indices(65, 65, 1).to(DEV))]
    gap = ((p2 - tol_ * tol_).abs() / torch.maximum(p2, torch.tensor(tol_ * tol_, device=DEV))).min().item()
    assert gap > 4 * tol(16), "the gap: fp64 decides every pair"
    assert 0 < int(want.sum()) < 65
    auto, exact = kmeans_collapsed(C.to(DEV), counts.to(DEV), tol_), kmeans_collapsed(C.to(DEV), counts.to(DEV), tol_, route="exact")
    print(f"collapsed, no unit image: route {auto.route}, overflow {auto.overflow}, candidates {auto.candidates}, losers {int(want.sum())}")
    assert auto.overflow and auto.route == "exact" and auto.candidates == 0
    assert exact.route == "exact" and not exact.overflow
    assert torch.equal(auto.losers.cpu(), want) and torch.equal(exact.losers.cpu(), want)


def test_assign_rows_of_mixed_norms():
    X, C = (t.to(DEV) for t in K.mixed_norms(1))
    brackets = R.candidate_brackets(X, C)
    for farthest in (False, True):
        both_routes(X, C, farthest, "norms 10^U(-1, 1)", brackets[farthest])


def test_assign_rows_of_widely_mixed_norms_whichever_route():
    """Norms over six decades: the fp32 distances cannot separate a small row's centres of large norm either, the bound says so
    (about 430 candidates per row for the nearest centre) and the call overflows.  Correct on whichever route it takes."""
    X, C = (t.to(DEV) for t in K.mixed_norms(3))
    for farthest in (False, True):
        res = both_routes(X, C, farthest, "norms 10^U(-3, 3)")
        print(f"norms 10^U(-3, 3) farthest={farthest}: route {res.route}, overflow {res.overflow}, candidates {res.candidates} of {res.capacity}")


@pytest.mark.parametrize("scale", K.SCALES, ids=["2^-40", "2^50"])
def test_assign_is_exact_under_a_power_of_two_rescaling(scale):
    """Every operation of the refined value scales exactly by a power of two (|entries| < 8, D = 128: no under- or overflow), so
    dist2 scales bit for bit and the indices stay; a difference is an absolute constant acting where it should not.  The filter
    still answers, with the candidates of the scaled input's own bracket."""
    from saev_amd.engine import kmeans_assign

    X, C = (t.to(DEV) for t in K.gaussian(*K.SCALED_SHAPE))
    assert float(X.abs().max()) < 8 and float(C.abs().max()) < 8
    sX, sC = X * scale, C * scale
    brackets = R.candidate_brackets(sX, sC)
    for farthest in (False, True):
        for route in ("auto", "exact"):
            base = kmeans_assign(X, C, farthest=farthest, route=route)
            res = kmeans_assign(sX, sC, farthest=farthest, route=route)
            assert torch.equal(res.dist2, base.dist2 * (scale * scale)), "dist2 scales bit for bit"
            assert torch.equal(res.indices, base.indices)
        both_routes(sX, sC, farthest, f"scaled by {scale:.3g}", brackets[farthest])


@pytest.mark.parametrize("D", [4, 68])
def test_group_and_update_at_the_switch_between_the_sort_paths(D):
    idx, k = K.group_edges()
    check_group_and_update("group edges", idx, k, D)
