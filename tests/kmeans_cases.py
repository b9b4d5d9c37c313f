"""The inputs of the k-means tests, as functions of nothing but their arguments (CPU tensors from seeded generators), so that the host
tests (test_kmeans_host_cpu.py) can check on the CPU, with the restated candidate rule, the conditions the GPU tests
(test_gpu_kmeans.py, test_gpu_kmeans_geometry.py) rely on for the very same tensors: that the filter can answer, that a count
passes a threshold, that a centred row is exactly zero."""

import torch

ASSIGN_SHAPES = [(1, 1, 4), (1, 300, 16), (300, 1, 16), (37, 129, 64), (129, 37, 68), (257, 1000, 128), (1000, 4097, 256), (300, 200, 4096)]
COLLAPSED_SHAPES = [(1, 16), (129, 16), (129, 68), (1000, 68), (1000, 1024)]
COLLAPSED_TOL = 0.5
GRID = (4000, 4000, 16)   # 32 x 32 = 1 024 tiles of 128 x 128: more than two per compute unit of any part up to 511 of them
MIXED_SPANS = (1, 3)      # row norms 10^U(-span, span)
SCALES = (2.0 ** -40, 2.0 ** 50)
SCALED_SHAPE = (257, 1000, 128)


def assign_capacity(n, k):
    return min(n * k, max(4096, 8 * n))


def collapsed_capacity(k):
    return max(1, min(k * (k - 1) // 2, max(4096, 8 * k)))


def gaussian(n, k, D):
    """Unit Gaussian rows against unit Gaussian centres with mean 0.25."""
    g = torch.Generator().manual_seed(1000 * n + k + D)
    return torch.randn(n, D, generator=g), torch.randn(k, D, generator=g) + 0.25


def far_from_the_origin(n=2000, k=300, D=128):
    """Activations with a large mean: rows = 100 + 0.01 randn, the centres k of them moved by 0.001 randn."""
    g = torch.Generator().manual_seed(11)
    X = 100 + 0.01 * torch.randn(n, D, generator=g)
    C = (X[torch.randperm(n, generator=g)[:k]] + 0.001 * torch.randn(k, D, generator=g)).contiguous()
    return X, C


def identical_centres():
    g = torch.Generator().manual_seed(9)
    C = torch.randn(1, 32, generator=g).repeat(65, 1)
    return torch.randn(65, 32, generator=g), C


def planted(k, D, tol_, seed):
    """Random centres far apart, with planted pairs at tol (1 -+ 1e-3) and at distance 0, equal and unequal counts on each side."""
    g = torch.Generator().manual_seed(seed)
    C = 5 * torch.randn(k, D, generator=g)
    counts = torch.randint(1, 50, (k,), generator=g).float()
    if k >= 20:
        u = torch.randn(8, D, generator=g)
        u /= u.norm(dim=1, keepdim=True)
        for p, (i, j, scale, ci, cj) in enumerate([(0, 1, 1 - 1e-3, 5, 5), (2, k - 1, 1 + 1e-3, 5, 5), (3, 7, 1 - 1e-3, 9, 2), (4, 9, 1 - 1e-3, 2, 9),
                                                  (5, 11, 0.0, 3, 3), (6, 13, 0.0, 4, 1), (8, 15, 1 + 1e-3, 1, 4), (k - 2, 17, 1 - 1e-3, 0, 0)]):
            C[j] = C[i] + u[p] * (tol_ * scale)
            counts[i], counts[j] = ci, cj
    return C, counts


def collapsed_case(k, D):
    return planted(k, D, COLLAPSED_TOL, 23 + k + D)


def three_centres(n=2 ** 20):
    """The API's largest n at the smallest D: three centres, and 2 000 rows with x_0 = 0, exact fp32 ties between centres 0 and 1
    (r = (0 - 1)^2 + y = (0 + 1)^2 + y, term by term)."""
    g = torch.Generator().manual_seed(41)
    C = torch.tensor([[1.0, 0, 0, 0], [-1.0, 0, 0, 0], [0, 2.0, 0, 0]])
    X = torch.randn(n, 4, generator=g)
    X[:2000, 0] = 0
    return X, C


def many_centres(k=2 ** 20):
    """The API's largest k: three rows against k Gaussian centres at D = 4."""
    g = torch.Generator().manual_seed(43)
    return torch.randn(3, 4, generator=g), torch.randn(k, 4, generator=g)


def tied_tiles():
    """Every centre has an exact copy 500 rows away: in another 128-wide tile and another lane group."""
    g = torch.Generator().manual_seed(47)
    C = torch.randn(1000, 64, generator=g)
    C[500:] = C[:500]
    return torch.randn(300, 64, generator=g), C


NO_IMAGE_ROW = 137  # (in the second 128-row tile)


def _integer_centres(g):
    return torch.randint(-8, 9, (64, 16), generator=g).float()


def no_image_row_of_x():
    """64 centres with integer entries in [-8, 8] (their column sums are exact in any order, and so is the division by 64) and
    one row of X that equals their mean: its centred copy is exactly zero."""
    g = torch.Generator().manual_seed(53)
    C = _integer_centres(g)
    X = 4 * torch.randn(200, 16, generator=g)
    X[NO_IMAGE_ROW] = (C.double().sum(dim=0) / 64).float()
    return X, C


def no_image_centre():
    """65 centres, the last the mean m of the 64 integer ones: the sum of all 65 is 65 m, exact in fp32 in any order (multiples
    of 1/64 below 2^11), and 65 m / 65 = m exactly, so centre 64 centres to zero.  Also the collapsed case, with unit counts."""
    g = torch.Generator().manual_seed(59)
    C = torch.cat([_integer_centres(g), torch.zeros(1, 16)])
    C[64] = (C[:64].double().sum(dim=0) / 64).float()
    return 4 * torch.randn(200, 16, generator=g), C


def mixed_norms(span):
    """Every row multiplied by 10^U(-span, span)."""
    g = torch.Generator().manual_seed(61 + span)
    X = torch.randn(1000, 64, generator=g) * 10.0 ** (2 * span * torch.rand(1000, 1, generator=g) - span)
    C = torch.randn(3000, 64, generator=g) * 10.0 ** (2 * span * torch.rand(3000, 1, generator=g) - span)
    return X, C


GROUP_EDGES_K = 5


def group_edges():
    """(index, k): centre 0 has exactly 4 096 rows (the longest segment sorted in LDS), centre 1 has 4 097 (the shortest one
    compacted from index), centre 2 two, centre 3 one, centre 4 none; 300 entries lie outside [0, k): -1, k and 2^31 - 1.  All
    interleaved by one permutation; n = 8 496 is no multiple of the 4 096-entry compaction step."""
    g = torch.Generator().manual_seed(67)
    idx = torch.cat([torch.full((4096,), 0), torch.full((4097,), 1), torch.full((2,), 2), torch.full((1,), 3),
                     torch.full((100,), -1), torch.full((100,), GROUP_EDGES_K), torch.full((100,), 2 ** 31 - 1)])
    return idx[torch.randperm(idx.numel(), generator=g)].to(torch.int32), GROUP_EDGES_K
