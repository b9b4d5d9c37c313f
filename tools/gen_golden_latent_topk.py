"""Generate the per-latent top-k golden vectors (G21) by RUNNING the upstream reference on the CPU (build container only).

Test infrastructure beside ``oracle/`` (it imports ``oracle/_refshim.py`` for the reference import shim and changes nothing
there).  The reference is read from its own location at generation time only; the output is data under ``tests/golden/``:

  g21_csr_topk    small scipy CSR matrices (indptr, indices, data, shape) and what the reference's
                  ``saev.helpers.csr_topk(arr, k=k, axis=0)`` returns for k in {1, 5, 20}: ``values`` and ``indices`` (k, n_cols).
                  Cases ``a`` (300 x 40) and ``b`` (257 x 1004) hold pairwise distinct nonzero values, some negative, an empty
                  column and a column with one entry.  Case ``ties`` (120 x 16) draws its values from four numbers; the reference's
                  indices follow no fixed rule there, so only its ``values`` are recorded.

Before it writes, the generator asserts that every recorded output equals the numpy restatement the tests use
(tests/latent_topk_restatement.py: nonzero entries, value descending then row ascending, zero padding), and that the reference
gives the same with ``batch_size`` 64 and 1024.

    python tools/gen_golden_latent_topk.py
"""

import importlib
import pathlib
import sys

import numpy as np
import scipy.sparse

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "oracle"))
sys.path.insert(0, str(ROOT / "tests"))
import _refshim  # noqa: E402
from latent_topk_restatement import restate_csr  # noqa: E402

OUT = ROOT / "tests" / "golden"
KS = (1, 5, 20)


def distinct_case(n_rows, n_cols, density, seed):
    rng = np.random.default_rng(seed)
    on = rng.random((n_rows, n_cols)) < density
    on[:, 3] = False                       # an empty column
    on[:, 5] = False
    on[n_rows // 2, 5] = True              # a column with one entry
    nnz = int(on.sum())
    mag = (rng.permutation(nnz) + 1).astype(np.float32) / 256  # pairwise distinct, exact in float32
    sign = np.where(rng.random(nnz) < 0.25, -1.0, 1.0).astype(np.float32)
    dense = np.zeros((n_rows, n_cols), dtype=np.float32)
    dense[on] = mag * sign
    assert np.unique(np.abs(dense[on])).size == nnz
    return scipy.sparse.csr_array(dense)


def ties_case(n_rows, n_cols, seed):
    rng = np.random.default_rng(seed)
    dense = rng.choice(np.array([1.0, 2.0, 3.0, -1.0], dtype=np.float32), size=(n_rows, n_cols))
    dense[rng.random((n_rows, n_cols)) < 0.5] = 0
    dense[:, 2] = 0
    return scipy.sparse.csr_array(dense.astype(np.float32))


def main():
    _refshim.install()
    helpers = importlib.import_module("saev.helpers")
    out = {}
    cases = {"a": distinct_case(300, 40, 0.2, 21), "b": distinct_case(257, 1004, 0.05, 22), "ties": ties_case(120, 16, 23)}
    for name, arr in cases.items():
        assert arr.data.dtype == np.float32 and arr.has_canonical_format
        out[f"{name}_shape"] = np.array(arr.shape, dtype=np.int64)
        out[f"{name}_indptr"], out[f"{name}_indices"], out[f"{name}_data"] = arr.indptr, arr.indices, arr.data
        for k in KS:
            got = helpers.csr_topk(arr, k=k, axis=0, batch_size=64)
            again = helpers.csr_topk(arr, k=k, axis=0, batch_size=1024)
            want_v, want_i, _ = restate_csr(arr.indptr, arr.indices, arr.data, arr.shape[1], k)
            assert got.values.dtype == np.float32 and got.indices.dtype == np.int64 and got.values.shape == (k, arr.shape[1])
            assert np.array_equal(got.values, again.values) and np.array_equal(got.values, want_v), (name, k)
            out[f"{name}_k{k}_values"] = got.values
            if name != "ties":
                assert np.array_equal(got.indices, again.indices) and np.array_equal(got.indices, want_i), (name, k)
                out[f"{name}_k{k}_indices"] = got.indices
        per = np.bincount(arr.indices, minlength=arr.shape[1])
        print(f"case {name}: {arr.shape}, {arr.nnz} entries, {int((arr.data < 0).sum())} negative, per column {per.min()}..{per.max()}")
    OUT.mkdir(parents=True, exist_ok=True)
    np.savez_compressed(OUT / "g21_csr_topk.npz", ks=np.array(KS, dtype=np.int64), **out)
    print(f"wrote g21_csr_topk.npz ({(OUT / 'g21_csr_topk.npz').stat().st_size / 1e3:.1f} kB)")


if __name__ == "__main__":
    main()
