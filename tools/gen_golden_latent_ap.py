"""Generate the latent AP golden vectors (G26) by RUNNING the upstream reference on the CPU (build container only).

Test infrastructure beside ``oracle/`` (it uses ``oracle/_refshim.py`` to import the reference's
``contrib/trait_discovery/src/tdiscovery/classification.py`` unchanged and changes nothing there).  The reference is read from its own
location at generation time only; the output is data under ``tests/golden/``:

  g26_latent_ap    600 rows x 24 latents x 9 columns.  Column 8's class never occurs and about 10 % of the rows have no class (-1).
                   No latent is without events; latent 0 has a single event, 1 fires on every row with distinct values (no ties),
                   2 fires on every row with one value (a single group of 600), 3 is a 0/1 latent, 4 and 5 are quantised to 1/2 and
                   1/4 (many groups of 2-40), 6-11 are signed, 12 stores a +0.0 and a -0.0 explicitly; the rest are sparse gammas.

It holds the CSR and the class ids; ``ref_ap`` (24 x 9 float32), the reference's ``compute_ap_for_latent`` on the dense columns;
``ref_batched_row``, its ``compute_ap_batched`` for the no-ties latent; ``exact_ap`` (float64), the contract evaluated with
``decimal`` at 80 digits (tests/latent_ap_restatement.py) and rounded once; ``n_events`` (24 x 9), the events per pair the tolerance
is made of; and ``eval_config_defaults``, the reference's ``EvalConfig()`` as a JSON string of plain values.

The generator refuses to write unless the fp64 restatement is within 1 float32 ulp of ``ref_ap`` and within the bound of
``exact_ap``.  ``compute_ap_batched`` works in float32 (a cumsum, a division and a sum over 600 ranks), and its own rounding puts it
2-6 float32 ulps from the exact value on most draws of the no-ties latent (24 of the first 25 seeds; the tie-aware value is at 0 on
all of them).  The fixture keeps the first seed where the reference's float32 error stays within 1 ulp in every column (2624), so
that the comparison the tests make shows the formulas agreeing and not that error; gen_golden_probe1d.py rejects seeds likewise.

    python tools/gen_golden_latent_ap.py
"""

import dataclasses
import json
import pathlib
import sys

import numpy as np
import scipy.sparse

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "oracle"))
sys.path.insert(0, str(ROOT / "tests"))
import _refshim  # noqa: E402
import latent_ap_restatement as R  # noqa: E402

GOLDEN = ROOT / "tests" / "golden"
N, S, C = 600, 24, 9
NO_TIES = 1


def reference_module():
    _refshim.install()
    sys.path.insert(0, str(_refshim.REFERENCE_ROOT / "contrib" / "trait_discovery" / "src"))
    import tdiscovery.classification as ref

    return ref


def design(seed):
    rng = np.random.default_rng(seed)
    cls = rng.integers(0, C - 1, size=N).astype(np.int32)  # column C - 1 never occurs
    cls[:C - 1] = np.arange(C - 1)
    cls[rng.random(N) < 0.10] = -1
    dense = np.zeros((N, S), dtype=np.float32)
    stored = np.zeros((N, S), dtype=bool)
    for j in range(S):
        on = rng.random(N) < rng.uniform(0.03, 0.4)
        on[rng.integers(0, N)] = True
        v = rng.gamma(2.0, 0.6, size=N).astype(np.float32) + np.float32(0.01)
        v = v + np.where(cls == j % (C - 1), rng.uniform(0.3, 1.5), 0.0).astype(np.float32)
        if 6 <= j < 12:
            v = v * np.where(rng.random(N) < 0.4, -1.0, 1.0).astype(np.float32)
        dense[:, j], stored[:, j] = np.where(on, v, 0), on
    stored[:, 0] = False
    stored[321, 0], dense[321, 0] = True, 0.75
    stored[:, 1] = True
    dense[:, 1] = rng.permutation(N).astype(np.float32) * np.float32(0.125) + np.float32(0.5)
    stored[:, 2], dense[:, 2] = True, 1.5
    dense[:, 3] = np.where(stored[:, 3], 1.0, 0.0)
    dense[:, 4] = np.where(stored[:, 4], np.ceil(dense[:, 4] * 2) / 2, 0.0)
    dense[:, 5] = np.where(stored[:, 5], np.ceil(dense[:, 5] * 4) / 4, 0.0)
    dense[:, 8] = np.where(stored[:, 8], np.sign(dense[:, 8]) * np.ceil(np.abs(dense[:, 8]) * 2) / 2, 0.0)  # signed and tied
    r = np.flatnonzero(stored[:, 12])[:2]
    dense = np.where(stored, dense, 0).astype(np.float32)
    dense[r[0], 12], dense[r[1], 12] = 0.0, -0.0
    rows, cols = np.nonzero(stored)
    csr = scipy.sparse.csr_matrix((dense[rows, cols], (rows, cols)), shape=(N, S))
    csr.sort_indices()
    assert csr.nnz == int(stored.sum())  # the stored zeros stay stored
    assert np.signbit(csr.data[(csr.data == 0)]).sum() == 1
    return csr, cls


def main():
    ref = reference_module()
    for seed in range(2600, 2640):
        if fixture(ref, seed):
            return
    raise RuntimeError("g26_latent_ap: no seed passes the generator's checks")


def fixture(ref, seed):
    csr, cls = design(seed)
    one_hot = np.zeros((N, C), dtype=np.float32)
    one_hot[np.flatnonzero(cls >= 0), cls[cls >= 0]] = 1.0
    n_pos = one_hot.sum(axis=0)
    dense = csr.toarray().astype(np.float32)
    ref_ap = np.stack([ref.compute_ap_for_latent(dense[:, j].copy(), one_hot, n_pos) for j in range(S)])
    ref_batched = ref.compute_ap_batched(dense[:, [NO_TIES]].copy(), one_hot, n_pos)[0]
    args = (csr.indptr.astype(np.int64), csr.indices.astype(np.int32), csr.data.astype(np.float32), N, S, cls, C)
    exact, pos, n_ev = R.exact_ap(*args)
    own, pos2, _ = R.latent_ap(*args)
    assert (pos == n_pos.astype(np.int64)).all() and (pos == pos2).all()
    ulp = int(R.ulps32(own.astype(np.float32), ref_ap).max())
    miss = float((np.abs(own - exact) / R.bound(n_ev)).max())
    batched = int(R.ulps32(ref_batched, exact[NO_TIES].astype(np.float32)).max())
    print(f"g26_latent_ap seed {seed}: nnz {csr.nnz}, restatement vs ref_ap {ulp} fp32 ulps, |restatement - exact| / bound {miss:.3g}, "
          f"batched vs exact on the no-ties latent {batched} ulps")
    assert ulp <= 1 and miss <= 1.0
    if batched > 1:  # the reference's float32 cumsum has drifted on this draw: a property of its arithmetic, not of the contract
        return False

    defaults = {}
    for f in dataclasses.fields(ref.EvalConfig):
        v = getattr(ref.EvalConfig(), f.name)
        defaults[f.name] = str(v) if isinstance(v, pathlib.PurePath) else [str(x) if isinstance(x, pathlib.PurePath) else x for x in v] \
            if isinstance(v, tuple) else v
    np.savez_compressed(GOLDEN / "g26_latent_ap.npz", indptr=args[0], indices=args[1], data=args[2], labels=cls, n_rows=N, n_latents=S,
                        n_classes=C, no_ties_latent=NO_TIES, ref_ap=ref_ap, ref_batched_row=ref_batched, exact_ap=exact, n_events=n_ev,
                        seed=seed, eval_config_defaults=np.str_(json.dumps(defaults, sort_keys=True)))
    return True


if __name__ == "__main__":
    main()
