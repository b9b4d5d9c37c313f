"""Generate the probe1d golden vectors (G23, G25) by RUNNING the upstream reference on the CPU (build container only).

Test infrastructure beside ``oracle/`` (it uses ``oracle/_refshim.py`` to import the reference's
``contrib/trait_discovery/src/tdiscovery/probe1d.py`` unchanged and changes nothing there).  The reference is read from its own
location at generation time only; the outputs are data under ``tests/golden/``:

  g23_probe1d_plain    600 rows x 48 latents x 11 classes, class_slab_size 8 (a ragged last slab), max_iter 30: two latents without
                       entries, one with a single entry, one firing on every row, one that separates a class perfectly, signed
                       values and an explicitly stored 0.0
  g23_probe1d_absent   600 x 40 x 12 with classes 4-7 never occurring, class_slab_size 4: that slab stops at iteration 1 while the
                       others run to 30
  g25_probe1d_groups   600 x 12 x 70, class_slab_size 32 (slabs of 32, 32 and 6 classes: the last one inside the second 64-class group
                       of the events kernel), classes 62-69 never occurring: the eight fill the last slab, which stops at iteration 1,
                       and the end of the second
  g25_probe1d_wide     600 x 8 x 151, class_slab_size 8 (19 slabs over three class groups), classes 64-71 never occurring: that slab
                       stops at iteration 1.  (The latents of both G25 designs are few so that each file stays below the G23 ones.)

Each holds the CSR, the class ids, the hyper-parameters; the reference's results with dtype=float64 (r64_*) and with its default
float32 (r32_*): coef, intercept, n_iter, qx and the five matrices of loss_matrix_with_aux; and the bands the tests use:

  loss_band    max over pairs of |L_R32 - L_R64|
  well_posed   pairs whose latent has at least 5 positive and 5 negative events for the class (a property of the data)
  coef_band    4 x the largest distance |a - b| / (1 + |b|) of R32's coefficients and intercepts to R64's over the well-posed pairs
  min_gap      the smallest |mu - 0.5| over all events, zero rows and pairs at R64's coefficients (a seed below 1e-9 is rejected)

A seed is also rejected when R32 leaves more than 0.5 % of all pairs outside coef_band, or when the numpy restatement of the
contract (tests/probe1d_restatement.py) does not reproduce R64's n_iter.

    python tools/gen_golden_probe1d.py [g23_probe1d_plain ...]     (no name: all four)
"""

import pathlib
import sys

import numpy as np
import scipy.sparse
import torch

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "oracle"))
sys.path.insert(0, str(ROOT / "tests"))
import _refshim  # noqa: E402
import probe1d_restatement as R  # noqa: E402

GOLDEN = ROOT / "tests" / "golden"
N = 600
HYPER = dict(ridge=1e-8, tol=1e-6, max_iter=30, lam_init=1e-3, lam_shrink=0.1, lam_grow=10.0, delta_logit=6.0)


def reference_module():
    _refshim.install()
    sys.path.insert(0, str(_refshim.REFERENCE_ROOT / "contrib" / "trait_discovery" / "src"))
    import tdiscovery.probe1d as ref

    return ref


def design(seed, n_latents, n_classes, present, special):
    rng = np.random.default_rng(seed)
    ids = rng.choice(np.asarray(present), size=N).astype(np.uint8)
    ids[:len(present)] = present  # every present class occurs
    dense = np.zeros((N, n_latents), dtype=np.float32)
    stored = np.zeros((N, n_latents), dtype=bool)
    for j in range(n_latents):
        on = rng.random(N) < rng.uniform(0.04, 0.35)
        v = rng.gamma(2.0, 0.6, size=N).astype(np.float32)
        liked = rng.choice(np.asarray(present), size=2, replace=False)
        v = v + np.where(np.isin(ids, liked), rng.uniform(0.3, 1.5), 0.0).astype(np.float32)
        if j % 3 == 0:
            v = v * np.where(rng.random(N) < 0.3, -1.0, 1.0).astype(np.float32)  # signed codes
        dense[:, j], stored[:, j] = np.where(on, v, 0), on
    if special:
        for j in (5, 17):  # no entries
            stored[:, j] = False
        stored[:, 9] = False
        stored[123, 9], dense[123, 9] = True, 1.25  # one entry
        stored[:, 3] = True  # fires on every row
        dense[:, 3] = rng.gamma(2.0, 0.5, size=N).astype(np.float32) + 0.05
        stored[:, 7] = ids == 2  # separates class 2
        dense[:, 7] = np.where(ids == 2, rng.uniform(0.5, 2.0, size=N), 0).astype(np.float32)
        r0 = int(np.flatnonzero(stored[:, 11])[0])
        dense[r0, 11] = 0.0  # an explicitly stored zero
    dense = np.where(stored, dense, 0).astype(np.float32)
    rows, cols = np.nonzero(stored)
    csr = scipy.sparse.csr_matrix((dense[rows, cols], (rows, cols)), shape=(N, n_latents))
    csr.sort_indices()
    assert csr.nnz == int(stored.sum())  # the stored zero stays stored
    return csr, ids


def run_reference(ref, csr, ids, n_classes, slab, dtype):
    x = torch.sparse_csr_tensor(torch.from_numpy(csr.indptr.astype(np.int64)), torch.from_numpy(csr.indices.astype(np.int64)),
                                torch.from_numpy(csr.data), size=csr.shape)
    y = torch.zeros(N, n_classes, dtype=torch.float32)
    y[torch.arange(N), torch.from_numpy(ids.astype(np.int64))] = 1.0
    probe = ref.Sparse1DProbe(n_latents=csr.shape[1], n_classes=n_classes, device="cpu", dtype=dtype, class_slab_size=slab, **HYPER)
    probe.log.setLevel("ERROR")
    probe.fit(x, y)
    loss, tp, fp, tn, fn = probe.loss_matrix_with_aux(x, y.bool())
    return dict(coef=probe.coef_.numpy(), intercept=probe.intercept_.numpy(), n_iter=probe.n_iter_.numpy(), qx=probe.latent_qx_.numpy(),
                loss=loss.numpy(), tp=tp.numpy(), fp=fp.numpy(), tn=tn.numpy(), fn=fn.numpy())


def distance(a, b):
    return np.abs(a.astype(np.float64) - b) / (1 + np.abs(b))


def fixture(ref, name, n_latents, n_classes, present, slab, special, seeds):
    for seed in seeds:
        csr, ids = design(seed, n_latents, n_classes, present, special)
        r64 = run_reference(ref, csr, ids, n_classes, slab, torch.float64)
        r32 = run_reference(ref, csr, ids, n_classes, slab, torch.float32)
        ymat = R.labels_matrix(ids, n_classes)
        starts, rows, vals, _ = R.prepare(csr.indptr, csr.indices, csr.data, n_latents)
        z, _ = R._event_logits(starts, vals, r64["intercept"], r64["coef"])
        gap = min(float(np.abs(R._sigma(z) - 0.5).min()), float(np.abs(R._sigma(r64["intercept"]) - 0.5).min()))
        pos_ev = R._segment_sums(ymat[rows].astype(np.float64), starts)[0]
        well = (pos_ev >= 5) & (np.diff(starts)[:, None] - pos_ev >= 5)
        d32 = np.maximum(distance(r32["coef"], r64["coef"]), distance(r32["intercept"], r64["intercept"]))
        if not well.any():
            print(f"{name} seed {seed}: no well-posed pair")  # (nothing to take coef_band from: the next seed)
            continue
        coef_band = 4.0 * float(d32[well].max())
        outside = float((d32 > coef_band).mean())
        loss_band = float(np.abs(r32["loss"].astype(np.float64) - r64["loss"].astype(np.float64)).max())
        hp = R.Hyper(class_slab_size=slab, **HYPER)
        own = R.fit(csr.indptr, csr.indices, csr.data, n_latents, ids, n_classes, hp)
        print(f"{name} seed {seed}: nnz {csr.nnz}, n_iter {r64['n_iter'].tolist()}, min gap {gap:.3g}, well-posed {int(well.sum())}/{well.size}, "
              f"coef_band {coef_band:.3g}, R32 outside {outside:.4f}, loss_band {loss_band:.3g}, restatement n_iter {own[2].tolist()}")
        if gap >= 1e-9 and outside <= 0.005 and (own[2] == r64["n_iter"]).all():
            break
    else:
        raise RuntimeError(f"{name}: no seed passes the generator's checks")
    out = dict(indptr=csr.indptr.astype(np.int64), indices=csr.indices.astype(np.int32), data=csr.data.astype(np.float32), labels=ids,
               n_rows=N, n_latents=n_latents, n_classes=n_classes, class_slab_size=slab, seed=seed, loss_band=loss_band, coef_band=coef_band,
               well_posed=well, min_gap=gap, **HYPER)
    out.update({f"r64_{k}": v for k, v in r64.items()})
    out.update({f"r32_{k}": v for k, v in r32.items()})
    np.savez_compressed(GOLDEN / f"{name}.npz", **out)


# name -> n_latents, n_classes, the classes that occur, class_slab_size, the special latents of G23, the seeds to try
FIXTURES = {
    "g23_probe1d_plain": (48, 11, list(range(11)), 8, True, range(2300, 2340)),
    "g23_probe1d_absent": (40, 12, [0, 1, 2, 3, 8, 9, 10, 11], 4, False, range(2400, 2440)),
    "g25_probe1d_groups": (12, 70, list(range(62)), 32, False, range(2500, 2540)),
    "g25_probe1d_wide": (8, 151, [k for k in range(151) if not 64 <= k < 72], 8, False, range(2600, 2640)),
}


def main(names):
    torch.set_num_threads(1)  # index_add_ on the CPU: one thread, one order
    ref = reference_module()
    for name in names or FIXTURES:
        fixture(ref, name, *FIXTURES[name])


if __name__ == "__main__":
    main(sys.argv[1:])
