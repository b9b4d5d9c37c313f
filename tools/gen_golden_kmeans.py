"""Generate the k-means golden vectors (G24) by RUNNING the upstream reference on the CPU (build container only).

Test infrastructure beside ``oracle/`` (it uses ``oracle/_refshim.py`` to import the reference's
``contrib/trait_discovery/src/tdiscovery/baselines.py`` unchanged and changes nothing there; the two stand-ins that shim lacks,
``submitit`` and the ``saev.data.Ordered*`` names, are added here).  The reference is read from its own location at generation time
only; the outputs are data under ``tests/golden/``:

  g24_kmeans_clustered   k = 96, D = 68, six batches of 512 rows around 96 well-separated points, collapse_tol 0.5: no empty
                         cluster, no collapsed centre
  g24_kmeans_events      the same k and D, batches of 64, 300, 512, 512, 512 rows: the first is smaller than k, so the centres
                         start duplicated, the duplicates are "empty" and are replaced by drawn rows, collapse and are re-seeded
                         from the farthest points
  g24_kmeans_baseline.pt the file the reference's own ``dump`` wrote for the final state of the first fixture

Each .npz holds the batches (values on a 2^-10 grid, so that the file compresses), every random draw in order (recorded by
wrapping torch.randperm / torch.randint while the reference runs), and after every step the reference's centres, counts and
last_batch_inertia_, with the fp64 inertia, the fp64 assignments and the loser mask of tests/kmeans_restatement.py.

A seed is rejected when an fp64 gap decides an argmin, a pair-versus-tolerance test or a farthest-point cut by less than 16 x the
fp32 tolerance (D + 3) 2^-24 (relative, on squared distances; exact ties between bit-identical centres are the tie rule's and
stay), or when the restatement does not reproduce the reference's centres and counts bit for bit.  ``inertia_band`` is 4 x the
largest |reference inertia - fp64 inertia| (the reference's cdist is the matmul form).

    python tools/gen_golden_kmeans.py
"""

import pathlib
import sys
import tempfile
import types

import numpy as np
import torch

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "oracle"))
sys.path.insert(0, str(ROOT / "tests"))
import _refshim  # noqa: E402
import kmeans_restatement as R  # noqa: E402

GOLDEN = ROOT / "tests" / "golden"
K, D, TOL = 96, 68, 0.5


def reference_module():
    import importlib

    ref = _refshim.install()
    if "submitit" not in sys.modules:
        sub = _refshim._mod("submitit")
        sub.core = _refshim._mod("submitit.core")
        sub.core.utils = _refshim._mod("submitit.core.utils", UncompletedJobError=type("UncompletedJobError", (Exception,), {}))
    ordered = importlib.import_module("saev.data.ordered")
    ref.data.OrderedConfig, ref.data.OrderedDataLoader = ordered.Config, ordered.DataLoader
    sys.path.insert(0, str(_refshim.REFERENCE_ROOT / "contrib" / "trait_discovery" / "src"))
    import tdiscovery.baselines as baselines

    return baselines


class Recorder:
    """Wraps torch.randperm / torch.randint and keeps what they returned, in order."""

    def __enter__(self):
        self.draws, self.kinds = [], []
        self._orig = {n: getattr(torch, n) for n in ("randperm", "randint")}
        for n, f in self._orig.items():
            setattr(torch, n, self._wrap(n, f))
        return self

    def _wrap(self, name, fn):
        def inner(*a, **k):
            out = fn(*a, **k)
            self.draws.append(out.numpy().astype(np.int64).copy())
            self.kinds.append(name)
            return out

        return inner

    def __exit__(self, *exc):
        for n, f in self._orig.items():
            setattr(torch, n, f)


def design(seed, sizes):
    rng = np.random.default_rng(seed)
    points = 3.0 * rng.standard_normal((K, D))
    out = []
    for n in sizes:
        x = points[rng.integers(0, K, size=n)] + 0.5 * rng.standard_normal((n, D))
        out.append((np.round(x * 1024.0) / 1024.0).astype(np.float32))
    return out


def min_gaps(log, X, need):
    """The smallest relative fp64 gaps of this step's decisions: (argmin, pair test, farthest cut)."""
    C = log.centers_before
    d2 = R.dist2_64(X, C)
    same = (C[log.assign][:, None, :] == C[None, :, :]).all(axis=2)  # centres bit-identical to the winner: the tie rule's
    best = d2[np.arange(X.shape[0]), log.assign]
    rest = np.where(same, np.inf, d2)
    runner = rest.min(axis=1)
    ok = np.isfinite(runner)
    g_arg = float(((runner[ok] - best[ok]) / runner[ok]).min()) if ok.any() else np.inf
    U = log.centers_updated
    p2 = R.dist2_64(U, U)[np.triu_indices(K, 1)]
    g_pair = float((np.abs(p2 - TOL * TOL) / np.maximum(p2, TOL * TOL)).min())
    g_far = np.inf
    if need > 0:
        f = np.sort(R.dist2_64(X, U).max(axis=1))[::-1][:need + 1]
        rel = (f[:-1] - f[1:]) / f[:-1]
        rel = rel[rel > 0]  # an exact tie (two rows that are each other's farthest centre) is the tie rule's: the lower row first
        g_far = float(rel.min()) if rel.size else np.inf
    return g_arg, g_pair, g_far


def run(ref, tag, sizes, seeds, dump_to=None):
    floor = 16.0 * R.tol(D)
    for seed in seeds:
        batches = design(seed, sizes)
        torch.manual_seed(seed)
        model = ref.MiniBatchKMeans(k=K, device="cpu", collapse_tol=TOL)
        st = R.State(k=K, collapse_tol=TOL)
        out = dict(k=K, D=D, collapse_tol=TOL, seed=seed, n_steps=len(sizes))
        gaps, ref_in, in64, same = [], [], [], True
        with Recorder() as rec:
            for t, X in enumerate(batches):
                n_before = len(rec.draws)
                model.partial_fit(torch.from_numpy(X))
                try:
                    log = R.step(st, X, list(rec.draws[n_before:]))  # the draws the reference made in this step
                except (ValueError, IndexError):  # another number of empties than the reference found: an fp32 decision of its
                    same = False
                    break
                gaps.append(min_gaps(log, X, int(log.losers.sum())))
                same &= np.array_equal(st.centers, model.cluster_centers_.numpy()) and np.array_equal(st.counts, model.cluster_counts_.numpy())
                ref_in.append(model.last_batch_inertia_)
                in64.append(log.inertia64)
                out.update({f"batch{t}": X, f"centers{t}": model.cluster_centers_.numpy().copy(), f"counts{t}": model.cluster_counts_.numpy().copy(),
                            f"assign{t}": log.assign.astype(np.int32), f"losers{t}": log.losers, f"n_empty{t}": log.n_empty})
        if not same:
            print(f"{tag} seed {seed}: the restatement leaves the reference's trajectory")
            continue
        g = np.asarray(gaps)
        band = 4.0 * float(np.abs(np.asarray(ref_in) - np.asarray(in64)).max())
        print(f"{tag} seed {seed}: draws {rec.kinds}, empties {[int(out[f'n_empty{t}']) for t in range(len(sizes))]}, losers "
              f"{[int(out[f'losers{t}'].sum()) for t in range(len(sizes))]}, min gaps (argmin, pair, far) {g.min(axis=0)} vs floor {floor:.3g}, "
              f"bit-equal {same}, inertia_band {band:.3g}")
        if same and g.min() >= floor:
            break
    else:
        raise RuntimeError(f"{tag}: no seed passes the generator's checks")
    out.update(ref_inertia=np.asarray(ref_in), inertia64=np.asarray(in64), inertia_band=band, min_gap=float(g.min()),
               draw_kinds=np.asarray(rec.kinds), n_draws=len(rec.draws))
    out.update({f"draw{i}": d for i, d in enumerate(rec.draws)})
    np.savez_compressed(GOLDEN / f"g24_kmeans_{tag}.npz", **out)
    if dump_to is not None:
        with tempfile.TemporaryDirectory() as tmp:
            fake_run = types.SimpleNamespace(ckpt=pathlib.Path(tmp) / "checkpoint" / "sae.pt")
            path = ref.dump(fake_run, ref.TrainConfig(k=K, collapse_tol=TOL, device="cpu"), model)
            dump_to.write_bytes(path.read_bytes())


def main():
    torch.set_num_threads(1)  # index_add_ on the CPU: one thread, one order
    ref = reference_module()
    run(ref, "clustered", [512] * 6, range(2400, 2440), dump_to=GOLDEN / "g24_kmeans_baseline.pt")
    run(ref, "events", [64, 300, 512, 512, 512], range(2400, 2440))


if __name__ == "__main__":
    main()
