"""Generate the probe metrics golden vectors (G28) by RUNNING the upstream reference on the CPU (build container only).

Test infrastructure beside ``oracle/`` (it uses ``oracle/_refshim.py`` to import the reference's
``contrib/trait_discovery/src/tdiscovery/metrics.py`` unchanged and changes nothing there).  The reference is read from its own
location at generation time only; the output is data under ``tests/golden/``:

  g28_probe_metrics   a run directory of 8 latents and 4 classes: a test split of 40 examples x 8 tokens = 320 rows and a train split
                      of another shape (30 x 8, so that the two shard directories get different names), ``max_k`` = 96.

The reference ranks tied scores in whatever order an unstable argsort leaves them, so its AP is well defined only where that order
cannot matter.  The design makes it so for every class's selected latent: the latent fires on EVERY row of the class (the rows on
which it is silent all tie at score b and none of them is of the class) and its firing rows have pairwise distinct float32 scores,
all different from b (values are multiples of 1/8, weights and biases multiples of 1/4: every score is exact).
  class 0   latent 0, w > 0: the class rows high, 60 other rows lower
  class 1   latent 1, w < 0: fires on all 320 rows (no zero block), the class rows lowest
  class 2   latent 2, w > 0   } one latent shared by two classes
  class 3   latent 2, w < 0   }
  latent 3  20 events: fewer than max_k, its top rows padded;  latents 4-7: 100-200 events, never selected
No latent has two events of one value: the reference's top rows do not say how equal values are ordered.

It holds the test split's CSR and labels, ``loss`` / ``weights`` / ``biases`` (float32, as probe1d writes them), the shapes of both
splits, the reference's five outputs, ``exact_ap`` (the exact rational AP of every selected pair, rounded once to float64) with
``exact_ap_fraction`` (the rationals as text), and ``ref_ap_distance``.  The generator ASSERTS that the reference's ``ap`` lies within
(2 N + 4) 2^-24 of the exact value for every class: one float32 rounding each for precision, recall and their product on the pos_c
rows where the recall step is non-zero, and the sequential float32 sum of N terms with partial sums of at most 1.  It also asserts
that precision and recall are reproduced on the bits from integer counts.

    python tools/gen_golden_probe_metrics.py
"""

import fractions
import pathlib
import sys
import tempfile

import numpy as np
import scipy.sparse

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "oracle"))
import _refshim  # noqa: E402

GOLDEN = ROOT / "tests" / "golden"
N_EX, TOKENS, S, C, MAX_K = 40, 8, 8, 4, 96
TRAIN_EX = 30
N = N_EX * TOKENS


def reference_module():
    _refshim.install()
    sys.path.insert(0, str(_refshim.REFERENCE_ROOT / "contrib" / "trait_discovery" / "src"))
    import tdiscovery.metrics as ref

    return ref


def design(seed=28):
    rng = np.random.default_rng(seed)
    labels = rng.integers(0, C, size=N).astype(np.uint8)
    dense = np.zeros((N, S), dtype=np.float32)
    grid = lambda k: (0.5 + 0.125 * rng.permutation(k)).astype(np.float32)  # noqa: E731  (k distinct multiples of 1/8)

    def fill(j, high_rows, low_rows):
        v = np.sort(grid(len(high_rows) + len(low_rows)))[::-1]
        dense[rng.permutation(high_rows), j] = v[:len(high_rows)]
        dense[rng.permutation(low_rows), j] = v[len(high_rows):]

    others = lambda c, k: rng.choice(np.flatnonzero(labels != c), size=k, replace=False)  # noqa: E731
    fill(0, np.flatnonzero(labels == 0), others(0, 60))
    fill(1, np.flatnonzero(labels != 1), np.flatnonzero(labels == 1))
    in23 = np.flatnonzero((labels == 2) | (labels == 3))
    dense[in23, 2] = grid(len(in23))
    extra = rng.choice(np.flatnonzero(labels < 2), size=25, replace=False)
    dense[extra, 2] = 40.0 + grid(25)
    dense[rng.choice(N, size=20, replace=False), 3] = grid(20)
    for j in range(4, S):
        rows = rng.choice(N, size=int(rng.integers(100, 200)), replace=False)
        dense[rows, j] = grid(len(rows))
    assert all(len(np.unique(dense[dense[:, j] != 0, j])) == (dense[:, j] != 0).sum() for j in range(S))
    csr = scipy.sparse.csr_matrix(dense)
    csr.sort_indices()
    loss = rng.uniform(1.0, 2.0, size=(S, C)).astype(np.float32)
    weights = (rng.integers(1, 9, size=(S, C)) * 0.25 * rng.choice([1.0, -1.0], size=(S, C))).astype(np.float32)
    biases = (rng.integers(-12, 5, size=(S, C)) * 0.25).astype(np.float32)
    for c, (j, w) in enumerate([(0, 0.75), (1, -1.25), (2, 0.5), (2, -0.25)]):
        loss[j, c], weights[j, c] = 0.125 + 0.0625 * c, w
    return csr, labels, loss, weights, biases


def exact_selected(csr, labels, loss, weights, biases):
    """The exact AP (a Fraction) of every class's selected pair; asserts the design's promise for it."""
    out = []
    dense = csr.toarray().astype(np.float32)
    for c, j in enumerate(np.argmin(loss, axis=0)):
        a = dense[:, j]
        s = a * weights[j, c] + biases[j, c]
        assert s.dtype == np.float32
        is_c = labels == c
        assert is_c.sum() > 0 and (a[is_c] != 0).all(), "the latent is silent on a row of its class"
        fired = s[a != 0]
        assert len(np.unique(fired)) == len(fired) and (fired != biases[j, c]).all(), "tied scores among the firing rows"
        order = np.argsort(-s.astype(np.float64), kind="stable")
        hits, total = 0, fractions.Fraction(0)
        for rank, row in enumerate(order, start=1):
            if is_c[row]:
                hits += 1
                total += fractions.Fraction(hits, rank)
        out.append(total / int(is_c.sum()))
    return out


def main():
    from saev_amd import disk
    from saev_amd.data import write_shards

    ref = reference_module()
    csr, labels, loss, weights, biases = design()
    exact = exact_selected(csr, labels, loss, weights, biases)
    with tempfile.TemporaryDirectory() as tmp:
        tmp = pathlib.Path(tmp)
        rng = np.random.default_rng(1)
        test_shards = write_shards(tmp, rng.standard_normal((N_EX, 1, TOKENS, 4)).astype(np.float32), labels=labels.reshape(N_EX, TOKENS))
        train_shards = write_shards(tmp, rng.standard_normal((TRAIN_EX, 1, TOKENS, 4)).astype(np.float32),
                                    labels=rng.integers(0, C, size=(TRAIN_EX, TOKENS)).astype(np.uint8))
        assert train_shards.name != test_shards.name
        run = disk.Run.new("g28probe", train_shards_dir=train_shards, val_shards_dir=test_shards, runs_root=tmp / "saev" / "runs")
        for shards, acts in ((train_shards, scipy.sparse.random(TRAIN_EX * TOKENS, S, density=0.2, format="csr", dtype=np.float32, random_state=2)),
                             (test_shards, csr)):
            (run.inference / shards.name).mkdir()
            scipy.sparse.save_npz(run.inference / shards.name / "token_acts.npz", acts)
        np.savez(run.inference / train_shards.name / "probe1d_metrics.npz", loss=loss, weights=weights, biases=biases)
        ref.worker_fn(ref.Config(run=run.run_dir, train_shards=train_shards, test_shards=test_shards, max_k=MAX_K))
        with np.load(run.inference / test_shards.name / f"probe1d_metrics__train-{train_shards.name}.npz") as z:
            got = {k: z[k] for k in z.files}
    assert sorted(got) == ["ap", "f1", "precision", "recall", "top_labels"]
    bound = (2 * N + 4) * 2.0 ** -24
    distance = np.array([abs(float(fractions.Fraction(float(a)) - x)) for a, x in zip(got["ap"], exact)])
    print(f"g28_probe_metrics: nnz {csr.nnz}, selected latents {np.argmin(loss, axis=0).tolist()}, ap {got['ap'].tolist()}, "
          f"|ref ap - exact| {distance.max():.3g} against a bound of {bound:.3g}")
    assert (distance <= bound).all()
    # precision and recall from integer counts, by the reference's float32 expressions
    j_c, cols = np.argmin(loss, axis=0), np.arange(C)
    s_nc = csr.toarray().astype(np.float32)[:, j_c] * weights[j_c, cols] + biases[j_c, cols]
    one_hot = labels[:, None] == cols[None, :]
    tp, pred, pos = ((s_nc > 0) & one_hot).sum(axis=0), (s_nc > 0).sum(axis=0), one_hot.sum(axis=0)
    from saev_amd.probe_metrics import scores_from_counts

    for mine, theirs in zip(scores_from_counts(tp, pred, pos), (got["precision"], got["recall"], got["f1"])):
        assert np.array_equal(mine, theirs) and mine.dtype == theirs.dtype
    assert (np.diff(csr.indptr).sum() == csr.nnz) and (np.bincount(csr.indices, minlength=S)[3] == 20 < MAX_K) and MAX_K > 64
    np.savez_compressed(GOLDEN / "g28_probe_metrics.npz", indptr=csr.indptr.astype(np.int64), indices=csr.indices.astype(np.int32),
                        data=csr.data.astype(np.float32), labels=labels, loss=loss, weights=weights, biases=biases, n_examples=N_EX,
                        tokens_per_example=TOKENS, train_examples=TRAIN_EX, n_latents=S, n_classes=C, max_k=MAX_K, ref_ap=got["ap"],
                        ref_precision=got["precision"], ref_recall=got["recall"], ref_f1=got["f1"], ref_top_labels=got["top_labels"],
                        exact_ap=np.array([float(x) for x in exact]), exact_ap_fraction=np.array([f"{x.numerator}/{x.denominator}" for x in exact]),
                        ref_ap_distance=distance, tp=tp, pred_pos=pred, pos=pos)


if __name__ == "__main__":
    main()
