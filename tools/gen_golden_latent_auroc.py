"""Generate the latent AUROC golden vectors (G29) by RUNNING the upstream reference on the CPU (build container only).

Test infrastructure beside ``oracle/`` (it uses ``oracle/_refshim.py`` to import the reference's ``contrib/mimics/src/mimics``
unchanged and changes nothing there).  The reference imports ``polars``, which this image lacks: a minimal stand-in module is
installed here (``DataFrame`` recording its columns, ``concat``, a no-op ``write_parquet``).  The reference is read from its own
location at generation time only; the output is data under ``tests/golden/``:

  g29_latent_auroc   designs ``d{i}_*``: a token CSR (indptr, indices, data) of n_images x tpi rows with values in quarters (ties
                     abound), negative stored values (a latent stored in every patch of some images with negative values only pins
                     the clamp of the pooling at 0), explicit +0.0 / -0.0 entries, an image with nothing stored, a latent stored in
                     every patch and one never stored; ``labels`` (one ``subspecies_view`` string per image: several pairs in both
                     views, labels in no task, one pair below ``min_samples``), ``pair_specs``, ``views`` and ``shape`` =
                     (n_images, tpi, S, min_samples, feature_chunk).  Recorded from the reference: ``task_names``, ``n_pos``,
                     ``n_neg`` (``build_task_specs``), ``pooled`` (``max_pool_csr``) and the eight columns ``col_*`` of ``score_run``.

The generator refuses to write unless the numpy restatement (tests/latent_auroc_restatement.py) reproduces the reference's ``auroc``
and supports on the float32 bits and its means within the derived bound, and the pair below ``min_samples`` is dropped.

    python tools/gen_golden_latent_auroc.py
"""

import pathlib
import sys
import tempfile
import types

import numpy as np
import scipy.sparse

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "oracle"))
sys.path.insert(0, str(ROOT / "tests"))
import _refshim  # noqa: E402
import latent_auroc_restatement as R  # noqa: E402

GOLDEN = ROOT / "tests" / "golden"
COLUMNS = ("run_id", "task", "feature_id", "auroc", "support_erato", "support_melpomene", "mean_act_erato", "mean_act_melpomene")
PAIRS = [("lativitta", "malleti"), ("cyrbia", "cythera"), ("notabilis", "plesseni")]  # the last one stays below min_samples
VIEWS = ["dorsal", "ventral"]
DESIGNS = [(80, 3, 24, 4, 7, 2900), (160, 4, 48, 10, 1024, 2901), (200, 3, 32, 10, 16, 2902)]  # n_images, tpi, S, min_samples, feature_chunk, seed


def install_polars_stand_in():
    class DataFrame:
        def __init__(self, data=None, **kw):
            self.columns = {k: np.asarray(v) for k, v in (data or {}).items()}

        @property
        def height(self):
            return len(next(iter(self.columns.values()))) if self.columns else 0

        def write_parquet(self, path):
            pass

    def concat(frames):
        return DataFrame({k: np.concatenate([f.columns[k] for f in frames]) for k in frames[0].columns})

    mod = types.ModuleType("polars")
    mod.DataFrame, mod.concat = DataFrame, concat
    sys.modules["polars"] = mod


def reference_module():
    _refshim.install()
    install_polars_stand_in()
    sys.path.insert(0, str(_refshim.REFERENCE_ROOT / "contrib" / "trait_discovery" / "src"))
    sys.path.insert(0, str(_refshim.REFERENCE_ROOT / "contrib" / "mimics" / "src"))
    import mimics.scoring as ref

    return ref


def labels_of(rng, n_images, min_samples):
    """One label per image: the first two pairs in both views with at least min_samples + 1 images a side, the third pair with fewer
    than min_samples melpomene images, and labels no task uses."""
    labels = []
    for e, m in PAIRS[:2]:
        for v in VIEWS:
            labels += [f"{e}_{v}"] * (min_samples + 1 + int(rng.integers(4))) + [f"{m}_{v}"] * (min_samples + 1 + int(rng.integers(4)))
    labels += ["notabilis_dorsal"] * min_samples + ["plesseni_dorsal"] * (min_samples - 2)
    assert len(labels) <= n_images - 4
    other = ["hydara_lateral", "unlabelled", "lativitta_lateral"]
    labels += [other[i % 3] for i in range(n_images - len(labels))]
    return [labels[i] for i in rng.permutation(n_images)]


def tokens_of(rng, n_images, tpi, s):
    """The token CSR: four to eight entries a patch, values in quarters from -1 to 3 (explicit zeros of both signs among them)."""
    indptr, indices, data = [0], [], []
    for i in range(n_images):
        for p in range(tpi):
            row = {}
            if i != 1:  # image 1: nothing stored
                for c in rng.choice(np.arange(2, s - 1), size=int(rng.integers(4, 9)), replace=False).tolist():
                    q = int(rng.integers(-4, 13))
                    row[c] = q / 4 if q else float(rng.choice([0.0, -0.0]))
                row[0] = -0.25 * (1 + int(rng.integers(4))) if i % 5 == 0 else 0.25 * int(rng.integers(1, 9))  # every patch; negative only in a fifth of the images
                if i % 3 == 0 or p > 0:
                    row[1] = -0.5 if i % 2 else 0.5 * (1 + p)  # negative only, but not in every patch of most images
            for c in sorted(row):
                indices.append(c)
                data.append(row[c])
            indptr.append(len(indices))
    return np.asarray(indptr, np.int64), np.asarray(indices, np.int32), np.asarray(data, np.float32)


def design(ref, i):
    n_images, tpi, s, min_samples, feature_chunk, seed = DESIGNS[i]
    rng = np.random.default_rng(seed)
    sv = labels_of(rng, n_images, min_samples)
    indptr, indices, data = tokens_of(rng, n_images, tpi, s)
    csr = scipy.sparse.csr_matrix((data, indices, indptr), shape=(n_images * tpi, s))
    assert csr.has_canonical_format and csr.nnz == len(data) and (data == 0).any() and np.signbit(data[data == 0]).any() and (data < 0).any()
    specs = ref.build_task_specs(sv, pair_specs=PAIRS, views=VIEWS, min_samples=min_samples)
    names = [spec.name for spec in specs]
    assert len(specs) == 4 and not any("notabilis" in name for name in names), names
    pooled = ref.max_pool_csr(csr, n_images, tpi)
    assert pooled.dtype == np.float32 and (pooled >= 0).all() and (pooled[1] == 0).all() and (pooled[:, s - 1] == 0).all()
    assert (pooled[::5, 0] == 0).all() and (pooled[:, 0] > 0).sum() == n_images - len(pooled[::5]) - 1  # the clamp
    with tempfile.TemporaryDirectory() as tmp:
        root = pathlib.Path(tmp)
        (root / "run0" / "inference" / "shard0").mkdir(parents=True)
        scipy.sparse.save_npz(root / "run0" / "inference" / "shard0" / "token_acts.npz", csr)
        frame = ref.score_run("run0", run_root_dpath=root, shard_id="shard0", task_specs=specs, n_images=n_images, feature_chunk=feature_chunk,
                              force_recompute=True)
    cols = frame.columns
    assert tuple(cols) == COLUMNS and all(cols[k].dtype == np.float32 for k in COLUMNS[3:]) and cols["feature_id"].dtype == np.int32

    # the restatement on the pooled matrix: classes = the labels, one task per spec
    labels = sorted(set(sv))
    cls = np.asarray([labels.index(x) for x in sv], dtype=np.int32)
    roles = np.zeros((len(specs), len(labels)), dtype=np.uint8)
    for t, name in enumerate(names):
        e, m = name.split("_vs_")
        roles[t, labels.index(e)], roles[t, labels.index(m)] = 1, 2
    p = scipy.sparse.csr_matrix(pooled)
    own = R.one_walk(p.indptr, p.indices, p.data, n_images, s, cls, roles)
    assert np.array_equal(own["u2"], R.by_pairs(p.indptr, p.indices, p.data, n_images, s, cls, roles))
    assert own["n_pos"].tolist() == [spec.n_pos for spec in specs] and own["n_neg"].tolist() == [spec.n_neg for spec in specs]
    bits = lambda x: np.ascontiguousarray(x, dtype=np.float32).reshape(-1).view(np.uint32)  # noqa: E731
    assert np.array_equal(bits(own["auroc"].T), cols["auroc"].view(np.uint32)), "auroc: the restatement is not the reference"
    worst = 0.0
    for role, side, n in (("neg", "erato", own["n_neg"]), ("pos", "melpomene", own["n_pos"])):
        nf = n[:, None].astype(np.float64)
        assert np.array_equal(bits(own[f"fire_{role}"].T / nf), cols[f"support_{side}"].view(np.uint32)), f"support_{side}"
        miss = np.abs((own[f"sum_{role}"].T / nf).reshape(-1) - cols[f"mean_act_{side}"].astype(np.float64))
        bound = R.mean_bound(nf, own[f"abs_{role}"].T).reshape(-1)
        assert (miss <= bound).all(), f"mean_act_{side}"
        worst = max(worst, float((miss / np.maximum(bound, 1e-300)).max()))
    ties = int((np.unique(cols["auroc"]).size))
    print(f"  d{i}: {n_images} images x {tpi} patches x {s} latents, nnz {len(data)}, tasks {names}, {ties} distinct auroc values, "
          f"auroc and supports on the float32 bits, means within {worst:.3g} of the bound")
    out = {"indptr": indptr, "indices": indices, "data": data, "labels": np.asarray(sv), "pair_specs": np.asarray(PAIRS), "views": np.asarray(VIEWS),
           "shape": np.asarray([n_images, tpi, s, min_samples, feature_chunk]), "task_names": np.asarray(names),
           "n_pos": np.asarray([spec.n_pos for spec in specs], dtype=np.int64), "n_neg": np.asarray([spec.n_neg for spec in specs], dtype=np.int64),
           "pooled": pooled, **{f"col_{k}": cols[k] for k in COLUMNS}}
    return {f"d{i}_{k}": v for k, v in out.items()}


def main():
    ref = reference_module()
    out = {"n_designs": np.asarray(len(DESIGNS))}
    for i in range(len(DESIGNS)):
        out.update(design(ref, i))
    cfg = ref.Config()
    out["config_defaults"] = np.asarray([str(cfg.min_samples), str(cfg.feature_chunk), str(cfg.force_recompute), cfg.slurm_acct, cfg.slurm_partition,
                                         str(cfg.n_hours), str(cfg.mem_gb), cfg.log_to, str(cfg.pair_specs), str(cfg.views), str(cfg.run_ids)])
    path = GOLDEN / "g29_latent_auroc.npz"
    np.savez_compressed(path, **out)
    print(f"wrote {path.name}: {path.stat().st_size} bytes")
    assert path.stat().st_size < 100_000


if __name__ == "__main__":
    main()
