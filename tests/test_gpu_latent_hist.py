"""The per-latent histograms and quantiles on the MI355X (include/saev_amd.h: LATENT HISTOGRAM) against the integer
restatement of the contract (tests/latent_hist_restatement.py, itself checked against np.histogram and np.quantile by the CPU
suite) on the cases of tests/latent_hist_cases.py: every count table, every locate step and every result on the bits."""

import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse
import torch

import latent_hist_cases as K
import latent_hist_restatement as R
from conftest import ROOT

pytestmark = [pytest.mark.gpu, pytest.mark.encoder_modes("f32")]  # context-free kernels: one encoder mode is enough
DEV = "cuda"
SELECT = [n for n in K.CASES if n not in ("flush0", "s_70001")]
_want = {}


def want_of(name, over):
    """The restatement of a case, computed once."""
    if (name, over) not in _want:
        c = K.get(name)
        lat, key, n = R.entries_of(c["indptr"], c["indices"], c["data"], c["S"])
        _want[name, over] = R.select(lat, key, c["S"], c["q"], over, n)
    return _want[name, over]


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a if dtype is None else a.astype(dtype))).to(DEV)


def blocks_of(c, splits=None, order=None):
    """The case's rows as CSR blocks on the device: cut at ``splits``, rows taken in ``order``."""
    indptr, n = c["indptr"], c["indptr"].size - 1
    splits = splits or (0, n)
    out = []
    for a, b in zip(splits[:-1], splits[1:]):
        if order is None:
            take, ptr = slice(indptr[a], indptr[b]), indptr[a:b + 1] - indptr[a]
        else:
            rows = order[a:b]
            take = np.concatenate([np.arange(indptr[r], indptr[r + 1]) for r in rows] + [np.zeros(0, np.int64)])
            ptr = np.concatenate([[0], np.cumsum(np.diff(indptr)[rows])])
        out.append((dev(ptr, np.int64), dev(c["indices"][take], np.int32), dev(c["data"][take], np.float32)))
    return out


def u32(t, width=None):
    t = t.cpu().to(torch.int64).numpy() & 0xFFFFFFFF
    return t if width is None else t[:, :width]


def run_select(c, over, blocks, check=None):
    from saev_amd.engine import LatentQuantiles

    acc = LatentQuantiles(c["S"], c["q"], DEV, over)
    for level in range(3):
        for b in blocks:
            acc.add_csr(*b)
        if check is not None:
            check(acc, level, located=False)
        acc.next_pass()
        if check is not None:
            check(acc, level, located=True)
    assert acc.done and acc.n_passes == 3
    return acc.result()


def same_result(got, want):
    for name in ("lower", "higher"):  # (an empty multiset: the one quiet NaN on both sides)
        np.testing.assert_array_equal(getattr(got, name).numpy().view(np.uint32), want[name].view(np.uint32), err_msg=name)
    np.testing.assert_array_equal(got.linear.numpy(), want["linear"])  # (NaN equals NaN here)
    finite = ~np.isnan(want["linear"])
    np.testing.assert_array_equal(got.linear.numpy()[finite].view(np.uint64), want["linear"][finite].view(np.uint64))
    np.testing.assert_array_equal(got.count.numpy(), want["count"])


@pytest.mark.parametrize("over", ["rows", "entries"])
@pytest.mark.parametrize("name", SELECT)
def test_every_table_and_every_locate_step_equal_the_restatement(name, over):
    c, want = K.get(name), want_of(name, over)
    T = 2 * len(c["q"])

    def check(acc, level, located):
        if not located:
            table = acc.counts0 if level == 0 else acc.counts
            np.testing.assert_array_equal(u32(table), want[f"counts{level}"], err_msg=f"counts{level}")
            return
        np.testing.assert_array_equal(u32(acc.prefix, T), want[f"prefix{level}"] & 0xFFFFFFFF, err_msg=f"prefix{level}")
        np.testing.assert_array_equal(u32(acc.rank, T), want[f"rank{level}"], err_msg=f"rank{level}")
        np.testing.assert_array_equal(acc.resolved.cpu().numpy()[:, :T], want["resolved"], err_msg=f"resolved{level}")

    got = run_select(c, over, blocks_of(c, c.get("splits")), check)
    same_result(got, want)
    again = run_select(c, over, blocks_of(c, c.get("splits")))  # two calls: the same bits
    for a, b in zip(dataclass_bits(got), dataclass_bits(again)):
        assert a == b


def dataclass_bits(res):
    return [getattr(res, n).numpy().tobytes() for n in ("lower", "higher", "linear", "count")]


@pytest.mark.parametrize("name", K.CASES)
def test_histogram_equals_the_restatement(name):
    from saev_amd.engine import LatentHist

    c = K.get(name)
    lat, key, n = R.entries_of(c["indptr"], c["indices"], c["data"], c["S"])
    hist = LatentHist(c["S"], DEV)
    for b in blocks_of(c, c.get("splits")):
        hist.add_csr(*b)
    assert int(hist.n_rows.item()) == n
    # the table through its non-zeros: (latent, bin, count) in row-major order (S = 70 001 is 1.1 GB of counters)
    at = torch.nonzero(hist.counts0)
    flat, cnt = np.unique(lat * 4096 + (key >> 20).astype(np.int64), return_counts=True)
    np.testing.assert_array_equal((at[:, 0] * 4096 + at[:, 1]).cpu().numpy(), flat)
    np.testing.assert_array_equal(u32(hist.counts0[at[:, 0], at[:, 1]]), cnt)
    if c["S"] > 4097:
        return
    want0 = R.counts0_of(lat, key, c["S"])
    np.testing.assert_array_equal(hist.read().numpy(), want0)
    for lo, hi in ((-16, 16), (-1, 1), (-126, 127)):
        got = hist.histogram(lo, hi)
        for g, w in zip(got, R.histogram(want0, lo, hi)):
            np.testing.assert_array_equal(g.numpy().view(np.uint32) if g.dtype == torch.float32 else g.numpy(), w.view(np.uint32) if w.dtype == np.float32 else w)
    hist.zero_()
    assert int(hist.counts0.abs().sum()) == 0 and int(hist.n_rows.item()) == 0


def _padded(c, rng, keep_frac=0.7):
    """The case as padded rows with row_nnz (junk past a row's count) and a keep mask; and the CSR of the kept rows."""
    n = c["indptr"].size - 1
    nnz = np.diff(c["indptr"])
    cap = int(nnz.max()) + 3
    idx = rng.integers(0, c["S"], (n, cap)).astype(np.int32)
    val = rng.standard_normal((n, cap)).astype(np.float32)
    for r in range(n):
        idx[r, :nnz[r]] = c["indices"][c["indptr"][r]:c["indptr"][r + 1]]
        val[r, :nnz[r]] = c["data"][c["indptr"][r]:c["indptr"][r + 1]]
    return idx, val, nnz.astype(np.int32), rng.random(n) < keep_frac


@pytest.mark.parametrize("name", ["ragged_0_300", "value_classes", "zero_block"])
def test_padded_rows_with_row_nnz_and_keep_equal_the_csr_form(name):
    from saev_amd.engine import LatentHist, LatentQuantiles

    c = K.get(name)
    idx, val, row_nnz, keep = _padded(c, np.random.default_rng(11))
    lat, key, n = R.entries_of(c["indptr"], c["indices"], c["data"], c["S"], keep)
    want = R.select(lat, key, c["S"], c["q"], "rows", n)
    half = idx.shape[0] // 2
    parts = [(dev(idx[a:b]), dev(val[a:b]), dev(row_nnz[a:b]), dev(keep[a:b])) for a, b in ((0, half), (half, idx.shape[0]))]
    acc, hist = LatentQuantiles(c["S"], c["q"], DEV, "rows"), LatentHist(c["S"], DEV)
    for level in range(3):
        for p in parts:
            acc.add(*p)
            if level == 0:
                hist.add(*p)
        acc.next_pass()
    same_result(acc.result(), want)
    np.testing.assert_array_equal(hist.read().numpy(), want["counts0"])
    assert int(hist.n_rows.item()) == n == int(keep.sum())
    # the CSR form with the same mask
    acc2 = LatentQuantiles(c["S"], c["q"], DEV, "rows")
    for level in range(3):
        acc2.add_csr(dev(c["indptr"]), dev(c["indices"]), dev(c["data"]), keep=dev(keep))
        acc2.next_pass()
    assert dataclass_bits(acc2.result()) == dataclass_bits(acc.result())
    # full rows without counts: every slot is a code
    full = LatentHist(c["S"], DEV)
    full.add(dev(idx), dev(val))
    flat_ptr = np.arange(0, idx.size + 1, idx.shape[1], dtype=np.int64)
    lat_f, key_f, _ = R.entries_of(flat_ptr, idx.reshape(-1), val.reshape(-1), c["S"])
    np.testing.assert_array_equal(full.read().numpy(), R.counts0_of(lat_f, key_f, c["S"]))


@pytest.mark.parametrize("over", ["rows", "entries"])
def test_one_chunk_seven_ragged_chunks_and_a_shuffled_order_give_the_same_bits(over):
    from saev_amd.engine import latent_quantiles

    c = K.get("ragged_0_300")
    n = c["indptr"].size - 1
    one = run_select(c, over, blocks_of(c))
    seven = run_select(c, over, blocks_of(c, (0, 1, 40, 41, 150, 151, 290, n)))
    order = np.random.default_rng(12).permutation(n)
    shuffled = run_select(c, over, blocks_of(c, (0, 100, n), order))
    assert dataclass_bits(one) == dataclass_bits(seven) == dataclass_bits(shuffled)
    same_result(one, want_of("ragged_0_300", over))
    # the one-shot function, from the host and from the device, in chunks that do not divide the rows
    host = latent_quantiles(c["indptr"], c["indices"], c["data"], n, c["S"], c["q"], over=over, chunk_rows=64, device=DEV)
    device = latent_quantiles(dev(c["indptr"]), dev(c["indices"]), dev(c["data"]), n, c["S"], c["q"], over=over, chunk_rows=n + 5)
    assert dataclass_bits(host) == dataclass_bits(one) == dataclass_bits(device)


@pytest.mark.parametrize("name", ["zero_block", "silent_and_dense", "q_eight"])
def test_rows_equal_entries_with_the_zeros_written_out(name):
    c = K.get(name)
    lat, key, n = R.entries_of(c["indptr"], c["indices"], c["data"], c["S"])
    silent = n - np.bincount(lat, minlength=c["S"])
    lat_z = np.concatenate([lat, np.repeat(np.arange(c["S"]), silent)])
    key_z = np.concatenate([key, np.full(int(silent.sum()), 0x80000000, dtype=np.uint32)])  # the key of +0.0
    want = R.select(lat_z, key_z, c["S"], c["q"], "entries", n)
    got = run_select(c, "rows", blocks_of(c))
    same_result(got, want)
    assert (got.count.numpy() == n).all()


def test_misuse_is_refused_on_the_device():
    from saev_amd import _lib
    from saev_amd.engine import LatentQuantiles

    c = K.get("zero_block")
    blocks = blocks_of(c)
    acc = LatentQuantiles(c["S"], c["q"], DEV)
    with pytest.raises(_lib.SaevError, match="0 of 3 passes"):
        acc.result()
    acc.add_csr(*blocks[0])
    acc.next_pass()
    acc.add_csr(*blocks_of(c, (0, 4))[0])  # fewer rows than the first pass
    with pytest.raises(_lib.SaevError, match="4 kept rows, the first pass 10"):
        acc.next_pass()
    got = run_select(c, "rows", blocks)
    acc = LatentQuantiles(c["S"], c["q"], DEV)
    for _ in range(3):
        acc.add_csr(*blocks[0])
        acc.next_pass()
    with pytest.raises(_lib.SaevError, match="three passes are done"):
        acc.add_csr(*blocks[0])
    with pytest.raises(_lib.SaevError, match="three passes are done"):
        acc.next_pass()
    assert dataclass_bits(acc.result()) == dataclass_bits(got)


def _contents(out):
    """What the pass's own artifacts hold (test_gpu_latent_topk._contents, which knows no activation_hist.pt)."""
    got = {}
    for p in sorted(out.iterdir()):
        if p.name == "token_acts.npz":
            csr = scipy.sparse.load_npz(p)
            got[p.name] = (csr.shape, csr.indptr.tobytes(), csr.indices.tobytes(), csr.data.tobytes())
        elif p.suffix == ".pt" and p.name != "activation_hist.pt":
            t = torch.load(p)
            got[p.name] = (t.dtype, tuple(t.shape), t.numpy().tobytes())
        elif p.name == "metrics.json":
            got[p.name] = p.read_text()
    return got


@pytest.mark.parametrize("tag", ["g14_inference_labels", "g19_inference_relu_plain"])
def test_inference_writes_activation_hist_and_activation_stats_follow(tmp_path, tag):
    from saev_amd import activation_stats
    from saev_amd.data import Metadata, OrderedConfig
    from saev_amd.framework import inference
    from test_gpu_latent_topk import _run_dir

    g, d, run = _run_dir(tmp_path, tag)
    out = run.inference / Metadata.load(d).hash
    cfg = inference.Config(run=run.run_dir, data=OrderedConfig(shards=d, layer=11, batch_size=int(g["batch_size"])),
                           n_dists=int(g["n_dists"]), ignore_labels=g["ignore_labels"].tolist())
    inference.worker_fn(cfg)
    plain = _contents(out)
    names = sorted(p.name for p in out.iterdir())
    forced = inference.Config(run=cfg.run, data=cfg.data, n_dists=cfg.n_dists, ignore_labels=cfg.ignore_labels, force_recompute=True)
    inference.worker_fn(forced, activation_hist=True)
    assert sorted(p.name for p in out.iterdir()) == sorted(names + ["activation_hist.pt"])
    assert _contents(out) == plain and len(plain) == 5  # every other artifact holds what it held
    csr = scipy.sparse.load_npz(out / "token_acts.npz")
    S = csr.shape[1]
    lat, key, n = R.entries_of(csr.indptr, csr.indices, csr.data, S)
    want0 = R.counts0_of(lat, key, S)
    got = torch.load(out / "activation_hist.pt")
    assert sorted(got) == ["counts0", "n_rows"] and got["counts0"].dtype == torch.int32 and 0 < got["n_rows"] <= csr.shape[0]
    assert got["n_rows"] == csr.shape[0] or "labels" in tag  # the kept tokens
    np.testing.assert_array_equal(got["counts0"].numpy(), want0)
    # rebuilt from token_acts.npz when only it is missing; removed by a pass that rewrites the codes without it
    (out / "activation_hist.pt").unlink()
    inference.worker_fn(cfg, activation_hist=True)
    assert torch.equal(torch.load(out / "activation_hist.pt")["counts0"], got["counts0"])
    inference.worker_fn(forced)
    assert not (out / "activation_hist.pt").exists() and _contents(out) == plain

    # activation_stats at token level, against the restatement of the stored codes
    q = (0.5, 0.95, 1.0)
    scfg = activation_stats.Config(run=run.run_dir, shards=d, q=q, chunk_rows=7, lo_exp=-8, hi_exp=4, device=DEV)
    path = activation_stats.worker_fn(scfg)
    assert path == out / "activation_stats.npz"
    want = R.select(lat, key, S, q, "rows", csr.shape[0])
    with np.load(path) as z:
        z = {k: z[k] for k in z.files}
    assert sorted(z) == sorted(activation_stats.KEYS) and str(z["over"]) == "rows" and str(z["level"]) == "token"
    for name, dt in (("lower", np.float32), ("higher", np.float32), ("linear", np.float64), ("count", np.int64), ("hist_counts", np.int64),
                     ("hist_n_neg", np.int64), ("hist_edges", np.float32), ("q", np.float64)):
        assert z[name].dtype == dt, name
    for name in ("lower", "higher", "linear", "count"):
        np.testing.assert_array_equal(z[name], want[name], err_msg=name)
    for got_h, want_h in zip((z["hist_counts"], z["hist_n_neg"], z["hist_edges"]), R.histogram(want0, -8, 4)):
        np.testing.assert_array_equal(got_h, want_h)
    np.testing.assert_array_equal(activation_stats.thresholds(path, 0.95), want["linear"][:, 1].astype(np.float32))
    np.testing.assert_array_equal(activation_stats.thresholds(path, 0.95, "higher"), want["higher"][:, 1])
    stamp = path.stat().st_mtime_ns
    activation_stats.worker_fn(scfg)
    assert path.stat().st_mtime_ns == stamp  # a current file is left alone

    # image level: the quantiles over images of the max-pooled, clamped codes; another question, so the file is rebuilt
    tpi = Metadata.load(d).content_tokens_per_example
    n_img = csr.shape[0] // tpi
    pooled = np.maximum(csr.toarray().astype(np.float32).reshape(n_img, tpi, S).max(axis=1), 0)
    icfg = activation_stats.Config(run=run.run_dir, shards=d, q=q, level="image", device=DEV)
    activation_stats.worker_fn(icfg)
    with np.load(path) as z:
        assert str(z["level"]) == "image" and (z["count"] == n_img).all()
        np.testing.assert_array_equal(z["lower"], np.quantile(pooled, q, axis=0, method="lower").T)
        np.testing.assert_array_equal(z["higher"], np.quantile(pooled, q, axis=0, method="higher").T)

    # the tool
    res = subprocess.run([sys.executable, str(ROOT / "tools" / "latent_quantiles.py"), "--run", str(run.run_dir), "--shards", str(d), "--q", "0.5",
                          "0.95", "--level", "image"], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    assert "q=0.95" in res.stdout and "share of latents whose quantile is 0" in res.stdout
