"""CPU-only tests of the per-latent histograms and quantiles (include/saev_amd.h: LATENT HISTOGRAM): the entries are
declared, exported and bound with the header's types; every argument check refuses a call before anything touches a device; the
integer restatement the GPU tests compare the kernels with (tests/latent_hist_restatement.py) against np.histogram and np.quantile
on every case of tests/latent_hist_cases.py and against the reference's recorded ``distributions``; and the host side of
saev_amd.activation_stats."""

import ctypes as C
import re
import subprocess

import numpy as np
import pytest
import torch

import latent_hist_cases as K
import latent_hist_restatement as R
from conftest import ROOT, load_golden

ENTRIES = ("saev_latent_hist_workspace_bytes", "saev_latent_hist_update", "saev_latent_hist_locate")
CTYPES = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64}
INVALID, UNSUPPORTED = -1, -3


def _lib():
    subprocess.run(["make", "-C", str(ROOT)], check=True, capture_output=True)
    from saev_amd import _lib

    return _lib, _lib.load()


def _ctype(decl: str, lib_mod):
    decl = decl.replace("const", "").strip()
    if "saev_latent_hist_state" in decl:
        return C.POINTER(lib_mod.SaevLatentHistState)
    if "saev_latent_hist_targets" in decl:
        return C.POINTER(lib_mod.SaevLatentHistTargets)
    if "*" in decl:
        return C.c_void_p
    return CTYPES[decl.split()[0]]


def test_entries_are_declared_exported_and_bound_with_the_headers_types():
    lib_mod, lib = _lib()
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "saev_amd.h").read_text(), flags=re.S)
    for name in ENTRIES:
        m = re.search(r"(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, f"{name} is not declared"
        args = [_ctype(re.sub(r"\w+\s*$", "", a.strip()), lib_mod) for a in m.group(2).split(",")]
        want_res, want_args = lib_mod._SIGNATURES[name]
        assert want_res is CTYPES[m.group(1)], name
        assert list(want_args) == args, name
        assert hasattr(lib, name) and name in lib_mod.EXPORTED_SYMBOLS
    assert lib.saev_abi_version() == 12 and lib_mod.ABI_VERSION == 12  # additive entries: the version stays
    assert re.search(r"#define\s+SAEV_AMD_ABI_VERSION\s+12\b", text)


@pytest.mark.parametrize("struct,cls", [("saev_latent_hist_state", "SaevLatentHistState"), ("saev_latent_hist_targets", "SaevLatentHistTargets")])
def test_struct_layouts_match_the_header(tmp_path, struct, cls):
    lib_mod, _ = _lib()
    cls = getattr(lib_mod, cls)
    fields = [f for f, _ in cls._fields_]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "saev_amd.h"', "int main(void) {", f'printf("size %zu\\n", sizeof({struct}));']
    src += [f'printf("{f} %zu\\n", offsetof({struct}, {f}));' for f in fields]
    src.append("return 0; }")
    (tmp_path / "layout.c").write_text("\n".join(src))
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True)
    want = dict(line.split() for line in subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.splitlines())
    assert C.sizeof(cls) == int(want["size"])
    for f in fields:
        assert getattr(cls, f).offset == int(want[f]), f


def _fake(i):
    return C.c_void_p((1 << 21) + 4096 * i)


PADDED = dict(idx=_fake(3), val=_fake(4))
CSR = dict(row_ptr=_fake(5), indices=_fake(6), data=_fake(7), nnz=800)
NO_PADDED = dict(idx=None, val=None)
# the fake device pointers are never dereferenced: a launch on them would fault, and this machine has no device to launch on
BAD_UPDATES = [
    ("negative_n", dict(n=-1), INVALID, "negative size"),
    ("s_2_31", dict(S=1 << 31), INVALID, "size above 2^31 - 1"),
    ("null_state", dict(state=None), INVALID, "no saev_latent_hist_state (or its struct_size is unset)"),
    ("level_minus_1", dict(level=-1), INVALID, "level must be 0, 1 or 2"),
    ("level_3", dict(level=3), INVALID, "level must be 0, 1 or 2"),
    ("t_zero", dict(level=1, T=0), UNSUPPORTED, "T must lie in [1, 16] at levels 1 and 2"),
    ("t_17", dict(level=2, T=17), UNSUPPORTED, "T must lie in [1, 16] at levels 1 and 2"),
    ("null_counts", dict(counts=None), INVALID, "a state pointer is NULL"),
    ("null_n_rows", dict(n_rows=None), INVALID, "a state pointer is NULL"),
    ("null_prefix", dict(level=1, T=4, prefix=None), INVALID, "a state pointer is NULL"),
    ("counts_misaligned", dict(counts=C.c_void_p((1 << 21) + 4)), INVALID, "the count and prefix tables must be 16-byte aligned"),
    ("table_2_32_level0", dict(S=(1 << 20)), UNSUPPORTED, "the count table must stay below 2^32 - 1 counters"),
    ("table_2_32_level1", dict(level=1, T=16, S=(1 << 18)), UNSUPPORTED, "the count table must stay below 2^32 - 1 counters"),
    ("both_forms", dict(CSR), INVALID, "give the codes as padded rows (idx, val) or as CSR (row_ptr, indices, data), one of the two"),
    ("neither_form", dict(NO_PADDED), INVALID, "give the codes as padded rows (idx, val) or as CSR (row_ptr, indices, data), one of the two"),
    ("idx_without_val", dict(val=None), INVALID, "idx and val come together"),
    ("csr_without_data", dict(NO_PADDED, **dict(CSR, data=None)), INVALID, "row_ptr, indices and data come together"),
    ("row_nnz_with_csr", dict(NO_PADDED, row_nnz=_fake(8), **CSR), INVALID, "row_nnz belongs to the padded form"),
    ("too_many_entries", dict(n=1 << 20, cap=1 << 12), UNSUPPORTED, "more than 2^31 - 1 entries in one batch"),
    ("workspace_too_small", dict(ws_short=1), INVALID, "workspace smaller than saev_latent_hist_workspace_bytes(entries, S)"),
    ("workspace_null", dict(ws=None), INVALID, "workspace smaller than saev_latent_hist_workspace_bytes(entries, S)"),
    ("workspace_misaligned", dict(ws=C.c_void_p((1 << 20) + 8)), INVALID, "workspace must be 256-byte aligned"),
]


def _update(lib_mod, lib, over):
    a = dict(PADDED, row_nnz=None, cap=8, row_ptr=None, indices=None, data=None, nnz=0, keep=None, n=100, S=512, level=0, T=0,
             counts=_fake(0), n_rows=_fake(1), prefix=_fake(2), ws=C.c_void_p(1 << 20), ws_short=0)
    a.update(over)
    st = lib_mod.SaevLatentHistState(struct_size=C.sizeof(lib_mod.SaevLatentHistState), level=a["level"], T=a["T"], counts=a["counts"],
                                     n_rows=a["n_rows"], prefix=a["prefix"])
    need = lib.saev_latent_hist_workspace_bytes(800, 512)
    assert need > 0 and need % 256 == 0
    return lib.saev_latent_hist_update(a["idx"], a["val"], a["row_nnz"], a["cap"], a["row_ptr"], a["indices"], a["data"], a["nnz"], a["keep"],
                                       a["n"], a["S"], a.get("state", C.byref(st)), a["ws"], need - a["ws_short"], None)


@pytest.mark.parametrize("case", BAD_UPDATES, ids=[c[0] for c in BAD_UPDATES])
def test_update_refuses_bad_arguments_without_a_device(case):
    lib_mod, lib = _lib()
    name, over, status, text = case
    assert _update(lib_mod, lib, over) == status, name
    assert lib.saev_last_error(None).decode() == "saev_latent_hist_update: " + text


BAD_LOCATES = [
    ("negative_s", dict(S=-1), INVALID, "negative size"),
    ("null_state", dict(state=None), INVALID, "no saev_latent_hist_state (or its struct_size is unset)"),
    ("null_targets", dict(targets=None), INVALID, "no saev_latent_hist_targets (or its struct_size is unset)"),
    ("level_3", dict(level=3), INVALID, "level must be 0, 1 or 2"),
    ("q_count_0", dict(Q=0), UNSUPPORTED, "Q must lie in [1, 8]"),
    ("q_count_9", dict(Q=9), UNSUPPORTED, "Q must lie in [1, 8]"),
    ("q_above_1", dict(q=(0.5, 1.0000001)), INVALID, "every q must lie in [0, 1]"),
    ("q_negative", dict(q=(-1e-9, 0.5)), INVALID, "every q must lie in [0, 1]"),
    ("q_nan", dict(q=(0.5, float("nan"))), INVALID, "every q must lie in [0, 1]"),
    ("t_is_not_2q", dict(level=1, T=6), INVALID, "the state's T must be 2 Q"),
    ("null_counts", dict(counts=None), INVALID, "a state pointer is NULL"),
    ("null_n_rows_over_rows", dict(n_rows=None), INVALID, "a state pointer is NULL"),
    ("null_rank", dict(rank=None), INVALID, "a target pointer is NULL"),
    ("null_linear_at_level_2", dict(level=2, T=4, linear=None), INVALID, "lower, higher and linear are written after level 2"),
    ("table_2_32", dict(S=1 << 20), UNSUPPORTED, "the count table must stay below 2^32 - 1 counters"),
]


def _locate(lib_mod, lib, over):
    a = dict(S=512, level=0, T=0, Q=2, q=(0.5, 0.9), over_rows=1, counts=_fake(0), n_rows=_fake(1), prefix=_fake(2), rank=_fake(3),
             resolved=_fake(4), count=_fake(5), lower=_fake(6), higher=_fake(7), linear=_fake(8))
    a.update(over)
    st = lib_mod.SaevLatentHistState(struct_size=C.sizeof(lib_mod.SaevLatentHistState), level=a["level"], T=a["T"], counts=a["counts"],
                                     n_rows=a["n_rows"], prefix=a["prefix"])
    tg = lib_mod.SaevLatentHistTargets(struct_size=C.sizeof(lib_mod.SaevLatentHistTargets), Q=a["Q"], over_rows=a["over_rows"],
                                       q=(C.c_double * 8)(*a["q"]), **{k: a[k] for k in ("prefix", "rank", "resolved", "count", "lower", "higher", "linear")})
    return lib.saev_latent_hist_locate(a.get("state", C.byref(st)), a.get("targets", C.byref(tg)), a["S"], None)


@pytest.mark.parametrize("case", BAD_LOCATES, ids=[c[0] for c in BAD_LOCATES])
def test_locate_refuses_bad_arguments_without_a_device(case):
    lib_mod, lib = _lib()
    name, over, status, text = case
    assert _locate(lib_mod, lib, over) == status, name
    assert lib.saev_last_error(None).decode() == "saev_latent_hist_locate: " + text


def test_empty_calls_are_accepted_and_touch_nothing():
    lib_mod, lib = _lib()
    assert _update(lib_mod, lib, dict(NO_PADDED, n=0, ws=None)) == 0
    assert _update(lib_mod, lib, dict(S=0)) == 0  # no latents: nothing to launch
    assert _locate(lib_mod, lib, dict(S=0)) == 0
    assert lib.saev_latent_hist_workspace_bytes(0, 0) == 256
    for e, S in [(-1, 64), (1 << 31, 64), (10, -1), (10, 1 << 31)]:
        assert lib.saev_latent_hist_workspace_bytes(e, S) == -1, (e, S)


def test_python_entries_refuse_bad_arguments():
    _lib()
    from saev_amd import activation_stats, engine

    with pytest.raises(ValueError, match="unsupported d_sae"):
        engine.LatentHist(0, "cuda")
    with pytest.raises(RuntimeError, match="no CPU path"):
        engine.LatentHist(64, "cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        engine.LatentQuantiles(64, (0.5,), "cpu")
    for q in ((), tuple([0.5] * 9)):
        with pytest.raises(ValueError, match="unsupported number of quantiles"):
            engine.LatentQuantiles(64, q, "cuda")
    with pytest.raises(ValueError, match=r"every q must lie in \[0, 1\]"):
        engine.LatentQuantiles(64, (0.5, 1.5), "cuda")
    with pytest.raises(ValueError, match="over must be"):
        engine.LatentQuantiles(64, (0.5,), "cuda", over="tokens")
    with pytest.raises(ValueError, match="lo_exp < hi_exp"):
        engine.hist_window(torch.zeros(2, 4096, dtype=torch.int64), 3, 3)
    for bad in (dict(level="pixel"), dict(over="tokens"), dict(q=()), dict(q=(2.0,)), dict(lo_exp=4, hi_exp=4)):
        with pytest.raises(ValueError):
            activation_stats.worker_fn(activation_stats.Config(**bad))


# ---- the restatement against numpy ---------------------------------------------------------------------------------------------------


def test_every_case_still_exercises_what_it_names():
    for name in K.CASES:
        c = K.get(name)
        assert c["holds"](c), name
        assert c["S"] <= 4097 or name == "s_70001"


def test_key_map_is_monotone_and_invertible_over_every_float_class():
    rng = np.random.default_rng(0)
    bits = np.concatenate([rng.integers(0, 1 << 32, 200_000, dtype=np.uint64).astype(np.uint32),
                           np.array([0, 1, 0x007FFFFF, 0x00800000, 0x7F7FFFFF, 0x7F800000, 0x80000000, 0x80000001, 0x807FFFFF, 0x80800000,
                                     0xFF7FFFFF, 0xFF800000, 0x3F800000, 0xBF800000], dtype=np.uint32)])
    v = bits.view(np.float32)
    v = v[~np.isnan(v)]
    key = R.key_of(v)
    np.testing.assert_array_equal(R.value_of(key).view(np.uint32), v.view(np.uint32))  # invertible, -0.0 and +0.0 apart
    order = np.argsort(key, kind="stable")
    sv, sk = v[order], key[order]
    assert (np.diff(sv.astype(np.float64)) >= 0).all()
    apart = np.diff(sk.astype(np.int64)) > 0
    assert ((np.diff(sv.astype(np.float64)) > 0) | ~apart | ((sv[1:] == 0) & (sv[:-1] == 0))).all()  # strictly increasing but for -0 < +0
    assert R.key_of(np.float32(0.0)) == 0x80000000 and (R.key_of(np.float32(-1e-45)) >> 20) == 2047  # the zero block's place


@pytest.mark.parametrize("name", [n for n in K.CASES if n != "s_70001"])
def test_histogram_equals_np_histogram_with_the_returned_edges(name):
    c = K.get(name)
    lat, key, _ = R.entries_of(c["indptr"], c["indices"], c["data"], c["S"])
    counts0 = R.counts0_of(lat, key, c["S"])
    vals = R.value_of(key)
    for lo, hi in ((-16, 16), (-3, 2), (-126, 127)):
        counts, n_neg, edges = R.histogram(counts0, lo, hi)
        assert edges.dtype == np.float32 and edges.size == 8 * (hi - lo) + 1 and counts.shape == (c["S"], 8 * (hi - lo) + 2)
        e = np.arange(lo, hi + 1, dtype=np.float64)[:, None]
        np.testing.assert_array_equal(edges.astype(np.float64), (np.exp2(e) * (1 + np.arange(8) / 8)).reshape(-1)[:edges.size])
        for j in np.unique(lat)[:64]:
            x = vals[lat == j].astype(np.float64)
            pos = x[x > 0]
            inside = pos[(pos >= edges[0]) & (pos < edges[-1])]  # (np.histogram closes its last bin on the right: cut it open)
            np.testing.assert_array_equal(counts[j, 1:-1], np.histogram(inside, bins=edges.astype(np.float64))[0])
            assert counts[j, 0] == (pos < edges[0]).sum() and counts[j, -1] == (pos >= edges[-1]).sum() and n_neg[j] == (x < 0).sum()
    # the device's merge (engine.hist_window, run here on a CPU tensor) is the same slice-and-merge
    from saev_amd.engine import hist_window

    got = hist_window(torch.from_numpy(counts0[:64]), -3, 2)
    for g, w in zip(got, R.histogram(counts0[:64], -3, 2)):
        np.testing.assert_array_equal(g.numpy(), w)


@pytest.mark.parametrize("over", ["rows", "entries"])
@pytest.mark.parametrize("name", [n for n in K.CASES if n not in ("flush0", "s_70001")])  # (those two are histogram cases)
def test_quantiles_equal_np_quantile_on_the_dense_matrix(name, over):
    c = K.get(name)
    lat, key, n = R.entries_of(c["indptr"], c["indices"], c["data"], c["S"])
    got = R.select(lat, key, c["S"], c["q"], over, n)
    dense = R.dense_of(c["indptr"], c["indices"], c["data"], c["S"])
    q = np.asarray(c["q"], dtype=np.float64)
    for j in range(c["S"]):
        x = dense[:, j] if over == "rows" else dense[:, j][dense[:, j] != 0]
        assert got["count"][j] == x.size
        if x.size == 0:
            assert np.isnan(got["lower"][j]).all() and np.isnan(got["higher"][j]).all() and np.isnan(got["linear"][j]).all()
            continue
        lower, higher = np.quantile(x, q, method="lower"), np.quantile(x, q, method="higher")
        # on the bits, but for the sign of a zero: the zero block is +0.0, numpy returns whichever zero the row stored
        for mine, ref in ((got["lower"][j], lower), (got["higher"][j], higher)):
            assert mine.dtype == np.float32 and ref.dtype == np.float32
            np.testing.assert_array_equal(np.where(mine == 0, np.float32(0), mine).view(np.uint32), np.where(ref == 0, np.float32(0), ref).view(np.uint32))
        if not np.isfinite(x).all():
            continue
        with np.errstate(over="ignore"):
            ref = np.quantile(x.astype(np.float64), q)
        # three fp64 roundings on magnitudes of at most twice max(|lower|, |higher|)
        bound = 4 * 2.0**-53 * np.maximum(np.abs(lower.astype(np.float64)), np.abs(higher.astype(np.float64)))
        assert (np.abs(got["linear"][j] - ref) <= bound).all(), (j, got["linear"][j], ref, bound)


@pytest.mark.parametrize("tag", ["g14_inference_plain", "g19_inference_relu_plain"])
def test_recorded_distributions_have_the_histogram_of_the_recorded_codes(tag):
    """``distributions`` is what the reference's own inference pass wrote: the dense activations of the first n_dists latents, one row
    per example, the example's last token (its rows are indexed by example_idx, so later tokens overwrite earlier ones and the rows
    past the last example stay zero).  The histogram of those columns' non-zero values is the histogram the restatement takes of
    the same tokens' recorded codes."""
    g = load_golden(tag)
    n_dists, (n_tokens, S) = int(g["n_dists"]), g["csr_shape"].tolist()
    n_examples = g["acts"].shape[0]
    tpe = n_tokens // n_examples
    dist = g["distributions"].numpy()
    assert dist.shape == (n_tokens, n_dists) and (dist[n_examples:] == 0).all() and (dist != 0).any()
    keep = np.zeros(n_tokens, dtype=bool)
    keep[tpe - 1::tpe] = True  # the last token of every example
    lat, key, n = R.entries_of(g["csr_indptr"].numpy(), g["csr_indices"].numpy(), g["csr_data"].numpy(), n_dists, keep)
    assert n == n_examples
    got = R.histogram(R.counts0_of(lat, key, n_dists))
    rows, cols = np.nonzero(dist)
    want = R.histogram(R.counts0_of(cols, R.key_of(dist[rows, cols]), n_dists))
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, b)
    # and np.histogram of the recorded columns themselves, with the returned edges
    counts, n_neg, edges = got
    for j in range(n_dists):
        x = dist[:n_examples, j].astype(np.float64)
        pos = x[x > 0]
        np.testing.assert_array_equal(counts[j, 1:-1], np.histogram(pos[(pos >= edges[0]) & (pos < edges[-1])], bins=edges.astype(np.float64))[0])
        assert n_neg[j] == (x < 0).sum() and counts[j, 0] + counts[j, -1] == ((pos < edges[0]) | (pos >= edges[-1])).sum()


# ---- activation_stats on the host ----------------------------------------------------------------------------------------------------


class _FakeHist:
    """engine.LatentHist with the restatement behind it (CPU tensors)."""

    def __init__(self, d_sae, device):
        self.S, self.counts0 = d_sae, np.zeros((d_sae, 4096), dtype=np.int64)

    def add_csr(self, indptr, indices, data, keep=None):
        lat, key, _ = R.entries_of(indptr.numpy(), indices.numpy(), data.numpy(), self.S)
        self.counts0 += R.counts0_of(lat, key, self.S)

    def histogram(self, lo, hi):
        from saev_amd.engine import hist_window

        return hist_window(torch.from_numpy(self.counts0), lo, hi)


def _fake_quantiles(indptr, indices, data, n_rows, n_latents, q, *, over="rows", chunk_rows=2**20, device=None, hist=None):
    from saev_amd.engine import LatentQuantilesHost

    lat, key, n = R.entries_of(indptr.numpy(), indices.numpy(), data.numpy(), n_latents)
    if hist is not None:
        hist.add_csr(indptr, indices, data)
    got = R.select(lat, key, n_latents, q, over, n)
    return LatentQuantilesHost(*(torch.from_numpy(got[k]) for k in ("lower", "higher", "linear", "count")))


def test_activation_stats_file_current_check_and_thresholds(tmp_path, monkeypatch):
    """worker_fn with the device pieces replaced by the restatement: the file's keys, dtypes and shapes, when it is rebuilt, and
    thresholds()."""
    import scipy.sparse

    from saev_amd import activation_stats, classification, engine

    c = K.get("ragged_0_300")
    out = tmp_path / "inference" / "hash"
    out.mkdir(parents=True)
    csr = scipy.sparse.csr_array((c["data"], c["indices"], c["indptr"]), shape=(c["indptr"].size - 1, c["S"]))
    scipy.sparse.save_npz(out / "token_acts.npz", csr)
    monkeypatch.setattr(activation_stats, "stats_path", lambda cfg: out / activation_stats.FNAME)
    monkeypatch.setattr(engine, "_hip_device", lambda who, device: torch.device("cpu"))
    monkeypatch.setattr(classification, "_csr_on", lambda a, dev: (torch.from_numpy(a.indptr.astype(np.int64)), torch.from_numpy(a.indices.astype(np.int32)),
                                                                   torch.from_numpy(a.data)))
    monkeypatch.setattr(engine, "LatentHist", _FakeHist)
    calls = []
    monkeypatch.setattr(engine, "latent_quantiles", lambda *a, **kw: (calls.append(kw["over"]), _fake_quantiles(*a, **kw))[1])
    cfg = activation_stats.Config(q=(0.5, 0.99), lo_exp=-4, hi_exp=4)
    path = activation_stats.worker_fn(cfg)
    S, Q, nb = c["S"], 2, 8 * 8
    with np.load(path) as z:
        z = {k: z[k] for k in z.files}
    assert sorted(z) == sorted(activation_stats.KEYS)
    want = {"q": (np.float64, (Q,)), "lower": (np.float32, (S, Q)), "higher": (np.float32, (S, Q)), "linear": (np.float64, (S, Q)),
            "count": (np.int64, (S,)), "hist_counts": (np.int64, (S, nb + 2)), "hist_n_neg": (np.int64, (S,)), "hist_edges": (np.float32, (nb + 1,))}
    for name, (dt, shape) in want.items():
        assert z[name].dtype == dt and z[name].shape == shape, name
    assert str(z["over"]) == "rows" and str(z["level"]) == "token" and (z["count"] == csr.shape[0]).all()
    assert z["hist_counts"].sum() + z["hist_n_neg"].sum() == (c["data"] != 0).sum()
    # current: left alone; another q, multiset or window: rebuilt; forced: rebuilt
    activation_stats.worker_fn(cfg)
    assert calls == ["rows"]
    for other in (dict(q=(0.5,)), dict(over="entries"), dict(lo_exp=-5), dict(hi_exp=5), dict(force_recompute=True)):
        before = len(calls)
        kw = dict(q=(0.5, 0.99), lo_exp=-4, hi_exp=4)
        kw.update(other)
        activation_stats.worker_fn(activation_stats.Config(**kw))
        assert len(calls) == before + 1, other
    assert activation_stats._current(path, cfg, S) and not activation_stats._current(path, cfg, S + 1)
    assert not activation_stats._current(path, activation_stats.Config(q=(0.5,), lo_exp=-4, hi_exp=4))
    assert not activation_stats._current(tmp_path / "missing.npz", cfg)
    # thresholds
    with np.load(path) as z:
        lower, linear = z["lower"], z["linear"]
    thr = activation_stats.thresholds(path, 0.99)
    assert thr.dtype == np.float32 and thr.shape == (S,) and thr.flags["C_CONTIGUOUS"]
    np.testing.assert_array_equal(thr, linear[:, 1].astype(np.float32))
    np.testing.assert_array_equal(activation_stats.thresholds(path, 0.5, "lower"), lower[:, 0])
    with pytest.raises(ValueError, match="not 0.9"):
        activation_stats.thresholds(path, 0.9)
    with pytest.raises(ValueError, match="method"):
        activation_stats.thresholds(path, 0.5, "nearest")
    with pytest.raises(FileNotFoundError):
        (out / "token_acts.npz").unlink()
        activation_stats.worker_fn(cfg)
