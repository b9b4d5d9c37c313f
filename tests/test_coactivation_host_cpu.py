"""CPU-only tests of COACTIVATION (include/saev_amd.h): the entries are declared, exported and bound with the header's
types and the ABI is still 12; every argument check refuses a call, in order, before anything touches a device; the workspace
arithmetic; the restatement the GPU tests lean on (tests/coactivation_restatement.py) against an independent pair-counting loop,
ties and 64-bit cross-products included; every case of tests/coactivation_cases.py has the property it was built for; and the
host side of saev_amd.alignment (file keys and dtypes, robustness, the row-count mismatch).  Everything is integers: equality only."""

import ctypes as C
import itertools
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse

import coactivation_cases as K
import coactivation_restatement as R
from conftest import ROOT

ENTRIES = ("saev_coactivation_chunk_rows", "saev_coactivation_window", "saev_coactivation_slots", "saev_coactivation_workspace_bytes", "saev_coactivation")
CTYPES = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float}
INVALID, UNSUPPORTED = -1, -3


def _lib():
    subprocess.run(["make", "-C", str(ROOT)], check=True, capture_output=True)
    from saev_amd import _lib

    return _lib, _lib.load()


def test_entries_are_declared_exported_and_bound_with_the_headers_types():
    lib_mod, lib = _lib()
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "saev_amd.h").read_text(), flags=re.S)
    for name in ENTRIES:
        m = re.search(r"(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, f"{name} is not declared"
        decls = [a.strip() for a in m.group(2).split(",")]
        args = [] if decls == ["void"] else [C.c_void_p if "*" in a else CTYPES[a.replace("const", "").split()[0]] for a in decls]
        want_res, want_args = lib_mod._SIGNATURES[name]
        assert want_res is CTYPES[m.group(1)], name
        assert list(want_args) == args, name
        assert hasattr(lib, name) and name in lib_mod.EXPORTED_SYMBOLS
    assert lib.saev_abi_version() == 12 and lib_mod.ABI_VERSION == 12  # additive entries: the version stays
    for name in ("SAEV_COACT_JACCARD 0", "SAEV_COACT_CONTAINMENT 1", "SAEV_COACT_ERR_COLUMN 1", "SAEV_COACT_ERR_VALUE 2", "SAEV_COACT_ERR_INDPTR 3"):
        assert re.search(r"#define\s+" + name.replace(" ", r"\s+") + r"\b", text)
    assert "coactivation.hip" in (ROOT / "Makefile").read_text()
    # the constants the cases are built around
    assert (lib.saev_coactivation_chunk_rows(), lib.saev_coactivation_window(), lib.saev_coactivation_slots()) == (K.CHUNK_ROWS, K.WINDOW, K.SLOTS)
    assert K.WINDOW * 4 <= 160 * 1024 - 4096  # the window's counters and the merge's few words fit the CU's 160 KB of LDS


def _fake(i):
    return C.c_void_p((1 << 21) + 4096 * i)


ARGS = ("a_indptr", "a_indices", "a_data", "nnz_a", "Sa", "b_indptr", "b_indices", "b_data", "nnz_b", "Sb", "N", "thr_a", "thr_b", "measure", "top_m",
        "n_a", "n_b", "out_index", "out_inter", "err", "ws", "ws_bytes", "stream")


def _good():
    return dict(a_indptr=_fake(0), a_indices=_fake(1), a_data=_fake(2), nnz_a=800, Sa=64, b_indptr=_fake(3), b_indices=_fake(4), b_data=_fake(5),
                nnz_b=700, Sb=48, N=100, thr_a=0.0, thr_b=0.0, measure=0, top_m=1, n_a=_fake(6), n_b=_fake(7), out_index=_fake(8), out_inter=_fake(9),
                err=_fake(10), ws=C.c_void_p(1 << 30), ws_bytes=1 << 40, stream=None)


# the fake device pointers are never dereferenced: a launch on them would fault, and this machine has no device to launch on.
# In the order the entry makes its refusals: each case breaks one argument and, with it, every LATER check (so the earlier one wins)
BAD = [
    ("negative_n", dict(N=-1), INVALID, "negative size"), ("negative_sa", dict(Sa=-1), INVALID, "negative size"),
    ("negative_sb", dict(Sb=-1), INVALID, "negative size"), ("negative_nnz_a", dict(nnz_a=-1), INVALID, "negative size"),
    ("negative_nnz_b", dict(nnz_b=-1), INVALID, "negative size"),
    ("n_2_31", dict(N=1 << 31), UNSUPPORTED, "below 2^31"), ("sa_2_31", dict(Sa=1 << 31), UNSUPPORTED, "below 2^31"),
    ("sb_2_31", dict(Sb=1 << 31), UNSUPPORTED, "below 2^31"), ("nnz_a_2_31", dict(nnz_a=1 << 31), UNSUPPORTED, "below 2^31"),
    ("nnz_b_2_31", dict(nnz_b=1 << 31), UNSUPPORTED, "below 2^31"),
    ("zero_n", dict(N=0), INVALID, "at least 1"), ("zero_sa", dict(Sa=0), INVALID, "at least 1"), ("zero_sb", dict(Sb=0), INVALID, "at least 1"),
    ("top_m_0", dict(top_m=0), INVALID, "top_m"), ("top_m_9", dict(top_m=9), INVALID, "top_m"),
    ("measure_2", dict(measure=2), INVALID, "measure"), ("measure_negative", dict(measure=-1), INVALID, "measure"),
    ("null_a_indptr", dict(a_indptr=None), INVALID, "must not be NULL"), ("null_n_a", dict(n_a=None), INVALID, "must not be NULL"),
    ("null_out_index", dict(out_index=None), INVALID, "must not be NULL"), ("null_out_inter", dict(out_inter=None), INVALID, "must not be NULL"),
    ("null_err", dict(err=None), INVALID, "must not be NULL"),
    ("null_a_indices", dict(a_indices=None), INVALID, "a_indices and a_data"), ("null_a_data", dict(a_data=None), INVALID, "a_indices and a_data"),
    ("null_n_b", dict(n_b=None), INVALID, "n_b comes with B"),
    ("null_b_indices", dict(b_indices=None), INVALID, "b_indices and b_data"), ("null_b_data", dict(b_data=None), INVALID, "b_indices and b_data"),
    ("null_workspace", dict(ws=None), INVALID, "workspace smaller"), ("short_workspace", dict(ws_bytes=255), INVALID, "workspace smaller"),
    ("unaligned_workspace", dict(ws=C.c_void_p((1 << 30) + 64)), INVALID, "256-byte aligned"),
]
STAGES = ["negative size", "below 2^31", "at least 1", "top_m", "measure", "must not be NULL", "a_indices and a_data", "n_b comes with B",
          "b_indices and b_data", "workspace smaller", "256-byte aligned"]


def _call(lib, a):
    return lib.saev_coactivation(*[a[k] for k in ARGS])


@pytest.mark.parametrize("case", BAD, ids=[c[0] for c in BAD])
def test_refuses_bad_arguments_without_a_device(case):
    _, lib = _lib()
    _, over, status, text = case
    a = _good()
    a.update(over)
    assert _call(lib, a) == status, lib.saev_last_error(None)
    msg = lib.saev_last_error(None).decode()
    assert msg.startswith("saev_coactivation: ") and text in msg, msg


def test_refusals_come_in_the_stated_order():
    _, lib = _lib()
    first = {}
    for _, over, _, text in BAD:
        first.setdefault(text, over)
    assert list(first) == STAGES
    for (t1, o1), (t2, o2) in itertools.combinations(first.items(), 2):
        if set(o1) & set(o2):
            continue
        a = _good()
        a.update(o1)
        a.update(o2)
        assert _call(lib, a) != 0
        assert t1 in lib.saev_last_error(None).decode(), (t1, t2, lib.saev_last_error(None))


def test_self_mode_ignores_the_b_arguments_in_its_checks():
    _, lib = _lib()
    a = _good()
    a.update(b_indptr=None, b_indices=None, b_data=None, n_b=None, Sb=-5, nnz_b=-5, ws_bytes=0)
    assert _call(lib, a) == INVALID and "workspace smaller" in lib.saev_last_error(None).decode()  # (the last check before a launch)


def test_workspace_size():
    _, lib = _lib()
    ws = lib.saev_coactivation_workspace_bytes
    base = (1000, 64, 48, 8000, 7000)
    assert ws(*base) > 0 and ws(*base) % 256 == 0
    grow = [(10**6, 64, 48, 8000, 7000), (1000, 4096, 48, 8000, 7000), (1000, 64, 40000, 8000, 7000), (1000, 64, 48, 10**7, 7000),
            (1000, 64, 48, 8000, 10**7)]
    for g in grow:
        assert ws(*g) >= ws(*base), g
    # monotone along every argument, through the points where the heavy bound and the number of counter rows change
    c, s = K.CHUNK_ROWS, K.SLOTS
    for i, values in enumerate([[1, 2, 10**6, 2**31 - 1], [1, 2, s - 1, s, s + 1, 10**6, 2**31 - 1], [1, 2, K.WINDOW - 1, K.WINDOW, K.WINDOW + 1, 2**20],
                                [0, 1, c, c + 1, 2 * (c + 1), s * (c + 1) - 1, s * (c + 1), (s + 1) * (c + 1), 2**31 - 1], [0, 1, 10**6, 2**31 - 1]]):
        big = [2**20, 2 * s, 1000, 2 * s * (c + 1), 1000]
        sizes = []
        for v in values:
            shape = list(big)
            shape[i] = v
            sizes.append(ws(*shape))
        assert all(x > 0 for x in sizes) and sizes == sorted(sizes), (i, sizes)
    # the event list and, with heavy latents possible, min(bound, slots) rows of Sb counters
    assert ws(10**6, 100, 200, c, 0) < ws(10**6, 100, 200, c + 1, 0)
    assert ws(2**20, 16384, 16384, 2**25, 2**25) >= 2**25 * 4 + s * 16384 * 4
    for bad in [(0, 1, 1, 0, 0), (1, 0, 1, 0, 0), (1, 1, 0, 0, 0), (-1, 1, 1, 0, 0), (1, 1, 1, -1, 0), (1, 1, 1, 0, -1), (1 << 31, 1, 1, 0, 0),
                (1, 1 << 31, 1, 0, 0), (1, 1, 1 << 31, 0, 0), (1, 1, 1, 1 << 31, 0), (1, 1, 1, 0, 1 << 31)]:
        assert ws(*bad) == -1, bad


# ---------------------------------------------------------------- the restatement ----------------------------------------------------


def _pair_counting(A, B, thr_a, thr_b, measure, top_m):
    """An independent route to the same answer: a loop over rows that counts pairs of firing latents in a dict, exact Fractions for
    the order."""
    from fractions import Fraction

    self_mode = B is None
    B = A if self_mode else B
    thr_b = thr_a if self_mode else thr_b
    n_a, n_b, pairs = np.zeros(A.shape[1], int), np.zeros(B.shape[1], int), {}
    for r in range(A.shape[0]):
        fa = [c for c, v in zip(A.indices[A.indptr[r]:A.indptr[r + 1]], A.data[A.indptr[r]:A.indptr[r + 1]]) if v > thr_a]
        fb = [c for c, v in zip(B.indices[B.indptr[r]:B.indptr[r + 1]], B.data[B.indptr[r]:B.indptr[r + 1]]) if v > thr_b]
        for c in fa:
            n_a[c] += 1
        for c in fb:
            n_b[c] += 1
        for p in itertools.product(fa, fb):
            pairs[p] = pairs.get(p, 0) + 1
    index, inter = np.full((A.shape[1], top_m), -1), np.zeros((A.shape[1], top_m), int)
    for a in range(A.shape[1]):
        cands = [(b, i) for (x, b), i in pairs.items() if x == a and not (self_mode and b == a)]
        if measure == "jaccard":
            key = lambda bi: (-Fraction(int(bi[1]), int(n_a[a] + n_b[bi[0]] - bi[1])), bi[0])  # noqa: E731
        else:
            key = lambda bi: (-bi[1], n_b[bi[0]], bi[0])  # noqa: E731
        for r, (b, i) in enumerate(sorted(cands, key=key)[:top_m]):
            index[a, r], inter[a, r] = b, i
    return index, inter, n_a, n_b


@pytest.mark.parametrize("measure", ["jaccard", "containment"])
@pytest.mark.parametrize("self_mode", [False, True])
def test_restatement_equals_pair_counting(measure, self_mode):
    rng = np.random.default_rng(4)
    vals = [-1.0, 0.0, 0.5, 1.0, 2.0]
    ties = 0
    for trial in range(6):
        # few rows and many latents: supports of 1-4 rows, so equal fractions with different numerators abound
        n, sa, sb = (12, 30, 40) if trial % 2 else (60, 20, 25)
        A = K.random_csr(rng, n, sa, rng.integers(0, 8, n), vals)
        B = None if self_mode else K.random_csr(rng, n, sb, rng.integers(0, 9, n), vals)
        thr_a, thr_b = [(0.0, 0.0), (0.5, -1.0), (-1.0, 0.5)][trial % 3]
        got = R.match(A, B, thr_a=thr_a, thr_b=thr_b, measure=measure, top_m=4)
        index, inter, n_a, n_b = _pair_counting(A, B, thr_a, thr_b, measure, 4)
        K._eq(got["index"], index)
        K._eq(got["intersection"], inter)
        K._eq(got["support_a"], n_a)
        K._eq(got["support_b"], n_b)
        value = got[measure]
        ties += int((value[:, :-1] == value[:, 1:]).sum())
    assert ties > 0  # some latent had two partners of equal value: the tie rules were used


def test_order_on_integers_near_the_64_bit_edge():
    """I < 2^31 and U < 2^32: the cross-products reach 2^63 and differ in their last units, where float64 cannot tell them apart."""
    top_i, top_u = 2**31 - 1, 2**32 - 1
    n_a = 2**31 - 1
    # b1: I = 2^31 - 1, n_b = 2^31 - 1 -> U = n_a (Jaccard 1);  b2: I = 2^31 - 2, n_b = 2^31 - 2 -> U = 2^31 - 1
    assert R.before("jaccard", n_a, top_i, top_i, 5, top_i - 1, top_i - 1, 3)
    # neighbouring fractions p/q and (p - 1)/(q - 1) with q = 2^32 - 1: equal in float64, ordered on integers
    i1, u1, i2, u2 = top_i, top_u, top_i - 1, top_u - 1
    nb1, nb2 = u1 - n_a + i1, u2 - n_a + i2
    assert i1 * u2 != i2 * u1 and i1 * u2 >= 2**62
    assert R.before("jaccard", n_a, i1, nb1, 9, i2, nb2, 1) == (i1 * u2 > i2 * u1)
    assert R.before("jaccard", n_a, i2, nb2, 1, i1, nb1, 9) == (i2 * u1 > i1 * u2)
    # exact ties: 1/2 against 2/4, and scaled up to the edge (2^30 / 2^31 against (2^30 - 1) / (2^31 - 2)): the index decides
    assert R.before("jaccard", 2, 2, 4, 3, 1, 1, 7) and not R.before("jaccard", 2, 1, 1, 7, 2, 4, 3)
    na = 2**30
    assert R.before("jaccard", na, 2**30, 2**31, 1, 2**30 - 1, 2**31 - 3, 2) and R.before("jaccard", na, 2**30 - 1, 2**31 - 3, 1, 2**30, 2**31, 2)
    # containment: I, then the smaller n_b, then the index
    assert R.before("containment", 10, 3, 99, 9, 2, 2, 0) and R.before("containment", 10, 3, 4, 9, 3, 5, 0) and R.before("containment", 10, 3, 4, 1, 3, 4, 2)
    assert [b for _, _, b in R.rank("containment", 4, [(2, 5, 1), (2, 3, 6), (1, 1, 2), (2, 3, 4)])] == [4, 6, 1, 2]


CASES = K.all_cases()


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_every_case_has_its_property(case):
    expected = R.match(case.A, case.B, **case.settings)
    case.holds(expected)
    sa = case.A.shape[1]
    sb = sa if case.B is None else case.B.shape[1]
    assert expected["index"].shape == (sa, case.top_m) and expected["index"].max() < sb and len(expected["support_b"]) == sb
    for m in (case.A,) if case.B is None else (case.A, case.B):
        assert m.has_canonical_format or R.firing(m, -np.inf).data.max() == 1  # canonical rows


def test_cases_cover_the_listed_ground():
    names = {c.name for c in CASES}
    assert len(names) == len(CASES)
    for w, tag in ((K.WINDOW, "window"), (K.SMALL_WINDOW, "small_window"), (K.MID_WINDOW, "mid_window")):
        assert {f"{tag}_sb_{w - 1}", f"{tag}_sb_{w}", f"{tag}_sb_{w + 1}"} <= names
    heavy = next(c for c in CASES if c.name == "heavy_lists")
    lens = sorted(np.diff(scipy.sparse.csc_matrix(heavy.A).indptr).tolist())
    c = K.CHUNK_ROWS
    assert {c - 1, c, c + 1, 3 * c + 5} <= set(lens)
    assert next(x for x in CASES if x.name == "many_heavy").A.shape[1] > K.SLOTS
    assert {c.top_m for c in CASES} >= {1, 3, 8} and {c.measure for c in CASES} == {"jaccard", "containment"}
    lens = np.diff(next(x for x in CASES if x.name == "row_lengths").A.indptr)
    assert {0, 1, 63, 64, 65, 300} <= set(lens.tolist())


# ---------------------------------------------------------------- alignment ----------------------------------------------------------


def _expected_arrays(A, B, **settings):
    from saev_amd import alignment

    e = R.match(A, B, **settings)
    return e, alignment.arrays_of(e["index"], e["intersection"], e["support_a"], e["support_b"], e["reverse_index"])


def test_alignment_arrays_keys_and_dtypes(tmp_path):
    from saev_amd import alignment

    rng = np.random.default_rng(8)
    A, B = K.random_csr(rng, 200, 24, 5), K.random_csr(rng, 200, 32, 4)
    for b in (B, None):
        e, z = _expected_arrays(A, b, top_m=3)
        assert tuple(z) == alignment.KEYS
        sb = 24 if b is None else 32
        want = dict(partner=(np.int32, (24, 3)), intersection=(np.int32, (24, 3)), jaccard=(np.float64, (24, 3)), support_a=(np.int32, (24,)),
                    support_b=(np.int32, (sb,)), mutual=(np.bool_, (24,)), reverse_partner=(np.int32, (sb,)))
        for k, (dt, shape) in want.items():
            assert z[k].dtype == dt and z[k].shape == shape, k
        K._eq(z["partner"], e["index"])
        assert np.array_equal(z["jaccard"], e["jaccard"], equal_nan=True) and np.array_equal(z["mutual"], e["mutual"])
        np.savez(tmp_path / "a.npz", **z)
        with np.load(tmp_path / "a.npz") as back:
            assert set(back.files) == set(alignment.KEYS)


def test_alignment_file_name():
    import pathlib

    from saev_amd import alignment

    cfg = alignment.Config(run_a=pathlib.Path("/r/abc"), run_b=pathlib.Path("/r/xyz"), shards="/data/shards/1a2b")
    assert alignment.alignment_fpath(cfg) == pathlib.Path("/r/abc/inference/1a2b/latent_alignment__xyz.npz")
    assert alignment.alignment_fpath(alignment.Config(run_a=pathlib.Path("/r/abc"), shards="1a2b")).name == "latent_alignment__self.npz"
    assert [f.name for f in __import__("dataclasses").fields(alignment.Config)] == ["run_a", "run_b", "shards", "level", "tokens_per_image", "top_k", "threshold",
                                                                                   "measure", "top_m", "device"]


def test_robustness_counts_mutual_partners_above_the_floor(tmp_path):
    from saev_amd import alignment

    rng = np.random.default_rng(12)
    A = K.random_csr(rng, 300, 16, 4)
    paths, hits = [], np.zeros(16, dtype=np.int64)
    for r in range(4):
        # run r: a permutation of A's latents, each with its own share (0 - 60 %) of its rows dropped -> mutual, Jaccard 0.4 - 1
        Bm = A.toarray()[:, rng.permutation(16)]
        Bm[rng.random(Bm.shape) < rng.uniform(0.0, 0.6, size=16)[None, :]] = 0
        e, z = _expected_arrays(A, scipy.sparse.csr_matrix(Bm, dtype=np.float32))
        np.savez(tmp_path / f"latent_alignment__run{r}.npz", **z)
        paths.append(tmp_path / f"latent_alignment__run{r}.npz")
        with np.errstate(invalid="ignore"):
            hits += e["mutual"] & (e["jaccard"][:, 0] >= 0.7)
    got = alignment.robustness(paths, min_jaccard=0.7)
    assert got.dtype == np.int32 and np.array_equal(got, hits) and got.max() > got.min()
    assert np.array_equal(alignment.robustness(paths[:1], min_jaccard=0.0), np.load(paths[0])["mutual"].astype(np.int32))
    with pytest.raises(ValueError, match="at least one"):
        alignment.robustness([])


def test_row_count_mismatch_names_both_files(tmp_path):
    from saev_amd import alignment

    rng = np.random.default_rng(2)
    for run, n in (("a", 64), ("b", 60)):
        d = tmp_path / run / "inference" / "shard0"
        d.mkdir(parents=True)
        scipy.sparse.save_npz(str(d / "token_acts.npz"), K.random_csr(rng, n, 8, 2))
    cfg = alignment.Config(run_a=tmp_path / "a", run_b=tmp_path / "b", shards="shard0")
    with pytest.raises(ValueError) as ei:
        alignment.worker_fn(cfg)
    msg = str(ei.value)
    assert str(tmp_path / "a") in msg and str(tmp_path / "b") in msg and "64" in msg and "60" in msg


def test_engine_refuses_before_a_device():
    import torch

    from saev_amd import engine

    z, e32, f32 = torch.zeros(2, dtype=torch.int64), torch.zeros(0, dtype=torch.int32), torch.zeros(0)
    A = (z, e32, f32)
    with pytest.raises(ValueError, match="measure"):
        engine.coactivation_match(A, n_rows=1, n_latents_a=1, measure="dice")
    with pytest.raises(ValueError, match="top_m"):
        engine.coactivation_match(A, n_rows=1, n_latents_a=1, top_m=9)
    with pytest.raises(ValueError, match="n_latents_b comes with B"):
        engine.coactivation_match(A, A, n_rows=1, n_latents_a=1)
    with pytest.raises(ValueError, match="n_latents_a"):
        engine.coactivation_match(A, n_rows=1, n_latents_a=0)
    with pytest.raises(ValueError, match="finite"):
        engine.coactivation_match(A, n_rows=1, n_latents_a=1, thr_a=float("nan"))
    with pytest.raises(RuntimeError, match="no CPU path"):
        engine.coactivation_match(A, n_rows=1, n_latents_a=1)
