"""CPU-only tests of the interventions (include/saev_amd.h: LATENT EDITS, CLASS FIRING COUNTS): the entries are
declared, exported and bound with the header's types and the ABI version stays; saev_edit's layout; every host-side refusal in
the stated order, with null pointers and without a device; EditSet's grouping; the restatement the GPU tests use against fixture
G30 (recorded from the reference's SparseAutoencoder) and against brute force; the report; the hook's slicing and write-back."""

import csv
import ctypes as C
import re
import subprocess

import numpy as np
import pytest
import torch

import interventions_restatement as IR
from conftest import ROOT

ENTRIES = ("saev_edit_plan_bytes", "saev_edit_plan_build", "saev_intervene_rows", "saev_class_fire_counts", "saev_class_fire_f1")
CTYPES = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64}
INVALID, UNSUPPORTED = -1, -3


def _lib():
    subprocess.run(["make", "-C", str(ROOT)], check=True, capture_output=True)
    from saev_amd import _lib

    return _lib, _lib.load()


def _ctype(decl: str, name: str, lib_mod):
    decl = decl.replace("const", "").strip()
    if "saev_edit" in decl:
        return C.POINTER(lib_mod.SaevEdit)
    if name == "thr_host":
        return C.POINTER(C.c_float)
    if "*" in decl:
        return C.c_void_p
    return CTYPES[decl.split()[0]]


def test_entries_are_declared_exported_and_bound_with_the_headers_types():
    lib_mod, lib = _lib()
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "saev_amd.h").read_text(), flags=re.S)
    for name in ENTRIES:
        m = re.search(r"(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, f"{name} is not declared"
        res = CTYPES[m.group(1)]
        args = []
        for a in m.group(2).split(","):
            a = a.strip()
            args.append(_ctype(re.sub(r"\w+\s*$", "", a), re.search(r"(\w+)\s*$", a).group(1), lib_mod))
        want_res, want_args = lib_mod._SIGNATURES[name]
        assert want_res is res, name
        assert list(want_args) == args, name
        assert hasattr(lib, name) and name in lib_mod.EXPORTED_SYMBOLS
    assert lib.saev_abi_version() == 12 and lib_mod.ABI_VERSION == 12  # additive entries: the version stays
    assert re.search(r"#define\s+SAEV_AMD_ABI_VERSION\s+12\b", text)
    for macro, value in (("SET", lib_mod.EDIT_SET), ("SCALE", lib_mod.EDIT_SCALE), ("ADD", lib_mod.EDIT_ADD), ("IF_ACTIVE", lib_mod.EDIT_IF_ACTIVE)):
        assert re.search(rf"#define\s+SAEV_EDIT_{macro}\s+{value}\b", text), macro
    assert (IR.SET, IR.SCALE, IR.ADD, IR.IF_ACTIVE) == (lib_mod.EDIT_SET, lib_mod.EDIT_SCALE, lib_mod.EDIT_ADD, lib_mod.EDIT_IF_ACTIVE)


def test_edit_layout_matches_header(tmp_path):
    lib_mod, _ = _lib()
    cls = lib_mod.SaevEdit
    fields = [f for f, _ in cls._fields_]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "saev_amd.h"', "int main(void) {", 'printf("size %zu\\n", sizeof(saev_edit));']
    src += [f'printf("{f} %zu\\n", offsetof(saev_edit, {f}));' for f in fields]
    src.append("return 0; }")
    (tmp_path / "layout.c").write_text("\n".join(src))
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True)
    want = dict(line.split() for line in subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.splitlines())
    assert C.sizeof(cls) == int(want["size"]) == 16
    for f in fields:
        assert getattr(cls, f).offset == int(want[f]), f


def _edits(lib_mod, recs):
    arr = (lib_mod.SaevEdit * max(len(recs), 1))()
    for i, r in enumerate(recs):
        arr[i] = lib_mod.SaevEdit(*r)
    return arr


def _refused(lib, rc, code, word):
    msg = (lib.saev_last_error(None) or b"").decode()
    assert rc == code and word in msg, (rc, msg)


def test_plan_build_refuses_in_the_stated_order():
    lib_mod, lib = _lib()
    fake = C.c_void_p(1 << 21)

    def build(recs, n_groups=0, S=100, n=None, plan=None, nbytes=0, arr=True):
        return lib.saev_edit_plan_build(_edits(lib_mod, recs) if arr else None, len(recs) if n is None else n, n_groups, S, plan, nbytes, None)

    ok = [(3, 0, 1.0, -1)]
    # 1. sizes -- before a bad latent is looked at
    bad_all = [(-5, 9, 1.0, 7)] * 300
    _refused(lib, build(bad_all, n=-1), INVALID, "negative")
    _refused(lib, build(bad_all, n_groups=-1), INVALID, "negative")
    _refused(lib, build(bad_all, S=-1), INVALID, "negative")
    _refused(lib, build(bad_all, n=65537), UNSUPPORTED, "65536")
    _refused(lib, build(bad_all, n_groups=65537), UNSUPPORTED, "65536")
    _refused(lib, build(bad_all, S=0), INVALID, "S must")
    _refused(lib, build(bad_all, S=1 << 31), INVALID, "S must")
    _refused(lib, build(ok, arr=False), INVALID, "NULL")
    # 2. latent before op, group, list length
    _refused(lib, build(bad_all), INVALID, "latent")
    _refused(lib, build([(100, 9, 1.0, 7)]), INVALID, "latent")
    # 3. op before group
    for op in (3, 7, 8, -1, 16):
        _refused(lib, build([(99, op, 1.0, 7)]), INVALID, "op")
    # 4. group before list length
    many = [(i, 0, 1.0, -1) for i in range(257)]
    _refused(lib, build(many + [(0, 0, 1.0, 0)], S=300), INVALID, "group")
    _refused(lib, build([(0, 0, 1.0, -2)], n_groups=3), INVALID, "group")
    _refused(lib, build([(0, 0, 1.0, 3)], n_groups=3), INVALID, "group")
    # 5. list length (global and a group's) before duplicates
    _refused(lib, build(many + [(0, 0, 1.0, -1)], S=300), UNSUPPORTED, "256")
    _refused(lib, build([(i % 7, 0, 1.0, 1) for i in range(257)], n_groups=2, S=300), UNSUPPORTED, "256")
    assert build([(i, 0, 1.0, -1) for i in range(256)] + [(i, 0, 1.0, 0) for i in range(256, 512)], n_groups=1, S=512) == 0
    # 6. duplicates: inside a list, and across the global list and a group's; two groups may share a latent
    _refused(lib, build([(4, 0, 1.0, -1), (5, 1, 2.0, -1), (4, 2, 1.0, -1)]), INVALID, "twice")
    _refused(lib, build([(4, 0, 1.0, 1), (4, 2, 1.0, 1)], n_groups=2), INVALID, "twice")
    _refused(lib, build([(4, 0, 1.0, -1), (4, 2, 1.0, 1)], n_groups=2), INVALID, "global list and in a group")
    assert build([(4, 0, 1.0, 0), (4, 2, 1.0, 1)], n_groups=2) == 0
    # 7. the plan: NULL with 0 bytes validates only; anything else must be large enough and aligned -- all before the device
    need = lib.saev_edit_plan_bytes(1, 0)
    assert need > 0 and need % 256 == 0
    assert build(ok) == 0 and build([]) == 0
    _refused(lib, build(ok, plan=None, nbytes=need), INVALID, "plan smaller")
    _refused(lib, build(ok, plan=fake, nbytes=need - 1), INVALID, "plan smaller")
    _refused(lib, build(ok, plan=C.c_void_p((1 << 21) + 16), nbytes=need), INVALID, "aligned")
    for e, g in ((-1, 0), (0, -1), (65537, 0), (0, 65537)):
        assert lib.saev_edit_plan_bytes(e, g) == -1
    assert lib.saev_edit_plan_bytes(65536, 65536) >= 16 * 65536 + 4 * 65538


def test_intervene_rows_refuses_before_the_device():
    _, lib = _lib()
    f = [C.c_void_p((1 << 21) + (1 << 16) * i) for i in range(8)]

    def call(n=4, D=8, S=16, cap=2, E=1, G=0, x=f[0], W=f[1], idx=f[2], val=f[3], plan=f[4], out=f[5]):
        return lib.saev_intervene_rows(x, n, D, W, S, idx, val, None, cap, plan, E, G, None, None, out, None, None)

    _refused(lib, call(n=-1), INVALID, "negative")
    _refused(lib, call(D=1 << 31), UNSUPPORTED, "2^31")
    _refused(lib, call(E=65537), UNSUPPORTED, "65536")
    _refused(lib, call(D=0), INVALID, "at least 1")
    assert call(n=0, x=None, W=None, out=None) == 0
    _refused(lib, call(x=None), INVALID, "NULL")
    _refused(lib, call(plan=None), INVALID, "plan")
    _refused(lib, call(idx=None), INVALID, "idx or val")
    _refused(lib, call(out=C.c_void_p(f[0].value + 16)), INVALID, "overlaps x")
    _refused(lib, call(out=C.c_void_p(f[1].value + 64)), INVALID, "overlaps W_dec")
    _refused(lib, call(out=C.c_void_p(f[3].value)), INVALID, "overlaps W_dec or the codes")


def test_class_fire_entries_refuse_in_the_stated_order():
    _, lib = _lib()
    f = [C.c_void_p((1 << 21) + (1 << 16) * i) for i in range(8)]

    def thr(*v):
        return (C.c_float * max(len(v), 1))(*v)

    def counts(cap=2, n=4, S=16, Cc=3, t=thr(0.0, 0.5), T=2, hist=f[4], label=f[3]):
        return lib.saev_class_fire_counts(f[0], f[1], None, cap, n, label, None, S, Cc, t, T, hist, f[5], f[6], None)

    def f1(S=16, Cc=3, T=2, hist=f[4], out=f[0]):
        return lib.saev_class_fire_f1(hist, f[5], f[6], S, Cc, T, None, out, f[1], None)

    _refused(lib, counts(n=-1, S=1 << 31), INVALID, "negative")
    _refused(lib, counts(S=-1, Cc=0), INVALID, "negative")
    _refused(lib, counts(S=1 << 31, Cc=0), UNSUPPORTED, "S must stay below")
    _refused(lib, counts(S=0, Cc=0), INVALID, "at least 1")
    _refused(lib, counts(Cc=0, T=9), UNSUPPORTED, "classes")
    _refused(lib, counts(Cc=4097, T=9), UNSUPPORTED, "classes")
    _refused(lib, counts(T=0, n=1 << 31), UNSUPPORTED, "thresholds")
    _refused(lib, counts(T=9, n=1 << 31), UNSUPPORTED, "thresholds")
    _refused(lib, counts(n=1 << 31, t=None), UNSUPPORTED, "below 2^31")
    _refused(lib, counts(n=1 << 20, cap=1 << 12, t=None), UNSUPPORTED, "below 2^31")
    _refused(lib, counts(t=None, S=1 << 30), INVALID, "thr is NULL")
    for bad in (thr(-0.5, 1.0), thr(0.5, 0.5), thr(1.0, 0.5), thr(0.0, float("nan"))):
        _refused(lib, counts(t=bad, S=1 << 30), INVALID, "ascending")
    _refused(lib, counts(S=1 << 30, hist=None), UNSUPPORTED, "C * T * S")
    _refused(lib, counts(hist=None), INVALID, "NULL")
    assert counts(n=0, label=None) == 0
    _refused(lib, counts(label=None), INVALID, "label")
    assert (3 * 2 * ((1 << 31) // 6 + 1)) >= 1 << 31
    _refused(lib, counts(S=(1 << 31) // 6 + 1), UNSUPPORTED, "C * T * S")
    _refused(lib, f1(S=-1), INVALID, "negative")
    _refused(lib, f1(Cc=0), UNSUPPORTED, "classes")
    _refused(lib, f1(T=9), UNSUPPORTED, "thresholds")
    _refused(lib, f1(S=1 << 30, hist=None), UNSUPPORTED, "C * T * S")
    _refused(lib, f1(hist=None), INVALID, "NULL")
    _refused(lib, f1(out=None), INVALID, "NULL")


def test_edit_set_groups_and_validates_without_a_device():
    _lib()
    from saev_amd import interventions as IV

    edits = [IV.Edit(5, "set", 1.0, group=1), IV.Edit(2, "scale", 0.0), IV.Edit(7, "add", -1.0, group=0, if_active=True), IV.Edit(9, group=1),
             IV.Edit(1, "set", 3.0)]
    es = IV.EditSet(edits, d_sae=16, n_groups=3)
    assert len(es) == 5 and es.lists == [[1, 4], [2], [0, 3], []]
    assert es.records[2] == (7, IR.ADD | IR.IF_ACTIVE, -1.0, 0) and es.records[1] == (2, IR.SCALE, 0.0, -1)
    with pytest.raises(ValueError, match="latent"):
        IV.EditSet([IV.Edit(16)], d_sae=16)
    with pytest.raises(ValueError, match="group"):
        IV.EditSet([IV.Edit(3, group=0)], d_sae=16)
    with pytest.raises(ValueError, match="twice"):
        IV.EditSet([IV.Edit(3), IV.Edit(3, "add", 1.0)], d_sae=16)
    with pytest.raises(ValueError, match="op"):
        IV.EditSet([IV.Edit(3, "clamp")], d_sae=16)
    assert IV.EditSet([], d_sae=16).lists == [[]]


@pytest.mark.parametrize("kind", ["topk", "relu"])
def test_restatement_matches_the_reference_on_g30(kind):
    g = IR.g30_case(kind)
    assert g["x"].shape == (48, 32) and g["W_dec"].shape == (128, 32)
    assert ((g["labels"] < 0) | (g["labels"] >= g["n_groups"])).sum() >= 2 and len(g["edits"]) == 1 + g["n_groups"]
    r = IR.intervene(g["x"], g["W_dec"], g["idx"], g["val"], g["row_nnz"], g["edits"], g["n_groups"], row_group=g["labels"])
    err = np.abs(g["out_ref"].astype(np.float64) - r["out"])
    assert (err <= g["bound_ref"]).all(), (err / g["bound_ref"]).max()
    assert r["rows_changed"][0] >= 40 and (r["rows_changed"][1:] > 0).all()  # the global SET and every class's
    assert (r["m"] >= 1).all() and r["m"].max() == 2


def test_coefficients_reproduce_fp32():
    f32 = np.float32
    assert IR.coefficient(f32(1.5), IR.SET, f32(1.5)) is None and IR.coefficient(f32(3.0), IR.SCALE, f32(1.0)) is None
    assert IR.coefficient(f32(0), IR.SET | IR.IF_ACTIVE, f32(2)) is None and IR.coefficient(f32(0), IR.ADD, f32(0)) is None
    assert IR.coefficient(f32(0.1), IR.SET, f32(0.3)) == f32(0.3) - f32(0.1)
    assert IR.coefficient(f32(7), IR.ADD | IR.IF_ACTIVE, f32(-2)) == f32(-2)
    # fmaf(v, f, -f) rounds once: a case where rounding the product first gives another float
    v, f = f32(1 + 2.0 ** -12), f32(1 + 2.0 ** -12)
    exact = float(v) * float(f) - float(f)  # exact in fp64: 2^-12 + 2^-24
    assert IR.coefficient(f, IR.SCALE, v) == f32(exact) != f32(f32(v * f) - f)
    assert IR.round_f32(__import__("fractions").Fraction(1) + __import__("fractions").Fraction(1, 2 ** 24)) == f32(1)  # tie to even


def test_fire_counts_restatement_against_brute_force():
    rng = np.random.default_rng(7)
    n, S, C_, thr = 60, 23, 4, np.array([0.0, 0.1, 0.3, 1.0], dtype=np.float32)
    f = np.where(rng.random((n, S)) < 0.3, rng.choice(np.array([0.05, 0.1, 0.2, 0.3, 0.30000001, 1.0, 2.0, -1.0], dtype=np.float32), (n, S)), 0).astype(np.float32)
    labels = rng.integers(-1, C_ + 1, n)
    keep = rng.random(n) < 0.8
    idx, val, nnz = IR.codes_of(f)
    hist, pos, n_rows_c = IR.fire_counts(idx, val, nnz, labels, keep, S, C_, thr)
    TP, POS = IR.suffix(hist, pos)
    TPd, POSd, nd = IR.fire_counts_dense(f, labels, keep, C_, thr)
    assert (TP == TPd).all() and (POS == POSd).all() and (n_rows_c == nd).all() and n_rows_c.sum() < n
    f1, best_t = IR.f1_from_counts(TP, POS, n_rows_c, mask=np.arange(S) % 5 != 0)
    assert f1.dtype == np.float32 and (f1[:, ::5] == -1).all() and (f1[:, 1] >= 0).all() and f1.max() <= 1
    # against the textbook formula in fp64, and the tie rule
    c, s = 1, 3
    t = int(best_t[c, s])
    tp, ps = TP[c, :, s], POS[:, s]
    ref = 2 * tp / np.maximum(2 * tp + (ps - tp) + (n_rows_c[c] - tp), 1e-10)
    assert abs(float(f1[c, s]) - ref.max()) < 1e-6 and t == int(np.argmax(ref >= ref.max() - 1e-9))


def test_class_results_match_the_definition_and_the_report(tmp_path):
    _lib()
    from saev_amd import interventions as IV

    g = torch.Generator().manual_seed(3)
    orig = torch.randint(1, 9, (5, 16), generator=g)
    mod = torch.where(torch.rand(5, 16, generator=g) < 0.4, torch.randint(1, 12, (5, 16), generator=g), orig)
    classes = range(1, 10)
    got = IV.compute_class_results(orig, mod, classes)
    want = IR.triple_loop(orig, mod, list(classes))
    assert [(r.class_id, r.n_orig_patches, r.n_changed_patches, r.n_other_patches, r.n_other_changed, r.change_distribution) for r in got] == want
    assert len(IV.compute_class_results(orig, mod)) == 150  # the reference's classes
    rep = IV.Report(method="automatic-feature", class_results=got, intervention_scale=-2.0)
    tot = sum(w[1] for w in want)
    assert rep.mean_target_change == sum(w[2] for w in want) / tot
    assert rep.mean_other_change == sum(w[4] for w in want) / sum(w[3] for w in want)
    assert rep.target_change_std == float(np.std([w[2] / w[1] if w[1] else 0.0 for w in want]))
    assert rep.other_change_std == float(np.std([w[4] / w[3] if w[3] else 0.0 for w in want]))
    empty = IV.Report("none", [], 0.0)
    assert empty.mean_target_change == 0.0 and empty.mean_other_change == 0.0
    IV.save([rep, rep], str(tmp_path / "sub" / "results.csv"))
    rows = list(csv.reader(open(tmp_path / "sub" / "results.csv")))
    assert rows[0] == ["method", "target_change", "target_std", "other_change", "other_std"] and len(rows) == 3
    assert rows[1][0] == "automatic-feature" and float(rows[1][1]) == rep.mean_target_change and float(rows[1][4]) == rep.other_change_std
    assert IV.unscaled(-2.0, 3.0) == -6.0 and IV.map_range(5, (0, 10), (0, 1)) == 0.5
    with pytest.raises(ValueError):
        IV.map_range(11, (0, 10), (0, 1))
    logits = torch.tensor([[[9.0, 1.0, 3.0, 2.0], [9.0, 5.0, 3.0, 2.0]]])
    assert IV.argmax_logits(logits).tolist() == [[2, 1]]


@pytest.mark.parametrize("tokens", [slice(1, None), slice(None)])
def test_hook_slices_and_writes_back(monkeypatch, tokens):
    _lib()
    from saev_amd import interventions as IV

    seen = {}

    def stub(sae, x, edits, *, row_group=None, row_keep=None, out=None, return_counts=False):
        assert x.is_contiguous() and x.ndim == 2 and out is not None and out.data_ptr() == x.data_ptr()
        seen["x"], seen["row_group"], seen["edits"] = x.clone(), row_group, edits
        out.mul_(2.0)
        return out

    monkeypatch.setattr(IV, "intervene", stub)
    b, t, d = 3, 5, 4
    n_sel = len(range(t)[tokens])
    groups = torch.arange(b * n_sel).reshape(b, n_sel)
    hook = IV.make_hook("sae", "edits", tokens=tokens, row_group=lambda: groups)
    output = torch.arange(b * t * d, dtype=torch.float32).reshape(b, t, d)
    before = output.clone()
    ptr = output.data_ptr()
    res = hook(None, (), output)
    assert res is output and output.data_ptr() == ptr
    assert torch.equal(seen["x"], before[:, tokens, :].reshape(-1, d)) and seen["edits"] == "edits"
    assert torch.equal(seen["row_group"], groups.reshape(-1))
    want = before.clone()
    want[:, tokens, :] *= 2.0
    assert torch.equal(output, want)
    if tokens == slice(1, None):
        assert torch.equal(output[:, 0], before[:, 0])  # CLS untouched


def test_random_vector_hook_adds_scaled_unit_vectors():
    _lib()
    from saev_amd import interventions as IV

    out = torch.zeros(2, 5, 16)
    IV.random_vector_hook(3.0, seed=1)(None, (), out)
    assert torch.equal(out[:, 0], torch.zeros(2, 16))
    torch.testing.assert_close(out[:, 1:].norm(dim=-1), torch.full((2, 4), 3.0))
    again = torch.zeros(2, 5, 16)
    IV.random_vector_hook(3.0, seed=1)(None, (), again)
    assert torch.equal(out, again)


def test_batch_topk_in_training_mode_is_refused():
    _lib()
    from saev_amd import interventions as IV
    from saev_amd.nn import modeling

    sae = modeling.SparseAutoencoder(modeling.SparseAutoencoderConfig(d_model=8, d_sae=32, activation=modeling.BatchTopK(top_k=4)))
    sae.train()
    with pytest.raises(RuntimeError, match="training mode"):
        IV.intervene(sae, torch.zeros(3, 8), [IV.Edit(1, "set", 1.0)])
    with pytest.raises(RuntimeError, match="training mode"):
        sae.intervene(torch.zeros(3, 8), [IV.Edit(1, "set", 1.0)])
    sae.eval()
    with pytest.raises(RuntimeError, match="HIP device"):  # past the mode check: the package has no CPU path
        sae.intervene(torch.zeros(3, 8), [IV.Edit(1, "set", 1.0)])
