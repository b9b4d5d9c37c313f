"""GPU tests of the interventions (include/saev_amd.h: LATENT EDITS, CLASS FIRING COUNTS) at the smallest shapes
where the kernels can go wrong.

The edit kernel against the fp64 restatement (tests/interventions_restatement.py), whose coefficients reproduce the kernel's fp32
values.  Tolerance, from the fmaf chain out = fmaf(c_m, W_m, ... fmaf(c_1, W_1, x)): m roundings, each relative u = 2^-24 of a
partial sum bounded by |x_d| + sum |c_e| |W_l_e,d|, so |error| <= gamma_m * that; the test uses gamma_{m+1} (the restatement's own
fp64 evaluation is far inside the extra link) plus m 2^-149 for links that round in the subnormal range.  Rows without a remaining
edit, in-place against out-of-place, and two calls are compared on the bits; rows_changed and the firing counts on the integers;
f1 on the float32 bits."""

import numpy as np
import pytest
import torch

import interventions_restatement as IR

pytestmark = [pytest.mark.gpu, pytest.mark.encoder_modes("f32")]

ROWS_PER_WG = 4  # one wave per row, four waves a workgroup (saev_amd/csrc/intervene.hip: IV_WAVES)


def _dev(a, dtype=None):
    return None if a is None else torch.as_tensor(np.asarray(a), dtype=dtype).cuda()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check_edit(x, W, idx, val, row_nnz, edits, n_groups, row_group=None, row_keep=None, expected=None):
    """Runs the kernel out of place, in place, once more and into a buffer of NaNs; compares with the restatement (``expected`` when
    the caller has it already); returns the restatement."""
    from saev_amd import engine

    S = W.shape[0]
    xd, Wd, idxd, vald = _dev(x), _dev(W), _dev(idx, torch.int32), _dev(val)
    nnzd, rgd, rkd = _dev(row_nnz, torch.int32), _dev(row_group, torch.int32), _dev(row_keep, torch.bool)
    plan = engine.build_edit_plan(edits, S, n_groups, "cuda")

    def run(out=None, src=xd):
        counts = torch.zeros(len(edits), device="cuda", dtype=torch.int64)
        res = engine.intervene_rows(src, Wd, idxd, vald, nnzd, plan, len(edits), n_groups, row_group=rgd, row_keep=rkd, out=out,
                                    rows_changed=counts)
        return res.cpu().numpy(), counts.cpu().numpy()

    got, counts = run()
    r = expected if expected is not None else IR.intervene(x, W, idx, val, row_nnz, edits, n_groups, row_group=row_group, row_keep=row_keep)
    untouched = r["m"] == 0
    assert (_bits(got[untouched]) == _bits(x[untouched])).all(), "a row without a remaining edit must come back on the bits"
    tol = IR.tolerance(r["mag"], r["m"])
    t = ~untouched
    err = np.abs(got[t].astype(np.float64) - r["out"][t])
    assert np.isfinite(got[t]).all() and (err <= tol[t]).all(), float((err / np.maximum(tol[t], 1e-300)).max())
    assert (counts == r["rows_changed"]).all(), (counts, r["rows_changed"])
    x2 = xd.clone()
    inplace, counts2 = run(out=x2, src=x2)
    assert (_bits(inplace) == _bits(got)).all() and (counts2 == counts).all(), "in place differs from out of place"
    again, _ = run()
    assert (_bits(again) == _bits(got)).all(), "two calls differ"
    given, _ = run(out=torch.full_like(xd, float("nan")))  # an element the kernel does not write stays NaN
    assert (_bits(given) == _bits(got)).all(), "an output buffer passed in differs from one allocated by the call"
    return r


def make_codes(rng, n, S, cap, nnz=None):
    """Distinct latents per row in random order; every slot filled (the slots past row_nnz hold latents too: they must be ignored)."""
    idx = np.stack([rng.permutation(S)[:cap] for _ in range(n)]).astype(np.int32) if cap <= S else None
    val = rng.uniform(0.25, 2.0, (n, cap)).astype(np.float32)
    if nnz is None:
        nnz = rng.integers(0, cap + 3, n).astype(np.int32)  # ragged: 0, full, and above the capacity
    return idx, val, nnz


def put(idx, val, b, slot, latent, value):
    """Latent at a slot of row b; wherever else the row held it gets another latent that no edit names."""
    other = idx[b] == latent
    idx[b, other] = FREE
    idx[b, slot], val[b, slot] = latent, value


FREE = 39  # a latent no test edits (S >= 40 everywhere below)


@pytest.mark.parametrize("D", [1, 3, 4, 7, 252, 256, 260, 516])
def test_every_width_and_row_count(D):
    """Scalar path (D % 4 != 0), less than one float4 trip of a wave (D = 252: 63 lanes), exactly one (256), one past it (260), two
    and one lane (516); n = 1 and rows per workgroup +- 1; all three ops, IF_ACTIVE on present and absent latents, latents 0 and
    S - 1, global and group lists together, row_group -1 / n_groups - 1 / n_groups, row_keep."""
    rng = np.random.default_rng(D)
    S, cap, G = 48, 5, 2
    edits = [(0, IR.SET, 1.5, -1), (S - 1, IR.SCALE, -0.5, -1), (7, IR.ADD | IR.IF_ACTIVE, 0.75, -1),
             (3, IR.SET | IR.IF_ACTIVE, -2.0, 0), (5, IR.ADD, 0.125, 1), (9, IR.SCALE | IR.IF_ACTIVE, 3.0, 1)]
    W = rng.standard_normal((S, D)).astype(np.float32)
    for n in (1, ROWS_PER_WG - 1, ROWS_PER_WG + 1, 11):
        x = rng.standard_normal((n, D)).astype(np.float32)
        idx, val, nnz = make_codes(rng, n, S, cap)
        for b in range(n):  # edited latents present in some rows, absent in others
            for j, lat in enumerate((0, S - 1, 7, 3, 9)):
                if rng.random() < 0.5:
                    put(idx, val, b, j, lat, np.float32(rng.uniform(0.5, 2.0)))
        row_group = rng.choice(np.array([-1, 0, G - 1, G], dtype=np.int32), n)
        row_keep = rng.random(n) < 0.8
        if n == 11:  # one row that is not kept, one with every edited latent present and a group list
            row_keep[0], row_keep[1], row_group[1], nnz[1] = False, True, G - 1, cap
            for j, lat in enumerate((0, S - 1, 7, 3, 9)):
                put(idx, val, 1, j, lat, np.float32(0.5 + j))
        r = check_edit(x, W, idx, val, nnz, edits, G, row_group=row_group, row_keep=row_keep)
        if n == 11:
            assert r["m"][1] == 5 and r["m"][0] == 0
    # no group vector, no keep vector, full rows (the TopK form)
    check_edit(x, W, idx, val, None, edits, G)


@pytest.mark.parametrize("cap", [1, 32, 63, 64, 65, 200])
def test_every_row_capacity_and_slot(cap):
    """The edited latent in the first slot, the last slot, slot 64 (the first of the second 64-slot search), past row_nnz, twice
    (the first match counts) and absent; ragged row_nnz with 0 and values above the capacity."""
    rng = np.random.default_rng(cap)
    S, D = 256, 8
    L = 0
    edits = [(L, IR.SET, 2.0, -1), (S - 1, IR.SCALE | IR.IF_ACTIVE, 3.0, -1), (17, IR.ADD | IR.IF_ACTIVE, 1.0, -1)]
    W = rng.standard_normal((S, D)).astype(np.float32)
    n = 8
    x = rng.standard_normal((n, D)).astype(np.float32)
    idx, val, _ = make_codes(rng, n, S, cap)
    for b in range(n):
        for lat in (L, S - 1, 17):
            idx[b, idx[b] == lat] = FREE
    nnz = np.full(n, cap, dtype=np.int32)
    put(idx, val, 0, 0, L, 0.5)
    put(idx, val, 1, cap - 1, S - 1, 0.75)
    put(idx, val, 2, min(64, cap - 1), 17, 1.25)
    put(idx, val, 2, cap // 2, L, 0.375) if cap > 2 else None
    nnz[3] = cap // 2
    put(idx, val, 3, cap - 1, S - 1, 9.0) if cap > 1 else None  # past row_nnz: absent
    if cap >= 4:
        idx[4, 1], val[4, 1] = S - 1, 0.5
        idx[4, 3], val[4, 3] = S - 1, 8.0  # a second slot with the same latent: ignored
    nnz[5] = 0
    put(idx, val, 5, 0, L, 4.0)
    nnz[6] = cap + 7  # reads as the capacity
    put(idx, val, 6, cap - 1, 17, 0.625)
    nnz[7] = -3  # reads as 0
    r = check_edit(x, W, idx, val, nnz, edits, 0)
    assert r["coef"][0][0] == (L, np.float32(1.5)) and r["coef"][5][0] == (L, np.float32(2.0))
    assert (S - 1, np.float32(1.5)) in r["coef"][1] and (17, np.float32(1.0)) in r["coef"][6]
    if cap > 1:
        assert all(lat != S - 1 for lat, _ in r["coef"][3])
    if cap >= 4:
        assert (S - 1, np.float32(1.0)) in r["coef"][4]


@pytest.mark.parametrize("n_list", [0, 1, 2, 17, 256])
@pytest.mark.parametrize("mode", ["global", "group", "both"])
def test_every_list_length(n_list, mode):
    rng = np.random.default_rng(n_list)
    S, D, cap, n, G = 600, 12, 8, 7, 3
    lat = rng.permutation(np.arange(40, S))
    edits = []
    if mode in ("global", "both"):
        edits += [(int(l), int(rng.integers(0, 3)), float(rng.uniform(0.5, 1.5)), -1) for l in lat[:n_list]]
    if mode in ("group", "both"):
        edits += [(int(l), int(rng.integers(0, 3)), float(rng.uniform(0.5, 1.5)), 1) for l in lat[n_list:2 * n_list]]
        edits += [(int(l), IR.ADD, 0.5, 2) for l in lat[:min(n_list, 2)] if mode == "group"]
    rng.shuffle(edits)
    W = (rng.standard_normal((S, D)) / 8).astype(np.float32)
    x = rng.standard_normal((n, D)).astype(np.float32)
    idx, val, nnz = make_codes(rng, n, S, cap)
    for b in range(n):
        if edits:
            put(idx, val, b, b % cap, edits[b % len(edits)][0], 1.0)
    row_group = np.array([1, 1, 0, 2, -1, G, 1], dtype=np.int32)
    r = check_edit(x, W, idx, val, nnz, edits, G, row_group=row_group)
    if n_list == 256 and mode == "both":
        assert r["m"].max() > 256  # a row takes the global list and its group's


def test_zero_coefficients_skip_the_decoder_row():
    """SCALE by 1 and SET to the present value give c = 0: the row comes back on the bits although W_dec[l] holds Inf and NaN, and
    so does IF_ACTIVE on an absent latent; rows_changed does not count them."""
    rng = np.random.default_rng(5)
    S, D, n, cap = 64, 260, 6, 4
    W = rng.standard_normal((S, D)).astype(np.float32)
    W[10], W[11], W[12] = np.inf, np.nan, -np.inf
    edits = [(10, IR.SCALE, 1.0, -1), (11, IR.SET, 0.625, -1), (12, IR.ADD | IR.IF_ACTIVE, 5.0, -1), (13, IR.ADD, 1.0, 0)]
    x = rng.standard_normal((n, D)).astype(np.float32)
    idx, val, _ = make_codes(rng, n, S, cap)
    for b in range(n):
        for lat in (10, 11, 12, 13):
            idx[b, idx[b] == lat] = FREE
        put(idx, val, b, 0, 10, 1.75)
        put(idx, val, b, 1, 11, 0.625)
    row_group = np.array([-1, 0, -1, 0, 1, -1], dtype=np.int32)
    r = check_edit(x, W, idx, val, None, edits, 1, row_group=row_group)
    assert r["m"].tolist() == [0, 1, 0, 1, 0, 0] and r["rows_changed"].tolist() == [0, 0, 0, 2]


@pytest.mark.parametrize("kind", ["topk", "relu"])
def test_g30_reference_output(kind):
    """The kernel on the reference's codes against the reference's recorded (x - x_hat) + decode(f_mod): within the reference's
    bound plus the kernel's own tolerance."""
    from saev_amd import engine

    g = IR.g30_case(kind)
    r = check_edit(g["x"], g["W_dec"], g["idx"], g["val"], g["row_nnz"], g["edits"], g["n_groups"], row_group=g["labels"])
    plan = engine.build_edit_plan(g["edits"], 128, g["n_groups"], "cuda")
    got = engine.intervene_rows(_dev(g["x"]), _dev(g["W_dec"]), _dev(g["idx"]), _dev(g["val"]), _dev(g["row_nnz"]), plan, len(g["edits"]),
                                g["n_groups"], row_group=_dev(g["labels"], torch.int32)).cpu().numpy()
    err = np.abs(got.astype(np.float64) - g["out_ref"].astype(np.float64))
    assert (err <= g["bound_ref"] + IR.tolerance(r["mag"], r["m"])).all()


def _module(kind: str):
    from saev_amd.nn import modeling

    act = {"topk": modeling.TopK(top_k=4), "relu": modeling.Relu(), "batch_topk": modeling.BatchTopK(top_k=4)}[kind]
    torch.manual_seed(11)
    sae = modeling.SparseAutoencoder(modeling.SparseAutoencoderConfig(d_model=32, d_sae=256, activation=act)).cuda().eval()
    with torch.no_grad():
        if kind == "relu":
            sae.b_enc.fill_(-1.0)
        if kind == "batch_topk":
            sae.activation.threshold.fill_(1.0)
    return sae


@pytest.mark.parametrize("kind", ["topk", "relu", "batch_topk"])
def test_module_intervene_against_the_restatement_on_its_own_codes(kind):
    from saev_amd import interventions as IV

    sae = _module(kind)
    x = torch.randn(3, 17, 32, generator=torch.Generator().manual_seed(12)).cuda()
    codes = sae.encode_sparse(x.reshape(-1, 32))
    idx, val = codes[0].cpu().numpy(), codes[1].cpu().numpy()
    nnz = codes[2].cpu().numpy() if len(codes) > 2 else None
    fired = np.bincount(idx[idx >= 0].ravel(), minlength=256) if nnz is None else np.bincount(
        np.concatenate([idx[b, :min(int(nnz[b]), idx.shape[1])] for b in range(len(idx))]), minlength=256)
    top = np.argsort(-fired)[:3]
    assert fired[top[0]] > 0
    edits = [IV.Edit(int(top[0]), "set", 4.0), IV.Edit(int(top[1]), "scale", 0.0, group=0, if_active=True), IV.Edit(int(top[2]), "add", -1.0, group=1)]
    row_group = torch.randint(-1, 3, (3, 17), generator=torch.Generator().manual_seed(13))
    row_keep = torch.rand(3, 17, generator=torch.Generator().manual_seed(14)) < 0.8
    out, counts = sae.intervene(x, edits, row_group=row_group, row_keep=row_keep, return_counts=True)
    assert out.shape == x.shape and out.data_ptr() != x.data_ptr()
    r = IR.intervene(x.reshape(-1, 32).cpu().numpy(), sae.W_dec.detach().cpu().numpy(), idx, val, nnz, [e.record() for e in edits], 2,
                     row_group=row_group.reshape(-1).numpy(), row_keep=row_keep.reshape(-1).numpy())
    got = out.reshape(-1, 32).cpu().numpy()
    err = np.abs(got.astype(np.float64) - r["out"])
    assert (err <= IR.tolerance(r["mag"], r["m"])).all() and (counts.cpu().numpy() == r["rows_changed"]).all()
    assert r["rows_changed"][0] > 0 and (_bits(got[r["m"] == 0]) == _bits(x.reshape(-1, 32).cpu().numpy()[r["m"] == 0])).all()
    x2 = x.clone()
    res = IV.intervene(sae, x2, IV.EditSet(edits, 256, 2), row_group=row_group, row_keep=row_keep, out=x2)
    assert res is x2 and torch.equal(x2, out)


# ---- class firing counts -----------------------------------------------------------------------------------------------------------

THRESHOLDS = {1: (0.0,), 4: (0.0, 0.1, 0.3, 1.0), 8: (0.0, 0.1, 0.2, 0.3, 0.5, 1.0, 2.0, 4.0)}


def _fire_case(rng, n, S, C_, cap, thr):
    thr32 = np.asarray(thr, dtype=np.float32)
    pool = np.concatenate([thr32, np.nextafter(thr32, np.float32(np.inf)), np.array([-1.0, 0.05, 7.0, np.nan], dtype=np.float32)])
    idx = np.stack([rng.permutation(S)[:cap] for _ in range(n)]).astype(np.int32)
    idx[rng.random((n, cap)) < 0.05] = -1  # padding
    val = rng.choice(pool, (n, cap)).astype(np.float32)
    nnz = rng.integers(0, cap + 2, n).astype(np.int32)
    labels = rng.integers(-1, C_ + 1, n).astype(np.int32)  # -1 and C are out of range
    labels[labels == C_ - 1] = 0  # the last class has no row: its denominators can be 0
    keep = rng.random(n) < 0.8
    return idx, val, nnz, labels, keep


def _check_f1(counts, hist, pos, n_rows_c, mask):
    TP, POS = IR.suffix(hist, pos)
    want, want_t = IR.f1_from_counts(TP, POS, n_rows_c, mask)
    f1, best_t = counts.f1(None if mask is None else torch.as_tensor(mask).cuda())
    assert (_bits(f1.cpu().numpy()) == _bits(want)).all() and (best_t.cpu().numpy() == want_t).all()
    return want, want_t


@pytest.mark.parametrize("T", [1, 4, 8])
@pytest.mark.parametrize("cap", [1, 5, 70])
def test_fire_counts_and_f1(T, cap):
    from saev_amd import engine

    rng = np.random.default_rng(100 * T + cap)
    n, S, C_ = 37, 70, 5
    thr = THRESHOLDS[T]
    idx, val, nnz, labels, keep = _fire_case(rng, n, S, C_, cap, thr)
    idx[idx == S - 1] = -1  # latent S - 1 never fires
    hist, pos, n_rows_c = IR.fire_counts(idx, val, nnz, labels, keep, S, C_, thr)
    one = engine.ClassFireCounts(S, C_, "cuda", thr)
    one.add(_dev(idx), _dev(val), _dev(nnz), _dev(labels), _dev(keep))
    assert (one.hist.cpu().numpy() == hist).all() and (one.pos.cpu().numpy() == pos).all() and (one.n_rows_c.cpu().numpy() == n_rows_c).all()
    assert n_rows_c[C_ - 1] == 0 and n_rows_c.sum() < n
    # two adds equal one add of the concatenation; labels as int64, the keep vector as bool
    two = engine.ClassFireCounts(S, C_, "cuda", thr)
    cut = 13
    two.add(_dev(idx[:cut]), _dev(val[:cut]), _dev(nnz[:cut]), _dev(labels[:cut].astype(np.int64)), _dev(keep[:cut]))
    two.add(_dev(idx[cut:]), _dev(val[cut:]), _dev(nnz[cut:]), _dev(labels[cut:].astype(np.int64)), _dev(keep[cut:]))
    assert torch.equal(two.hist, one.hist) and torch.equal(two.pos, one.pos) and torch.equal(two.n_rows_c, one.n_rows_c)
    mask = np.arange(S) % 7 != 3
    want, want_t = _check_f1(one, hist, pos, n_rows_c, mask)
    assert (want[:, ~mask] == -1).all() and (want[C_ - 1, S - 1] == 0) and (want[:, mask] >= 0).all()  # masked; a zero denominator
    _check_f1(one, hist, pos, n_rows_c, None)
    # full rows (no row_nnz), no keep vector
    full = engine.ClassFireCounts(S, C_, "cuda", thr)
    full.add(_dev(idx), _dev(val), None, _dev(labels))
    h2, p2, c2 = IR.fire_counts(idx, val, None, labels, None, S, C_, thr)
    assert (full.hist.cpu().numpy() == h2).all() and (full.pos.cpu().numpy() == p2).all() and (full.n_rows_c.cpu().numpy() == c2).all()


def test_fire_count_ties_contention_and_one_latent():
    from saev_amd import engine

    # one latent in each of 4096 rows: every atomic lands on the same few words and the count is exact; S = 1
    n = 4096
    idx = np.zeros((n, 1), dtype=np.int32)
    val = np.where(np.arange(n) % 4 == 0, 0.2, 5.0).astype(np.float32)[:, None]
    labels = (np.arange(n) % 3 == 0).astype(np.int32)
    c = engine.ClassFireCounts(1, 2, "cuda", (0.0, 0.1, 0.3, 1.0))
    c.add(_dev(idx), _dev(val), None, _dev(labels))
    hist, pos, n_rows_c = IR.fire_counts(idx, val, None, labels, None, 1, 2, (0.0, 0.1, 0.3, 1.0))
    assert int(pos.sum()) == n and (c.hist.cpu().numpy() == hist).all() and (c.pos.cpu().numpy() == pos).all()
    assert (c.n_rows_c.cpu().numpy() == n_rows_c).all() and int(c.pos[1, 0]) == n // 4 and int(c.pos[3, 0]) == n - n // 4
    _check_f1(c, hist, pos, n_rows_c, None)
    # a tie over the thresholds goes to the lowest: a latent whose every value clears the highest threshold
    S = 6
    idx = np.tile(np.arange(2, dtype=np.int32), (9, 1))
    val = np.stack([np.full(9, 3.0), np.linspace(0.05, 1.2, 9)], axis=1).astype(np.float32)
    labels = np.array([0, 0, 0, 1, 1, 1, 1, 0, 1], dtype=np.int32)
    t = engine.ClassFireCounts(S, 2, "cuda", (0.0, 0.1, 0.3, 1.0))
    t.add(_dev(idx), _dev(val), None, _dev(labels))
    hist, pos, n_rows_c = IR.fire_counts(idx, val, None, labels, None, S, 2, (0.0, 0.1, 0.3, 1.0))
    want, want_t = _check_f1(t, hist, pos, n_rows_c, None)
    assert want_t[0, 0] == 0 and want_t[1, 0] == 0 and want[0, 0] == np.float32(8.0) / (np.float32(13.0) + np.float32(1e-10))
    assert want_t[1, 1] > 0  # the rising latent separates class 1 better at a higher threshold
    latents, scores, thr = t.lookup(top_k=2)
    assert latents.shape == (2, 2) and latents[1, 0] == 1 and scores[1, 0] == want[1, 1] and abs(float(thr[1, 0]) - (0.0, 0.1, 0.3, 1.0)[want_t[1, 1]]) < 1e-6


def test_get_latent_lookup_on_a_module():
    """Two batches (the second with a keep vector) through the module's own encoder: the scores are the k largest restated F1 of
    every class, each reported latent holds its score, a masked latent is never chosen, a skipped class gets latent 0."""
    from saev_amd import interventions as IV

    sae = _module("topk")
    g = torch.Generator().manual_seed(31)
    x1, x2 = torch.randn(2, 16, 32, generator=g).cuda(), torch.randn(29, 32, generator=g).cuda()
    l1, l2 = torch.randint(0, 4, (2, 16), generator=g), torch.randint(-1, 5, (29,), generator=g)
    keep2 = torch.rand(29, generator=g) < 0.8
    sparsity = torch.rand(256, generator=g) * 0.05
    got = IV.get_latent_lookup(sae, [(x1, l1), (x2, l2, keep2)], n_classes=4, sparsity=sparsity, max_freq=0.03, top_k=3)
    rows = torch.cat([x1.reshape(-1, 32), x2])
    idx, val = (c.cpu().numpy() for c in sae.encode_sparse(rows))
    labels = torch.cat([l1.reshape(-1), l2]).numpy()
    keep = torch.cat([torch.ones(32, dtype=torch.bool), keep2]).numpy()
    hist, pos, n_rows_c = IR.fire_counts(idx, val, None, labels, keep, 256, 4, (0.0, 0.1, 0.3, 1.0))
    mask = (sparsity < 0.03).numpy()
    f1, best_t = IR.f1_from_counts(*IR.suffix(hist, pos), n_rows_c, mask)
    assert got.latents.shape == (4, 3) and (_bits(got.scores.numpy()) == _bits(-np.sort(-f1, axis=1)[:, :3])).all()
    for c in range(4):
        for j in range(3):
            lat = int(got.latents[c, j])
            assert mask[lat] and f1[c, lat] == got.scores[c, j] and abs(float(got.thresholds[c, j]) - (0.0, 0.1, 0.3, 1.0)[best_t[c, lat]]) < 1e-6
    assert int(got.lookup[0]) == 0 and got.lookup[1:].tolist() == got.latents[1:, 0].tolist()


# ---- the hook ----------------------------------------------------------------------------------------------------------------------


def _vit_and_head():
    from saev_amd.data import vit

    torch.manual_seed(21)
    model = vit.VisionTransformer(d_model=32, depth=2, heads=2, patch=4, image=16).cuda().eval()
    head = torch.nn.Linear(32, 7).cuda().eval()
    return model, head


def test_hooked_forward_equals_the_forward_with_the_output_replaced_by_hand():
    from saev_amd import interventions as IV

    model, head = _vit_and_head()
    sae = _module("topk")
    images = torch.randn(3, 3, 16, 16, generator=torch.Generator().manual_seed(22)).cuda()
    block = model.blocks[0]
    seen = {}
    with torch.no_grad():
        h = block.register_forward_hook(lambda m, a, out: seen.__setitem__("clean", out.clone()))
        model(images)
        h.remove()
        clean = seen["clean"]
        rows = clean[:, 1:, :].reshape(-1, 32).contiguous()
        idx, val = (c.cpu().numpy() for c in sae.encode_sparse(rows))
        top = np.argsort(-np.bincount(idx.ravel(), minlength=256))[:2]
        edits = IV.EditSet([IV.Edit(int(top[0]), "set", 6.0), IV.Edit(int(top[1]), "scale", -1.0, group=1)], 256, n_groups=2)
        row_group = torch.randint(0, 2, (3, 16), generator=torch.Generator().manual_seed(23))
        h1 = block.register_forward_hook(IV.make_hook(sae, edits, row_group=row_group))
        h2 = block.register_forward_hook(lambda m, a, out: seen.__setitem__("hooked", out.clone()))
        final = model(images)
        h1.remove(), h2.remove()
        hooked = seen["hooked"]
        # at the hook: the CLS token on the bits, the patches at the kernel's tolerance
        assert torch.equal(hooked[:, 0], clean[:, 0])
        r = IR.intervene(rows.cpu().numpy(), sae.W_dec.detach().cpu().numpy(), idx, val, None, edits.records, 2, row_group=row_group.reshape(-1).numpy())
        err = np.abs(hooked[:, 1:].reshape(-1, 32).cpu().numpy().astype(np.float64) - r["out"])
        assert (err <= IR.tolerance(r["mag"], r["m"])).all() and (r["m"] >= 1).all()
        assert not torch.equal(hooked[:, 1:], clean[:, 1:])
        # downstream of the same tensor: bit-equal
        assert torch.equal(final, model.norm(model.blocks[1](hooked)))
    assert len(block._forward_hooks) == 0


def test_evaluate_edits_counts_and_removes_its_hook():
    from saev_amd import interventions as IV

    model, head = _vit_and_head()
    sae = _module("topk")
    g = torch.Generator().manual_seed(24)
    batches = [{"image": torch.randn(2, 3, 16, 16, generator=g).cuda(), "patch_labels": torch.randint(0, 3, (2, 16), generator=g)} for _ in range(2)]
    edits = IV.EditSet([IV.Edit(l, "set", 40.0, group=grp) for grp, l in enumerate((3, 50, 111))], 256, n_groups=3)
    block = model.blocks[0]
    classes = range(1, 7)
    report = IV.evaluate_edits(model, block, head, sae, edits, batches, method="automatic-feature", scale=-2.0, row_group_key="patch_labels",
                               classes=classes)
    assert len(block._forward_hooks) == 0
    orig, mod = [], []
    with torch.no_grad():
        for b in batches:
            orig.append(IV.argmax_logits(head(model(b["image"])[:, 1:, :])))
            h = block.register_forward_hook(IV.make_hook(sae, edits, row_group=b["patch_labels"]))
            mod.append(IV.argmax_logits(head(model(b["image"])[:, 1:, :])))
            h.remove()
    want = IR.triple_loop(torch.cat(orig).cpu(), torch.cat(mod).cpu(), list(classes))
    got = [(r.class_id, r.n_orig_patches, r.n_changed_patches, r.n_other_patches, r.n_other_changed, r.change_distribution) for r in report.class_results]
    assert got == want and report.method == "automatic-feature" and report.intervention_scale == -2.0
    assert sum(w[2] for w in want) > 0, "the edits must change some predictions for the counts to mean something"

    def broken(module, args, output):
        raise KeyError("from the hook")

    with pytest.raises(KeyError):
        IV.evaluate_edits(model, block, head, sae, edits, [batches[0]["image"]], method="x", scale=0.0, hook=broken)
    assert len(block._forward_hooks) == 0
