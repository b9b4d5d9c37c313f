"""Builders of the inputs of the interventions' geometry tests (tests/test_interventions_cases_host_cpu.py,
tests/test_gpu_interventions_geometry.py): the latent edits past one pass of a wave over D, past one grid of rows, off the 16-byte
alignment and at the limits of the plan; the firing counts past their three grid caps, at 4096 classes and past 2^24.  Every case
carries its inputs, its settings and a ``holds(expected)`` check of the property it was built for, where ``expected`` is what
tests/interventions_restatement.py makes of it.  The CPU test runs every ``holds`` and pins the constants below to the text of
saev_amd/csrc/intervene.hip; the GPU test demands that the device equals ``expected``.  A module, not a test file."""

from __future__ import annotations

import dataclasses
import functools
from typing import Callable

import numpy as np

import interventions_restatement as IR

# saev_amd/csrc/intervene.hip and entry_util.h, asserted by the CPU test: a retune must fail there, not move the cases off their edges
IV_WAVES, IV_TRIPS, IV_MAX_GRID, IV_MAX_LIST, IV_CNT_SLOTS = 4, 4, 2048, 256, 256
IV_MAX_EDITS = IV_MAX_GROUPS = 65536
CF_THREADS, CF_CODES_MAX_GRID, CF_ROWS_MAX_GRID, CF_F1_MAX_GRID = 256, 8192, 1024, 8192
ENTRY_MAX_C = 4096

GRID_ROWS = IV_MAX_GRID * IV_WAVES              # the rows of one stride of iv_rows_kernel
CODES_SPAN = CF_CODES_MAX_GRID * CF_THREADS     # the code slots, rows and (class, latent) pairs of one stride of the firing kernels
ROWS_SPAN = CF_ROWS_MAX_GRID * CF_THREADS
F1_SPAN = CF_F1_MAX_GRID * CF_THREADS

SET, SCALE, ADD, IF_ACTIVE = IR.SET, IR.SCALE, IR.ADD, IR.IF_ACTIVE
FREE = 39  # a latent no case edits (S >= 40 everywhere below)


def passes(D: int, vec: bool) -> int:
    """Trips of iv_apply's outer loop over a row of D floats: a pass is 64 lanes x IV_TRIPS elements, float4 or float."""
    nv = D // 4 if vec else D
    return -(-nv // (64 * IV_TRIPS))


def plan_positions(edits, n_groups: int) -> np.ndarray:
    """The position in the plan of every edit: the global list, then the groups' lists, the caller's order inside a list."""
    order = np.argsort(np.array([e[3] for e in edits], dtype=np.int64), kind="stable")
    at = np.empty(len(edits), dtype=np.int64)
    at[order] = np.arange(len(edits))
    return at


def exact_in_f32(v: np.ndarray) -> np.ndarray:
    """Which of these integers (below 2^53) float32 holds exactly."""
    v = np.asarray(v, dtype=np.int64)
    return v.astype(np.float32).astype(np.float64) == v.astype(np.float64)


@dataclasses.dataclass
class EditCase:
    name: str
    x: np.ndarray
    W: np.ndarray
    idx: np.ndarray
    val: np.ndarray
    row_nnz: np.ndarray | None
    edits: list
    n_groups: int
    holds: Callable[[dict], None]
    row_group: np.ndarray | None = None
    row_keep: np.ndarray | None = None
    offsets: tuple = ()            # alignment cases: the sets of tensors moved one float off 16 bytes
    prefill: np.ndarray | None = None  # counts cases: what rows_changed holds before the call

    @property
    def args(self) -> tuple:
        return self.x, self.W, self.idx, self.val, self.row_nnz, self.edits, self.n_groups

    @functools.cached_property
    def expected(self) -> dict:
        return IR.intervene_fast(*self.args, row_group=self.row_group, row_keep=self.row_keep)


@dataclasses.dataclass
class FireCase:
    name: str
    idx: np.ndarray
    val: np.ndarray
    row_nnz: np.ndarray | None
    labels: np.ndarray
    keep: np.ndarray | None
    S: int
    C: int
    thr: tuple
    holds: Callable[[dict], None]
    mask: np.ndarray | None = None
    repeats: int = 1               # the batch is added this many times to one ClassFireCounts

    @functools.cached_property
    def expected(self) -> dict:
        hist, pos, n_rows_c = (self.repeats * a for a in IR.fire_counts_fast(self.idx, self.val, self.row_nnz, self.labels, self.keep, self.S, self.C, self.thr))
        f1, best_t = IR.f1_from_counts(*IR.suffix(hist, pos), n_rows_c, self.mask)
        return dict(hist=hist, pos=pos, n_rows_c=n_rows_c, f1=f1, best_t=best_t)


def _codes(rng, n: int, S: int, cap: int, ragged: bool = True):
    """Distinct latents per row in random order, every slot filled (the slots past row_nnz hold latents too: they must be ignored)."""
    idx = rng.permuted(np.tile(np.arange(S, dtype=np.int32), (n, 1)), axis=1)[:, :cap].copy()
    val = rng.uniform(0.25, 2.0, (n, cap)).astype(np.float32)
    nnz = rng.integers(0, cap + 3, n).astype(np.int32) if ragged else np.full(n, cap, dtype=np.int32)  # 0, full, above the capacity
    return idx, val, nnz


def _put(idx, val, b, slot, latent, value):
    """Latent at a slot of row b; wherever else the row held it gets the latent no case edits."""
    idx[b, idx[b] == latent] = FREE
    idx[b, slot], val[b, slot] = latent, value


def _ops_applied(case: EditCase, e: dict) -> set:
    return {case.edits[i][1] & 3 for i in e["applied"]}


# ---- widths: the passes of a wave over D ---------------------------------------------------------------------------------------------

def six_edits(S: int) -> list:
    return [(0, SET, 1.5, -1), (S - 1, SCALE, -0.5, -1), (7, ADD | IF_ACTIVE, 0.75, -1),
            (3, SET | IF_ACTIVE, -2.0, 0), (5, ADD, 0.125, 1), (9, SCALE | IF_ACTIVE, 3.0, 1)]


# D -> (float4 route, passes of the outer loop, elements of the last pass)
WIDTHS = {1020: (True, 1, 255), 1024: (True, 1, 256), 1028: (True, 2, 1), 1280: (True, 2, 64), 2052: (True, 3, 1), 4100: (True, 5, 1),
          255: (False, 1, 255), 257: (False, 2, 1), 258: (False, 2, 2), 511: (False, 2, 255), 513: (False, 3, 1), 1027: (False, 5, 3)}


def width_case(D: int, name: str | None = None, keep=(False, True, True, True, True), seed: int = 0) -> EditCase:
    """Five rows (or as many as ``keep`` has) under the global list and two group lists with all three ops: row 1 holds every
    edited latent and takes the global list and group 1's, row 2 group 0's, the others an out-of-range group or none."""
    vec, n_pass, last = WIDTHS[D]
    rng = np.random.default_rng(1000 * seed + D)
    S, cap, G, n = 48, 5, 2, len(keep)
    edits = six_edits(S)
    W = rng.standard_normal((S, D)).astype(np.float32)
    x = rng.standard_normal((n, D)).astype(np.float32)
    idx, val, nnz = _codes(rng, n, S, cap)
    for b in range(n):
        for lat in (0, S - 1, 7, 3, 9, 5):
            idx[b, idx[b] == lat] = FREE
    row_group = np.array([1, G - 1, 0, G, -1, 0, 1, -1, G][:n], dtype=np.int32)
    for b in range(n):
        if b % 4 != 0:  # rows 0, 4, 8 hold no edited latent: only SET and ADD remain for them
            nnz[b] = cap
            for j, lat in enumerate((0, S - 1, 7, 3, 9)):
                _put(idx, val, b, j, lat, np.float32(0.5 + j + b / 8))
    case = EditCase(name or f"width_{'float4' if vec else 'scalar'}_{D}", x, W, idx, val, nnz, edits, G, None, row_group=row_group,
                    row_keep=np.array(keep, dtype=bool))

    def holds(e):
        assert (D % 4 == 0) == vec and passes(D, vec) == n_pass, (D, passes(D, vec))
        nv = D // 4 if vec else D
        assert nv - (n_pass - 1) * 64 * IV_TRIPS == last  # what the last pass holds: a full pass, one lane, or a ragged set of lanes
        kept = np.array(keep, dtype=bool)
        assert (e["m"][~kept] == 0).all() and (e["m"][kept] >= 1).all()
        assert _ops_applied(case, e) == {SET, SCALE, ADD}
        groups = {case.edits[i][3] for i in e["applied"]}
        assert -1 in groups and groups & {0, 1}, groups  # the global list and a group's list in one row
        assert e["m"][1] == 5
    case.holds = holds
    return case


def inplace_long_lists() -> EditCase:
    """Two lists of 256 edits in one row (m > 256: the unroll-2 edit loop over an odd and an even count) at D = 1028, where the
    second pass holds one float4."""
    rng = np.random.default_rng(256)
    S, D, cap, n, G = 600, 1028, 8, 7, 3
    lat = rng.permutation(np.arange(40, S))
    edits = [(int(l), int(rng.integers(0, 3)), float(rng.uniform(0.5, 1.5)), -1) for l in lat[:IV_MAX_LIST]]
    edits += [(int(l), int(rng.integers(0, 3)), float(rng.uniform(0.5, 1.5)), 1) for l in lat[IV_MAX_LIST:2 * IV_MAX_LIST]]
    rng.shuffle(edits)
    edits = [tuple(e) for e in edits]
    W = (rng.standard_normal((S, D)) / 8).astype(np.float32)
    x = rng.standard_normal((n, D)).astype(np.float32)
    idx, val, nnz = _codes(rng, n, S, cap)
    for b in range(n):
        _put(idx, val, b, b % cap, edits[b][0], 1.0)
    row_group = np.array([1, 1, 0, 2, -1, G, 1], dtype=np.int32)

    def holds(e):
        assert passes(D, True) == 2 and e["m"].max() > IV_MAX_LIST
        assert len({int(v) % 2 for v in e["m"]}) == 2  # odd and even list lengths
    return EditCase("inplace_512_edits_1028", x, W, idx, val, nnz, edits, G, holds, row_group=row_group)


def inplace_gap() -> EditCase:
    """In place at three passes: rows without a remaining edit (left alone, never read) between rows with edits."""
    case = width_case(2052, "inplace_gap_2052", keep=(True, True, False, True, False, False, True, True, False), seed=1)
    inner = case.holds

    def holds(e):
        inner(e)
        m = e["m"]
        assert any(m[b - 1] >= 1 and m[b] == 0 and m[b + 1] >= 1 for b in range(1, len(m) - 1)), m
        assert passes(2052, True) >= 2
    case.holds = holds
    return case


def alignment_case(D: int) -> EditCase:
    """D % 4 == 0; the GPU test moves x, out and W_dec one float off 16 bytes, one at a time and together."""
    if D == 1028:
        case = width_case(1028, "align_1028", seed=2)
    else:
        rng = np.random.default_rng(8)
        S, cap, G, n = 48, 5, 2, 6
        W = rng.standard_normal((S, D)).astype(np.float32)
        x = rng.standard_normal((n, D)).astype(np.float32)
        idx, val, nnz = _codes(rng, n, S, cap, ragged=False)
        for b in range(n):
            for j, lat in enumerate((0, S - 1, 7, 3, 9)):
                _put(idx, val, b, j, lat, np.float32(0.5 + j))
        case = EditCase(f"align_{D}", x, W, idx, val, nnz, six_edits(S), G, None, row_group=np.array([1, 0, -1, 1, G, 0], dtype=np.int32),
                        row_keep=np.array([True, True, False, True, True, True]))
    inner = case.holds
    case.offsets = (("x",), ("out",), ("W",), ("x", "out", "W"))

    def holds(e):
        if inner is not None:
            inner(e)
        assert D % 4 == 0 and (D * 4) % 16 == 0  # every row of a tensor one float off is one float off: the whole call is scalar
        assert (e["m"] == 0).any() and (e["m"] >= 2).any()
    case.holds = holds
    return case


# ---- rows: the stride of a wave over the rows past one grid --------------------------------------------------------------------------

# the kind of row a wave meets on its first, second and third stride, by (row within the grid) % 3
STRIDE_KINDS = (("long", "none", "short"), ("long", "short", "none"), ("short", "long", "global"))
LONG_LIST = 70  # more than one 64-record load of phase 1


def row_stride_case(n: int) -> EditCase:
    """D = 8.  Group 0 has 70 edits, group 1 two, group 2 none; the global list one ADD.  A row is long (group 0), short (group
    1), global (group 2: the global edit alone) or none (not kept) by STRIDE_KINDS, so that one wave meets an edited row, an
    unedited row and an edited row again, and lists of falling length, on successive strides."""
    rng = np.random.default_rng(n)
    S, D, cap, G = 128, 8, 4, 3
    edits = [(0, ADD, 0.5, -1)]
    edits += [(40 + k, (SET, SCALE, ADD, ADD | IF_ACTIVE, SET | IF_ACTIVE)[k % 5], float(0.5 + k / 64), 0) for k in range(LONG_LIST)]
    edits += [(1, SET, 2.0, 1), (2, ADD, -0.75, 1)]
    W = (rng.standard_normal((S, D)) / 8).astype(np.float32)
    x = rng.standard_normal((n, D)).astype(np.float32)
    idx, val, nnz = _codes(rng, n, S, cap)
    b = np.arange(n)
    kind = np.array([[("long", "short", "global", "none").index(k) for k in row] for row in STRIDE_KINDS])[(b % GRID_ROWS) % 3, np.minimum(b // GRID_ROWS, 2)]
    row_group = np.array([0, 1, 2, -1], dtype=np.int32)[kind]
    row_keep = kind != 3

    def holds(e):
        m = e["m"]
        assert (e["rows_changed"] >= 1).all(), "every edit is counted at least once"
        if n <= GRID_ROWS:
            assert n in (GRID_ROWS - 1, GRID_ROWS)  # one stride: the last workgroup short of a row, and full
            return
        over = n - GRID_ROWS
        assert (m[:over] > 0)[m[GRID_ROWS:GRID_ROWS + over] > 0].any(), "no wave has edits on two strides"
        assert (m[:over] > m[GRID_ROWS:GRID_ROWS + over])[m[GRID_ROWS:GRID_ROWS + over] > 0].any(), "long, then short"
        assert (m[GRID_ROWS:GRID_ROWS + over] > m[:over]).any(), "short, then long"
        if n > 2 * GRID_ROWS:
            third = n - 2 * GRID_ROWS
            a, c, d = m[:third], m[GRID_ROWS:GRID_ROWS + third], m[2 * GRID_ROWS:]
            assert ((a > 0) & (c == 0) & (d > 0)).any(), "edited, unedited, edited"
            assert ((a > c) & (c > 0) & (d == 0)).any(), "long, short, none"
    return EditCase(f"row_stride_{n}", x, W, idx, val, nnz, edits, G, holds, row_group=row_group, row_keep=row_keep)


# ---- rows_changed: added to, and three contenders of one slot --------------------------------------------------------------------------


def counts_case() -> EditCase:
    """Three groups of 256 edits: plan positions p, p + 256 and p + 512 share slot p of the workgroup's table, and the four rows of
    workgroup 0 belong to the three groups.  rows_changed starts from distinct values, one above 2^32."""
    rng = np.random.default_rng(77)
    S, D, cap, G = 300, 8, 6, 3
    n = 2 * IV_WAVES + 1
    edits = [(40 + k, (ADD, SET | IF_ACTIVE, SCALE)[k % 3], float(0.25 + k / 128), g) for g in range(G) for k in range(IV_MAX_LIST)]
    W = (rng.standard_normal((S, D)) / 8).astype(np.float32)
    x = rng.standard_normal((n, D)).astype(np.float32)
    idx, val, nnz = _codes(rng, n, S, cap)
    row_group = np.array([0, 1, 2, 0, 1, 2, -1, 0, 2], dtype=np.int32)
    prefill = 3 * np.arange(len(edits), dtype=np.int64) + 1
    prefill[5] = 2 ** 32 + 7
    prefill[IV_CNT_SLOTS + 5] = 2 ** 40 + 1

    def holds(e):
        assert len(edits) >= 3 * IV_CNT_SLOTS and G >= 3 and (prefill > 0).all() and len(set(prefill.tolist())) == len(edits) and prefill.max() > 2 ** 32
        at = plan_positions(edits, G)
        rows_at = {int(at[i]): set(r.tolist()) for i, r in e["applied"].items()}
        first = set(range(IV_WAVES))  # the rows of workgroup 0
        triple = [p for p in range(IV_CNT_SLOTS) if all(rows_at.get(p + k * IV_CNT_SLOTS, set()) & first for k in range(3))]
        assert triple, "no slot with three contenders inside one workgroup"
        assert len({int(row_group[b]) for b in first}) == 3
        assert _ops_applied(case, e) == {SET, SCALE, ADD}
    case = EditCase("counts_prefilled_three_contenders", x, W, idx, val, nnz, edits, G, holds, row_group=row_group, prefill=prefill)
    return case


def plan_limits_case() -> EditCase:
    """E = G = 65536, one edit per group (a ptr array of G + 2 entries); the rows' groups are drawn over -1, 0, 1, G - 2, G - 1, G."""
    rng = np.random.default_rng(65536)
    S, D, cap, n = 64, 8, 4, 24
    E = G = IV_MAX_EDITS
    edits = [(i % S, (SET, SCALE, ADD)[i % 3], 1.5, i) for i in range(E)]
    W = rng.standard_normal((S, D)).astype(np.float32)
    x = rng.standard_normal((n, D)).astype(np.float32)
    idx, val, nnz = _codes(rng, n, S, cap, ragged=False)
    pool = np.array([-1, 0, 1, G - 2, G - 1, G], dtype=np.int32)
    row_group = pool[np.arange(n) % len(pool)]
    for b in range(n):
        g = int(row_group[b])
        if 0 <= g < G:
            _put(idx, val, b, b % cap, edits[g][0], np.float32(0.5 + b / 32))
    used = [0, 1, G - 2, G - 1]

    def holds(e):
        assert len(edits) == IV_MAX_EDITS and G == IV_MAX_GROUPS
        assert np.nonzero(e["rows_changed"])[0].tolist() == used and (e["rows_changed"][used] == n // len(pool)).all()
        outside = (row_group < 0) | (row_group >= G)
        assert (e["m"][outside] == 0).all() and (e["m"][~outside] == 1).all() and outside.sum() == 2 * (n // len(pool))
        assert {edits[g][1] for g in used} == {SET, SCALE, ADD}
    return EditCase("plan_limits_65536", x, W, idx, val, nnz, edits, G, holds, row_group=row_group)


EDIT_CASES: dict[str, Callable[[], EditCase]] = {}
for _D, (_vec, _, _) in WIDTHS.items():
    EDIT_CASES[f"width_{'float4' if _vec else 'scalar'}_{_D}"] = functools.partial(width_case, _D)
EDIT_CASES["inplace_512_edits_1028"] = inplace_long_lists
EDIT_CASES["inplace_gap_2052"] = inplace_gap
for _n in (GRID_ROWS - 1, GRID_ROWS, GRID_ROWS + 5, 2 * GRID_ROWS + 3):
    EDIT_CASES[f"row_stride_{_n}"] = functools.partial(row_stride_case, _n)
EDIT_CASES["plan_limits_65536"] = plan_limits_case

ALIGN_CASES: dict[str, Callable[[], EditCase]] = {f"align_{_D}": functools.partial(alignment_case, _D) for _D in (1028, 8)}
COUNT_CASES: dict[str, Callable[[], EditCase]] = {"counts_prefilled_three_contenders": counts_case}


# ---- firing counts -------------------------------------------------------------------------------------------------------------------

THR4 = (0.0, 0.1, 0.3, 1.0)


def _fire_inputs(rng, n: int, S: int, C: int, cap: int, thr, every_row: int | None = None):
    """Random codes with values on, next to and away from the thresholds (NaN and a negative among them), padding slots, latents one past the last, ragged
    row_nnz, a keep vector and labels over [-1, C]; ``every_row``: a latent that sits in slot 0 of every row."""
    thr32 = np.asarray(thr, dtype=np.float32)
    pool = np.concatenate([thr32, np.nextafter(thr32, np.float32(np.inf)), np.array([-1.0, 0.05, 7.0, np.nan], dtype=np.float32)])
    if S < cap:  # a few latents, repeated inside a row: every count is large
        idx = rng.integers(0, S, (n, cap)).astype(np.int32)
    elif S >= 4 * cap:  # distinct latents in a row without a permutation of S per row
        idx = ((rng.integers(0, S, n)[:, None] + np.arange(cap)[None, :] * (S // cap)) % S).astype(np.int32)
    else:
        idx = rng.permuted(np.tile(np.arange(S, dtype=np.int32), (n, 1)), axis=1)[:, :cap].copy()
    idx[rng.random((n, cap)) < 0.05] = -1  # padding
    idx[rng.random((n, cap)) < 0.01] = S   # and a latent one past the last
    val = rng.choice(pool, (n, cap)).astype(np.float32)
    if every_row is not None:
        idx[:, 1:][idx[:, 1:] == every_row] = -1
        idx[:, 0], val[:, 0] = every_row, 7.0
    nnz = rng.integers(0, cap + 2, n).astype(np.int32)
    labels = rng.integers(-1, C + 1, n).astype(np.int32)  # -1 and C are out of range
    keep = rng.random(n) < 0.8
    return idx, val, nnz, labels, keep


def _head_nnz(row_nnz, n: int, cap: int, entries: int):
    """row_nnz with every code slot of flat index >= ``entries`` cut off: what a kernel without its stride would see."""
    nnz = np.full(n, cap, dtype=np.int64) if row_nnz is None else np.clip(np.asarray(row_nnz, dtype=np.int64), 0, cap)
    return np.minimum(nnz, np.clip(entries - np.arange(n, dtype=np.int64) * cap, 0, cap)).astype(np.int32)


def _caps_holds(case: FireCase, entries_rel: str, rows_rel: str):
    n, cap = case.idx.shape

    def holds(e):
        total = n * cap
        assert {"past": total > CODES_SPAN + 1, "at": total == CODES_SPAN, "one_past": total == CODES_SPAN + 1}[entries_rel], total
        assert {"past": n > ROWS_SPAN, "at": n == ROWS_SPAN}[rows_rel], n
        assert e["pos"].sum(axis=0).max() > 2 ** 16, "a latent's count must pass 16 bits"
        assert (case.labels == -1).any() and (case.labels == case.C).any() and not case.keep.all()
        assert len(set(np.clip(case.row_nnz, 0, cap).tolist())) == cap + 1  # ragged: every length from 0 to the capacity
        if total > CODES_SPAN:  # the code slots past one stride are counted
            head = IR.fire_counts_fast(case.idx, case.val, _head_nnz(case.row_nnz, n, cap, CODES_SPAN), case.labels, case.keep, case.S, case.C, case.thr)
            assert e["hist"].sum() - head[0].sum() >= 1 and e["pos"].sum() - head[1].sum() >= 1
        if n > ROWS_SPAN:  # and so are the rows
            ok = (case.labels[ROWS_SPAN:] >= 0) & (case.labels[ROWS_SPAN:] < case.C) & case.keep[ROWS_SPAN:]
            assert ok.any()
    return holds


def fire_caps_case(n: int, cap: int, entries_rel: str, rows_rel: str) -> FireCase:
    rng = np.random.default_rng(n + cap)
    S, C = 2, 5  # two latents, so that each one's count passes 2^16
    idx, val, nnz, labels, keep = _fire_inputs(rng, n, S, C, cap, THR4)
    # the last row, which ends in the last code slot of the call, counts: kept, labelled, full, above every threshold
    labels[-3:], keep[-3:], nnz[-3:] = (C - 1, 0, 2), True, cap
    idx[-1, -1], val[-1, -1] = S - 1, 7.0
    idx[-1, :-1][idx[-1, :-1] == S - 1] = -1
    case = FireCase(f"fire_{n}x{cap}", idx, val, nnz, labels, keep, S, C, THR4, None)
    case.holds = _caps_holds(case, entries_rel, rows_rel)
    return case


def f1_cap_case() -> FireCase:
    """C = 4096, T = 1, S = 513: C * S is past one stride of cf_f1_kernel; the tail of the (class, latent) pairs holds masked
    latents and classes with rows."""
    rng = np.random.default_rng(4096)
    C, S, cap, n = ENTRY_MAX_C, 513, 4, 3000
    idx, val, nnz, labels, keep = _fire_inputs(rng, n, S, C, cap, (0.0,))
    first_tail_class = F1_SPAN // S  # the class the second stride begins in
    labels[-400:] = rng.integers(first_tail_class, C, 400)
    labels[-1], keep[-400:] = C - 1, True
    mask = np.arange(S) % 7 != 3
    mask[S - 1] = False

    def holds(e):
        assert C * S > F1_SPAN and C == ENTRY_MAX_C
        tail_f1 = e["f1"].reshape(-1)[F1_SPAN:]
        tail_masked = np.tile(~mask, C)[F1_SPAN:]
        assert tail_masked.any() and (tail_f1[tail_masked] == -1).all() and (tail_f1[~tail_masked] > 0).any()
        assert e["n_rows_c"][C - 1] > 0 and (e["n_rows_c"] == 0).any()
    return FireCase("f1_cap_c4096_s513", idx, val, nnz, labels, keep, S, C, (0.0,), holds, mask=mask)


def rows_cap_c4096_case() -> FireCase:
    """C = 4096 with more rows than one stride of cf_rows_kernel: 16 KiB of counters in LDS and a stride."""
    rng = np.random.default_rng(4097)
    C, S, cap, n = ENTRY_MAX_C, 520, 2, ROWS_SPAN + 3
    thr = (0.0, 0.3)
    idx, val, nnz, labels, keep = _fire_inputs(rng, n, S, C, cap, thr)
    labels[-3:], keep[-3:] = (C - 1, 0, C // 2), True
    mask = np.arange(S) % 5 != 1

    def holds(e):
        assert n > ROWS_SPAN and C == ENTRY_MAX_C and C * S > F1_SPAN
        ok = (labels >= 0) & (labels < C) & keep
        head = np.bincount(labels[:ROWS_SPAN][ok[:ROWS_SPAN]], minlength=C)
        assert (e["n_rows_c"] - head).sum() == 3 and e["n_rows_c"][C - 1] > head[C - 1] and (e["n_rows_c"] > 0).all()
        assert len(set(e["best_t"].reshape(-1).tolist())) == 2
    return FireCase("rows_cap_c4096", idx, val, nnz, labels, keep, S, C, thr, holds, mask=mask)


def f1_mutated(TP, POS, n_rows_c):
    """What F1 becomes when 2 TP is formed as 2.f * float(TP) and the denominator is summed in fp32, for T = 1: the slip the
    2^24 case exists to catch."""
    f32 = np.float32
    FP, FN = POS[None] - TP, n_rows_c[:, None, None] - TP
    num = f32(2) * TP.astype(f32)
    den = ((num + FP.astype(f32)).astype(f32) + FN.astype(f32)).astype(f32) + f32(1e-10)
    return (num / den).astype(f32)[:, 0, :]


def past_2p24_case() -> FireCase:
    """One batch just past the rows cap, added 79 times: latent 0 sits in every row and class 0 holds nine rows in ten, so 2 TP and
    2 TP + FP + FN pass 2^25 on odd multiples of 2 -- integers float32 does not hold."""
    rng = np.random.default_rng(24)
    C, S, cap, n, k = 4, 8, 2, ROWS_SPAN + 3, 79
    idx, val, nnz, labels, keep = _fire_inputs(rng, n, S, C, cap, (0.0,), every_row=0)
    nnz[:] = rng.integers(1, cap + 2, n)
    labels[:] = np.where(rng.random(n) < 0.9, 0, rng.integers(-1, C + 1, n))
    keep[:] = rng.random(n) < 0.97
    ok = (labels >= 0) & (labels < C) & keep
    n0 = int((ok & (labels == 0)).sum())
    free = np.nonzero(~keep & (labels == 0))[0]
    if n0 % 2 == 0:  # TP[0, 0, 0] odd: 2 TP k is then an odd multiple of 2
        keep[free[0]] = True
        free = free[1:]
    if (int(((labels >= 0) & (labels < C) & keep).sum()) + int((keep & (labels == 0)).sum())) % 2 == 0:  # POS + n_rows_c odd
        other = np.nonzero(~keep & (labels == 1))[0]
        keep[other[0]] = True

    def holds(e):
        TP, POS = IR.suffix(e["hist"], e["pos"])
        num, den = 2 * TP, 2 * TP + (POS[None] - TP) + (e["n_rows_c"][:, None, None] - TP)
        assert num[0, 0, 0] > 2 ** 24 and den[0, 0, 0] > 2 ** 24
        assert (~exact_in_f32(num)).any(), "no numerator that float32 does not hold"
        assert (~exact_in_f32(den)).any(), "no denominator that float32 does not hold"
        assert not exact_in_f32(num[0, 0, 0]) and not exact_in_f32(den[0, 0, 0])
        slipped = f1_mutated(TP, POS, e["n_rows_c"])
        assert (slipped.view(np.uint32) != e["f1"].view(np.uint32)).any(), "the fp32-summed denominator gives the same bits: the case proves nothing"
        assert n > ROWS_SPAN and int(e["hist"].max()) < 2 ** 32
    return FireCase("f1_past_2p24", idx, val, nnz, labels, keep, S, C, (0.0,), holds, repeats=k)


FIRE_CASES: dict[str, Callable[[], FireCase]] = {
    "fire_caps_both": functools.partial(fire_caps_case, ROWS_SPAN + 3, 9, "past", "past"),
    "fire_entries_at_cap": functools.partial(fire_caps_case, ROWS_SPAN, CODES_SPAN // ROWS_SPAN, "at", "at"),
    "fire_entries_one_past_cap": functools.partial(fire_caps_case, (CODES_SPAN + 1) // 3, 3, "one_past", "past"),
    "f1_cap_c4096_s513": f1_cap_case,
    "rows_cap_c4096": rows_cap_c4096_case,
    "f1_past_2p24": past_2p24_case,
}
