"""Inputs of the single-op forward tests (tests/test_gpu_forward_ops.py on the GPU, tests/test_forward_ops_host_cpu.py without one),
at the smallest shapes that reach each edge of select_dense_kernel, decode_kernel<NV> with x == nullptr, scatter_dense_kernel and
gather_rows_kernel.  What a case claims to reach is a field of the case; the host test computes it from the inputs.

select_dense_kernel: 256 threads, one float4 each per trip of 1 024 elements; four radix passes over the key bytes 3, 2, 1, 0
(forward_ops_restatement.keys), lane l of the first wave owning histogram bins 4l .. 4l + 3; then a compaction in trips of 1 024."""

import dataclasses
import typing as tp

import numpy as np

from forward_ops_restatement import from_keys, keys

TRIP = 1024
WIDTHS = (4, 8, 1020, 1024, 1028, 2052, 16388)
KS = (1, 2, 33, 64, 65, 100, 1030)


def _bits(b) -> np.ndarray:
    return np.asarray(b, dtype=np.uint32).view(np.float32)


@dataclasses.dataclass(frozen=True)
class SelectCase:
    id: str
    S: int
    build: tp.Callable[[], tuple]   # () -> (h (n, S) float32, k, mask (S,) int32 or None)
    byte: int | None = None         # the k-th and (k+1)-th key of every row first differ in this byte (0 = least significant)
    digit: tuple | None = None      # (byte, value): the k-th key of every row has this digit there, and shares the bytes above with the (k+1)-th
    bin_exact: int | None = None    # the k-th key's top byte, with exactly k keys whose top byte is at least that
    tie_trips: bool = False         # the kept ties lie on both sides of a 1 024-element trip border
    ties_run_out: bool = False      # ... and ties that are left out, or strictly greater elements, follow in a later trip
    tie_free: bool = False          # finite, pairwise different values
    eligible: int | None = None     # number of eligible latents of the mask


def _place(rng, top, rest):
    """One row: the values of `top` and `rest` at random positions."""
    row = np.concatenate([top, rest])
    return row[rng.permutation(len(row))]


# ---- the four byte passes --------------------------------------------------------------------------------------------------------

_BYTE_BASE = (0x3F812300, 0x3F810045, 0x3F001234, 0x00345678)  # byte p of base p is 0x00, so base + j 256^p carries nowhere


def byte_pass(p: int, sign: bool, S: int, k: int, seed: int):
    """Values with the bits base + j 256^p (j < 251; j < 127 in the top byte: finite), with the sign bit set if `sign`: all keys
    share the bytes above p, and the cut falls between two neighbouring j."""
    def build():
        rng = np.random.default_rng(seed)
        js = np.arange(127 if p == 3 else 251, dtype=np.uint32)
        vals = _bits(np.uint32(_BYTE_BASE[p]) + js * np.uint32(256 ** p) + np.uint32(0x80000000 if sign else 0))
        cls = vals[np.argsort(-keys(vals).astype(np.int64))]  # classes from the largest key down
        b = len(cls) // 2
        rows = []
        for _ in range(2):
            top = np.concatenate([cls[b:b + 1], rng.choice(cls[:b + 1], k - 1)])
            rest = np.concatenate([cls[b + 1:b + 2], rng.choice(cls[b + 1:], S - k - 1)])
            rows.append(_place(rng, top, rest))
        return np.stack(rows), k, None
    return SelectCase(f"byte{p}{'neg' if sign else 'pos'}-S{S}k{k}", S, build, byte=p)


def _key_bytes(rng, n: int, p: int, digit) -> np.ndarray:
    """n keys: the bytes above p those of 0xC0123456 (floats of a few units), byte p = digit (an array or a scalar), the bytes below random."""
    hi = np.uint32(0xC0123456) & np.uint32((0xFFFFFFFF << (8 * (p + 1))) & 0xFFFFFFFF)
    lo = rng.integers(0, 256 ** p, n, dtype=np.uint64).astype(np.uint32) if p else np.zeros(n, dtype=np.uint32)
    return hi | (np.broadcast_to(np.asarray(digit, dtype=np.uint32), (n,)) << np.uint32(8 * p)) | lo


def digit_edge(p: int, d: int, S: int, k: int, seed: int):
    """The cut digit of the pass over byte p is 0xFF -- the k winners are exactly the keys with that digit -- or 0x00: half of the
    winners lie above, the others are chosen among the keys with digit 0x00 by the bytes below (byte 0: by latent index)."""
    assert d in (0x00, 0xFF) and 1 <= k < S
    def build():
        rng = np.random.default_rng(seed)
        rows = []
        for _ in range(2):
            if d == 0xFF:
                top = _key_bytes(rng, k, p, 0xFF)
                rest = _key_bytes(rng, S - k, p, np.concatenate([[0xFE], rng.integers(0, 0xFF, S - k - 1)]))
            else:
                top = _key_bytes(rng, k // 2, p, rng.integers(1, 256, k // 2))
                rest = _key_bytes(rng, S - k // 2, p, 0x00)
            rows.append(from_keys(_place(rng, top, rest)))
        return np.stack(rows), k, None
    return SelectCase(f"digit{p}-{d:02x}-S{S}k{k}", S, build, digit=(p, d))


def bin_edge(d: int, S: int, k: int, seed: int):
    """First pass: the k-th key's top byte is d = 4l + j, and EXACTLY k keys have a top byte >= d (running + count == need in
    lane l's bin j); d = 0 needs k = S."""
    assert (d > 0 and 1 <= k < S) or (d == 0 and k == S)
    def build():
        rng = np.random.default_rng(seed)
        low = lambda n: rng.integers(0, 1 << 24, n, dtype=np.uint64).astype(np.uint32)
        rows = []
        for _ in range(2):
            tb = np.concatenate([[d], rng.integers(d, min(d + 40, 255) + 1, k - 1)]).astype(np.uint32)
            top = (tb << np.uint32(24)) | low(k)
            rb = rng.integers(max(d - 40, 0), max(d, 1), S - k).astype(np.uint32)
            rest = (rb << np.uint32(24)) | low(S - k)
            rows.append(from_keys(_place(rng, top, rest)))
        return np.stack(rows), k, None
    return SelectCase(f"bin{d}-S{S}k{k}", S, build, bin_exact=d)


# ---- special values --------------------------------------------------------------------------------------------------------------

P_NAN, N_NAN, P_NAN1 = 0x7FC00000, 0xFFC00000, 0x7F800001
SPECIALS = _bits([P_NAN, N_NAN, P_NAN1, 0x7F800000, 0xFF800000, 0x00000000, 0x80000000, 0x00000001, 0x80000001,
                  0x007FFFFF, 0x807FFFFF, 0x7F7FFFFF, 0xFF7FFFFF])


def specials8(k: int, which: int):
    def build():
        if which == 0:  # -0.0 in front of +0.0; both NaNs, both infinities, both smallest subnormals
            h = _bits([0x80000000, 0x00000000, N_NAN, P_NAN, 0xFF800000, 0x7F800000, 0x00000001, 0x80000001])
        else:           # zeros of both signs over negative values: the cut falls among the zeros
            h = np.concatenate([_bits([0x80000000, 0x00000000, 0x00000000, 0x80000000]), np.float32([-1, -1, -2, -3])])
        return h[None].copy(), k, None
    return SelectCase(f"specials8-{which}-k{k}", 8, build)


def specials_wide(S: int, k: int, seed: int):
    """Every special value twice among S small normal values of both signs (so the zeros and subnormals lie mid-row in the order)."""
    def build():
        rng = np.random.default_rng(seed)
        h = (1e-3 * rng.standard_normal((2, S))).astype(np.float32)
        for b in range(2):
            pos = rng.choice(S, 2 * len(SPECIALS), replace=False)
            h[b, pos] = np.concatenate([SPECIALS, SPECIALS])
        return h, k, None
    return SelectCase(f"specials-S{S}k{k}", S, build)


# ---- widths and selection sizes, tie-free ---------------------------------------------------------------------------------------------


def width(S: int, k: int):
    def build():
        rng = np.random.default_rng(1000 * S + k)
        # (S float32 normals collide now and then: draw twice as many, keep S different ones, in random order)
        h = np.stack([rng.permutation(np.unique(rng.standard_normal(2 * S + 8).astype(np.float32)))[:S] for _ in range(3)])
        return h, k, None
    return SelectCase(f"w{S}k{k}", S, build, tie_free=True)


# ---- ties across the compaction's trips -------------------------------------------------------------------------------------------


def all_equal(S: int, k: int, run_out: bool):
    def build():
        h = np.stack([np.full(S, 1.0, dtype=np.float32), _bits(np.full(S, 0x80000000, dtype=np.uint32))])  # 1.0s; -0.0s
        return h, k, None
    return SelectCase(f"alleq-S{S}k{k}", S, build, tie_trips=True, ties_run_out=run_out)


def ties_then_greater():
    """S = 2052, k = 1030: the cut value 1.0 at 0 .. 1099 but for two places, strictly greater elements at 5 (first trip), 1050 (second
    trip, behind the last kept tie at 1026), 1500 and 2051 (third trip); 0.5 elsewhere.  1026 ties are kept: 0 .. 1026 without 5."""
    def build():
        h = np.full((1, 2052), 0.5, dtype=np.float32)
        h[0, :1100] = 1.0
        h[0, [5, 1050, 1500, 2051]] = [2.0, 3.0, 4.0, 5.0]
        return h, 1030, None
    return SelectCase("ties-then-greater", 2052, build, tie_trips=True, ties_run_out=True)


def ties_over_border():
    """S = 1028: ties at 1020 .. 1027 of which 6 are kept (1020 .. 1025: two in the second trip), 27 greater elements in front."""
    def build():
        h = np.full((1, 1028), -2.0, dtype=np.float32)
        h[0, 1020:] = -1.0
        h[0, 100:127] = np.arange(27, dtype=np.float32)
        return h, 33, None
    return SelectCase("ties-over-border", 1028, build, tie_trips=True, ties_run_out=True)


# ---- masks -------------------------------------------------------------------------------------------------------------------------


def masked(S: int, k: int, eligible: int, seed: int, tag: str = ""):
    """Random values with +inf, +NaN and the five largest finite values masked out; `eligible` latents carry the mask words
    1, -1, 2 in turn."""
    def build():
        rng = np.random.default_rng(seed)
        h = rng.standard_normal((2, S)).astype(np.float32)
        out = rng.choice(S, min(7, S - eligible), replace=False)
        big = _bits([0x7F800000, P_NAN]).tolist() + [50.0, 60.0, 70.0, 80.0, 90.0]
        h[:, out] = np.float32(big[:len(out)])
        ok = np.setdiff1d(np.arange(S), out)
        on = rng.choice(ok, eligible, replace=False)
        mask = np.zeros(S, dtype=np.int32)
        mask[on] = np.resize(np.int32([1, -1, 2]), eligible)
        return h, k, mask
    return SelectCase(f"mask{tag}-S{S}k{k}e{eligible}", S, build, eligible=eligible)


def masked_all_equal():
    """All-equal rows of 2 052 with every other latent eligible (1 026) and k = 1 030: the eligible ones run out in the third trip."""
    def build():
        h = np.full((2, 2052), 3.0, dtype=np.float32)
        mask = np.zeros(2052, dtype=np.int32)
        mask[::2] = 1
        return h, 1030, mask
    return SelectCase("mask-alleq-S2052k1030e1026", 2052, build, eligible=1026)


def _select_cases():
    out = []
    # byte passes: the k-th and (k+1)-th key part in byte p, both signs; two widths of work (2 threads; 257 threads -> a second trip)
    for p in range(4):
        for sign in (False, True):
            out.append(byte_pass(p, sign, 8, 3, seed=10 * p + sign))
            out.append(byte_pass(p, sign, 1028, 65, seed=100 + 10 * p + sign))
    for p in range(4):
        for d in (0x00, 0xFF):
            out.append(digit_edge(p, d, 1028, 100, seed=200 + 10 * p + (d & 1)))
    for d, S, k in ((0, 1028, 1028), (3, 1028, 1020), (132, 1028, 33), (135, 1028, 64), (252, 1028, 2), (255, 1028, 1), (255, 8, 7)):
        out.append(bin_edge(d, S, k, seed=300 + d))
    for which in (0, 1):
        for k in range(1, 9):
            out.append(specials8(k, which))
    for k in (13, 100, 510, 1019):
        out.append(specials_wide(1020, k, seed=400 + k))
    for S in WIDTHS:
        for k in sorted({k for k in KS + (S - 1, S) if 1 <= k <= S}):
            out.append(width(S, k))
    out += [all_equal(2052, 1030, True), all_equal(16388, 1030, True), all_equal(16388, 16388, False), all_equal(1028, 1028, False),
            ties_then_greater(), ties_over_border()]
    for S, k in ((1028, 33), (8, 3)):
        for e in (k + 1, k, k - 1, 0):
            out.append(masked(S, k, e, seed=500 + S + e))
    out += [masked(1028, 65, 1, seed=600), masked(2052, 1030, 1029, seed=601), masked_all_equal()]
    ids = [c.id for c in out]
    assert len(set(ids)) == len(ids)
    return tuple(out)


SELECT_CASES = _select_cases()
SELECT_WIDTHS = tuple(sorted({c.S for c in SELECT_CASES}))


def is_short(case: SelectCase, k: int) -> bool:
    """Fewer eligible latents than k: the case goes through the C entry with caller-owned, pre-filled outputs."""
    return case.eligible is not None and case.eligible < k


# ---- decode ------------------------------------------------------------------------------------------------------------------------

DEC_S = 64
DEC_D = (4, 36, 252, 256, 260, 516, 772, 1028, 1536, 1664, 2048, 2560, 3584, 4092, 4096)   # 516, 772, 1028: NV 3, 4, 5 with one float4 in the last group
DEC_NV = (1, 1, 1, 1, 2, 3, 4, 5, 6, 8, 8, 12, 16, 16, 16)   # the template dispatch_nv picks (sparse.hip)
DEC_K = (1, 63, 64, 65, 130)
DEC_N = (1, 3, 4, 5)
DEC_PREFIXES = ((1, DEC_S), (DEC_S,), (5, 6, DEC_S), (1, 2, 3, 5, 8, 13, 21, 22, 23, 30, 40, 41, 50, 60, 63, DEC_S))


def dispatch_nv(D: int) -> int:
    """sparse.hip: dispatch_nv."""
    nv = (D // 4 + 63) // 64
    return nv if nv <= 6 else 8 if nv <= 8 else 12 if nv <= 12 else 16


@dataclasses.dataclass(frozen=True)
class DecodeCase:
    D: int
    k: int
    n: int
    prefixes: tuple
    seed: int

    @property
    def id(self) -> str:
        return f"D{self.D}k{self.k}n{self.n}p{len(self.prefixes)}"


def decode_cases(D: int):
    i = DEC_D.index(D)
    return tuple(DecodeCase(D, k, DEC_N[(i + j) % 4], DEC_PREFIXES[(i + 2 * j + j // 2) % 4], seed=31 * i + j) for j, k in enumerate(DEC_K))


def decode_params(D: int):
    """(W_dec (S, D), b_dec (D,)) float32 of the decode cases at this width."""
    rng = np.random.default_rng(7000 + D)
    return rng.standard_normal((DEC_S, D)).astype(np.float32), rng.standard_normal(D).astype(np.float32)


def decode_codes(c: DecodeCase):
    """(idx int32, val float32), (n, k): latents in no order, 0 and S - 1 and a duplicate among them; -1 slots first, last and in
    the middle (k = 1: the first batch row is a -1 slot when there is a second)."""
    rng = np.random.default_rng(c.seed)
    idx = rng.integers(0, DEC_S, (c.n, c.k)).astype(np.int32)
    val = rng.standard_normal((c.n, c.k)).astype(np.float32)
    if c.k >= 8:
        idx[:, 1], idx[:, 2], idx[:, 3], idx[:, 4] = 0, DEC_S - 1, 17, 17
        idx[:, 0] = idx[:, c.k // 2] = idx[:, -1] = -1
        if c.k > 64:
            idx[:, 63] = idx[:, 64] = -1  # both sides of the 64-code chunk border
    elif c.n > 1:
        idx[0, 0] = -1
    return idx, val


def without_pads(idx, val):
    """One batch row's codes with the -1 slots removed (at least one slot stays)."""
    keep = idx >= 0
    if not keep.any():
        return idx[:1], val[:1]
    return idx[keep], val[keep]


# ---- scatter, gather, encode -------------------------------------------------------------------------------------------------------

SCATTER_CASES = ((1, 1, 8), (1, 257, 1028), (257, 1, 8), (65537, 1, 8))  # (n, k, S): n k = 1, 257, 257, 65 537 (a 257th workgroup holding one code)


def scatter_codes(n: int, k: int, S: int):
    """Distinct latents per row, with -1 and S (both dropped) among them."""
    rng = np.random.default_rng(n * 131 + k)
    idx = np.stack([rng.permutation(S + 2)[:k] - 1 for _ in range(n)]).astype(np.int32) if k > 1 else rng.integers(-1, S + 1, (n, 1)).astype(np.int32)
    val = rng.standard_normal((n, k)).astype(np.float32)
    if n * k > 1:
        idx.flat[0], idx.flat[-1] = -1, S
    return idx, val


GATHER_D = (4, 252, 256, 260, 4096)
GATHER_N = (1, 3, 4, 5, 1027)
GATHER_POOL_ROWS = 37


def gather_inputs(D: int, n: int):
    rng = np.random.default_rng(D + n)
    pool = rng.standard_normal((GATHER_POOL_ROWS, D)).astype(np.float32)
    rows = rng.integers(0, GATHER_POOL_ROWS, n).astype(np.int64)
    rows[0] = GATHER_POOL_ROWS - 1
    if n > 2:
        rows[1], rows[2] = 0, 0
    return pool, rows


def encode_rows():
    """The distinct (d_model, d_sae) of step_restatement.SHAPES, each with the first row that has it."""
    from step_restatement import SHAPES

    seen, out = set(), []
    for row in SHAPES:
        if (row.d, row.s) not in seen:
            seen.add((row.d, row.s))
            out.append(row)
    return tuple(out)
