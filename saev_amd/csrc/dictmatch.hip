// Dictionary match: for every row a_i of A (Sa, D) its nearest neighbour among the rows b_j of B (Sb, D) by cosine similarity,
//     value[i] = max_j s_ij,  index[i] = the smallest j that attains it,  s_ij = c_ij or |c_ij|,  c_ij = <a_i, b_j> / (||a_i|| ||b_j||),
// without an Sa x Sb product in memory.  Self mode (B absent) matches A against itself with the pair j == i excluded.  It is the
// per-row form of coherence.hip's scheme and shares that file's prepare pass and pair bound (kernels.h).  The entry point is
// saev_dictionary_match (include/saev_amd.h: DICTIONARY MATCH); DESIGN.md 3.16 has the proof and the numbers.
//
//   prepare   coherence.hip's, once per operand: fp32 norms, fp16 images h = fp16(2^13 w^), the bounds {||w^||, ||d||} per row.
//   pass 1    fp16 MFMA over all (I, J) tiles (128 rows of A x 128 rows of B): per pair c~ and E_ij; per (row i, tile J) the largest
//             s~ + E is stored, the largest s~ - E is raised into L_i (integer max on a monotone key).
//   pass 2    the tiles in which some row has max(s~ + E) >= L_i again: every pair with s~ + E >= L_i goes into the candidate list.
//   refine    each candidate's dot product of the fp32 rows a^_i, b^_j in a fixed k order, raised into best[i] as the integer
//             (value key, ~j): the largest value, then the smallest j, whatever order the list is in.
//   exact     fp32 MFMA (v_mfma_f32_32x32x2_f32) over every tile into the same best[i]: the caller's "exact" route, or the fallback
//             when the list overflowed (its kernel exits at once otherwise).
//   finalize  value and index per row; NaN for a row that meets a row whose normalised form is not finite.
//
// Both MFMA kernels put the rows of B on the M side and the rows of A on the N side of the product: in the 32x32 accumulator layout
// a lane then holds 16 B rows of ONE A row per block, so every per-A-row reduction is in-lane plus one shuffle across the halves.
#include "common.h"
#include "kernels.h"

#include <algorithm>

namespace {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));
typedef unsigned long long u64;

constexpr int CT = COH_TILE;          // tile edge: 128 rows of A by 128 rows of B
constexpr int CK = COH_KSTAGE;        // k per LDS stage of the fp16 filter (64)
constexpr int CLDS = CK + 8;          // (+8 fp16 of padding: row pitch 144 B, ds_read_b128 conflict-free)
constexpr int XK = 32;                // k per LDS stage of the fp32 exact route
constexpr int XLDS = XK + 4;          // (row pitch 144 B)

// control words (uint32) at the start of the workspace
constexpr int CTL_NAN_A = 0;  // ~(first row of A whose normalised form is not finite), 0: none
constexpr int CTL_NAN_B = 1;  // the same for B (self mode: unused, B's word is A's)
constexpr int CTL_TILES = 2;  // tiles pass 2 recomputed
constexpr int CTL_CNT = 4;    // (uint64 at words 4-5) candidates pass 2 found, also those past the capacity

struct DmDev {
    const float* A;
    const float* B;           // self mode: A
    int Sa, Sb, D, Dp, Sap, nTA, cap, route, self, absolute;
    long ntiles;
    float gam;                // accumulation term of the bound (pass 1 and refine together)
    const float* nrmA;        // (Sa) fp32 row norms
    const float* nrmB;
    const float2* rnA;        // (Sa) {||a^_i||, ||d_i||}, both rounded up
    const float2* rnB;
    const uint16_t* imgA;     // (Sap, Dp) fp16 image, zero past Sa rows and D columns
    const uint16_t* imgB;
    uint32_t* ctl;
    uint32_t* Lkey;           // (Sap) f2ukey of L_i = max_j s~_ij - E_ij
    u64* best;                // (Sa) f2ukey(value) << 32 | ~j, 0: none yet
    float* hi;                // (nTB, Sap) max over the tile's columns of s~ + E
    int2* cand;               // (cap) {i, j}
};

__device__ __forceinline__ u64 cand_count(const uint32_t* ctl) { return *reinterpret_cast<const u64*>(ctl + CTL_CNT); }

// fp16 filter.  PASS 1: per (row, tile) max of s~ + E (stored) and s~ - E (into L_i); PASS 2: the tiles that can hold a row's
// maximum, every pair with s~ + E >= L_i appended to the candidate list (one atomic per wave).  128 x 128 tile per workgroup, four
// waves of 64 x 64 (2 x 2 v_mfma_f32_32x32x16_f16), k in stages of 64 through LDS with the next stage's global loads issued before
// the MFMAs: coherence.hip's filter on a rectangle, with the rows of A on the accumulator's columns.
template <int PASS>
__global__ __launch_bounds__(256, 2) void dm_filter_kernel(DmDev a) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) uint16_t As[CT][CLDS];
    __shared__ __attribute__((aligned(16))) uint16_t Bs[CT][CLDS];
    __shared__ float2 rA[CT], rB[CT];
    __shared__ float red[2][2][CT];  // pass 1: [lo, hi][wave row][row of A]; pass 2: red[0][0] holds L_i of the tile's rows
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int wm = (w >> 1) * 64, wn = (w & 1) * 64;  // wm: rows of B, wn: rows of A
    const int r32 = lane & 31, h = lane >> 5;
    const int ar = t >> 3, ac = (t & 7) * 8;  // load slots: rows ar + 32 q (q < 4), 8 fp16 at ac
    for (long tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
        const int It = (int)(tile % a.nTA), Jt = (int)(tile / a.nTA);
        __syncthreads();  // the previous tile's epilogue has read rA / rB / red
        bool live = false;
        if (t < CT) {
            const int gi = It * CT + t;
            rA[t] = gi < a.Sa ? a.rnA[gi] : make_float2(0.f, 0.f);
            if (PASS == 2) {
                const float L = gi < a.Sa ? ukey2f(a.Lkey[gi]) : __builtin_nanf("");  // (key 0, no finite pair: NaN, nothing passes)
                red[0][0][t] = L;
                live = gi < a.Sa && a.hi[(size_t)Jt * a.Sap + gi] >= L;
            }
        } else {
            const int gj = Jt * CT + (t - CT);
            rB[t - CT] = gj < a.Sb ? a.rnB[gj] : make_float2(0.f, 0.f);
        }
        if (PASS == 2 && !__syncthreads_or(live)) continue;  // (workgroup-uniform)
        const uint16_t* Ag = a.imgA + (size_t)It * CT * a.Dp;
        const uint16_t* Bg = a.imgB + (size_t)Jt * CT * a.Dp;
        u16x8 ra[4], rb[4];
        auto load = [&](int k0) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                ra[q] = *reinterpret_cast<const u16x8*>(Ag + (size_t)(ar + 32 * q) * a.Dp + k0 + ac);
                rb[q] = *reinterpret_cast<const u16x8*>(Bg + (size_t)(ar + 32 * q) * a.Dp + k0 + ac);
            }
        };
        f32x16 acc[2][2];  // [block of B rows][block of A rows]
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
        load(0);
        for (int k0 = 0; k0 < a.Dp; k0 += CK) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                *reinterpret_cast<u16x8*>(&As[ar + 32 * q][ac]) = ra[q];
                *reinterpret_cast<u16x8*>(&Bs[ar + 32 * q][ac]) = rb[q];
            }
            __syncthreads();
            if (k0 + CK < a.Dp) load(k0 + CK);
#pragma unroll
            for (int ks = 0; ks < CK; ks += 16) {
                half8 fa[2], fb[2];
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    fb[i] = __builtin_bit_cast(half8, *reinterpret_cast<const u16x8*>(&Bs[wm + 32 * i + r32][ks + 8 * h]));
                    fa[i] = __builtin_bit_cast(half8, *reinterpret_cast<const u16x8*>(&As[wn + 32 * i + r32][ks + 8 * h]));
                }
#pragma unroll
                for (int ib = 0; ib < 2; ++ib)
#pragma unroll
                    for (int ia = 0; ia < 2; ++ia)
                        acc[ib][ia] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fb[ib], fa[ia], acc[ib][ia], 0, 0, 0);
            }
            __syncthreads();
        }
        // C/D map of 32x32x16: column (a row of A) = lane & 31, row (a row of B) = (r & 3) + 8 (r >> 2) + 4 h
        if constexpr (PASS == 1) {
#pragma unroll
            for (int ia = 0; ia < 2; ++ia) {
                const int n = wn + 32 * ia + r32, gi = It * CT + n;
                const float2 bi = rA[n];
                float lo = NEG_INF, hi = NEG_INF;
#pragma unroll
                for (int ib = 0; ib < 2; ++ib)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int m = wm + 32 * ib + (r & 3) + 8 * (r >> 2) + 4 * h, gj = Jt * CT + m;
                        if (gj < a.Sb && !(a.self && gi == gj)) {
                            float c = acc[ib][ia][r] * COH_IMG_UNSCALE;
                            if (a.absolute) c = fabsf(c);
                            const float e = coh_pair_bound(bi, rB[m], a.gam);
                            lo = fmaxf(lo, c - e);  // (a NaN pair raises neither)
                            hi = fmaxf(hi, c + e);
                        }
                    }
                lo = fmaxf(lo, __shfl_xor(lo, 32, 64));
                hi = fmaxf(hi, __shfl_xor(hi, 32, 64));
                if (h == 0) { red[0][w >> 1][n] = lo; red[1][w >> 1][n] = hi; }
            }
            __syncthreads();
            if (t < CT && It * CT + t < a.Sa) {
                const int gi = It * CT + t;
                a.hi[(size_t)Jt * a.Sap + gi] = fmaxf(red[1][0][t], red[1][1][t]);
                // (the plain read skips the atomic for all but the few tiles that raise L_i; the final value is the max either way)
                const uint32_t key = f2ukey(fmaxf(red[0][0][t], red[0][1][t]));
                if (key > __hip_atomic_load(&a.Lkey[gi], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&a.Lkey[gi], key);
            }
        } else {
            u64 keep = 0;  // bit 32 ia + 16 ib + r: this element is a candidate
            int cnt = 0;
#pragma unroll
            for (int ia = 0; ia < 2; ++ia) {
                const int n = wn + 32 * ia + r32, gi = It * CT + n;
                const float2 bi = rA[n];
                const float L = red[0][0][n];
#pragma unroll
                for (int ib = 0; ib < 2; ++ib)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int m = wm + 32 * ib + (r & 3) + 8 * (r >> 2) + 4 * h, gj = Jt * CT + m;
                        if (gj < a.Sb && !(a.self && gi == gj)) {
                            float c = acc[ib][ia][r] * COH_IMG_UNSCALE;
                            if (a.absolute) c = fabsf(c);
                            if (c + coh_pair_bound(bi, rB[m], a.gam) >= L) { keep |= 1ull << (32 * ia + 16 * ib + r); ++cnt; }
                        }
                    }
            }
            int incl = cnt;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int v = __shfl_up(incl, o, 64);
                if (lane >= o) incl += v;
            }
            const int tot = __shfl(incl, 63, 64);
            if (tot > 0) {  // (wave-uniform)
                u64 base = 0;
                if (lane == 63) base = atomicAdd(reinterpret_cast<u64*>(a.ctl + CTL_CNT), (u64)tot);
                const uint32_t blo = __shfl((uint32_t)base, 63, 64), bhi = __shfl((uint32_t)(base >> 32), 63, 64);
                u64 slot = (((u64)bhi << 32) | blo) + (u64)(incl - cnt);
                for (; keep != 0; keep &= keep - 1, ++slot) {
                    const int b = __builtin_ctzll(keep), ia = b >> 5, ib = (b >> 4) & 1, r = b & 15;
                    if (slot < (u64)a.cap)
                        a.cand[slot] = make_int2(It * CT + wn + 32 * ia + r32, Jt * CT + wm + 32 * ib + (r & 3) + 8 * (r >> 2) + 4 * h);
                }
            }
            if (t == 0) atomicAdd(&a.ctl[CTL_TILES], 1u);
        }
    }
}

// exact refinement: one wave per candidate, sum_k (a_ik / n_i)(b_jk / n_j) as fmas in k order per lane (k = 4 q + e, q = lane
// mod 64), then the xor butterfly -- the value depends on (i, j), A and B only, not on the candidate's place in the list; the row's
// result is an integer max on (value key, ~j), so the order of the list cannot show
__global__ __launch_bounds__(256) void dm_refine_kernel(DmDev a) {
#pragma clang fp contract(off)
    const u64 n = cand_count(a.ctl);
    if (n > (u64)a.cap) return;  // overflow: the exact route answers
    const int lane = threadIdx.x & 63;
    const int nq = a.D >> 2;
    for (long c = (long)blockIdx.x * 4 + (threadIdx.x >> 6); c < (long)n; c += (long)gridDim.x * 4) {
        const int2 pr = a.cand[c];
        const float ni = a.nrmA[pr.x], nj = a.nrmB[pr.y];
        const f32x4* wi = reinterpret_cast<const f32x4*>(a.A + (size_t)pr.x * a.D);
        const f32x4* wj = reinterpret_cast<const f32x4*>(a.B + (size_t)pr.y * a.D);
        float s = 0.f;
        for (int q = lane; q < nq; q += 64) {
            const f32x4 x = wi[q], y = wj[q];
#pragma unroll
            for (int e = 0; e < 4; ++e) s = __builtin_fmaf(x[e] / ni, y[e] / nj, s);
        }
        s = wave_sum(s);
        if (a.absolute) s = fabsf(s);
        if (lane == 0 && s == s) atomicMax(&a.best[pr.x], ((u64)f2ukey(s) << 32) | (uint32_t)~(uint32_t)pr.y);
    }
}

// exact route: fp32 MFMA (v_mfma_f32_32x32x2_f32) on a^ and b^, divided on the way into LDS; per row of A and tile the best
// (value key, ~j), raised into best[i]
__global__ __launch_bounds__(256, 2) void dm_exact_kernel(DmDev a) {
    if (a.route != SAEV_MATCH_EXACT && !(cand_count(a.ctl) > (u64)a.cap)) return;
    __shared__ __attribute__((aligned(16))) float As[CT][XLDS];
    __shared__ __attribute__((aligned(16))) float Bs[CT][XLDS];
    __shared__ float nA[CT], nB[CT];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int wm = (w >> 1) * 64, wn = (w & 1) * 64;  // wm: rows of B, wn: rows of A
    const int r32 = lane & 31, h = lane >> 5;
    const int ar = t >> 3, ac = (t & 7) * 4;  // load slots: rows ar + 32 q (q < 4), 4 floats at ac
    for (long tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
        const int It = (int)(tile % a.nTA), Jt = (int)(tile / a.nTA);
        __syncthreads();  // the previous tile's stages have read nA / nB
        {
            const int rr = (t < CT ? It : Jt) * CT + (t & (CT - 1));
            if (t < CT) nA[t] = rr < a.Sa ? a.nrmA[rr] : 1.f; else nB[t - CT] = rr < a.Sb ? a.nrmB[rr] : 1.f;
        }
        __syncthreads();
        f32x4 ra[4], rb[4];
        auto load = [&](int k0) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int k = k0 + ac, ri = It * CT + ar + 32 * q, rj = Jt * CT + ar + 32 * q;
                ra[q] = (k < a.D && ri < a.Sa) ? *reinterpret_cast<const f32x4*>(a.A + (size_t)ri * a.D + k) : f32x4{0.f, 0.f, 0.f, 0.f};
                rb[q] = (k < a.D && rj < a.Sb) ? *reinterpret_cast<const f32x4*>(a.B + (size_t)rj * a.D + k) : f32x4{0.f, 0.f, 0.f, 0.f};
            }
        };
        f32x16 acc[2][2];  // [block of B rows][block of A rows]
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
        load(0);
        for (int k0 = 0; k0 < a.D; k0 += XK) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float ni = nA[ar + 32 * q], nj = nB[ar + 32 * q];
                f32x4 x, y;
#pragma unroll
                for (int e = 0; e < 4; ++e) { x[e] = ra[q][e] / ni; y[e] = rb[q][e] / nj; }
                *reinterpret_cast<f32x4*>(&As[ar + 32 * q][ac]) = x;
                *reinterpret_cast<f32x4*>(&Bs[ar + 32 * q][ac]) = y;
            }
            __syncthreads();
            if (k0 + XK < a.D) load(k0 + XK);
#pragma unroll
            for (int kc = 0; kc < XK; kc += 8) {
                f32x4 fa[2], fb[2];
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    fb[i] = *reinterpret_cast<const f32x4*>(&Bs[wm + 32 * i + r32][kc + 4 * h]);
                    fa[i] = *reinterpret_cast<const f32x4*>(&As[wn + 32 * i + r32][kc + 4 * h]);
                }
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int ib = 0; ib < 2; ++ib)
#pragma unroll
                        for (int ia = 0; ia < 2; ++ia)
                            acc[ib][ia] = __builtin_amdgcn_mfma_f32_32x32x2f32(fb[ib][e], fa[ia][e], acc[ib][ia], 0, 0, 0);
            }
            __syncthreads();
        }
#pragma unroll
        for (int ia = 0; ia < 2; ++ia) {
            const int gi = It * CT + wn + 32 * ia + r32;
            u64 bk = 0;
#pragma unroll
            for (int ib = 0; ib < 2; ++ib)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int gj = Jt * CT + wm + 32 * ib + (r & 3) + 8 * (r >> 2) + 4 * h;
                    float v = acc[ib][ia][r];
                    if (a.absolute) v = fabsf(v);
                    if (gi < a.Sa && gj < a.Sb && !(a.self && gi == gj) && v == v) {
                        const u64 k = ((u64)f2ukey(v) << 32) | (uint32_t)~(uint32_t)gj;
                        bk = k > bk ? k : bk;
                    }
                }
            const uint32_t olo = __shfl_xor((uint32_t)bk, 32, 64), ohi = __shfl_xor((uint32_t)(bk >> 32), 32, 64);
            const u64 ok = ((u64)ohi << 32) | olo;
            bk = ok > bk ? ok : bk;
            if (h == 0 && bk != 0) atomicMax(&a.best[gi], bk);
        }
    }
}

// the result per row of A, and info = {route taken, candidates found, tiles pass 2 recomputed, list capacity}
__global__ __launch_bounds__(256) void dm_finalize_kernel(DmDev a, float* out_value, int32_t* out_index, int32_t* out_info) {
    const bool none = a.self && a.Sa < 2;  // no admissible pair
    const u64 n = none ? 0ull : cand_count(a.ctl);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const bool over = n > (u64)a.cap;
        out_info[0] = a.route == SAEV_MATCH_EXACT ? SAEV_MATCH_EXACT : (over ? SAEV_MATCH_OVERFLOW : SAEV_MATCH_FILTERED);
        out_info[1] = n > 0x7fffffffull ? 0x7fffffff : (int32_t)n;
        out_info[2] = none ? 0 : (int32_t)a.ctl[CTL_TILES];
        out_info[3] = a.cap;
    }
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.Sa) return;
    float v = __builtin_nanf("");
    int32_t j = -1;
    if (none) {
        v = 0.f;
    } else if (!(a.rnA[i].x <= 3.0e38f)) {  // a^_i is not finite: every pair is NaN, the smallest admissible j
        j = (a.self && i == 0) ? 1 : 0;
    } else if (a.ctl[a.self ? CTL_NAN_A : CTL_NAN_B] != 0) {  // (self mode: not row i itself, which is finite)
        j = (int32_t)~a.ctl[a.self ? CTL_NAN_A : CTL_NAN_B];
    } else if (a.best[i] != 0) {
        v = ukey2f((uint32_t)(a.best[i] >> 32));
        j = (int32_t)~(uint32_t)a.best[i];
    }
    out_value[i] = v;
    out_index[i] = j;
}

long round_up(long v, long m) { return (v + m - 1) / m * m; }

int persistent_grid(long work) {
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    return (int)std::max<long>(1, std::min<long>(work, 2L * cus));
}

}  // namespace

DmLayout dictmatch_layout(long Sa, long Sb, int D) {
    DmLayout L{};
    L.Sap = (int)round_up(Sa, CT);
    L.Sbp = (int)round_up(Sb, CT);
    L.Dp = (int)round_up(D, CK);
    L.nTA = L.Sap / CT;
    L.nTB = L.Sbp / CT;
    L.ntiles = (long)L.nTA * L.nTB;
    L.cap = (int)std::max<long>(1, std::min<long>(Sa * Sb, std::max<long>(DM_CAND_MIN, DM_CAND_PER_ROW * Sa)));
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += (bytes + 255) / 256 * 256; return o; };
    L.off_ctl = take(64);
    L.off_L = take((size_t)L.Sap * 4);
    L.off_best = take((size_t)Sa * 8);
    L.zero_bytes = off;
    L.off_nrmA = take((size_t)Sa * 4);
    L.off_rnA = take((size_t)Sa * 8);
    L.off_imgA = take((size_t)L.Sap * L.Dp * 2);
    L.off_nrmB = take((size_t)Sb * 4);
    L.off_rnB = take((size_t)Sb * 8);
    L.off_imgB = take((size_t)L.Sbp * L.Dp * 2);
    L.off_hi = take((size_t)L.nTB * L.Sap * 4);
    L.off_cand = take((size_t)L.cap * 8);
    L.bytes = off;
    return L;
}

hipError_t launch_dictmatch(const float* A, int Sa, const float* B, int Sb, int D, int absolute, int route, uint8_t* ws,
                            const DmLayout& L, float* out_value, int32_t* out_index, int32_t* out_info, hipStream_t s) {
    const bool self = B == nullptr;
    DmDev a{};
    a.A = A; a.B = self ? A : B; a.Sa = Sa; a.Sb = self ? Sa : Sb; a.D = D; a.Dp = L.Dp; a.Sap = L.Sap; a.nTA = L.nTA;
    a.cap = L.cap; a.route = route; a.self = self; a.absolute = absolute != 0; a.ntiles = L.ntiles;
    a.gam = coh_gamma(L.Dp);
    a.ctl = reinterpret_cast<uint32_t*>(ws + L.off_ctl);
    a.Lkey = reinterpret_cast<uint32_t*>(ws + L.off_L);
    a.best = reinterpret_cast<u64*>(ws + L.off_best);
    a.hi = reinterpret_cast<float*>(ws + L.off_hi);
    a.cand = reinterpret_cast<int2*>(ws + L.off_cand);
    float* nrmA = reinterpret_cast<float*>(ws + L.off_nrmA);
    float2* rnA = reinterpret_cast<float2*>(ws + L.off_rnA);
    uint16_t* imgA = reinterpret_cast<uint16_t*>(ws + L.off_imgA);
    float* nrmB = self ? nrmA : reinterpret_cast<float*>(ws + L.off_nrmB);
    float2* rnB = self ? rnA : reinterpret_cast<float2*>(ws + L.off_rnB);
    uint16_t* imgB = self ? imgA : reinterpret_cast<uint16_t*>(ws + L.off_imgB);
    a.nrmA = nrmA; a.rnA = rnA; a.imgA = imgA; a.nrmB = nrmB; a.rnB = rnB; a.imgB = imgB;
    hipError_t e = hipMemsetAsync(ws + L.off_ctl, 0, L.zero_bytes, s);
    if (e != hipSuccess) return e;
    if (!(self && Sa < 2)) {
        e = launch_coh_prepare(A, Sa, D, L.Sap, L.Dp, nrmA, rnA, imgA, a.ctl + CTL_NAN_A, s);
        if (e != hipSuccess) return e;
        if (!self) {
            e = launch_coh_prepare(B, Sb, D, L.Sbp, L.Dp, nrmB, rnB, imgB, a.ctl + CTL_NAN_B, s);
            if (e != hipSuccess) return e;
        }
        const int grid = persistent_grid(L.ntiles);
        if (route == SAEV_MATCH_AUTO) {
            hipLaunchKernelGGL(dm_filter_kernel<1>, dim3(grid), dim3(256), 0, s, a);
            hipLaunchKernelGGL(dm_filter_kernel<2>, dim3(grid), dim3(256), 0, s, a);
            hipLaunchKernelGGL(dm_refine_kernel, dim3((int)std::min<long>((L.cap + 3) / 4, 2048)), dim3(256), 0, s, a);
        }
        hipLaunchKernelGGL(dm_exact_kernel, dim3(grid), dim3(256), 0, s, a);
    }
    hipLaunchKernelGGL(dm_finalize_kernel, dim3((Sa + 255) / 256), dim3(256), 0, s, a, out_value, out_index, out_info);
    return hipGetLastError();
}
