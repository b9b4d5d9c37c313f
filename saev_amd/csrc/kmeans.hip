// Mini-batch k-means (the reference's default baseline, tdiscovery/baselines.py MiniBatchKMeans): the four device stages of one
// partial_fit without an n x k or k x k distance matrix in memory.  Entry points: saev_kmeans_assign / _group / _update / _collapsed
// (include/saev_amd.h: K-MEANS); DESIGN.md 3.18 has the bound, its proof and the numbers.
//
//   the refined value   r_ij = fp32 sum over k = 0 .. D-1, in that order, of (x_ik - c_jk)^2, uncontracted: km_acc4 is the one
//                       function that forms it, four k at a time; the refinement, the exact routes and the pair test all call it.
//   assign    per row of X the smallest (farthest != 0: the largest) r_ij and the smallest j attaining it.  Route AUTO is
//             dictmatch.hip's scheme with a bound for squared distances: X and C are centred on the mean of the centres (fp32
//             copies in the workspace), coherence.hip's prepare pass gives their unit-row fp16 images, an fp16 MFMA pass over all
//             128 x 128 tiles gives per pair s~_ij and E_ij >= |s~_ij - r_ij| (km_pair, evaluated in fp64) and per row the bound
//             L_i; a second pass over the tiles that can hold a candidate writes the list; each candidate is recomputed with
//             km_acc4 and raised into best[i] by an integer max on (key(value), ~j).  Route EXACT (asked for, or the fallback when
//             the list overflowed or a centred row has no unit image) computes every pair with km_acc4 into the same best[i].
//   group     histogram, exclusive scan, placement, and an in-place ascending sort of each centre's rows: a stable counting
//             sort's result whatever order the placement's atomics came in.
//   update    the running-mean update in place: one thread per (centre, four columns) walks its rows in ascending order.
//   collapsed the same filter in self mode over the upper-triangle tiles with a threshold epilogue; every candidate pair, or on
//             the exact route every pair, is tested with km_acc4 and stores its loser's flag (idempotent).
#include "common.h"
#include "kernels.h"

#include <algorithm>

namespace {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));
typedef unsigned long long u64;

constexpr int CT = COH_TILE;          // tile edge of the filter: 128 rows of X by 128 centres
constexpr int CK = COH_KSTAGE;        // k per LDS stage of the fp16 filter (64)
constexpr int CLDS = CK + 8;          // (+8 fp16 of padding: row pitch 144 B, ds_read_b128 conflict-free)
constexpr int ET = 64;                // tile edge of the exact routes: 64 x 64 pairs, 4 x 4 per thread
constexpr int SORT_LDS = 4096;        // group: segments up to this many rows are sorted in LDS, longer ones compacted from index
constexpr int SORT_CHUNK = 256 * 16;  // group: entries of index per step of that compaction (16 per thread)
constexpr int MU_CHUNKS = 64;         // partial column sums of the centring vector

// control words (uint32) at the start of the workspace
constexpr int CTL_BAD_X = 0;      // coherence.hip's prepare: ~(first centred row of X without a finite unit image), 0: none
constexpr int CTL_BAD_C = 1;      // the same for the centres
constexpr int CTL_TILES = 2;      // tiles the second pass recomputed
constexpr int CTL_NONFINITE = 3;  // 1: X or C holds an inf or a NaN
constexpr int CTL_CNT = 4;        // (uint64 at words 4-5) candidates found, also those past the capacity

constexpr int MODE_PASS1 = 1, MODE_PASS2 = 2, MODE_PAIRS = 3;

struct alignas(8) KmRow {  // what the bound needs of one centred row w' (fp32): see km_pair
    double sq;             // ||w'||^2, summed in fp64
    double rt;             // sqrt(sq)
    float2 rn;             // prepare's {||w^||, ||d||}, both rounded up (w^ = w' / nrm, d = w^ - 2^-13 image)
    float nrm;             // prepare's fp32 norm of w', the divisor of w^
    float pad;
};

struct KmDev {
    const float* X;           // (n, D) the caller's rows; collapsed: the centres
    const float* C;           // (k, D) the caller's centres
    int n, k, D, Dp, np, nTX, nTC, cap, route, far;
    long ntiles;
    float gam;                // accumulation term of the cosine bound (coh_gamma)
    double tau;               // relative error of the refined value: 1.001 (D + 3) 2^-24
    double thr2;              // collapsed: tol^2
    float tol;
    const KmRow* rowX;        // (n)
    const KmRow* rowC;        // (k)
    const uint16_t* imgX;     // (np, Dp) fp16 image of the centred rows, zero past n rows and D columns
    const uint16_t* imgC;
    uint32_t* ctl;
    u64* Lkey;                // (np) d2ukey of L_i = max_j g~_ij - E_ij, g = -s (nearest) or s (farthest)
    u64* best;                // (n) key(value) << 32 | ~j, 0: none yet
    double* hi;               // (nTC, np) max over the tile's centres of g~ + E
    int2* cand;               // (cap) {i, j}
    const float* counts;      // collapsed: cluster_counts
    uint8_t* loser;           // collapsed: out_loser
};

// The refined value, four k at a time: s + (x0 - c0)^2 + ... in this order, every operation rounded once.  Callers pass ascending k.
__device__ __forceinline__ float km_acc4(float s, f32x4 x, f32x4 c) {
#pragma clang fp contract(off)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float d = x[e] - c[e];
        const float p = d * d;
        s = s + p;
    }
    return s;
}
__device__ __forceinline__ float km_r(const float* x, const float* c, int D) {
    const f32x4* x4 = reinterpret_cast<const f32x4*>(x);
    const f32x4* c4 = reinterpret_cast<const f32x4*>(c);
    float s = 0.f;
#pragma unroll 4
    for (int q = 0; q < (D >> 2); ++q) s = km_acc4(s, x4[q], c4[q]);
    return s;
}

// order-preserving double -> uint64 key (larger double, larger key; never 0 for a non-NaN)
__device__ __forceinline__ u64 d2ukey(double d) {
    const u64 b = (u64)__double_as_longlong(d);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double ukey2d(u64 k) {
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}
__device__ __forceinline__ double shfl_xor_d(double v, int o) {
    const long long b = __double_as_longlong(v);
    const uint32_t lo = __shfl_xor((uint32_t)b, o, 64), hi = __shfl_xor((uint32_t)((u64)b >> 32), o, 64);
    return __longlong_as_double((long long)(((u64)hi << 32) | lo));
}
__device__ __forceinline__ u64 shfl_xor_u64(u64 v, int o) {
    const uint32_t lo = __shfl_xor((uint32_t)v, o, 64), hi = __shfl_xor((uint32_t)(v >> 32), o, 64);
    return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 cand_count(const uint32_t* ctl) { return *reinterpret_cast<const u64*>(ctl + CTL_CNT); }
// the filter cannot answer: no unit image of some centred row (a row equal to the centring vector, a norm that leaves fp32)
__device__ __forceinline__ bool no_image(const uint32_t* ctl) { return (ctl[CTL_BAD_X] | ctl[CTL_BAD_C]) != 0; }
__device__ __forceinline__ bool exact_answers(const KmDev& a) {
    return a.route == SAEV_KMEANS_EXACT || no_image(a.ctl) || cand_count(a.ctl) > (u64)a.cap;
}
// the row's result key: nearest keeps the smallest value, farthest the largest, both by an integer max; then the smallest j
__device__ __forceinline__ u64 best_key(float r, int j, int far) {
    const uint32_t v = far ? f2ukey(r) : ~f2ukey(r);
    return ((u64)v << 32) | (uint32_t)~(uint32_t)j;
}

// s~_ij and E_ij >= |s~_ij - r_ij| of one pair from the filter's accumulator (DESIGN.md 3.18 derives every term).  x', c' are the
// centred fp32 rows, x^ = x' / nx and c^ = c' / nc their unit images' sources, c~ = 2^-26 acc the filter's cosine.
//   s~  = ||x'||^2 + ||c'||^2 - 2 nx nc c~
//   E1  = 2 nx nc (E_cos + 1.25e-7 ||x^|| ||c^||) + 1e-12 (||x'||^2 + ||c'||^2)     >= |s~ - ||x' - c'||^2|
//   up  = sqrt(max(s~ + E1, 0))                                                      >= ||x' - c'||
//   rho = 5.97e-8 (||x'|| + ||c'||)                                                  >= | ||x' - c'|| - ||x - c|| |  (centring)
//   dl  = rho (2 up + rho)                                                           >= | ||x' - c'||^2 - ||x - c||^2 |
//   E   = E1 + dl + tau (up^2 + dl), tau = 1.001 (D + 3) 2^-24                       (the fp32 difference form against ||x - c||^2)
// All in fp64 with 1e-9 relative and 1e-30 absolute on top; a non-finite result makes the pair a candidate (the callers compare
// so that a NaN passes).
__device__ __forceinline__ void km_pair(const KmDev& a, float acc, const KmRow& x, const KmRow& c, double* s, double* E) {
    const double ct = (double)(acc * COH_IMG_UNSCALE);
    const double P = (double)x.nrm * (double)c.nrm;
    const double ecos = (double)coh_pair_bound(x.rn, c.rn, a.gam) + 1.25e-7 * (double)x.rn.x * (double)c.rn.x;
    const double ss = x.sq + c.sq;
    const double st = ss - 2.0 * P * ct;
    const double E1 = 2.0 * P * ecos + 1e-12 * ss;
    const double up2 = fmax(st + E1, 0.0);
    const double up = sqrt(up2) * (1.0 + 1e-12);
    const double rho = 5.97e-8 * (x.rt + c.rt);
    const double dl = rho * (2.0 * up + rho);
    *s = st;
    *E = (E1 + dl + a.tau * (up2 + dl)) * (1.0 + 1e-9) + 1e-30;
}

// ---- preparation: finiteness, the centring vector, the centred copies ---------------------------------------------------------
// partial column sums of the centres: chunk b of the rows, thread t the column quads t, t + 256, ...
__global__ __launch_bounds__(256) void km_colsum_kernel(const float* __restrict__ C, int k, int D, int per, float* part) {
    const int r0 = blockIdx.x * per, r1 = min(k, r0 + per);
    for (int q = threadIdx.x; q < (D >> 2); q += 256) {
        f32x4 s = {0.f, 0.f, 0.f, 0.f};
        for (int r = r0; r < r1; ++r) s += *reinterpret_cast<const f32x4*>(C + (size_t)r * D + 4 * q);
        *reinterpret_cast<f32x4*>(part + (size_t)blockIdx.x * D + 4 * q) = s;
    }
}
// mu = the fp32 mean of the centres to a few ulps (any finite vector serves: distances do not depend on it); 0 where not finite
__global__ __launch_bounds__(256) void km_mu_kernel(const float* part, int chunks, int k, int D, float* mu) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= D) return;
    float s = 0.f;
    for (int b = 0; b < chunks; ++b) s += part[(size_t)b * D + c];
    s /= (float)k;
    mu[c] = fabsf(s) <= 3.0e38f ? s : 0.f;
}
// one wave per row: w' = fl(w - mu), ||w'||^2 in fp64, and the finiteness of w itself
__global__ __launch_bounds__(256) void km_center_kernel(const float* __restrict__ W, int S, int D, const float* __restrict__ mu,
                                                        float* Wc, KmRow* row, uint32_t* ctl) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= S) return;
    double sq = 0.0;
    bool bad = false;
    for (int q = lane; q < (D >> 2); q += 64) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(W + (size_t)r * D + 4 * q);
        const f32x4 m = *reinterpret_cast<const f32x4*>(mu + 4 * q);
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            bad |= !(fabsf(v[e]) <= 3.4028234663852886e38f);
            o[e] = v[e] - m[e];
            sq += (double)o[e] * (double)o[e];
        }
        *reinterpret_cast<f32x4*>(Wc + (size_t)r * D + 4 * q) = o;
    }
    sq = wave_sum_d(sq);
    const u64 badm = __ballot(bad);
    if (lane == 0) {
        row[r].sq = sq;
        row[r].rt = sqrt(sq);
        if (badm) ctl[CTL_NONFINITE] = 1u;
    }
}
// prepare's norm and bounds into the row records
__global__ __launch_bounds__(256) void km_rows_kernel(int S, const float* nrm, const float2* rn, KmRow* row) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= S) return;
    row[r].nrm = nrm[r];
    row[r].rn = rn[r];
    row[r].pad = 0.f;
}

// ---- the fp16 filter -----------------------------------------------------------------------------------------------------------
// dictmatch.hip's filter with km_pair as its epilogue: 128 x 128 tile per workgroup, four waves of 64 x 64 (2 x 2
// v_mfma_f32_32x32x16_f16), the centres on the M side and the rows of X on the N side, so that a lane holds 16 centres of ONE row per
// block.  With g = -s (nearest) or s (farthest): PASS1 stores per (row, tile) the largest g~ + E and raises the largest g~ - E into
// L_i; PASS2 revisits the tiles where some row has max(g~ + E) >= L_i and appends every pair with g~ + E >= L_i; PAIRS (collapsed,
// X = C) walks the tiles I <= J once and appends every pair i < j with s~ - E < tol^2.  Every comparison is written so that a NaN
// keeps the pair.
template <int MODE>
__global__ __launch_bounds__(256, 2) void km_filter_kernel(KmDev a) {
#pragma clang fp contract(off)
    if (a.ctl[CTL_NONFINITE] != 0 || no_image(a.ctl)) return;
    __shared__ __attribute__((aligned(16))) uint16_t As[CT][CLDS];
    __shared__ __attribute__((aligned(16))) uint16_t Bs[CT][CLDS];
    __shared__ KmRow rA[CT], rB[CT];
    __shared__ double red[2][2][CT];  // pass 1: [lo, hi][wave row][row of X]; pass 2: red[0][0] holds L_i of the tile's rows
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int wm = (w >> 1) * 64, wn = (w & 1) * 64;  // wm: centres, wn: rows of X
    const int r32 = lane & 31, h = lane >> 5;
    const int ar = t >> 3, ac = (t & 7) * 8;  // load slots: rows ar + 32 q (q < 4), 8 fp16 at ac
    const double sg = a.far ? 1.0 : -1.0;
    const double INF = __builtin_huge_val();
    for (long tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
        const int It = (int)(tile % a.nTX), Jt = (int)(tile / a.nTX);
        if (MODE == MODE_PAIRS && It > Jt) continue;  // (workgroup-uniform)
        __syncthreads();  // the previous tile's epilogue has read rA / rB / red
        bool live = false;
        if (t < CT) {
            const int gi = It * CT + t;
            KmRow z{};
            rA[t] = gi < a.n ? a.rowX[gi] : z;
            if (MODE == MODE_PASS2) {
                const u64 key = gi < a.n ? a.Lkey[gi] : 0ull;
                const double L = key != 0 ? ukey2d(key) : -INF;  // (no key: everything of the row stays)
                red[0][0][t] = L;
                live = gi < a.n && !(a.hi[(size_t)Jt * a.np + gi] < L);
            }
        } else {
            const int gj = Jt * CT + (t - CT);
            KmRow z{};
            rB[t - CT] = gj < a.k ? a.rowC[gj] : z;
        }
        if (MODE == MODE_PASS2) {
            if (!__syncthreads_or(live)) continue;  // (workgroup-uniform)
        }
        const uint16_t* Ag = a.imgX + (size_t)It * CT * a.Dp;
        const uint16_t* Bg = a.imgC + (size_t)Jt * CT * a.Dp;
        u16x8 ra[4], rb[4];
        auto load = [&](int k0) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                ra[q] = *reinterpret_cast<const u16x8*>(Ag + (size_t)(ar + 32 * q) * a.Dp + k0 + ac);
                rb[q] = *reinterpret_cast<const u16x8*>(Bg + (size_t)(ar + 32 * q) * a.Dp + k0 + ac);
            }
        };
        f32x16 acc[2][2];  // [block of centres][block of rows]
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
        // C/D map of 32x32x16: column (a row of X) = lane & 31, row (a centre) = (r & 3) + 8 (r >> 2) + 4 h
        if constexpr (MODE == MODE_PASS1) {
#pragma unroll
            for (int ia = 0; ia < 2; ++ia) {
                const int nn = wn + 32 * ia + r32;
                const KmRow xi = rA[nn];
                double lo = -INF, hi = -INF;
#pragma unroll
                for (int ib = 0; ib < 2; ++ib)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int m = wm + 32 * ib + (r & 3) + 8 * (r >> 2) + 4 * h, gj = Jt * CT + m;
                        if (gj < a.k) {
                            double s, E;
                            km_pair(a, acc[ib][ia][r], xi, rB[m], &s, &E);
                            const double g = sg * s, gl = g - E, gh = g + E;
                            lo = fmax(lo, gl);               // (a NaN does not raise L_i)
                            hi = gh == gh ? fmax(hi, gh) : INF;  // (a NaN keeps the tile)
                        }
                    }
                lo = fmax(lo, shfl_xor_d(lo, 32));
                hi = fmax(hi, shfl_xor_d(hi, 32));
                if (h == 0) { red[0][w >> 1][nn] = lo; red[1][w >> 1][nn] = hi; }
            }
            __syncthreads();
            if (t < CT && It * CT + t < a.n) {
                const int gi = It * CT + t;
                a.hi[(size_t)Jt * a.np + gi] = fmax(red[1][0][t], red[1][1][t]);
                // (the plain read skips the atomic for all but the few tiles that raise L_i; the final value is the max either way)
                const u64 key = d2ukey(fmax(red[0][0][t], red[0][1][t]));
                if (key > __hip_atomic_load(&a.Lkey[gi], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&a.Lkey[gi], key);
            }
        } else {
            u64 keep = 0;  // bit 32 ia + 16 ib + r: this element is a candidate
            int cnt = 0;
#pragma unroll
            for (int ia = 0; ia < 2; ++ia) {
                const int nn = wn + 32 * ia + r32, gi = It * CT + nn;
                const KmRow xi = rA[nn];
                const double L = MODE == MODE_PASS2 ? red[0][0][nn] : 0.0;
#pragma unroll
                for (int ib = 0; ib < 2; ++ib)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int m = wm + 32 * ib + (r & 3) + 8 * (r >> 2) + 4 * h, gj = Jt * CT + m;
                        const bool in = MODE == MODE_PASS2 ? (gi < a.n && gj < a.k) : (gi < gj && gj < a.k);
                        if (in) {
                            double s, E;
                            km_pair(a, acc[ib][ia][r], xi, rB[m], &s, &E);
                            const bool c = MODE == MODE_PASS2 ? !(sg * s + E < L) : !(s - E >= a.thr2);
                            if (c) { keep |= 1ull << (32 * ia + 16 * ib + r); ++cnt; }
                        }
                    }
            }
            const int incl = wave_scan_incl(cnt, lane);
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

// ---- refinement and the exact routes -----------------------------------------------------------------------------------------
// one thread per candidate: r_ij by km_r, raised into best[i] (assign) or tested against tol (collapsed).  The value depends on
// (i, j), X and C only, and both results are order-free, so the order of the list cannot show.
template <int PAIRS>
__global__ __launch_bounds__(256) void km_refine_kernel(KmDev a) {
    if (a.ctl[CTL_NONFINITE] != 0 || exact_answers(a)) return;
    const long n = (long)cand_count(a.ctl);
    for (long c = (long)blockIdx.x * 256 + threadIdx.x; c < n; c += (long)gridDim.x * 256) {
        const int2 pr = a.cand[c];
        const float r = km_r(a.X + (size_t)pr.x * a.D, a.C + (size_t)pr.y * a.D, a.D);
        if (PAIRS) {
            if (sqrtf(r) < a.tol) a.loser[a.counts[pr.x] <= a.counts[pr.y] ? pr.x : pr.y] = 1;
        } else if (r == r) {
            atomicMax(&a.best[pr.x], best_key(r, pr.y, a.far));
        }
    }
}

// every pair by km_acc4: a 64 x 64 tile per workgroup, thread (ty, tx) the rows 4 ty .. 4 ty + 3 against the centres tx + 16 jj.
// Rows and centres past the end are clamped for the loads and dropped from the result.
template <int PAIRS>
__global__ __launch_bounds__(256) void km_exact_kernel(KmDev a) {
    if (a.ctl[CTL_NONFINITE] != 0 || !exact_answers(a)) return;
    const int t = threadIdx.x, ty = t >> 4, tx = t & 15;
    const int nq = a.D >> 2;
    const int nTi = (a.n + ET - 1) / ET, nTj = (a.k + ET - 1) / ET;
    for (long tile = blockIdx.x; tile < (long)nTi * nTj; tile += gridDim.x) {
        const int It = (int)(tile % nTi), Jt = (int)(tile / nTi);
        if (PAIRS && It > Jt) continue;
        const f32x4* xp[4];
        const f32x4* cp[4];
        int gi[4], gj[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            gi[e] = It * ET + 4 * ty + e;
            gj[e] = Jt * ET + tx + 16 * e;
            xp[e] = reinterpret_cast<const f32x4*>(a.X + (size_t)min(gi[e], a.n - 1) * a.D);
            cp[e] = reinterpret_cast<const f32x4*>(a.C + (size_t)min(gj[e], a.k - 1) * a.D);
        }
        float s[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) s[i][j] = 0.f;
        for (int q = 0; q < nq; ++q) {
            f32x4 xv[4], cv[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) { xv[e] = xp[e][q]; cv[e] = cp[e][q]; }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) s[i][j] = km_acc4(s[i][j], xv[i], cv[j]);
        }
        if (PAIRS) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (gi[i] < gj[j] && gj[j] < a.k && sqrtf(s[i][j]) < a.tol)
                        a.loser[a.counts[gi[i]] <= a.counts[gj[j]] ? gi[i] : gj[j]] = 1;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                u64 bk = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (gi[i] < a.n && gj[j] < a.k && s[i][j] == s[i][j]) {
                        const u64 key = best_key(s[i][j], gj[j], a.far);
                        bk = key > bk ? key : bk;
                    }
#pragma unroll
                for (int o = 1; o < 16; o <<= 1) {  // (the 16 tx of one ty are 16 consecutive lanes)
                    const u64 ok = shfl_xor_u64(bk, o);
                    bk = ok > bk ? ok : bk;
                }
                if (tx == 0 && bk != 0) atomicMax(&a.best[gi[i]], bk);
            }
        }
    }
}

// info = {route taken (SAEV_KMEANS_NONFINITE: X or C holds an inf or a NaN), candidates found, tiles recomputed, capacity}
__device__ void km_info(const KmDev& a, int32_t* out_info) {
    const u64 n = cand_count(a.ctl);
    const bool fell = no_image(a.ctl) || n > (u64)a.cap;
    out_info[0] = a.ctl[CTL_NONFINITE] != 0 ? SAEV_KMEANS_NONFINITE
                  : a.route == SAEV_KMEANS_EXACT ? SAEV_KMEANS_EXACT : (fell ? SAEV_KMEANS_OVERFLOW : SAEV_KMEANS_FILTERED);
    out_info[1] = n > 0x7fffffffull ? 0x7fffffff : (int32_t)n;
    out_info[2] = (int32_t)a.ctl[CTL_TILES];
    out_info[3] = a.cap;
}
__global__ __launch_bounds__(256) void km_finalize_kernel(KmDev a, float* out_dist2, int32_t* out_index, int32_t* out_info) {
    if (blockIdx.x == 0 && threadIdx.x == 0) km_info(a, out_info);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const u64 b = a.best[i];
    const bool bad = a.ctl[CTL_NONFINITE] != 0;
    float v = __builtin_nanf("");
    int32_t j = bad ? -1 : 0;  // (-1: saev_kmeans_group ignores the row, so a step built on these outputs changes nothing)
    if (b != 0 && !bad) {
        const uint32_t key = (uint32_t)(b >> 32);
        v = ukey2f(a.far ? key : ~key);
        j = (int32_t)~(uint32_t)b;
    }
    out_dist2[i] = v;
    out_index[i] = j;
}
__global__ void km_info_kernel(KmDev a, int32_t* out_info) { km_info(a, out_info); }

// ---- group -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void km_hist_kernel(const int32_t* __restrict__ index, int n, int k, int32_t* counts) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int j = index[i];
    if (j >= 0 && j < k) atomicAdd(&counts[j], 1);
}
// exclusive scan of counts into starts[0 .. k], one workgroup: thread t owns a contiguous slice.  counts is cleared for the
// placement, which counts it up again.
__global__ __launch_bounds__(1024) void km_scan_kernel(int32_t* counts, int k, int32_t* starts) {
    __shared__ int tot[1024];
    const int t = threadIdx.x;
    const int per = (k + 1023) / 1024, j0 = min(k, t * per), j1 = min(k, j0 + per);
    int s = 0;
    for (int j = j0; j < j1; ++j) s += counts[j];
    tot[t] = s;
    __syncthreads();
    if (t == 0) {
        int run = 0;
        for (int i = 0; i < 1024; ++i) { const int v = tot[i]; tot[i] = run; run += v; }
        starts[k] = run;
    }
    __syncthreads();
    int run = tot[t];
    for (int j = j0; j < j1; ++j) { starts[j] = run; run += counts[j]; counts[j] = 0; }
}
__global__ __launch_bounds__(256) void km_place_kernel(const int32_t* __restrict__ index, int n, int k, int32_t* counts,
                                                       const int32_t* __restrict__ starts, int32_t* rows) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int j = index[i];
    if (j >= 0 && j < k) rows[starts[j] + atomicAdd(&counts[j], 1)] = i;
}
// each centre's rows into ascending order.  A segment of up to SORT_LDS rows is sorted in LDS by a bitonic network of ascending
// compare-exchanges on the first m slots of the next power of two (partners past m count as +inf and never move).  A longer one
// is written afresh: its ascending list is {i : index[i] == j}, a stable compaction of index in chunks of SORT_CHUNK entries
// (thread t owns 16 consecutive entries, a wave scan and four wave totals give its offset).  At most n / SORT_LDS centres are
// that long, each read of index is one pass.  A workgroup takes the centres j = block, block + grid, ...
__global__ __launch_bounds__(256) void km_sort_kernel(const int32_t* __restrict__ index, int n, int k, const int32_t* __restrict__ starts,
                                                      int32_t* rows) {
    __shared__ int32_t buf[SORT_LDS];
    __shared__ int wsum[4];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    for (int j = blockIdx.x; j < k; j += gridDim.x) {
        const int s0 = starts[j], m = starts[j + 1] - s0;
        if (m < 2) continue;  // (workgroup-uniform)
        if (m > SORT_LDS) {
            int base = 0;  // matches before this chunk (workgroup-uniform)
            for (int c0 = 0; c0 < n; c0 += SORT_CHUNK) {
                const int i0 = c0 + t * 16;
                uint32_t hit = 0;
#pragma unroll
                for (int e = 0; e < 16; ++e)
                    if (i0 + e < n && index[i0 + e] == j) hit |= 1u << e;
                const int cnt = __popc(hit);
                const int incl = wave_scan_incl(cnt, lane);
                if (lane == 63) wsum[w] = incl;
                __syncthreads();
                int off = base + incl - cnt, tot = 0;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (q < w) off += wsum[q];
                    tot += wsum[q];
                }
                __syncthreads();  // wsum is read before the next chunk writes it
#pragma unroll
                for (int e = 0; e < 16; ++e)
                    if ((hit >> e) & 1u) {
                        if (off < m) rows[s0 + off] = i0 + e;  // (off < m always: counts came from this index)
                        ++off;
                    }
                base += tot;
            }
            continue;
        }
        __syncthreads();  // the previous centre's copy-out has read buf
        for (int i = t; i < m; i += 256) buf[i] = rows[s0 + i];
        __syncthreads();
        int P = 2;
        while (P < m) P <<= 1;
        for (int size = 2; size <= P; size <<= 1) {
            for (int stride = size >> 1; stride > 0; stride >>= 1) {
                const bool first = stride == (size >> 1);
                for (int i = t; i < m; i += 256) {
                    const int p = first ? (i ^ (size - 1)) : (i ^ stride);
                    if (p > i && p < m) {
                        const int32_t x = buf[i], y = buf[p];
                        if (x > y) { buf[i] = y; buf[p] = x; }
                    }
                }
                __syncthreads();
            }
        }
        for (int i = t; i < m; i += 256) rows[s0 + i] = buf[i];
    }
}

// ---- update ------------------------------------------------------------------------------------------------------------------
// thread = (centre j, column quad q): sums = x_r0 + x_r1 + ... over the centre's rows in ascending order (a one-thread
// index_add_ into zeros), or the one replacement row; then c = (c prev + sums) / (prev + count), each operation rounded once
__global__ __launch_bounds__(256) void km_update_kernel(const float* __restrict__ X, int n, int D, int k, const int32_t* __restrict__ starts,
                                                        const int32_t* __restrict__ rows, const int32_t* __restrict__ repl,
                                                        float* centers, const float* __restrict__ counts) {
#pragma clang fp contract(off)
    const int nq = D >> 2;
    const long id = (long)blockIdx.x * 256 + threadIdx.x;
    if (id >= (long)k * nq) return;
    const int j = (int)(id / nq), q = (int)(id % nq);
    const int s0 = starts[j], m = starts[j + 1] - s0;
    f32x4 sum = {0.f, 0.f, 0.f, 0.f};
    float cnt = (float)m;
    if (m > 0) {
        auto row = [&](int i) { return *reinterpret_cast<const f32x4*>(X + (size_t)rows[s0 + i] * D + 4 * q); };
        int i = 0;
        for (; i + 8 <= m; i += 8) {  // eight loads in flight, added in row order all the same
            f32x4 x[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) x[u] = row(i + u);
#pragma unroll
            for (int u = 0; u < 8; ++u)
#pragma unroll
                for (int e = 0; e < 4; ++e) sum[e] = sum[e] + x[u][e];
        }
        for (; i < m; ++i) {
            const f32x4 x = row(i);
#pragma unroll
            for (int e = 0; e < 4; ++e) sum[e] = sum[e] + x[e];
        }
    } else if (repl != nullptr && repl[j] >= 0 && repl[j] < n) {
        sum = *reinterpret_cast<const f32x4*>(X + (size_t)repl[j] * D + 4 * q);
        cnt = 1.f;
    }
    if (cnt > 0.f) {
        const float prev = counts[j], tot = prev + cnt;
        f32x4* cp = reinterpret_cast<f32x4*>(centers + (size_t)j * D + 4 * q);
        f32x4 c = *cp;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float a = c[e] * prev;
            const float b = a + sum[e];
            c[e] = b / tot;
        }
        *cp = c;
    }
}
// cluster_counts += the batch counts (after the centres have read the previous ones)
__global__ __launch_bounds__(256) void km_counts_kernel(int n, int k, const int32_t* __restrict__ starts, const int32_t* __restrict__ repl,
                                                        float* counts) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= k) return;
    const int m = starts[j + 1] - starts[j];
    const float cnt = m > 0 ? (float)m : ((repl != nullptr && repl[j] >= 0 && repl[j] < n) ? 1.f : 0.f);
    if (cnt > 0.f) counts[j] = counts[j] + cnt;
}
// the fp64 mean of dist2 in a fixed order: thread t sums i = t, t + 1024, ..., then a tree over the 1024 partials
__global__ __launch_bounds__(1024) void km_inertia_kernel(const float* __restrict__ dist2, int n, double* out) {
    __shared__ double part[1024];
    const int t = threadIdx.x;
    double s = 0.0;
    for (int i = t; i < n; i += 1024) s += (double)dist2[i];
    part[t] = s;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if (t < o) part[t] += part[t + o];
        __syncthreads();
    }
    if (t == 0) *out = part[0] / (double)n;
}

long round_up(long v, long m) { return (v + m - 1) / m * m; }

int persistent_grid(long work) {
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    return (int)std::max<long>(1, std::min<long>(work, 2L * cus));
}

// the centring vector, the centred copies, their images and the row records of one operand
hipError_t prepare_operand(const float* W, int S, int D, int Sp, int Dp, const float* mu, uint8_t* ws, size_t off_c, size_t off_row,
                           size_t off_nrm, size_t off_rn, size_t off_img, uint32_t* ctl, int bad_word, hipStream_t s) {
    float* Wc = reinterpret_cast<float*>(ws + off_c);
    KmRow* row = reinterpret_cast<KmRow*>(ws + off_row);
    float* nrm = reinterpret_cast<float*>(ws + off_nrm);
    float2* rn = reinterpret_cast<float2*>(ws + off_rn);
    hipLaunchKernelGGL(km_center_kernel, dim3((S + 3) / 4), dim3(256), 0, s, W, S, D, mu, Wc, row, ctl);
    hipError_t e = launch_coh_prepare(Wc, S, D, Sp, Dp, nrm, rn, reinterpret_cast<uint16_t*>(ws + off_img), ctl + bad_word, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(km_rows_kernel, dim3((S + 255) / 256), dim3(256), 0, s, S, nrm, rn, row);
    return hipGetLastError();
}

hipError_t centring_vector(const float* C, int k, int D, uint8_t* ws, const KmLayout& L, hipStream_t s) {
    const int per = (k + MU_CHUNKS - 1) / MU_CHUNKS, chunks = (k + per - 1) / per;
    float* part = reinterpret_cast<float*>(ws + L.off_part);
    hipLaunchKernelGGL(km_colsum_kernel, dim3(chunks), dim3(256), 0, s, C, k, D, per, part);
    hipLaunchKernelGGL(km_mu_kernel, dim3((D + 255) / 256), dim3(256), 0, s, part, chunks, k, D, reinterpret_cast<float*>(ws + L.off_mu));
    return hipGetLastError();
}

}  // namespace

KmLayout kmeans_layout(long n, long k, int D) {
    KmLayout L{};
    L.np = (int)round_up(n, CT);
    L.kp = (int)round_up(k, CT);
    L.Dp = (int)round_up(D, CK);
    L.nTX = L.np / CT;
    L.nTC = L.kp / CT;
    L.ntiles = (long)L.nTX * L.nTC;
    L.cap = (int)std::max<long>(1, std::min<long>(n * k, std::max<long>(KM_CAND_MIN, KM_CAND_PER_ROW * n)));
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += (bytes + 255) / 256 * 256; return o; };
    L.off_ctl = take(64);
    L.off_L = take((size_t)L.np * 8);
    L.off_best = take((size_t)n * 8);
    L.zero_bytes = off;
    L.off_mu = take((size_t)D * 4);
    L.off_part = take((size_t)MU_CHUNKS * D * 4);
    L.off_Xc = take((size_t)n * D * 4);
    L.off_rowX = take((size_t)n * sizeof(KmRow));
    L.off_nrmX = take((size_t)n * 4);
    L.off_rnX = take((size_t)n * 8);
    L.off_imgX = take((size_t)L.np * L.Dp * 2);
    L.off_Cc = take((size_t)k * D * 4);
    L.off_rowC = take((size_t)k * sizeof(KmRow));
    L.off_nrmC = take((size_t)k * 4);
    L.off_rnC = take((size_t)k * 8);
    L.off_imgC = take((size_t)L.kp * L.Dp * 2);
    L.off_hi = take((size_t)L.nTC * L.np * 8);
    L.off_cand = take((size_t)L.cap * 8);
    L.bytes = off;
    return L;
}

hipError_t launch_kmeans_assign(const float* X, int n, const float* C, int k, int D, int farthest, int route, uint8_t* ws,
                                const KmLayout& L, float* out_dist2, int32_t* out_index, int32_t* out_info, hipStream_t s) {
    if (k == 1) route = SAEV_KMEANS_EXACT;  // the one centre is mu and has no unit image: nothing to filter, and no overflow to report
    KmDev a{};
    a.X = X; a.C = C; a.n = n; a.k = k; a.D = D; a.Dp = L.Dp; a.np = L.np; a.nTX = L.nTX; a.nTC = L.nTC; a.cap = L.cap;
    a.route = route; a.far = farthest != 0; a.ntiles = L.ntiles;
    a.gam = coh_gamma(L.Dp);
    a.tau = 1.001 * (double)(D + 3) * 5.9604644775390625e-08;
    a.rowX = reinterpret_cast<const KmRow*>(ws + L.off_rowX);
    a.rowC = reinterpret_cast<const KmRow*>(ws + L.off_rowC);
    a.imgX = reinterpret_cast<const uint16_t*>(ws + L.off_imgX);
    a.imgC = reinterpret_cast<const uint16_t*>(ws + L.off_imgC);
    a.ctl = reinterpret_cast<uint32_t*>(ws + L.off_ctl);
    a.Lkey = reinterpret_cast<u64*>(ws + L.off_L);
    a.best = reinterpret_cast<u64*>(ws + L.off_best);
    a.hi = reinterpret_cast<double*>(ws + L.off_hi);
    a.cand = reinterpret_cast<int2*>(ws + L.off_cand);
    hipError_t e = hipMemsetAsync(ws + L.off_ctl, 0, L.zero_bytes, s);
    if (e != hipSuccess) return e;
    // (the exact route needs the finiteness word only; the centred copies carry it, so both routes prepare)
    e = centring_vector(C, k, D, ws, L, s);
    if (e != hipSuccess) return e;
    const float* mu = reinterpret_cast<const float*>(ws + L.off_mu);
    e = prepare_operand(X, n, D, L.np, L.Dp, mu, ws, L.off_Xc, L.off_rowX, L.off_nrmX, L.off_rnX, L.off_imgX, a.ctl, CTL_BAD_X, s);
    if (e != hipSuccess) return e;
    e = prepare_operand(C, k, D, L.kp, L.Dp, mu, ws, L.off_Cc, L.off_rowC, L.off_nrmC, L.off_rnC, L.off_imgC, a.ctl, CTL_BAD_C, s);
    if (e != hipSuccess) return e;
    if (route == SAEV_KMEANS_AUTO) {
        const int grid = persistent_grid(L.ntiles);
        hipLaunchKernelGGL(km_filter_kernel<MODE_PASS1>, dim3(grid), dim3(256), 0, s, a);
        hipLaunchKernelGGL(km_filter_kernel<MODE_PASS2>, dim3(grid), dim3(256), 0, s, a);
        hipLaunchKernelGGL(km_refine_kernel<0>, dim3((int)std::min<long>((L.cap + 255) / 256, 4096)), dim3(256), 0, s, a);
    }
    const long etiles = (long)((n + ET - 1) / ET) * ((k + ET - 1) / ET);
    hipLaunchKernelGGL(km_exact_kernel<0>, dim3((int)std::min<long>(etiles, 8192)), dim3(256), 0, s, a);
    hipLaunchKernelGGL(km_finalize_kernel, dim3((n + 255) / 256), dim3(256), 0, s, a, out_dist2, out_index, out_info);
    return hipGetLastError();
}

hipError_t launch_kmeans_collapsed(const float* C, int k, int D, float tol, const float* counts, int route, uint8_t* ws,
                                   const KmLayout& L, uint8_t* out_loser, int32_t* out_info, hipStream_t s) {
    if (k == 1) route = SAEV_KMEANS_EXACT;  // (no pair: reported as the exact route, not as an overflow)
    KmDev a{};
    a.X = C; a.C = C; a.n = k; a.k = k; a.D = D; a.Dp = L.Dp; a.np = L.np; a.nTX = L.nTX; a.nTC = L.nTX;
    a.cap = (int)std::max<long>(1, std::min<long>((long)k * (k - 1) / 2, L.cap));
    a.route = route; a.ntiles = (long)L.nTX * L.nTX;
    a.gam = coh_gamma(L.Dp);
    a.tau = 1.001 * (double)(D + 3) * 5.9604644775390625e-08;
    a.tol = tol; a.thr2 = (double)tol * (double)tol;
    a.rowX = a.rowC = reinterpret_cast<const KmRow*>(ws + L.off_rowX);
    a.imgX = a.imgC = reinterpret_cast<const uint16_t*>(ws + L.off_imgX);
    a.ctl = reinterpret_cast<uint32_t*>(ws + L.off_ctl);
    a.cand = reinterpret_cast<int2*>(ws + L.off_cand);
    a.counts = counts; a.loser = out_loser;
    hipError_t e = hipMemsetAsync(ws + L.off_ctl, 0, 64, s);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(out_loser, 0, (size_t)k, s);
    if (e != hipSuccess) return e;
    e = centring_vector(C, k, D, ws, L, s);
    if (e != hipSuccess) return e;
    const float* mu = reinterpret_cast<const float*>(ws + L.off_mu);
    e = prepare_operand(C, k, D, L.np, L.Dp, mu, ws, L.off_Xc, L.off_rowX, L.off_nrmX, L.off_rnX, L.off_imgX, a.ctl, CTL_BAD_X, s);
    if (e != hipSuccess) return e;
    if (k >= 2 && tol > 0.f) {  // (no pair, or no distance below tol: no losers)
        if (route == SAEV_KMEANS_AUTO) {
            hipLaunchKernelGGL(km_filter_kernel<MODE_PAIRS>, dim3(persistent_grid(a.ntiles)), dim3(256), 0, s, a);
            hipLaunchKernelGGL(km_refine_kernel<1>, dim3((int)std::min<long>((a.cap + 255) / 256, 4096)), dim3(256), 0, s, a);
        }
        const long et = (k + ET - 1) / ET;
        hipLaunchKernelGGL(km_exact_kernel<1>, dim3((int)std::min<long>(et * et, 8192)), dim3(256), 0, s, a);
    }
    hipLaunchKernelGGL(km_info_kernel, dim3(1), dim3(1), 0, s, a, out_info);
    return hipGetLastError();
}

hipError_t launch_kmeans_group(const int32_t* index, int n, int k, int32_t* counts, int32_t* starts, int32_t* rows, hipStream_t s) {
    hipError_t e = hipMemsetAsync(counts, 0, (size_t)k * 4, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(km_hist_kernel, dim3((n + 255) / 256), dim3(256), 0, s, index, n, k, counts);
    hipLaunchKernelGGL(km_scan_kernel, dim3(1), dim3(1024), 0, s, counts, k, starts);
    hipLaunchKernelGGL(km_place_kernel, dim3((n + 255) / 256), dim3(256), 0, s, index, n, k, counts, starts, rows);
    hipLaunchKernelGGL(km_sort_kernel, dim3(std::min(k, 4096)), dim3(256), 0, s, index, n, k, starts, rows);
    return hipGetLastError();
}

hipError_t launch_kmeans_update(const float* X, int n, int D, int k, const int32_t* starts, const int32_t* rows, const int32_t* repl,
                                float* centers, float* counts, double* out_inertia, const float* dist2, hipStream_t s) {
    const long work = (long)k * (D >> 2);
    hipLaunchKernelGGL(km_update_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, s, X, n, D, k, starts, rows, repl, centers, counts);
    hipLaunchKernelGGL(km_counts_kernel, dim3((k + 255) / 256), dim3(256), 0, s, n, k, starts, repl, counts);
    if (out_inertia != nullptr && dist2 != nullptr)
        hipLaunchKernelGGL(km_inertia_kernel, dim3(1), dim3(1024), 0, s, dist2, n, out_inertia);
    return hipGetLastError();
}

// ---- the C entries (include/saev_amd.h: K-MEANS) ----------------------------------------------------------------------------
extern "C" {

int64_t saev_kmeans_workspace_bytes(int64_t n, int64_t k, int64_t D) {
    const int64_t smax = (int64_t)1 << 20;
    if (n < 1 || n > smax || k < 1 || k > smax || D < 4 || D > 4096 || D % 4 != 0) return -1;
    return (int64_t)kmeans_layout(n, k, (int)D).bytes;
}

int saev_kmeans_assign(const float* X, int64_t n, const float* C, int64_t k, int64_t D, int32_t farthest, int32_t route,
                       void* workspace, int64_t workspace_bytes, float* out_dist2, int32_t* out_index, int32_t* out_info, void* stream) {
    const int64_t need = saev_kmeans_workspace_bytes(n, k, D);
    if (need < 0 || (route != SAEV_KMEANS_AUTO && route != SAEV_KMEANS_EXACT)) return SAEV_INVALID_ARG;
    if (!X || !C || !workspace || !out_dist2 || !out_index || !out_info) return SAEV_INVALID_ARG;
    if (workspace_bytes < need || ((uintptr_t)workspace & 255) != 0 || ((uintptr_t)X & 15) != 0 || ((uintptr_t)C & 15) != 0)
        return SAEV_INVALID_ARG;
    const KmLayout L = kmeans_layout(n, k, (int)D);
    if (launch_kmeans_assign(X, (int)n, C, (int)k, (int)D, farthest, route, static_cast<uint8_t*>(workspace), L, out_dist2, out_index,
                             out_info, (hipStream_t)stream) != hipSuccess)
        return SAEV_HIP_ERROR;
    return SAEV_OK;
}

int saev_kmeans_group(const int32_t* index, int64_t n, int64_t k, int32_t* counts, int32_t* starts, int32_t* rows, void* stream) {
    const int64_t smax = (int64_t)1 << 20;
    if (n < 1 || n > smax || k < 1 || k > smax || !index || !counts || !starts || !rows) return SAEV_INVALID_ARG;
    if (launch_kmeans_group(index, (int)n, (int)k, counts, starts, rows, (hipStream_t)stream) != hipSuccess) return SAEV_HIP_ERROR;
    return SAEV_OK;
}

int saev_kmeans_update(const float* X, int64_t n, int64_t D, int64_t k, const int32_t* starts, const int32_t* rows,
                       const int32_t* repl_rows, float* centers, float* cluster_counts, double* out_inertia, const float* dist2,
                       void* stream) {
    const int64_t smax = (int64_t)1 << 20;
    if (n < 1 || n > smax || k < 1 || k > smax || D < 4 || D > 4096 || D % 4 != 0) return SAEV_INVALID_ARG;
    if (!X || !starts || !rows || !centers || !cluster_counts) return SAEV_INVALID_ARG;
    if (((uintptr_t)X & 15) != 0 || ((uintptr_t)centers & 15) != 0) return SAEV_INVALID_ARG;
    if (launch_kmeans_update(X, (int)n, (int)D, (int)k, starts, rows, repl_rows, centers, cluster_counts, out_inertia, dist2,
                             (hipStream_t)stream) != hipSuccess)
        return SAEV_HIP_ERROR;
    return SAEV_OK;
}

int saev_kmeans_collapsed(const float* C, int64_t k, int64_t D, float tol, const float* cluster_counts, int32_t route, void* workspace,
                          int64_t workspace_bytes, uint8_t* out_loser, int32_t* out_info, void* stream) {
    const int64_t need = saev_kmeans_workspace_bytes(k, k, D);
    if (need < 0 || (route != SAEV_KMEANS_AUTO && route != SAEV_KMEANS_EXACT)) return SAEV_INVALID_ARG;
    if (!C || !cluster_counts || !workspace || !out_loser || !out_info) return SAEV_INVALID_ARG;
    if (workspace_bytes < need || ((uintptr_t)workspace & 255) != 0 || ((uintptr_t)C & 15) != 0) return SAEV_INVALID_ARG;
    const KmLayout L = kmeans_layout(k, k, (int)D);
    if (launch_kmeans_collapsed(C, (int)k, (int)D, tol, cluster_counts, route, static_cast<uint8_t*>(workspace), L, out_loser, out_info,
                                (hipStream_t)stream) != hipSuccess)
        return SAEV_HIP_ERROR;
    return SAEV_OK;
}

}  // extern "C"
