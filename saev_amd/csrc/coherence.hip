// Dictionary coherence max_{i<j} |<w_i, w_j>| / (||w_i|| ||w_j||) of an (S, D) fp32 matrix without an S x S product in memory:
// an fp16 MFMA filter with a rigorous per-pair error bound, then the exact fp32 dot products of the few pairs that can still be
// the maximum.  The entry point is saev_dictionary_coherence (include/saev_amd.h: COHERENCE); DESIGN.md 3.11 has the proof and
// the numbers.
//
//   prepare   one wave per row: the fp32 norm n_i, w_i / n_i (never stored: every reader divides again, bit for bit), the
//             fp16 image h_i = fp16(2^13 w_i / n_i) with fp16 subnormals flushed to zero here -- the MFMA consumes exactly
//             these values -- and two upper bounds per row: ||w_i / n_i|| and ||d_i||, d_i = w_i / n_i - 2^-13 h_i.
//   pass 1    fp16 MFMA over the upper-triangle tiles (I <= J, 128 x 128 rows): per pair c~ = <h_i, h_j> 2^-26 and the bound E_ij;
//             per tile max(|c~| + E) is stored, max(|c~| - E) goes into the global lower bound L.
//   pass 2    the tiles whose max(|c~| + E) reaches L again: every pair with |c~| + E >= L goes into the candidate list.
//   refine    each candidate's dot product of the fp32 rows w_i / n_i, in a fixed k order.
//   exact     fp32 MFMA (v_mfma_f32_32x32x2_f32) over the whole upper triangle: the caller's "exact" route, or the fallback when
//             the list overflowed (its kernel exits at once otherwise).
//   finalize  the max, ties to the lexicographically smallest (i, j); NaN when a row's normalised form is not finite.
#include "common.h"
#include "kernels.h"

#include <algorithm>

namespace {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));

constexpr int CT = COH_TILE;          // tile edge: 128 rows of W on each side of a tile
constexpr int CK = COH_KSTAGE;        // k per LDS stage of the fp16 filter (64)
constexpr int CLDS = CK + 8;          // (+8 fp16 of padding: row pitch 144 B, ds_read_b128 conflict-free)
constexpr int XK = 32;                // k per LDS stage of the fp32 exact route
constexpr int XLDS = XK + 4;          // (row pitch 144 B)
constexpr float IMG_SCALE = 8192.f;   // 2^13: |w / n| <= 1 puts the largest element of a row in [2^13 / sqrt(D), 2^13]
constexpr float IMG_UNSCALE = COH_IMG_UNSCALE;          // 2^-26, both operands' scales
constexpr float F16_MIN_NORMAL = 6.103515625e-05f;      // 2^-14

// control words (uint32) at the start of the workspace
constexpr int CTL_NAN = 0;    // ~(first row whose normalised form is not finite), 0: none
constexpr int CTL_L = 1;      // f2ukey of L = max over pairs of |c~| - E
constexpr int CTL_TILES = 2;  // tiles pass 2 recomputed
constexpr int CTL_CNT = 4;    // (uint64 at words 4-5) candidates pass 2 found, also those past the capacity

struct CohDev {
    const float* W;
    int S, D, Dp, cap, route;
    long ntiles;
    float gam;                // accumulation term of the bound (pass 1 and refine together)
    float* nrm;               // (S) fp32 row norms
    float2* rn;               // (S) {||w_i / n_i||, ||d_i||}, both rounded up
    uint16_t* img;            // (Sp, Dp) fp16 image, zero past S rows and D columns
    uint32_t* ctl;
    float* tile_hi;           // (ntiles) max |c~| + E of the tile
    uint4* best;              // (ntiles) exact route: {key, i, j, 0} of the tile
    int2* cand;               // (cap)
    float* val;               // (cap) refined |c|
};

__device__ __forceinline__ uint32_t wave_max_u(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ uint32_t wave_min_u(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, (uint32_t)__shfl_xor(v, o, 64));
    return v;
}

__device__ __forceinline__ unsigned long long cand_count(const uint32_t* ctl) {
    return *reinterpret_cast<const unsigned long long*>(ctl + CTL_CNT);
}

// tile t of the upper triangle in column order: t = J (J + 1) / 2 + I, 0 <= I <= J
__device__ __forceinline__ void tile_ij(long t, int* I, int* J) {
    long j = (long)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
    while (j * (j + 1) / 2 > t) --j;
    while ((j + 1) * (j + 2) / 2 <= t) ++j;
    *J = (int)j;
    *I = (int)(t - j * (j + 1) / 2);
}

// one wave per row of the padded image; rows past S are written as zeros
__global__ __launch_bounds__(256) void coh_prepare_kernel(const float* __restrict__ W, int S, int D, int Dp, float* nrm, float2* rn,
                                                          uint16_t* img, uint32_t* ctl) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    _Float16* out = reinterpret_cast<_Float16*>(img) + (size_t)r * Dp;
    if (r >= S) {
        for (int k = lane * 8; k < Dp; k += 512) *reinterpret_cast<u16x8*>(out + k) = u16x8{0, 0, 0, 0, 0, 0, 0, 0};
        return;
    }
    const f32x4* p = reinterpret_cast<const f32x4*>(W + (size_t)r * D);
    const int nq = D >> 2;
    float ss = 0.f;
    for (int q = lane; q < nq; q += 64) {
        const f32x4 v = p[q];
#pragma unroll
        for (int e = 0; e < 4; ++e) ss = __builtin_fmaf(v[e], v[e], ss);
    }
    const float n = sqrtf(wave_sum(ss));
    double wsq = 0.0, dsq = 0.0;
    bool bad = false;
    for (int k = lane * 8; k < Dp; k += 512) {
        half8 hv;
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (k + 4 * g < D) v = p[(k >> 2) + g];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float u = k + 4 * g < D ? v[e] / n : 0.f;
                bad |= !(fabsf(u) <= 3.0e38f);
                const float s = u * IMG_SCALE;
                _Float16 hh = (_Float16)s;
                if (fabsf((float)hh) < F16_MIN_NORMAL) hh = (_Float16)0.f;
                const float d = s - (float)hh;  // exact: s and its 11-bit rounding share their leading bits
                hv[4 * g + e] = hh;
                wsq += (double)u * (double)u;
                dsq += (double)d * (double)d;
            }
        }
        *reinterpret_cast<half8*>(out + k) = hv;
    }
    wsq = wave_sum_d(wsq);
    dsq = wave_sum_d(dsq);
    const unsigned long long badm = __ballot(bad);
    if (lane == 0) {
        nrm[r] = n;
        const float up = 1.0f + 9.5367431640625e-07f;  // 1 + 2^-20: covers the double -> float roundings
        rn[r] = make_float2((float)sqrt(wsq) * up, (float)(sqrt(dsq) * (1.0 / IMG_SCALE)) * up);
        if (badm) atomicMax(&ctl[CTL_NAN], ~(uint32_t)r);
    }
}

// fp16 filter.  PASS 1: tile maxima of |c~| + E (stored) and |c~| - E (into L); PASS 2: the tiles that can hold the maximum, every
// pair with |c~| + E >= L appended to the candidate list (one atomic per wave).  128 x 128 tile per workgroup, four waves of 64 x 64
// (2 x 2 v_mfma_f32_32x32x16_f16), k in stages of 64 through LDS with the next stage's global loads issued before the MFMAs.
template <int PASS>
__global__ __launch_bounds__(256, 2) void coh_filter_kernel(CohDev a) {
    if (a.ctl[CTL_NAN] != 0) return;
    __shared__ __attribute__((aligned(16))) uint16_t As[CT][CLDS];
    __shared__ __attribute__((aligned(16))) uint16_t Bs[CT][CLDS];
    __shared__ float2 rI[CT], rJ[CT];
    __shared__ float red[2][4];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int wm = (w >> 1) * 64, wn = (w & 1) * 64;
    const int r32 = lane & 31, h = lane >> 5;
    const int ar = t >> 3, ac = (t & 7) * 8;  // load slots: rows ar + 32 q (q < 4), 8 fp16 at ac
    const float L = PASS == 2 ? ukey2f(a.ctl[CTL_L]) : 0.f;
    for (long tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
        if (PASS == 2 && !(a.tile_hi[tile] >= L)) continue;  // (workgroup-uniform)
        int I, J;
        tile_ij(tile, &I, &J);
        const uint16_t* Ag = a.img + (size_t)I * CT * a.Dp;
        const uint16_t* Bg = a.img + (size_t)J * CT * a.Dp;
        __syncthreads();  // the previous tile's epilogue has read rI / rJ / red
        {
            const int rr = (t < CT ? I : J) * CT + (t & (CT - 1));
            const float2 v = rr < a.S ? a.rn[rr] : make_float2(0.f, 0.f);
            if (t < CT) rI[t] = v; else rJ[t - CT] = v;
        }
        u16x8 ra[4], rb[4];
        auto load = [&](int k0) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                ra[q] = *reinterpret_cast<const u16x8*>(Ag + (size_t)(ar + 32 * q) * a.Dp + k0 + ac);
                rb[q] = *reinterpret_cast<const u16x8*>(Bg + (size_t)(ar + 32 * q) * a.Dp + k0 + ac);
            }
        };
        f32x16 acc[2][2];
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
                    fa[i] = __builtin_bit_cast(half8, *reinterpret_cast<const u16x8*>(&As[wm + 32 * i + r32][ks + 8 * h]));
                    fb[i] = __builtin_bit_cast(half8, *reinterpret_cast<const u16x8*>(&Bs[wn + 32 * i + r32][ks + 8 * h]));
                }
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[i], fb[j], acc[i][j], 0, 0, 0);
            }
            __syncthreads();
        }
        // C/D map of 32x32x16: column (a J row) = lane & 31, row (an I row) = (r & 3) + 8 (r >> 2) + 4 h
        if constexpr (PASS == 1) {
            float lo = NEG_INF, hi = NEG_INF;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int m = wm + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * h, n = wn + 32 * j + r32;
                        const int gi = I * CT + m, gj = J * CT + n;
                        if (gi < gj && gj < a.S) {
                            const float c = fabsf(acc[i][j][r]) * IMG_UNSCALE;
                            const float e = coh_pair_bound(rI[m], rJ[n], a.gam);
                            lo = fmaxf(lo, c - e);
                            hi = fmaxf(hi, c + e);
                        }
                    }
            lo = wave_max(lo);
            hi = wave_max(hi);
            if (lane == 0) { red[0][w] = lo; red[1][w] = hi; }
            __syncthreads();
            if (t == 0) {
                lo = fmaxf(fmaxf(red[0][0], red[0][1]), fmaxf(red[0][2], red[0][3]));
                hi = fmaxf(fmaxf(red[1][0], red[1][1]), fmaxf(red[1][2], red[1][3]));
                a.tile_hi[tile] = hi;
                // (the plain read skips the atomic for all but the few tiles that raise L; the final value is the max either way)
                const uint32_t key = f2ukey(lo);
                if (key > __hip_atomic_load(&a.ctl[CTL_L], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&a.ctl[CTL_L], key);
            }
        } else {
            unsigned long long keep = 0;  // bit 16 (2 i + j) + r: this element is a candidate
            int cnt = 0;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int m = wm + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * h, n = wn + 32 * j + r32;
                        const int gi = I * CT + m, gj = J * CT + n;
                        if (gi < gj && gj < a.S) {
                            const float c = fabsf(acc[i][j][r]) * IMG_UNSCALE;
                            if (c + coh_pair_bound(rI[m], rJ[n], a.gam) >= L) { keep |= 1ull << (16 * (2 * i + j) + r); ++cnt; }
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
                unsigned long long base = 0;
                if (lane == 63) base = atomicAdd(reinterpret_cast<unsigned long long*>(a.ctl + CTL_CNT), (unsigned long long)tot);
                const uint32_t blo = __shfl((uint32_t)base, 63, 64), bhi = __shfl((uint32_t)(base >> 32), 63, 64);
                unsigned long long slot = (((unsigned long long)bhi << 32) | blo) + (unsigned long long)(incl - cnt);
                for (; keep != 0; keep &= keep - 1, ++slot) {  // bit b = 16 (2 i + j) + r, ascending
                    const int b = __builtin_ctzll(keep), i = b >> 5, j = (b >> 4) & 1, r = b & 15;
                    if (slot < (unsigned long long)a.cap)
                        a.cand[slot] = make_int2(I * CT + wm + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * h, J * CT + wn + 32 * j + r32);
                }
            }
            if (t == 0) atomicAdd(&a.ctl[CTL_TILES], 1u);
        }
    }
}

// exact refinement: one wave per candidate, sum_k (w_ik / n_i)(w_jk / n_j) as fmas in k order per lane (k = 4 q + e, q = lane
// mod 64), then the xor butterfly -- the value depends on (i, j) and W only, not on the candidate's place in the list
__global__ __launch_bounds__(256) void coh_refine_kernel(CohDev a) {
#pragma clang fp contract(off)
    if (a.ctl[CTL_NAN] != 0) return;
    const unsigned long long n = cand_count(a.ctl);
    if (n > (unsigned long long)a.cap) return;  // overflow: the exact route answers
    const int lane = threadIdx.x & 63;
    const int nq = a.D >> 2;
    for (long c = (long)blockIdx.x * 4 + (threadIdx.x >> 6); c < (long)n; c += (long)gridDim.x * 4) {
        const int2 pr = a.cand[c];
        const float ni = a.nrm[pr.x], nj = a.nrm[pr.y];
        const f32x4* wi = reinterpret_cast<const f32x4*>(a.W + (size_t)pr.x * a.D);
        const f32x4* wj = reinterpret_cast<const f32x4*>(a.W + (size_t)pr.y * a.D);
        float s = 0.f;
        for (int q = lane; q < nq; q += 64) {
            const f32x4 x = wi[q], y = wj[q];
#pragma unroll
            for (int e = 0; e < 4; ++e) s = __builtin_fmaf(x[e] / ni, y[e] / nj, s);
        }
        s = wave_sum(s);
        if (lane == 0) a.val[c] = fabsf(s);
    }
}

// (key, pair) order of the result: larger |c| first, then the lexicographically smaller (i, j)
__device__ __forceinline__ bool better(uint32_t k1, unsigned long long p1, uint32_t k2, unsigned long long p2) {
    return k1 > k2 || (k1 == k2 && p1 < p2);
}
__device__ __forceinline__ void wave_best(uint32_t* k, unsigned long long* p) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t k2 = __shfl_xor(*k, o, 64);
        const uint32_t lo = __shfl_xor((uint32_t)*p, o, 64), hi = __shfl_xor((uint32_t)(*p >> 32), o, 64);
        const unsigned long long p2 = ((unsigned long long)hi << 32) | lo;
        if (better(k2, p2, *k, *p)) { *k = k2; *p = p2; }
    }
}

// exact route: fp32 MFMA (v_mfma_f32_32x32x2_f32) on w / n, divided on the way into LDS; per tile the best (|c|, i, j)
__global__ __launch_bounds__(256, 2) void coh_exact_kernel(CohDev a) {
    if (a.ctl[CTL_NAN] != 0) return;
    if (a.route != SAEV_COH_EXACT && !(cand_count(a.ctl) > (unsigned long long)a.cap)) return;
    __shared__ __attribute__((aligned(16))) float As[CT][XLDS];
    __shared__ __attribute__((aligned(16))) float Bs[CT][XLDS];
    __shared__ float nI[CT], nJ[CT];
    __shared__ uint32_t rk[4], ri[4];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int wm = (w >> 1) * 64, wn = (w & 1) * 64;
    const int r32 = lane & 31, h = lane >> 5;
    const int ar = t >> 3, ac = (t & 7) * 4;  // load slots: rows ar + 32 q (q < 4), 4 floats at ac
    for (long tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
        int I, J;
        tile_ij(tile, &I, &J);
        __syncthreads();  // the previous tile's epilogue has read nI / nJ / rk / rp
        {
            const int rr = (t < CT ? I : J) * CT + (t & (CT - 1));
            const float v = rr < a.S ? a.nrm[rr] : 1.f;
            if (t < CT) nI[t] = v; else nJ[t - CT] = v;
        }
        __syncthreads();
        f32x4 ra[4], rb[4];
        auto load = [&](int k0) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int k = k0 + ac, ri = I * CT + ar + 32 * q, rj = J * CT + ar + 32 * q;
                ra[q] = (k < a.D && ri < a.S) ? *reinterpret_cast<const f32x4*>(a.W + (size_t)ri * a.D + k) : f32x4{0.f, 0.f, 0.f, 0.f};
                rb[q] = (k < a.D && rj < a.S) ? *reinterpret_cast<const f32x4*>(a.W + (size_t)rj * a.D + k) : f32x4{0.f, 0.f, 0.f, 0.f};
            }
        };
        f32x16 acc[2][2];
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
                const float ni = nI[ar + 32 * q], nj = nJ[ar + 32 * q];
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
                    fa[i] = *reinterpret_cast<const f32x4*>(&As[wm + 32 * i + r32][kc + 4 * h]);
                    fb[i] = *reinterpret_cast<const f32x4*>(&Bs[wn + 32 * i + r32][kc + 4 * h]);
                }
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int i = 0; i < 2; ++i)
#pragma unroll
                        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i][e], fb[j][e], acc[i][j], 0, 0, 0);
            }
            __syncthreads();
        }
        // the tile's largest key, then the smallest in-tile index (m << 7 | n) that holds it: (i, j) order within a tile is
        // (m, n) order.  Two 32-bit reductions (key 0: no pair)
        uint32_t bk = 0;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int gi = I * CT + wm + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * h, gj = J * CT + wn + 32 * j + r32;
                    const uint32_t k = (gi < gj && gj < a.S) ? f2ukey(fabsf(acc[i][j][r])) : 0u;
                    bk = k > bk ? k : bk;
                }
        bk = wave_max_u(bk);
        if (lane == 0) rk[w] = bk;
        __syncthreads();
        bk = max(max(rk[0], rk[1]), max(rk[2], rk[3]));
        uint32_t bi = 0xffffffffu;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int m = wm + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * h, n = wn + 32 * j + r32;
                    const int gi = I * CT + m, gj = J * CT + n;
                    const bool hit = gi < gj && gj < a.S && f2ukey(fabsf(acc[i][j][r])) == bk;
                    const uint32_t v = hit ? (uint32_t)(m << 7 | n) : 0xffffffffu;
                    bi = v < bi ? v : bi;
                }
        bi = wave_min_u(bi);
        if (lane == 0) ri[w] = bi;
        __syncthreads();
        if (t == 0) {
            bi = min(min(ri[0], ri[1]), min(ri[2], ri[3]));
            a.best[tile] = bk == 0 ? make_uint4(0u, 0xffffffffu, 0xffffffffu, 0u)
                                   : make_uint4(bk, (uint32_t)(I * CT) + (bi >> 7), (uint32_t)(J * CT) + (bi & 127u), 0u);
        }
    }
}

// the result: value, (i, j) and info = {route taken, candidates found, tiles pass 2 recomputed, list capacity}
__global__ __launch_bounds__(1024) void coh_finalize_kernel(CohDev a, float* out_value, int32_t* out_pair, int32_t* out_info) {
    __shared__ uint32_t sk[16];
    __shared__ unsigned long long sp[16];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const unsigned long long n = a.S >= 2 ? cand_count(a.ctl) : 0ull;
    const bool exact = a.route == SAEV_COH_EXACT || n > (unsigned long long)a.cap;
    if (t == 0) {
        out_info[0] = a.route == SAEV_COH_EXACT ? SAEV_COH_EXACT : (exact ? SAEV_COH_OVERFLOW : SAEV_COH_FILTERED);
        out_info[1] = n > 0x7fffffffull ? 0x7fffffff : (int32_t)n;
        out_info[2] = a.S >= 2 ? (int32_t)a.ctl[CTL_TILES] : 0;
        out_info[3] = a.cap;
    }
    if (a.S < 2) {  // no pair: triu(1) of a 1 x 1 matrix is 0
        if (t == 0) { *out_value = 0.f; out_pair[0] = -1; out_pair[1] = -1; }
        return;
    }
    const uint32_t nan_inv = a.ctl[CTL_NAN];
    if (nan_inv != 0) {  // the smallest pair that holds the first such row
        if (t == 0) {
            const int r = (int)~nan_inv;
            *out_value = __builtin_nanf("");
            out_pair[0] = 0;
            out_pair[1] = r == 0 ? 1 : r;
        }
        return;
    }
    uint32_t bk = 0;
    unsigned long long bp = ~0ull;
    if (exact) {
        for (long i = t; i < a.ntiles; i += 1024) {
            const uint4 b = a.best[i];
            const unsigned long long p = ((unsigned long long)b.y << 32) | b.z;
            if (better(b.x, p, bk, bp)) { bk = b.x; bp = p; }
        }
    } else {
        for (long i = t; i < (long)n; i += 1024) {
            const int2 c = a.cand[i];
            const uint32_t k = f2ukey(a.val[i]);
            const unsigned long long p = ((unsigned long long)(uint32_t)c.x << 32) | (uint32_t)c.y;
            if (better(k, p, bk, bp)) { bk = k; bp = p; }
        }
    }
    wave_best(&bk, &bp);
    if (lane == 0) { sk[w] = bk; sp[w] = bp; }
    __syncthreads();
    if (t == 0) {
        for (int v = 1; v < 16; ++v)
            if (better(sk[v], sp[v], bk, bp)) { bk = sk[v]; bp = sp[v]; }
        *out_value = ukey2f(bk);
        out_pair[0] = (int32_t)(bp >> 32);
        out_pair[1] = (int32_t)(uint32_t)bp;
    }
}

long round_up(long v, long m) { return (v + m - 1) / m * m; }

int persistent_grid(long work) {
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    return (int)std::max<long>(1, std::min<long>(work, 2L * cus));
}

}  // namespace

CohLayout coherence_layout(int S, int D) {
    CohLayout L{};
    L.Sp = (int)round_up(S, CT);
    L.Dp = (int)round_up(D, CK);
    L.nT = L.Sp / CT;
    L.ntiles = (long)L.nT * (L.nT + 1) / 2;
    const long pairs = (long)S * (S - 1) / 2;
    L.cap = (int)std::max<long>(1, std::min<long>(pairs, COH_MAX_CANDIDATES));
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += (bytes + 255) / 256 * 256; return o; };
    L.off_ctl = take(64);
    L.off_nrm = take((size_t)S * 4);
    L.off_rn = take((size_t)S * 8);
    L.off_img = take((size_t)L.Sp * L.Dp * 2);
    L.off_hi = take((size_t)L.ntiles * 4);
    L.off_best = take((size_t)L.ntiles * 16);
    L.off_cand = take((size_t)L.cap * 8);
    L.off_val = take((size_t)L.cap * 4);
    L.bytes = off;
    return L;
}

hipError_t launch_coh_prepare(const float* W, int S, int D, int Sp, int Dp, float* nrm, float2* rn, uint16_t* img, uint32_t* nan_word,
                              hipStream_t s) {
    static_assert(CTL_NAN == 0, "coh_prepare_kernel raises ctl[CTL_NAN]: the word it is given");
    hipLaunchKernelGGL(coh_prepare_kernel, dim3(Sp / 4), dim3(256), 0, s, W, S, D, Dp, nrm, rn, img, nan_word);
    return hipGetLastError();
}

hipError_t launch_coherence(const float* W, int S, int D, int route, uint8_t* ws, const CohLayout& L, float* out_value,
                            int32_t* out_pair, int32_t* out_info, hipStream_t s) {
    CohDev a{};
    a.W = W; a.S = S; a.D = D; a.Dp = L.Dp; a.cap = L.cap; a.route = route; a.ntiles = L.ntiles;
    a.gam = coh_gamma(L.Dp);
    a.nrm = reinterpret_cast<float*>(ws + L.off_nrm);
    a.rn = reinterpret_cast<float2*>(ws + L.off_rn);
    a.img = reinterpret_cast<uint16_t*>(ws + L.off_img);
    a.ctl = reinterpret_cast<uint32_t*>(ws + L.off_ctl);
    a.tile_hi = reinterpret_cast<float*>(ws + L.off_hi);
    a.best = reinterpret_cast<uint4*>(ws + L.off_best);
    a.cand = reinterpret_cast<int2*>(ws + L.off_cand);
    a.val = reinterpret_cast<float*>(ws + L.off_val);
    hipError_t e = hipMemsetAsync(a.ctl, 0, 64, s);
    if (e != hipSuccess) return e;
    if (S >= 2) {
        e = launch_coh_prepare(W, S, D, L.Sp, L.Dp, a.nrm, a.rn, a.img, a.ctl + CTL_NAN, s);
        if (e != hipSuccess) return e;
        const int grid = persistent_grid(L.ntiles);
        if (route == SAEV_COH_AUTO) {
            hipLaunchKernelGGL(coh_filter_kernel<1>, dim3(grid), dim3(256), 0, s, a);
            hipLaunchKernelGGL(coh_filter_kernel<2>, dim3(grid), dim3(256), 0, s, a);
            hipLaunchKernelGGL(coh_refine_kernel, dim3((int)std::min<long>((L.cap + 3) / 4, 2048)), dim3(256), 0, s, a);
        }
        hipLaunchKernelGGL(coh_exact_kernel, dim3(grid), dim3(256), 0, s, a);
    }
    hipLaunchKernelGGL(coh_finalize_kernel, dim3(1), dim3(1024), 0, s, a, out_value, out_pair, out_info);
    return hipGetLastError();
}
