// Muon on the two weight matrices (torch.optim.Muon, torch >= 2.9): momentum, Newton-Schulz orthogonalisation in bf16 on
// v_mfma_f32_32x32x16_bf16, decoupled weight decay and the update.  Both matrices run in the (d_model, d_sae) orientation --
// torch transposes the taller one -- so the decoder's (S, D) gradient is transposed on its way in and its update on its way
// out.  The orientation is zero-padded to (Dp, Sp) = multiples of 128: zero rows / columns stay exactly zero through every
// product and epilogue, so the GEMMs below run on whole 128 x 128 tiles with no bounds checks.
#include "common.h"
#include "kernels.h"

#include <algorithm>

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ float bf2f(uint16_t h) { return __uint_as_float((uint32_t)h << 16); }
__device__ __forceinline__ uint16_t f2bf(float f) {  // round to nearest even; a NaN stays a (quiet) NaN
    const uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40u);
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

constexpr int MT = 64;  // tile edge of the element-wise passes

// torch's lerp (ATen Lerp.h) as its kernels evaluate it, with the one rounding of the contracted form spelled out:
// weight < 0.5: self + weight * (end - self); else end - (end - self) * (1 - weight)
__device__ __forceinline__ float lerp_t(float self, float end, float w) {
#pragma clang fp contract(off)
    return fabsf(w) < 0.5f ? __builtin_fmaf(w, end - self, self) : __builtin_fmaf(w - 1.f, end - self, end);
}

__device__ __forceinline__ double block_sum_d(double v, double* red) {
    v = wave_sum_d(v);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) red[w] = v;
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x == 0)
        for (int i = 0; i < (int)(blockDim.x >> 6); ++i) t += red[i];
    return t;
}

// momentum buffer m <- lerp(m, g', 1 - mu), u = lerp(g', m, mu) (nesterov) or m, X = bf16(u) in the (D, S) orientation, and
// one double per workgroup: the sum of squares of its X elements.  g' = g * grad_scale * clip coefficient (the coefficient from
// the device sum of squares, as the fused Adam forms it).  trans: the source is (S, D) row-major (W_dec), else (D, S).
__global__ __launch_bounds__(256) void muon_momentum_kernel(MuonMomArgs a) {
#pragma clang fp contract(off)
    __shared__ uint16_t xs[MT][MT + 2];
    __shared__ double red[4];
    const float norm = a.grad_scale * (float)sqrt(*a.sumsq);
    const float coef = a.max_norm >= 0.f ? fminf(a.max_norm / (norm + 1e-6f), 1.f) : 1.f;
    const float gs = a.grad_scale * coef;
    const int s0 = blockIdx.x * MT, d0 = blockIdx.y * MT, t = threadIdx.x;
    for (int it = 0; it < MT * MT / 256; ++it) {
        const int e = it * 256 + t;
        const int dl = a.trans ? (e & 63) : (e >> 6), sl = a.trans ? (e >> 6) : (e & 63);
        const int d = d0 + dl, s = s0 + sl;
        uint16_t x = 0;
        if (d < a.D && s < a.S) {
            const long i = a.trans ? (long)s * a.D + d : (long)d * a.S + s;
            const float g = a.g[i] * gs;
            const float m = lerp_t(a.m[i], g, a.w_buf);
            a.m[i] = m;
            x = f2bf(a.nesterov ? lerp_t(g, m, a.mu) : m);
        }
        xs[dl][sl] = x;
    }
    __syncthreads();
    double sq = 0.0;
    for (int it = 0; it < MT * MT / 256; ++it) {
        const int e = it * 256 + t, dl = e >> 6, sl = e & 63;
        const int d = d0 + dl, s = s0 + sl;
        if (d < a.D && s < a.S) {
            const float x = bf2f(xs[dl][sl]);
            a.X[(long)d * a.ldx + s] = xs[dl][sl];
            sq += (double)x * (double)x;
        }
    }
    const double tot = block_sum_d(sq, red);
    if (t == 0) a.sq_part[blockIdx.y * gridDim.x + blockIdx.x] = tot;
}

// a caller's bf16 (D, S) matrix into the padded orientation, with the same per-workgroup squares
__global__ __launch_bounds__(256) void muon_load_kernel(const uint16_t* __restrict__ src, int D, int S, uint16_t* X, int ldx,
                                                       double* sq_part) {
    __shared__ double red[4];
    const int s0 = blockIdx.x * MT, d0 = blockIdx.y * MT, t = threadIdx.x;
    double sq = 0.0;
    for (int it = 0; it < MT * MT / 256; ++it) {
        const int e = it * 256 + t, d = d0 + (e >> 6), s = s0 + (e & 63);
        if (d < D && s < S) {
            const uint16_t h = src[(long)d * S + s];
            X[(long)d * ldx + s] = h;
            const float x = bf2f(h);
            sq += (double)x * (double)x;
        }
    }
    const double tot = block_sum_d(sq, red);
    if (t == 0) sq_part[blockIdx.y * gridDim.x + blockIdx.x] = tot;
}

// ||X|| from the per-workgroup squares in a fixed order, rounded to bf16 and clamped as torch's bf16 norm() / clamp() leave it
__global__ __launch_bounds__(256) void muon_norm_kernel(const double* sq_part, int nb, float eps, float* nrm) {
    __shared__ double red[4];
    double v = 0.0;
    for (int i = threadIdx.x; i < nb; i += 256) v += sq_part[i];
    const double tot = block_sum_d(v, red);
    if (threadIdx.x == 0) *nrm = bf2f(f2bf(fmaxf(bf2f(f2bf((float)sqrt(tot))), eps)));
}

// X /= nrm: each element divided in fp32 and rounded to bf16 (torch's bf16 div_)
__global__ __launch_bounds__(256) void muon_scale_kernel(uint16_t* X, long n8, const float* nrm_p) {
    const float nrm = *nrm_p;
    for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < n8; q += (long)gridDim.x * 256) {
        u16x8 x = reinterpret_cast<u16x8*>(X)[q];
#pragma unroll
        for (int j = 0; j < 8; ++j) x[j] = f2bf(bf2f(x[j]) / nrm);
        reinterpret_cast<u16x8*>(X)[q] = x;
    }
}

// p <- p * decay - adj_lr * X(^T): the X tile through LDS so that both orientations of W are walked along their rows
__global__ __launch_bounds__(256) void muon_apply_kernel(float* W, const uint16_t* __restrict__ X, int ldx, int D, int S, int trans,
                                                        float decay, float adj_lr) {
#pragma clang fp contract(off)
    __shared__ uint16_t xs[MT][MT + 2];
    const int s0 = blockIdx.x * MT, d0 = blockIdx.y * MT, t = threadIdx.x;
    for (int it = 0; it < MT * MT / 256; ++it) {
        const int e = it * 256 + t, dl = e >> 6, sl = e & 63;
        const int d = d0 + dl, s = s0 + sl;
        xs[dl][sl] = (d < D && s < S) ? X[(long)d * ldx + s] : (uint16_t)0;
    }
    __syncthreads();
    for (int it = 0; it < MT * MT / 256; ++it) {
        const int e = it * 256 + t;
        const int dl = trans ? (e & 63) : (e >> 6), sl = trans ? (e >> 6) : (e & 63);
        const int d = d0 + dl, s = s0 + sl;
        if (d < D && s < S) {
            const long i = trans ? (long)s * D + d : (long)d * S + s;
            const float p = W[i] * decay;
            W[i] = __builtin_fmaf(-adj_lr, bf2f(xs[dl][sl]), p);
        }
    }
}

// ---- bf16 GEMM: C (M x N) = A (M x K, row-major) . B, fp32 accumulate ----------------------------------------------------
// B_NN = false: B is given as Bt (N x K, row-major) -- both operands contiguous in k (X X^T, G G with G symmetric);
// B_NN = true:  B is (K x N, row-major) and is transposed on its way into LDS (U X).
// 128 x 128 tile per workgroup, four waves of 64 x 64 (2 x 2 MFMA 32x32x16 tiles), k in steps of 32 through LDS, the next
// step's global loads issued before the current step's MFMAs.  Split-K: blockIdx.z takes k range [z kper, (z+1) kper) and
// writes its fp32 tile to P[z]; muon_reduce_kernel sums the splits in order z = 0, 1, ... (no atomics: bit-reproducible).
// Without split-K the epilogue bf16(alpha acc + beta Cin) runs here.  sym: only tiles on or above the diagonal run.
constexpr int GT = 128, GK = 32, LDS_K = GK + 8;  // (+8 bf16 of padding: row pitch 80 B)

template <bool B_NN>
__global__ __launch_bounds__(256, 2) void muon_gemm_kernel(MuonGemmArgs g) {
    const int bn = blockIdx.x, bm = blockIdx.y, z = blockIdx.z;
    if (g.sym && bn < bm) return;
    __shared__ __attribute__((aligned(16))) uint16_t As[GT][LDS_K];
    __shared__ __attribute__((aligned(16))) uint16_t Bs[GT][LDS_K];  // [n][k]
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int wm = (w >> 1) * 64, wn = (w & 1) * 64;
    const int k_lo = z * g.kper, k_hi = min(g.K, k_lo + g.kper);
    const uint16_t* A = g.A + (long)bm * GT * g.lda;
    // per-thread global load slots: A (and Bt) rows r = t / 4 and 64 + t / 4, 8 k at (t & 3) * 8; B (NN): k rows t / 16 and
    // 16 + t / 16, 8 n at (t & 15) * 8
    const int ar = t >> 2, ac = (t & 3) * 8;
    const int bk = t >> 4, bc = (t & 15) * 8;
    u16x8 ra[2], rb[2];
    auto load = [&](int k0) {
        ra[0] = *reinterpret_cast<const u16x8*>(A + (long)ar * g.lda + k0 + ac);
        ra[1] = *reinterpret_cast<const u16x8*>(A + (long)(ar + 64) * g.lda + k0 + ac);
        if constexpr (B_NN) {
            const uint16_t* B = g.B + (long)bn * GT;
            rb[0] = *reinterpret_cast<const u16x8*>(B + (long)(k0 + bk) * g.ldb + bc);
            rb[1] = *reinterpret_cast<const u16x8*>(B + (long)(k0 + bk + 16) * g.ldb + bc);
        } else {
            const uint16_t* B = g.B + (long)bn * GT * g.ldb;
            rb[0] = *reinterpret_cast<const u16x8*>(B + (long)ar * g.ldb + k0 + ac);
            rb[1] = *reinterpret_cast<const u16x8*>(B + (long)(ar + 64) * g.ldb + k0 + ac);
        }
    };
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    if (k_lo < k_hi) load(k_lo);
    const int r32 = lane & 31, h = lane >> 5;
    for (int k0 = k_lo; k0 < k_hi; k0 += GK) {
        *reinterpret_cast<u16x8*>(&As[ar][ac]) = ra[0];
        *reinterpret_cast<u16x8*>(&As[ar + 64][ac]) = ra[1];
        if constexpr (B_NN) {
#pragma unroll
            for (int j = 0; j < 8; ++j) { Bs[bc + j][bk] = rb[0][j]; Bs[bc + j][bk + 16] = rb[1][j]; }
        } else {
            *reinterpret_cast<u16x8*>(&Bs[ar][ac]) = rb[0];
            *reinterpret_cast<u16x8*>(&Bs[ar + 64][ac]) = rb[1];
        }
        __syncthreads();
        if (k0 + GK < k_hi) load(k0 + GK);
#pragma unroll
        for (int ks = 0; ks < GK; ks += 16) {
            bf16x8 fa[2], fb[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                fa[i] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u16x8*>(&As[wm + 32 * i + r32][ks + 8 * h]));
                fb[i] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u16x8*>(&Bs[wn + 32 * i + r32][ks + 8 * h]));
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
    }
    // C/D map of 32x32x16: column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 h
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = bm * GT + wm + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * h;
                const int n = bn * GT + wn + 32 * j + r32;
                if (g.P) {
                    g.P[(long)z * g.M * g.N + (long)m * g.N + n] = acc[i][j][r];
                } else {
#pragma clang fp contract(off)
                    float v = g.alpha * acc[i][j][r];
                    if (g.Cin) v = v + g.beta * bf2f(g.Cin[(long)m * g.ldc + n]);
                    g.C[(long)m * g.ldc + n] = f2bf(v);
                }
            }
}

// C = bf16(alpha sum_z P[z] + beta Cin), splits in order; sym: element (i, j) is read at (min, max) -- the result is exactly
// symmetric whatever the MFMA's internal order on the diagonal tiles
__global__ __launch_bounds__(256) void muon_reduce_kernel(MuonGemmArgs g, int splits) {
#pragma clang fp contract(off)
    const long MN = (long)g.M * g.N;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < MN; e += (long)gridDim.x * 256) {
        int i = (int)(e / g.N), j = (int)(e % g.N);
        if (g.sym && i > j) { const int tmp = i; i = j; j = tmp; }
        const long src = (long)i * g.N + j;
        float acc = 0.f;
        for (int z = 0; z < splits; ++z) acc += g.P[(long)z * MN + src];
        float v = g.alpha * acc;
        if (g.Cin) v = v + g.beta * bf2f(g.Cin[(long)i * g.ldc + j]);
        g.C[e / g.N * (long)g.ldc + e % g.N] = f2bf(v);
    }
}

int round_up(long v, int m) { return (int)((v + m - 1) / m * m); }

// k tiles per split and the number of splits of a product: about 512 workgroups in flight, at most max_splits
void gemm_splits(int tm, int tn, int kt, bool sym, int max_splits, int* kper_t, int* splits) {
    const int tiles = sym ? tm * (tm + 1) / 2 : tm * tn;
    int n = std::min(max_splits, std::max(1, (512 + tiles - 1) / tiles));
    n = std::min(n, kt);
    *kper_t = (kt + n - 1) / n;
    *splits = (kt + *kper_t - 1) / *kper_t;
}

// A symmetric product always goes through the partials and muon_reduce_kernel, one split or several: the GEMM computes the
// upper tiles only, the reduce writes both triangles.
hipError_t gemm(MuonGemmArgs g, bool nn, int max_splits, float* P, hipStream_t s) {
    const int tm = g.M / GT, tn = g.N / GT, kt = g.K / GK;
    int kper_t = 0, splits = 0;
    gemm_splits(tm, tn, kt, g.sym != 0, max_splits, &kper_t, &splits);
    g.kper = kper_t * GK;
    const bool reduce = splits > 1 || g.sym;
    g.P = reduce ? P : nullptr;
    if (nn) hipLaunchKernelGGL(muon_gemm_kernel<true>, dim3(tn, tm, splits), dim3(256), 0, s, g);
    else hipLaunchKernelGGL(muon_gemm_kernel<false>, dim3(tn, tm, splits), dim3(256), 0, s, g);
    if (reduce) {
        const long MN = (long)g.M * g.N;
        hipLaunchKernelGGL(muon_reduce_kernel, dim3((int)std::min<long>((MN + 255) / 256, 2048)), dim3(256), 0, s, g, splits);
    }
    return hipGetLastError();
}

}  // namespace

MuonLayout muon_layout(int D, int S) {
    MuonLayout L{};
    L.Dp = round_up(D, GT); L.Sp = round_up(S, GT);
    L.nb = ((S + MT - 1) / MT) * ((D + MT - 1) / MT);
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += (bytes + 255) / 256 * 256; return o; };
    const size_t xb = (size_t)L.Dp * L.Sp * 2, gb = (size_t)L.Dp * L.Dp * 2;
    L.off_X[0] = take(xb); L.off_X[1] = take(xb);
    L.off_G = take(gb); L.off_U = take(gb);
    // the partials of the two symmetric products (X X^T: k = Sp, G G: k = Dp), sized by the splits they take
    int kper_t = 0, sp_gram = 0, sp_gg = 0;
    gemm_splits(L.Dp / GT, L.Dp / GT, L.Sp / GK, true, MUON_MAX_SPLITS, &kper_t, &sp_gram);
    gemm_splits(L.Dp / GT, L.Dp / GT, L.Dp / GK, true, MUON_MAX_SPLITS, &kper_t, &sp_gg);
    L.splits = std::max(sp_gram, sp_gg);
    L.off_P = take((size_t)L.splits * L.Dp * L.Dp * 4);
    L.off_sq = take((size_t)L.nb * 8);
    L.off_nrm = take(4);
    L.bytes = off;
    return L;
}

hipError_t launch_muon_momentum(const MuonMomArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(muon_momentum_kernel, dim3((a.S + MT - 1) / MT, (a.D + MT - 1) / MT), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_muon_load(const uint16_t* src, int D, int S, uint16_t* X, int ldx, double* sq_part, hipStream_t s) {
    hipLaunchKernelGGL(muon_load_kernel, dim3((S + MT - 1) / MT, (D + MT - 1) / MT), dim3(256), 0, s, src, D, S, X, ldx, sq_part);
    return hipGetLastError();
}

hipError_t launch_muon_apply(float* W, const uint16_t* X, int ldx, int D, int S, int trans, float decay, float adj_lr, hipStream_t s) {
    hipLaunchKernelGGL(muon_apply_kernel, dim3((S + MT - 1) / MT, (D + MT - 1) / MT), dim3(256), 0, s, W, X, ldx, D, S, trans, decay, adj_lr);
    return hipGetLastError();
}

int muon_newton_schulz(uint8_t* ws, const MuonLayout& L, int D, int S, int normalize, int steps, float a, float b, float c, float eps,
                       hipStream_t s, hipError_t* err) {
    uint16_t* X[2] = {reinterpret_cast<uint16_t*>(ws + L.off_X[0]), reinterpret_cast<uint16_t*>(ws + L.off_X[1])};
    uint16_t* G = reinterpret_cast<uint16_t*>(ws + L.off_G);
    uint16_t* U = reinterpret_cast<uint16_t*>(ws + L.off_U);
    float* P = reinterpret_cast<float*>(ws + L.off_P);
    const double* sq = reinterpret_cast<const double*>(ws + L.off_sq);
    hipError_t e = hipSuccess;
    if (normalize) {
        const long n8 = (long)L.Dp * L.Sp / 8;
        float* nrm = reinterpret_cast<float*>(ws + L.off_nrm);
        hipLaunchKernelGGL(muon_norm_kernel, dim3(1), dim3(256), 0, s, sq, L.nb, eps, nrm);
        hipLaunchKernelGGL(muon_scale_kernel, dim3((int)std::min<long>((n8 + 255) / 256, 2048)), dim3(256), 0, s, X[0], n8, (const float*)nrm);
        if ((e = hipGetLastError()) != hipSuccess) { *err = e; return -1; }
    }
    int cur = 0;
    for (int it = 0; it < steps; ++it) {
        MuonGemmArgs g{};
        // G = X X^T (upper tiles, split-K)
        g.A = X[cur]; g.lda = L.Sp; g.B = X[cur]; g.ldb = L.Sp; g.M = L.Dp; g.N = L.Dp; g.K = L.Sp;
        g.C = G; g.ldc = L.Dp; g.alpha = 1.f; g.beta = 0.f; g.Cin = nullptr; g.sym = 1;
        if ((e = gemm(g, false, MUON_MAX_SPLITS, P, s)) != hipSuccess) { *err = e; return -1; }
        // U = b G + c G G (G symmetric: G itself is G^T)
        g.A = G; g.lda = L.Dp; g.B = G; g.ldb = L.Dp; g.K = L.Dp;
        g.C = U; g.alpha = c; g.beta = b; g.Cin = G; g.sym = 1;
        if ((e = gemm(g, false, MUON_MAX_SPLITS, P, s)) != hipSuccess) { *err = e; return -1; }
        // X' = a X + U X
        g.A = U; g.lda = L.Dp; g.B = X[cur]; g.ldb = L.Sp; g.M = L.Dp; g.N = L.Sp; g.K = L.Dp;
        g.C = X[cur ^ 1]; g.ldc = L.Sp; g.alpha = 1.f; g.beta = a; g.Cin = X[cur]; g.sym = 0;
        if ((e = gemm(g, true, 1, P, s)) != hipSuccess) { *err = e; return -1; }
        cur ^= 1;
    }
    (void)D; (void)S;
    return cur;
}
