// Batch statistics of the host's log block, evaluate() and the inference pass (include/saev_amd.h: BATCH STATISTICS; DESIGN.md
// 3.12): everything those three need from a batch x, its reconstruction x_hat and its codes, as streaming reductions with no
// n x D or n x k temporary.
//
//   dense    one pass over x and x_hat.  Workgroup g owns the rows [g rpb, (g + 1) rpb); a thread owns up to four float4 column
//            groups (q = qi + 256 j) and, where the row is narrower than the workgroup, one of R = 256 / P row phases.  Every
//            sum is fp64: x and x_hat widen exactly, r = x - x_hat is one rounding, x^2 and r^2 are fmas.  A thread adds its rows in
//            ascending order; the row phases, the lanes of a wave (xor butterfly) and the waves are combined in a fixed order.
//            Each workgroup leaves [n_kept, sum x, sum x^2, sum r, sum r^2, 0, 0, 0 | column sums (D)] in the workspace.
//   finish   column c of the partials summed in workgroup order (sixteen slices of the workgroups, then the slices in order) and
//            added to -- or, with SAEV_BATCH_OVERWRITE, stored over -- the caller's accumulators.  No floating-point atomic:
//            col_sum and scalars are the same bits from run to run.
//   codes    one thread per slot of the padded code rows: integer atomics into n_pos, fp64 vector atomics into value_sum
//            (reproducible to fp64 rounding only: the order of the adds is not fixed), plain stores of 1 into live.
//   row norm one wave per decoder row: the squares exact in fp64, their sum in lane order and butterfly, the square root rounded
//            to fp32 (the correctly rounded fp32 norm), the norms of a wave's rows added in row order, then waves, workgroups.
#include "common.h"
#include "kernels.h"

#include <algorithm>
#include <cstring>
#include <string>

namespace {

constexpr int BS_MAX_GROUPS = 1024;   // workgroups of the dense pass (rows of partials in the workspace)
constexpr int BS_ROWS_PER_GROUP = 16; // fewest rows a workgroup takes
constexpr int BS_NSCAL = 8;           // scalars in front of the column sums of a partial row
constexpr int RN_MAX_GROUPS = 1024;   // workgroups of the row-norm pass

// NJ: float4 column groups per thread (D <= 1024 NJ); XH: x_hat present.  lgP: log2 of the threads that share a row.
template <int NJ, bool XH>
__global__ __launch_bounds__(256) void bs_dense_kernel(const float* __restrict__ x, const float* __restrict__ xh,
                                                       const uint8_t* __restrict__ keep, int n, int D, int rpb, int lgP,
                                                       double* __restrict__ part) {
    constexpr int U = NJ == 1 ? 4 : (NJ == 2 ? 2 : 1);  // rows in flight per thread: 8 x 16 B loads at every width
    __shared__ double sm[256 * 4];
    __shared__ double sw[4][5];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int nq = D >> 2, P = 1 << lgP, R = 256 >> lgP;
    const int qi = t & (P - 1), rs = t >> lgP;
    const int row0 = blockIdx.x * rpb, row1 = min(n, row0 + rpb);
    double col[NJ][4];
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) col[j][e] = 0.0;
    double sx = 0.0, sxx = 0.0, sr = 0.0, srr = 0.0, nk = 0.0;
    for (int rb = row0 + rs; rb < row1; rb += R * U) {
        f32x4 a[U][NJ], b[U][NJ];
        uint8_t kept[U];
#pragma unroll
        for (int u = 0; u < U; ++u) kept[u] = keep == nullptr ? (uint8_t)1 : keep[min(rb + u * R, row1 - 1)];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            // every load is issued, from a clamped (valid) address, and masked afterwards: the 2 U NJ loads of an iteration are
            // in flight together instead of one branch and one wait per row
            const int r = rb + u * R, rc = min(r, row1 - 1);
            const bool on = r < row1 && kept[u] != 0;
            if (on && qi == 0) nk += 1.0;
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int q = qi + 256 * j, qc = min(q, nq - 1);
                const size_t at = (size_t)rc * D + 4 * qc;
                a[u][j] = *reinterpret_cast<const f32x4*>(x + at);
                if (XH) b[u][j] = *reinterpret_cast<const f32x4*>(xh + at);
                if (!(on && q < nq)) {
                    a[u][j] = f32x4{0.f, 0.f, 0.f, 0.f};
                    if (XH) b[u][j] = f32x4{0.f, 0.f, 0.f, 0.f};
                }
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int j = 0; j < NJ; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const double xv = (double)a[u][j][e];
                    col[j][e] += xv;
                    sx += xv;
                    sxx = __builtin_fma(xv, xv, sxx);
                    if (XH) {
                        const double rv = xv - (double)b[u][j][e];
                        sr += rv;
                        srr = __builtin_fma(rv, rv, srr);
                    }
                }
    }
    double* out = part + (size_t)blockIdx.x * (BS_NSCAL + D);
    // scalars: lanes by butterfly, waves in order
    nk = wave_sum_d(nk); sx = wave_sum_d(sx); sxx = wave_sum_d(sxx); sr = wave_sum_d(sr); srr = wave_sum_d(srr);
    if (lane == 0) { sw[w][0] = nk; sw[w][1] = sx; sw[w][2] = sxx; sw[w][3] = sr; sw[w][4] = srr; }
    if (R > 1) {
#pragma unroll
        for (int e = 0; e < 4; ++e) sm[t * 4 + e] = col[0][e];
    }
    __syncthreads();
    if (t < BS_NSCAL) out[t] = t < 5 ? ((sw[0][t] + sw[1][t]) + sw[2][t]) + sw[3][t] : 0.0;
    if (R > 1) {  // (NJ == 1) row phases in order
        if (rs == 0 && qi < nq) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                double s = sm[qi * 4 + e];
                for (int p = 1; p < R; ++p) s += sm[(p * P + qi) * 4 + e];
                out[BS_NSCAL + 4 * qi + e] = s;
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int q = qi + 256 * j;
            if (q < nq) {
#pragma unroll
                for (int e = 0; e < 4; ++e) out[BS_NSCAL + 4 * q + e] = col[j][e];
            }
        }
    }
}

// 16 columns x 16 slices of the G partial rows per workgroup
__global__ __launch_bounds__(256) void bs_finish_kernel(const double* __restrict__ part, int G, int D, int overwrite,
                                                        double* scalars, double* col_sum) {
    __shared__ double sm[16][16];
    const int t = threadIdx.x, cl = t & 15, s = t >> 4;
    const int C = BS_NSCAL + D, c = blockIdx.x * 16 + cl;
    double acc = 0.0;
    if (c < C) {
        const int g0 = (int)((long)s * G / 16), g1 = (int)((long)(s + 1) * G / 16);
        for (int g = g0; g < g1; ++g) acc += part[(size_t)g * C + c];
    }
    sm[s][cl] = acc;
    __syncthreads();
    if (s == 0 && c < C) {
        double tot = sm[0][cl];
        for (int p = 1; p < 16; ++p) tot += sm[p][cl];
        double* dst = c < BS_NSCAL ? (scalars ? scalars + c : nullptr) : (col_sum ? col_sum + (c - BS_NSCAL) : nullptr);
        if (dst) *dst = overwrite ? tot : *dst + tot;
    }
}

__global__ __launch_bounds__(256) void bs_codes_kernel(const int32_t* __restrict__ idx, const float* __restrict__ val,
                                                       const int32_t* __restrict__ row_nnz, const uint8_t* __restrict__ keep,
                                                       long total, int cap, int S, float live_eps, unsigned long long* n_pos,
                                                       double* value_sum, int32_t* live) {
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const long row = e / cap;
        const int slot = (int)(e - row * cap);
        if (keep != nullptr && keep[row] == 0) continue;
        if (row_nnz != nullptr && slot >= row_nnz[row]) continue;  // (a count above cap reads as cap: slot < cap always)
        const int i = idx[e];
        if (i < 0 || i >= S) continue;
        const float v = val[e];
        if (n_pos != nullptr && v > 0.f) atomicAdd(n_pos + i, 1ull);
        if (value_sum != nullptr && v != 0.f) unsafeAtomicAdd(value_sum + i, (double)v);
        if (live != nullptr && fabsf(v) > live_eps) live[i] = 1;
    }
}

__global__ __launch_bounds__(256) void rn_rows_kernel(const float* __restrict__ W, int S, int D, double* __restrict__ part) {
    __shared__ double sw[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int nq = D >> 2;
    double acc = 0.0;
    for (int r = blockIdx.x * 4 + w; r < S; r += gridDim.x * 4) {
        const f32x4* p = reinterpret_cast<const f32x4*>(W + (size_t)r * D);
        double ss = 0.0;
        for (int q0 = 0; q0 < nq; q0 += 256) {
            f32x4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int q = q0 + 64 * u + lane;
                v[u] = q < nq ? p[q] : f32x4{0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int e = 0; e < 4; ++e) ss = __builtin_fma((double)v[u][e], (double)v[u][e], ss);
        }
        ss = wave_sum_d(ss);
        acc += (double)(float)sqrt(ss);
    }
    if (lane == 0) sw[w] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = ((sw[0] + sw[1]) + sw[2]) + sw[3];
}

__global__ __launch_bounds__(256) void rn_finish_kernel(const double* __restrict__ part, int G, int S, double* out) {
    __shared__ double sw[4];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    double acc = 0.0;
    for (int g = 4 * t; g < min(G, 4 * t + 4); ++g) acc += part[g];
    acc = wave_sum_d(acc);
    if (lane == 0) sw[w] = acc;
    __syncthreads();
    if (t == 0) *out = (((sw[0] + sw[1]) + sw[2]) + sw[3]) / (double)S;
}

int bs_groups(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>(BS_MAX_GROUPS, (n + BS_ROWS_PER_GROUP - 1) / BS_ROWS_PER_GROUP)); }

template <int NJ>
void launch_dense(bool has_xh, int G, hipStream_t s, const float* x, const float* xh, const uint8_t* keep, int n, int D, int rpb,
                  int lgP, double* part) {
    if (has_xh) hipLaunchKernelGGL((bs_dense_kernel<NJ, true>), dim3(G), dim3(256), 0, s, x, xh, keep, n, D, rpb, lgP, part);
    else hipLaunchKernelGGL((bs_dense_kernel<NJ, false>), dim3(G), dim3(256), 0, s, x, xh, keep, n, D, rpb, lgP, part);
}

thread_local std::string g_free_err;

int refuse(int code, const std::string& msg) {
    g_free_err = msg;
    return code;
}

}  // namespace

const char* free_error() { return g_free_err.empty() ? "null context" : g_free_err.c_str(); }
int free_refuse(int code, const char* msg) { return refuse(code, msg); }

int64_t saev_batch_stats_workspace_bytes(int64_t n, int64_t D) {
    if (n < 0 || n > 0x7fffffffLL || D < 4 || D > 4096 || D % 4 != 0) return -1;
    const int64_t bytes = (int64_t)bs_groups(n) * (BS_NSCAL + D) * 8;
    return (bytes + 255) / 256 * 256;
}

int saev_batch_stats(const float* x, const float* x_hat, const int32_t* idx, const float* val, const int32_t* row_nnz,
                     const uint8_t* keep, int64_t n, int64_t D, int64_t S, int64_t cap, const saev_batch_acc* acc, void* workspace,
                     int64_t workspace_bytes, void* stream) {
    if (n < 0 || D < 0 || S < 0 || cap < 0) return refuse(SAEV_INVALID_ARG, "saev_batch_stats: negative size");
    if (n > 0x7fffffffLL || S > 0x7fffffffLL || cap > 0x7fffffffLL) return refuse(SAEV_INVALID_ARG, "saev_batch_stats: size above 2^31 - 1");
    if (D < 4 || D % 4 != 0) return refuse(SAEV_UNSUPPORTED, "saev_batch_stats: d_model must be a positive multiple of 4");
    if (D > 4096) return refuse(SAEV_UNSUPPORTED, "saev_batch_stats: d_model above 4096");
    if (!acc || acc->struct_size < (int32_t)(3 * sizeof(int32_t))) return refuse(SAEV_INVALID_ARG, "saev_batch_stats: no saev_batch_acc (or its struct_size is unset)");
    saev_batch_acc a;
    std::memset(&a, 0, sizeof a);
    std::memcpy(&a, acc, std::min<size_t>(sizeof a, (size_t)acc->struct_size));
    if (a.flags & ~SAEV_BATCH_OVERWRITE) return refuse(SAEV_INVALID_ARG, "saev_batch_stats: unknown flag");
    if (n == 0) return SAEV_OK;
    if (!x) return refuse(SAEV_INVALID_ARG, "saev_batch_stats: x is NULL");
    const bool dense = a.col_sum || a.scalars;
    const bool codes = (a.n_pos || a.value_sum || a.live) && cap > 0 && S > 0;
    if (dense) {
        if (((uintptr_t)x & 15) != 0 || ((uintptr_t)x_hat & 15) != 0) return refuse(SAEV_INVALID_ARG, "saev_batch_stats: x and x_hat must be 16-byte aligned");
        const int64_t need = saev_batch_stats_workspace_bytes(n, D);
        if (!workspace || workspace_bytes < need) return refuse(SAEV_INVALID_ARG, "saev_batch_stats: workspace smaller than saev_batch_stats_workspace_bytes(n, D)");
        if (((uintptr_t)workspace & 255) != 0) return refuse(SAEV_INVALID_ARG, "saev_batch_stats: workspace must be 256-byte aligned");
    }
    if (codes && (!idx || !val)) return refuse(SAEV_INVALID_ARG, "saev_batch_stats: idx / val are NULL");
    hipStream_t s = (hipStream_t)stream;
    const int overwrite = (a.flags & SAEV_BATCH_OVERWRITE) != 0;
    if (dense) {
        const int nq = (int)D / 4, NJ = (nq + 255) / 256;
        int lgP = 8;
        if (nq < 256) { lgP = 0; while ((1 << lgP) < nq) ++lgP; }
        const int rpb = (int)((n + bs_groups(n) - 1) / bs_groups(n));
        const int G = (int)((n + rpb - 1) / rpb);
        double* part = static_cast<double*>(workspace);
        const bool xh = x_hat != nullptr;
        switch (NJ) {
            case 1: launch_dense<1>(xh, G, s, x, x_hat, keep, (int)n, (int)D, rpb, lgP, part); break;
            case 2: launch_dense<2>(xh, G, s, x, x_hat, keep, (int)n, (int)D, rpb, lgP, part); break;
            case 3: launch_dense<3>(xh, G, s, x, x_hat, keep, (int)n, (int)D, rpb, lgP, part); break;
            default: launch_dense<4>(xh, G, s, x, x_hat, keep, (int)n, (int)D, rpb, lgP, part); break;
        }
        hipLaunchKernelGGL(bs_finish_kernel, dim3((BS_NSCAL + (int)D + 15) / 16), dim3(256), 0, s, part, G, (int)D, overwrite, a.scalars, a.col_sum);
    }
    if (overwrite && S > 0) {
        if (a.n_pos && hipMemsetAsync(a.n_pos, 0, (size_t)S * 8, s) != hipSuccess) return refuse(SAEV_HIP_ERROR, "saev_batch_stats: hipMemsetAsync failed");
        if (a.value_sum && hipMemsetAsync(a.value_sum, 0, (size_t)S * 8, s) != hipSuccess) return refuse(SAEV_HIP_ERROR, "saev_batch_stats: hipMemsetAsync failed");
    }
    if (codes) {
        const long total = (long)n * cap;
        const int grid = (int)std::min<long>((total + 255) / 256, 8192);
        hipLaunchKernelGGL(bs_codes_kernel, dim3(grid), dim3(256), 0, s, idx, val, row_nnz, keep, total, (int)cap, (int)S, a.live_eps,
                           reinterpret_cast<unsigned long long*>(a.n_pos), a.value_sum, a.live);
    }
    if (hipGetLastError() != hipSuccess) return refuse(SAEV_HIP_ERROR, "saev_batch_stats: kernel launch failed");
    return SAEV_OK;
}

int saev_row_norm_mean(const float* W, int64_t S, int64_t D, double* out, void* workspace, int64_t workspace_bytes, void* stream) {
    if (S < 1 || S > 0x7fffffffLL || D < 0) return refuse(SAEV_INVALID_ARG, "saev_row_norm_mean: needs 1 <= S < 2^31 rows");
    if (D < 4 || D % 4 != 0) return refuse(SAEV_UNSUPPORTED, "saev_row_norm_mean: d_model must be a positive multiple of 4");
    if (D > 4096) return refuse(SAEV_UNSUPPORTED, "saev_row_norm_mean: d_model above 4096");
    if (!W || !out) return refuse(SAEV_INVALID_ARG, "saev_row_norm_mean: W or out is NULL");
    if (((uintptr_t)W & 15) != 0 || ((uintptr_t)out & 7) != 0) return refuse(SAEV_INVALID_ARG, "saev_row_norm_mean: W must be 16-byte aligned, out 8-byte");
    if (!workspace || workspace_bytes < SAEV_ROW_NORM_WORKSPACE_BYTES || ((uintptr_t)workspace & 255) != 0)
        return refuse(SAEV_INVALID_ARG, "saev_row_norm_mean: workspace of SAEV_ROW_NORM_WORKSPACE_BYTES bytes, 256-byte aligned");
    static_assert(RN_MAX_GROUPS * 8 <= SAEV_ROW_NORM_WORKSPACE_BYTES, "row-norm workspace");
    hipStream_t s = (hipStream_t)stream;
    const int G = (int)std::min<int64_t>(RN_MAX_GROUPS, (S + 3) / 4);
    double* part = static_cast<double*>(workspace);
    hipLaunchKernelGGL(rn_rows_kernel, dim3(G), dim3(256), 0, s, W, (int)S, (int)D, part);
    hipLaunchKernelGGL(rn_finish_kernel, dim3(1), dim3(256), 0, s, part, G, (int)S, out);
    if (hipGetLastError() != hipSuccess) return refuse(SAEV_HIP_ERROR, "saev_row_norm_mean: kernel launch failed");
    return SAEV_OK;
}
