// ReLU SAE forward: encoder with a sparse, variable-length output, decode and scatter of variable-length rows.
//
// relu_encode_kernel    f = relu(x W_enc + b_enc) (reference nn/modeling.py:343-347 encode, :150-156 ReluActivation) without a
//                       dense h.  One workgroup owns RE_BM rows and sweeps ALL latents of them in ascending tiles of RE_BN, so
//                       the compaction needs no cross-workgroup ordering: per tile, every lane ballots its positives, the
//                       position of an entry in its row is the row's running count + the positives of the lanes (and the own
//                       columns) before it, and the running count grows by the tile's total.  Entries come out in ascending
//                       latent order.  A row's count keeps growing past row_cap (only the first row_cap entries are stored), so
//                       row_nnz is exact and the caller can size a second launch from it.
//                       Arithmetic: exact fp32 (one fmaf per product, k-ordered), on the vector ALU.
// relu_decode_kernel    x_hat[b, p, :] = b_dec + sum_{j < row_nnz[b], idx < prefixes[p]} val W_dec[idx]; cost ~ row_nnz.
// relu_scatter_kernel   f_out[b, idx] = val for j < row_nnz[b] (dense f_x for API compatibility).
#include "common.h"
#include "kernels.h"

namespace {

constexpr int RE_BM = 32;   // rows per workgroup
constexpr int RE_BN = 128;  // latents per tile
constexpr int RE_BK = 16;   // d_model per LDS stage
constexpr int RE_THREADS = 256;

// Thread (ty = tid / 32, tx = tid % 32) holds rows ty*4 .. +3 and latents tx*4 .. +3 of the tile.  Lanes 0-31 of a wave hold one
// group of four rows, lanes 32-63 the next: a row's 128 latents live in one half-wave, in ascending lane order.
__global__ __launch_bounds__(RE_THREADS) void relu_encode_kernel(ReluEncodeArgs a) {
    __shared__ float xs[RE_BK][RE_BM];  // x chunk, transposed
    __shared__ float ws[RE_BK][RE_BN];  // W_enc chunk
    const int tid = threadIdx.x, tx = tid & 31, ty = tid >> 5;
    const int row0 = blockIdx.x * RE_BM;
    const int D = a.D, S = a.S;
    const uint32_t lane = tid & 63;
    const uint64_t half = lane < 32 ? 0x00000000ffffffffull : 0xffffffff00000000ull;
    const uint64_t below = ((1ull << lane) - 1ull) & half;
    int cnt[4] = {0, 0, 0, 0};  // running positives of this thread's four rows (the same in every lane of the half-wave)

    for (int n0 = 0; n0 < S; n0 += RE_BN) {
        float acc[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
        for (int k0 = 0; k0 < D; k0 += RE_BK) {
            // x: 32 rows x 16 columns = 128 float4 (threads 0-127); D % 4 == 0, so a float4 is wholly in or out
            if (tid < 128) {
                const int r = tid >> 2, kq = (tid & 3) * 4, gr = row0 + r, gk = k0 + kq;
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (gr < a.n_rows && gk < D) v = *reinterpret_cast<const f32x4*>(a.x + (size_t)gr * D + gk);
#pragma unroll
                for (int e = 0; e < 4; ++e) xs[kq + e][r] = v[e];
            }
            // W_enc: 16 rows x 128 latents = 512 float4, two per thread; S % 4 == 0
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int q = tid + h * RE_THREADS, kr = q >> 5, c = (q & 31) * 4, gk = k0 + kr, gc = n0 + c;
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (gk < D && gc < S) v = *reinterpret_cast<const f32x4*>(a.W_enc + (size_t)gk * S + gc);
                *reinterpret_cast<f32x4*>(&ws[kr][c]) = v;
            }
            __syncthreads();
#pragma unroll
            for (int kk = 0; kk < RE_BK; ++kk) {
                const f32x4 xv = *reinterpret_cast<const f32x4*>(&xs[kk][ty * 4]);
                const f32x4 wv = *reinterpret_cast<const f32x4*>(&ws[kk][tx * 4]);
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_fmaf(xv[i], wv[j], acc[i][j]);
            }
            __syncthreads();
        }
        // epilogue: bias, ReLU, ordered compaction into the padded rows
        const int c0 = n0 + tx * 4;
        float bias[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) bias[j] = c0 + j < S ? a.b_enc[c0 + j] : 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = row0 + ty * 4 + i;
            float v[4];
            bool p[4];
            uint64_t m[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                v[j] = acc[i][j] + bias[j];
                p[j] = r < a.n_rows && c0 + j < S && v[j] > 0.f;
                m[j] = __ballot(p[j]);
            }
            int before = 0, total = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                before += __popcll(m[j] & below);
                total += __popcll(m[j] & half);
            }
            int pos = cnt[i] + before;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (p[j]) {
                    if (pos < a.row_cap) {
                        a.idx_out[(size_t)r * a.row_cap + pos] = c0 + j;
                        a.val_out[(size_t)r * a.row_cap + pos] = v[j];
                    }
                    ++pos;
                }
            }
            cnt[i] += total;
        }
    }
    if (tx == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = row0 + ty * 4 + i;
            if (r < a.n_rows) {
                a.row_nnz_out[r] = cnt[i];
                if (cnt[i] > a.row_cap) atomicMax(a.max_nnz_out, cnt[i]);
            }
        }
    }
}

// One workgroup per row; each thread owns float4 columns t*4 + 1024 m of the row.  The entries must be in ascending latent order
// when there are several prefixes (the encoder writes them so): a prefix's reconstruction is stored when the first entry at or past
// its cut arrives.
constexpr int RD_THREADS = 256;
constexpr int RD_NV = 4;  // float4 per thread: d_model <= 4096

__global__ __launch_bounds__(RD_THREADS) void relu_decode_kernel(ReluDecodeArgs a) {
    const int b = blockIdx.x, t = threadIdx.x, D = a.D;
    const int nnz = min(a.row_nnz[b], a.row_cap);
    const int32_t* idx = a.idx + (size_t)b * a.row_cap;
    const float* val = a.val + (size_t)b * a.row_cap;
    float* out = a.x_hats + (size_t)b * a.n_prefixes * D;
    f32x4 acc[RD_NV];
#pragma unroll
    for (int m = 0; m < RD_NV; ++m) {
        const int c = (t + m * RD_THREADS) * 4;
        acc[m] = c < D ? *reinterpret_cast<const f32x4*>(a.b_dec + c) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    auto store = [&](int p) {
#pragma unroll
        for (int m = 0; m < RD_NV; ++m) {
            const int c = (t + m * RD_THREADS) * 4;
            if (c < D) *reinterpret_cast<f32x4*>(out + (size_t)p * D + c) = acc[m];
        }
    };
    int p = 0;
    for (int j = 0; j < nnz; ++j) {
        const int i = idx[j];
        const float v = val[j];
        while (p < a.n_prefixes - 1 && i >= a.prefixes[p]) store(p++);
        const float* w = a.W_dec + (size_t)i * D;
#pragma unroll
        for (int m = 0; m < RD_NV; ++m) {
            const int c = (t + m * RD_THREADS) * 4;
            if (c < D) {
                const f32x4 wv = *reinterpret_cast<const f32x4*>(w + c);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[m][e] = __builtin_fmaf(v, wv[e], acc[m][e]);
            }
        }
    }
    while (p < a.n_prefixes) store(p++);
}

__global__ void relu_scatter_kernel(const int32_t* idx, const float* val, const int32_t* row_nnz, int row_cap, int S, float* f_out) {
    const int b = blockIdx.x;
    const int nnz = min(row_nnz[b], row_cap);
    for (int j = threadIdx.x; j < nnz; j += blockDim.x)
        f_out[(size_t)b * S + idx[(size_t)b * row_cap + j]] = val[(size_t)b * row_cap + j];
}

}  // namespace

hipError_t launch_relu_encode(const ReluEncodeArgs& a, hipStream_t s) {
    if (a.n_rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(relu_encode_kernel, dim3((a.n_rows + RE_BM - 1) / RE_BM), dim3(RE_THREADS), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_relu_decode(const ReluDecodeArgs& a, hipStream_t s) {
    if (a.n_rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(relu_decode_kernel, dim3(a.n_rows), dim3(RD_THREADS), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_relu_scatter(const int32_t* idx, const float* val, const int32_t* row_nnz, int row_cap, int n_rows, int S,
                               float* f_out, hipStream_t s) {
    if (n_rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(relu_scatter_kernel, dim3(n_rows), dim3(256), 0, s, idx, val, row_nnz, row_cap, S, f_out);
    return hipGetLastError();
}
