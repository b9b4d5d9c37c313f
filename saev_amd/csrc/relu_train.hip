// The element-wise passes of the dense ReLU train step (include/saev_amd.h: RELU TRAINING; host sequence in ctx_relu_train.hip).
// The step's five contractions run on the split-fp16 MFMA kernel (gemm_encode_f16x3.hip); what is left are three passes over
// matrices the contractions wrote, each of which also leaves what the next contraction's operand split needs:
//
// relu_act_kernel      h (n x S) -> f = max(h, 0) in place; per row L0 = count(f > 0) and L1 = sum f, accumulated in fp64 and
//                      stored into the row's RowStats (stats_reduce_kernel adds the rows in a fixed order); fired[s] = 1 where any
//                      row has f > 0 (training only); the workgroup's max f (part[blockIdx.x]).  One wave per row: S x 4 bytes
//                      read and written, n x S x 8 bytes in all (2 x 2.1 GB at configs[1]).
// relu_mse_kernel      x_hat, x (n x D) -> the reference's rescaled squared error per row (objectives.py:224-237), sum (x - x_hat)^2
//                      and sum x^2 in fp64, g = dL/dx_hat = gscale (x_hat - x) and the workgroup's max |g|.  3 x n x D x 4 bytes.
// relu_dact_kernel     dA (n x S), f -> dH = (dA + l1c) where f > 0, else 0, in place; the column sums of dH over each block of
//                      RT_ROWS rows (colpart[block][s], added in block order by relu_colsum_kernel: db_enc); the workgroup's
//                      max |dH|.  n x S x 12 bytes.
// relu_pow2_kernel     the per-workgroup maxima -> the power-of-two operand scale {2^e, 1} of the fp16 split (one small launch, as
//                      auxk.hip's pow2_parts_kernel: no "last workgroup finishes" atomics).
// No floating-point atomics anywhere: every sum has a fixed order, two runs on the same inputs give the same bits.
#include "common.h"
#include "kernels.h"

namespace {

__device__ __forceinline__ float rt_block_max4(float m, float* sh) {
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = m;
    __syncthreads();
    return fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
}

// one wave per row, four rows per workgroup; lane l takes the float4s l, l + 64, ... of its row (S % 4 == 0)
__global__ __launch_bounds__(256) void relu_act_kernel(float* __restrict__ h, int n_rows, int S, int training, int32_t* __restrict__ fired,
                                                        RowStats* __restrict__ rowstats, float* __restrict__ part) {
    __shared__ float sh[4];
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    float fmx = 0.f;
    if (row < n_rows) {
        f32x4* hr = reinterpret_cast<f32x4*>(h + (size_t)row * S);
        const int S4 = S >> 2;
        int l0 = 0;
        double l1 = 0.0;
        for (int q = lane; q < S4; q += 64) {
            f32x4 v = hr[q];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const bool on = v[e] > 0.f;
                v[e] = on ? v[e] : 0.f;
                if (on) {
                    l0 += 1;
                    l1 += (double)v[e];
                    fmx = fmaxf(fmx, v[e]);
                    // (a plain store of the same value by whoever sees the latent fire; the read keeps all but the first few away)
                    if (training && fired[4 * q + e] == 0) fired[4 * q + e] = 1;
                }
            }
            hr[q] = v;
        }
        l0 = wave_sum_i(l0);
        l1 = wave_sum_d(l1);
        if (lane == 0) { rowstats[row].l0 = (float)l0; rowstats[row].l1 = (float)l1; }
    }
    fmx = rt_block_max4(fmx, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = fmx;
}

// one wave per row, four rows per workgroup (D % 4 == 0).  The arithmetic of the squared error and of g is the decode kernels'
// (sparse.hip: decode_kernel), so that a ReLU step and a TopK step report the same loss for the same reconstruction.
__global__ __launch_bounds__(256) void relu_mse_kernel(const float* __restrict__ x, const float* __restrict__ x_hat, int n_rows, int D,
                                                        const float* __restrict__ upper, float gscale, float* __restrict__ g,
                                                        RowStats* __restrict__ rowstats, float* __restrict__ part) {
    __shared__ float sh[4];
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    float gmx = 0.f;
    if (row < n_rows) {
        const f32x4* xr = reinterpret_cast<const f32x4*>(x + (size_t)row * D);
        const f32x4* hr = reinterpret_cast<const f32x4*>(x_hat + (size_t)row * D);
        f32x4* gr = reinterpret_cast<f32x4*>(g + (size_t)row * D);
        const float u = fmaxf(*upper, 1e-12f);
        float sse_scaled = 0.f;
        double sse64 = 0.0, sumsq64 = 0.0;
        for (int q = lane; q < (D >> 2); q += 64) {
            const f32x4 xv = xr[q], hv = hr[q];
            f32x4 gv;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float t = hv[e] / u - xv[e] / u;
                sse_scaled += t * t * u * u;
                gv[e] = gscale * t * u;
                gmx = fmaxf(gmx, fabsf(gv[e]));
                const float r = xv[e] - hv[e];
                sse64 += (double)r * (double)r;
                sumsq64 += (double)xv[e] * (double)xv[e];
            }
            gr[q] = gv;
        }
        sse_scaled = wave_sum(sse_scaled);
        sse64 = wave_sum_d(sse64);
        sumsq64 = wave_sum_d(sumsq64);
        if (lane == 0) {
            RowStats* rs = rowstats + row;  // (l0 / l1 are relu_act_kernel's)
            rs->sse_scaled = sse_scaled; rs->aux_sse = 0.f; rs->sse64 = sse64; rs->sumsq64 = sumsq64;
        }
    }
    gmx = rt_block_max4(gmx, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = gmx;
}

constexpr int RT_ROWS = 64;     // rows per workgroup of relu_dact_kernel
constexpr int RT_COLS = 1024;   // columns per workgroup: one float4 per thread

// workgroup (bx, by): columns [1024 bx, +1024) of rows [64 by, +64); a thread keeps the column sums of its four columns in registers
// and adds the rows in ascending order
__global__ __launch_bounds__(256) void relu_dact_kernel(float* __restrict__ dA, const float* __restrict__ f, int n_rows, int S, float l1c,
                                                         float* __restrict__ colpart, float* __restrict__ part) {
    __shared__ float sh[4];
    const int q = blockIdx.x * 256 + threadIdx.x;  // float4 column
    const int r0 = blockIdx.y * RT_ROWS, r1 = min(n_rows, r0 + RT_ROWS);
    float mx = 0.f;
    if (4 * q < S) {
        f32x4 cs = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int r = r0; r < r1; ++r) {
            const size_t o = (size_t)r * (S >> 2) + q;
            const f32x4 fv = reinterpret_cast<const f32x4*>(f)[o];
            f32x4 d = reinterpret_cast<f32x4*>(dA)[o];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                d[e] = fv[e] > 0.f ? d[e] + l1c : 0.f;
                cs[e] += d[e];
                mx = fmaxf(mx, fabsf(d[e]));
            }
            reinterpret_cast<f32x4*>(dA)[o] = d;
        }
        reinterpret_cast<f32x4*>(colpart + (size_t)blockIdx.y * S)[q] = cs;
    }
    mx = rt_block_max4(mx, sh);
    if (threadIdx.x == 0) part[blockIdx.y * gridDim.x + blockIdx.x] = mx;
}

// out[s] = sum over the row blocks, in block order, of colpart[block][s]
__global__ __launch_bounds__(256) void relu_colsum_kernel(const float* __restrict__ colpart, int n_blocks, int S, float* __restrict__ out) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= S) return;
    float t = 0.f;
    for (int b = 0; b < n_blocks; ++b) t += colpart[(size_t)b * S + s];
    out[s] = t;
}

// {2^e, 1} with 2^e max in [2^13, 2^14) (1 when the matrix is all zero or not finite): auxk.hip's pow2_parts_kernel
__global__ __launch_bounds__(256) void relu_pow2_kernel(const float* __restrict__ part, int n, float* __restrict__ pair) {
    __shared__ float sh[4];
    float m = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) m = fmaxf(m, part[i]);
    m = rt_block_max4(m, sh);
    if (threadIdx.x == 0) {
        pair[0] = (m > 0.f && m < 3.0e38f) ? exp2f(13.0f - floorf(log2f(m))) : 1.0f;
        pair[1] = 1.0f;
    }
}

}  // namespace

int relu_act_parts(int n_rows) { return (n_rows + 3) / 4; }
int relu_dact_row_blocks(int n_rows) { return (n_rows + RT_ROWS - 1) / RT_ROWS; }
int relu_dact_parts(int n_rows, int S) { return relu_dact_row_blocks(n_rows) * ((S + RT_COLS - 1) / RT_COLS); }

hipError_t launch_relu_act(float* h, int n_rows, int S, int training, int32_t* fired, RowStats* rowstats, float* part, float* pair,
                           hipStream_t s) {
    const int nb = relu_act_parts(n_rows);
    hipLaunchKernelGGL(relu_act_kernel, dim3(nb), dim3(256), 0, s, h, n_rows, S, training, fired, rowstats, part);
    hipLaunchKernelGGL(relu_pow2_kernel, dim3(1), dim3(256), 0, s, part, nb, pair);
    return hipGetLastError();
}

hipError_t launch_relu_mse(const float* x, const float* x_hat, int n_rows, int D, const float* upper, float gscale, float* g,
                           RowStats* rowstats, float* part, float* pair, hipStream_t s) {
    const int nb = relu_act_parts(n_rows);
    hipLaunchKernelGGL(relu_mse_kernel, dim3(nb), dim3(256), 0, s, x, x_hat, n_rows, D, upper, gscale, g, rowstats, part);
    hipLaunchKernelGGL(relu_pow2_kernel, dim3(1), dim3(256), 0, s, part, nb, pair);
    return hipGetLastError();
}

hipError_t launch_relu_dact(float* dA, const float* f, int n_rows, int S, float l1c, float* colpart, float* db_enc, float* part,
                            float* pair, hipStream_t s) {
    const dim3 grid((S + RT_COLS - 1) / RT_COLS, relu_dact_row_blocks(n_rows));
    hipLaunchKernelGGL(relu_dact_kernel, grid, dim3(256), 0, s, dA, f, n_rows, S, l1c, colpart, part);
    hipLaunchKernelGGL(relu_colsum_kernel, dim3((S + 255) / 256), dim3(256), 0, s, colpart, (int)grid.y, S, db_enc);
    hipLaunchKernelGGL(relu_pow2_kernel, dim3(1), dim3(256), 0, s, part, (int)(grid.x * grid.y), pair);
    return hipGetLastError();
}
