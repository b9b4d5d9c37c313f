// The training half of the concept audit (include/saev_amd.h: SPARSE LINEAR): pooling of a token CSR to one dense
// row per image, and the L1-penalised (multinomial) logistic regression fitted on those rows.
//
//   pool     a workgroup per (image, range of SL_POOL_RANGE latents), the range's fp32 accumulators and patch counts in LDS.  The
//            image's patches are applied in ascending order with a barrier between them; within a patch the columns are distinct
//            (canonical rows), so the read-modify-write of an accumulator is a plain LDS access.  max competes with an implicit 0
//            where a latent is stored in fewer than tpi patches; mean is the fp32 sum in patch order and one fp32 division.  The
//            output is written once, as full lines.
//   solver   FISTA with backtracking on L and function-value restart, all fp64, the intercept carried as column S of the weight
//            arrays (x = 1, no penalty).  Per iteration five launches, each leaving on the state block's predicate in its first
//            instructions:
//              resid    thread per row: the logits of the extrapolated point y = w + beta (w - w_prev) are the same combination
//                       of the two kept logit arrays; r = p - onehot and the row's loss
//              grad     workgroup = 256 columns x one row chunk, K fp64 accumulators per lane, rows in ascending order
//              step     thread per column: the chunk partials added in chunk order, times C; the KKT terms of y; the
//                       soft-threshold step; the block's shares of <g, d>, |d|^2, |w_new|_1, |y|_1
//              forward  wave per four rows (one at K > 16), lanes over columns, K accumulators a row, a butterfly: the logits and
//                       the loss of w_new
//              control  one workgroup: the sums in a fixed order and the decision -- done (KKT of y within tol), reject (L doubles,
//                       the gradient is kept), restart (F rose under momentum: t = 1 from w) or accept (the three buffers rotate)
//            No float atomics, every sum in an order fixed by the shape: two fits give the same bits.
#include "entry_util.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace {

constexpr int SL_MAX_K = 64;
constexpr int SL_COLS = 256;      // columns of a grad / step workgroup
constexpr int SL_MAX_CHUNKS = 32; // row chunks of the gradient

// ---------------------------------------------------------------- pooling -----------------------------------------------------------

template <int MEAN>
__global__ __launch_bounds__(256) void sl_pool_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                                      const float* __restrict__ data, int64_t nnz, int tpi, int S,
                                                      float* __restrict__ out, int32_t* __restrict__ err) {
    __shared__ float acc[SL_POOL_RANGE];
    __shared__ int32_t cnt[SL_POOL_RANGE];
    const int img = blockIdx.x;
    const int lo = blockIdx.y * SL_POOL_RANGE;
    const int len = min(SL_POOL_RANGE, S - lo);
    for (int i = threadIdx.x; i < len; i += 256) {
        acc[i] = MEAN ? 0.f : NEG_INF;
        cnt[i] = 0;
    }
    __syncthreads();
    int bad = 0;
    const int64_t row0 = (int64_t)img * tpi;
    for (int p = 0; p < tpi; ++p) {
        int64_t e0 = indptr[row0 + p], e1 = indptr[row0 + p + 1];
        if (e0 < 0 || e1 < e0 || e1 > nnz) { bad = SAEV_POOL_ERR_INDPTR; e0 = e1 = 0; }  // (the same in every thread)
        for (int64_t e = e0 + threadIdx.x; e < e1; e += 256) {
            const int col = indices[e];
            const float v = data[e];
            if ((unsigned)col >= (unsigned)S) { bad = max(bad, SAEV_POOL_ERR_COLUMN); continue; }
            if (!(fabsf(v) <= 3.402823466e38f)) bad = max(bad, SAEV_POOL_ERR_VALUE);
            const int c = col - lo;
            if (c < 0 || c >= len) continue;
            if (MEAN) acc[c] = acc[c] + v;
            else { acc[c] = fmaxf(acc[c], v); cnt[c] = cnt[c] + 1; }
        }
        __syncthreads();  // the next patch may hold the same columns
    }
    if (bad) atomicMax(err, bad);
    const float den = (float)tpi;
    float* dst = out + (size_t)img * S + lo;
    for (int i = threadIdx.x; i < len; i += 256) {
        const float a = acc[i];
        dst[i] = MEAN ? a / den : (cnt[i] < tpi ? fmaxf(a, 0.f) : a);
    }
}

// ---------------------------------------------------------------- solver ------------------------------------------------------------

struct SlArgs {
    const float* X;
    const int32_t* y;
    int64_t n;
    int S, S1, K, Kc, chunk_rows, n_chunks, col_blocks;
    double C, tol;
    double* state;
    int32_t* err;
    double* W[3];
    double* Z[3];
    double *G, *part, *r, *loss_y, *loss_n, *bp;
};

enum { ST_IT = SAEV_L1_STATE_ITER, ST_L = SAEV_L1_STATE_L, ST_T = SAEV_L1_STATE_T, ST_BETA = SAEV_L1_STATE_BETA, ST_F = SAEV_L1_STATE_F,
       ST_FY = SAEV_L1_STATE_FY, ST_KKT = SAEV_L1_STATE_KKT, ST_OBJ = SAEV_L1_STATE_OBJ, ST_DONE = SAEV_L1_STATE_DONE,
       ST_NEED = SAEV_L1_STATE_NEED_GRAD, ST_IW = SAEV_L1_STATE_CUR, ST_IP = SAEV_L1_STATE_PREV, ST_IN = SAEV_L1_STATE_NEXT,
       ST_REJECTS = SAEV_L1_STATE_REJECTS, ST_RESTARTS = SAEV_L1_STATE_RESTARTS, ST_L1Y = 15 };

// the loss of one row and (optionally) r = p - onehot from its Kc logits z; K == 2 has one logit and the positive class 1
template <typename Get, typename Put>
__device__ __forceinline__ double sl_row_loss(int K, int yi, Get z, Put put) {
    if (K == 2) {
        const double v = z(0);
        const double e = exp(-fabs(v));
        const double sp = log1p(e);  // softplus(-|v|)
        const double p = v >= 0 ? 1.0 / (1.0 + e) : e / (1.0 + e);
        put(0, p - (double)yi);
        return (yi ? fmax(-v, 0.0) : fmax(v, 0.0)) + sp;
    }
    double m = z(0);
    for (int k = 1; k < K; ++k) m = fmax(m, z(k));
    double s = 0.0;
    for (int k = 0; k < K; ++k) s += exp(z(k) - m);
    const double lse = m + log(s);
    for (int k = 0; k < K; ++k) put(k, exp(z(k) - lse) - (k == yi ? 1.0 : 0.0));
    return lse - z(yi);
}

// a class id outside [0, K) sets the error word (sl_check_kernel); clamped, it cannot take a read out of the row's logits
__device__ __forceinline__ int sl_class(int y, int K) { return min(max(y, 0), K - 1); }

__global__ __launch_bounds__(256) void sl_check_kernel(const float* __restrict__ X, size_t total, const int32_t* __restrict__ y, int64_t n,
                                                       int K, int32_t* __restrict__ err) {
    int bad = 0;
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += stride)
        if (!(fabsf(X[i]) <= 3.402823466e38f)) bad = SAEV_L1_ERR_VALUE;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < (size_t)n; i += stride)
        if ((unsigned)y[i] >= (unsigned)K) bad = max(bad, SAEV_L1_ERR_CLASS);
    if (bad) atomicMax(err, bad);
}

__global__ void sl_init_kernel(double* state, double F0) {
    if (threadIdx.x >= SAEV_L1_STATE_WORDS) return;
    double v = 0.0;
    switch (threadIdx.x) {
        case ST_L: case ST_T: case ST_NEED: case ST_IP: v = 1.0; break;
        case ST_IN: v = 2.0; break;
        case ST_F: v = F0; break;
        default: break;
    }
    state[threadIdx.x] = v;
}

__global__ __launch_bounds__(256) void sl_resid_kernel(SlArgs a) {
    if (a.state[ST_DONE] != 0.0 || a.state[ST_NEED] == 0.0) return;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const double beta = a.state[ST_BETA];
    const double* z = a.Z[(int)a.state[ST_IW]] + (size_t)i * a.Kc;
    const double* zp = a.Z[(int)a.state[ST_IP]] + (size_t)i * a.Kc;
    double* r = a.r + (size_t)i * a.Kc;
    a.loss_y[i] = sl_row_loss(a.K, sl_class(a.y[i], a.K), [&](int k) { return z[k] + beta * (z[k] - zp[k]); }, [&](int k, double v) { r[k] = v; });
}

template <int KT>
__global__ __launch_bounds__(256) void sl_grad_kernel(SlArgs a) {
    if (a.state[ST_DONE] != 0.0 || a.state[ST_NEED] == 0.0) return;
    const int col = blockIdx.x * SL_COLS + threadIdx.x;
    if (col >= a.S1) return;
    const int chunk = blockIdx.y;
    const int64_t r0 = (int64_t)chunk * a.chunk_rows, r1 = min(a.n, r0 + a.chunk_rows);
    double acc[KT];
#pragma unroll
    for (int k = 0; k < KT; ++k) acc[k] = 0.0;
    const bool ones = col == a.S;
    const float* x = a.X + (ones ? 0 : col);
    for (int64_t i = r0; i < r1; ++i) {
        const double xv = ones ? 1.0 : (double)x[(size_t)i * a.S];
        const double* r = a.r + (size_t)i * a.Kc;
#pragma unroll
        for (int k = 0; k < KT; ++k)
            if (k < a.Kc) acc[k] = fma(r[k], xv, acc[k]);
    }
#pragma unroll
    for (int k = 0; k < KT; ++k)
        if (k < a.Kc) a.part[((size_t)chunk * a.Kc + k) * a.S1 + col] = acc[k];
}

// the sum over a workgroup of 256 in a fixed order; the result is valid in thread 0
__device__ __forceinline__ double sl_block_sum(double v, double* lds) {
    v = wave_sum_d(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((lds[0] + lds[1]) + lds[2]) + lds[3];
}
__device__ __forceinline__ double sl_block_max(double v, double* lds) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmax(fmax(lds[0], lds[1]), fmax(lds[2], lds[3]));
}

__global__ __launch_bounds__(256) void sl_step_kernel(SlArgs a) {
    __shared__ double lds[4];
    if (a.state[ST_DONE] != 0.0) return;
    const bool need = a.state[ST_NEED] != 0.0;
    const double L = a.state[ST_L], beta = a.state[ST_BETA], inv = 1.0 / L;
    const double* W = a.W[(int)a.state[ST_IW]];
    const double* Wp = a.W[(int)a.state[ST_IP]];
    double* Wn = a.W[(int)a.state[ST_IN]];
    const int col = blockIdx.x * SL_COLS + threadIdx.x;
    double kkt = 0.0, lin = 0.0, d2 = 0.0, l1n = 0.0, l1y = 0.0;
    if (col < a.S1) {
        for (int k = 0; k < a.Kc; ++k) {
            const size_t at = (size_t)k * a.S1 + col;
            double g;
            if (need) {
                g = 0.0;
                for (int ch = 0; ch < a.n_chunks; ++ch) g += a.part[((size_t)ch * a.Kc + k) * a.S1 + col];
                g *= a.C;
                a.G[at] = g;
            } else {
                g = a.G[at];
            }
            const double w = W[at];
            const double yv = w + beta * (w - Wp[at]);
            double wn, res;
            if (col < a.S) {
                res = yv > 0.0 ? fabs(g + 1.0) : yv < 0.0 ? fabs(g - 1.0) : fmax(fabs(g) - 1.0, 0.0);
                const double u = yv - g * inv;
                wn = u > inv ? u - inv : u < -inv ? u + inv : 0.0;
                l1n += fabs(wn);
                l1y += fabs(yv);
            } else {  // the intercept: no penalty
                res = fabs(g);
                wn = yv - g * inv;
            }
            kkt = fmax(kkt, res);
            const double d = wn - yv;
            lin += g * d;
            d2 += d * d;
            Wn[at] = wn;
        }
    }
    lin = sl_block_sum(lin, lds);
    d2 = sl_block_sum(d2, lds);
    l1n = sl_block_sum(l1n, lds);
    l1y = sl_block_sum(l1y, lds);
    kkt = sl_block_max(kkt, lds);
    if (threadIdx.x == 0) {
        double* bp = a.bp + (size_t)blockIdx.x * 8;
        bp[0] = lin; bp[1] = d2; bp[2] = l1n; bp[3] = l1y; bp[4] = kkt;
    }
}

// RB rows per wave: a weight is read once per RB elements of X (each row's sum keeps its own order: lanes over columns, a butterfly)
template <int KT, int RB>
__global__ __launch_bounds__(256) void sl_forward_kernel(SlArgs a) {
    if (a.state[ST_DONE] != 0.0) return;
    const int lane = threadIdx.x & 63;
    const int64_t row0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * RB;
    if (row0 >= a.n) return;
    const int in = (int)a.state[ST_IN];
    const double* Wn = a.W[in];
    const int rows = (int)min((int64_t)RB, a.n - row0);
    const float* x = a.X + (size_t)row0 * a.S;
    double acc[RB][KT];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
        for (int k = 0; k < KT; ++k) acc[rb][k] = 0.0;
    for (int c = lane; c < a.S; c += 64) {
        double xv[RB];
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) xv[rb] = rb < rows ? (double)x[(size_t)rb * a.S + c] : 0.0;
#pragma unroll
        for (int k = 0; k < KT; ++k)
            if (k < a.Kc) {
                const double w = Wn[(size_t)k * a.S1 + c];
#pragma unroll
                for (int rb = 0; rb < RB; ++rb) acc[rb][k] = fma(xv[rb], w, acc[rb][k]);
            }
    }
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
        for (int k = 0; k < KT; ++k)
            if (k < a.Kc) acc[rb][k] = wave_sum_d(acc[rb][k]) + Wn[(size_t)k * a.S1 + a.S];
    if (lane != 0) return;
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
        if (rb >= rows) break;
        double* z = a.Z[in] + (size_t)(row0 + rb) * a.Kc;
#pragma unroll
        for (int k = 0; k < KT; ++k)
            if (k < a.Kc) z[k] = acc[rb][k];
        a.loss_n[row0 + rb] = sl_row_loss(a.K, sl_class(a.y[row0 + rb], a.K), [&](int k) { return z[k]; }, [](int, double) {});
    }
}

// the sum of v[0 .. n) in an order fixed by n: thread t takes t, t + 256, ..., then the workgroup's tree
__device__ __forceinline__ double sl_strided_sum(const double* v, int64_t n, int stride, double* lds) {
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 256) s += v[(size_t)i * stride];
    return sl_block_sum(s, lds);
}

// final = 0: the decision of one iteration.  final = 1: after resid / grad / step at beta = 0, the KKT residual and the objective of
// the iterate itself (a fit that ran out of iterations); nothing else moves.
__global__ __launch_bounds__(256) void sl_control_kernel(SlArgs a, int final) {
    __shared__ double lds[4];
    double* st = a.state;
    if (st[ST_DONE] != 0.0) return;
    const bool need = st[ST_NEED] != 0.0;
    const double sum_n = sl_strided_sum(a.loss_n, a.n, 1, lds);
    const double sum_y = need ? sl_strided_sum(a.loss_y, a.n, 1, lds) : 0.0;
    const double lin = sl_strided_sum(a.bp + 0, a.col_blocks, 8, lds);
    const double d2 = sl_strided_sum(a.bp + 1, a.col_blocks, 8, lds);
    const double l1n = sl_strided_sum(a.bp + 2, a.col_blocks, 8, lds);
    const double l1y = sl_strided_sum(a.bp + 3, a.col_blocks, 8, lds);
    double kkt = 0.0;
    for (int i = threadIdx.x; i < a.col_blocks; i += 256) kkt = fmax(kkt, a.bp[(size_t)i * 8 + 4]);
    kkt = sl_block_max(kkt, lds);
    if (threadIdx.x != 0) return;
    if (need) { st[ST_FY] = a.C * sum_y; st[ST_L1Y] = l1y; st[ST_KKT] = kkt; }
    const double fy = st[ST_FY];
    if (final) {
        st[ST_OBJ] = fy + st[ST_L1Y];
        return;
    }
    st[ST_IT] += 1.0;
    if (st[ST_KKT] <= a.tol) {  // y itself is the answer
        st[ST_OBJ] = fy + st[ST_L1Y];
        st[ST_DONE] = 1.0;
        return;
    }
    const double L = st[ST_L], fn = a.C * sum_n;
    if (!(fn <= fy + lin + 0.5 * L * d2 + 1e-12 * fabs(fy))) {  // not a sufficient decrease: the same gradient, half the step
        st[ST_L] = 2.0 * L;
        st[ST_NEED] = 0.0;
        st[ST_REJECTS] += 1.0;
        return;
    }
    st[ST_NEED] = 1.0;
    const double Fn = fn + l1n;
    if (st[ST_BETA] != 0.0 && Fn > st[ST_F]) {  // the objective rose under momentum: start again from w, without it
        st[ST_T] = 1.0;
        st[ST_BETA] = 0.0;
        st[ST_RESTARTS] += 1.0;
        return;
    }
    const double t = st[ST_T], tn = 0.5 * (1.0 + sqrt(1.0 + 4.0 * t * t));
    st[ST_BETA] = (t - 1.0) / tn;
    st[ST_T] = tn;
    st[ST_F] = Fn;
    const double iw = st[ST_IW], ip = st[ST_IP], in = st[ST_IN];
    st[ST_IP] = iw;
    st[ST_IW] = in;
    st[ST_IN] = ip;
}

__global__ void sl_unmomentum_kernel(double* st) {
    if (st[ST_DONE] != 0.0) return;
    st[ST_T] = 1.0;
    st[ST_BETA] = 0.0;
    st[ST_NEED] = 1.0;
}

__global__ __launch_bounds__(256) void sl_out_kernel(SlArgs a, double* __restrict__ coef, double* __restrict__ intercept, double* __restrict__ scalars) {
    const double* st = a.state;
    const double beta = st[ST_BETA];
    const double* W = a.W[(int)st[ST_IW]];
    const double* Wp = a.W[(int)st[ST_IP]];
    const auto at_y = [&](size_t at) { const double w = W[at]; return w + beta * (w - Wp[at]); };
    const size_t total = (size_t)a.Kc * a.S;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const size_t k = i / a.S, c = i % a.S;
        coef[i] = at_y(k * a.S1 + c);
    }
    if (blockIdx.x == 0 && threadIdx.x < a.Kc) {
        double mean = 0.0;
        if (a.K > 2) {
            for (int k = 0; k < a.Kc; ++k) mean += at_y((size_t)k * a.S1 + a.S);
            mean /= (double)a.Kc;
        }
        intercept[threadIdx.x] = at_y((size_t)threadIdx.x * a.S1 + a.S) - mean;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        scalars[0] = st[ST_IT]; scalars[1] = st[ST_KKT]; scalars[2] = st[ST_OBJ]; scalars[3] = st[ST_DONE]; scalars[4] = st[ST_L];
        scalars[5] = st[ST_REJECTS]; scalars[6] = st[ST_RESTARTS]; scalars[7] = 0.0;
    }
}

bool sl_shape_ok(int64_t n, int64_t S, int64_t K) { return n >= 1 && n <= 0x7fffffffLL && S >= 1 && S <= 0x40000000LL && K >= 2 && K <= SL_MAX_K; }

void sl_layout(int64_t n, int64_t S, int64_t K, saev_l1_logistic_layout* L) {
    std::memset(L, 0, sizeof *L);
    L->struct_size = (int32_t)sizeof *L;
    L->coef_rows = (int32_t)(K == 2 ? 1 : K);
    L->chunk_rows = 64 * ((n + 64 * SL_MAX_CHUNKS - 1) / (64 * SL_MAX_CHUNKS));
    L->n_chunks = (n + L->chunk_rows - 1) / L->chunk_rows;
    L->col_blocks = (S + 1 + SL_COLS - 1) / SL_COLS;
    const int64_t Kc = L->coef_rows, S1 = S + 1;
    WsCarve ws;
    L->off_err = ws.take(64);
    L->off_state = ws.take(8 * SAEV_L1_STATE_WORDS);
    L->off_w = ws.take(3 * round256(8 * Kc * S1));
    L->off_z = ws.take(3 * round256(8 * Kc * n));
    L->off_g = ws.take(8 * Kc * S1);
    L->off_part = ws.take(8 * L->n_chunks * Kc * S1);
    L->off_r = ws.take(8 * Kc * n);
    L->off_loss = ws.take(2 * round256(8 * n));
    L->off_bp = ws.take(8 * 8 * L->col_blocks);
    L->total_bytes = ws.at;
}

const char* sl_args(SlArgs* a, const float* X, const int32_t* y, int64_t n, int64_t S, int64_t K, double C, double tol, void* workspace,
                    int64_t workspace_bytes, saev_l1_logistic_layout* L) {
    if (n < 0 || S < 0 || K < 0) return "negative size";
    if (K < 2) return "fewer than two classes";
    if (!sl_shape_ok(n, S, K)) return nullptr;
    if (!(C > 0.0) || !std::isfinite(C)) return "C must be positive and finite";
    if (!(tol >= 0.0)) return "kkt_tol must not be negative";
    if (!X || !y) return "X and y must not be NULL";
    sl_layout(n, S, K, L);
    if (!workspace || workspace_bytes < L->total_bytes) return "workspace smaller than saev_l1_logistic_workspace_bytes(n, S, K)";
    if (((uintptr_t)workspace & 255) != 0) return "workspace must be 256-byte aligned";
    uint8_t* ws = static_cast<uint8_t*>(workspace);
    const int64_t Kc = L->coef_rows, S1 = S + 1;
    a->X = X; a->y = y; a->n = n; a->S = (int)S; a->S1 = (int)S1; a->K = (int)K; a->Kc = (int)Kc;
    a->chunk_rows = (int)L->chunk_rows; a->n_chunks = (int)L->n_chunks; a->col_blocks = (int)L->col_blocks;
    a->C = C; a->tol = tol;
    a->state = reinterpret_cast<double*>(ws + L->off_state);
    a->err = reinterpret_cast<int32_t*>(ws + L->off_err);
    for (int i = 0; i < 3; ++i) {
        a->W[i] = reinterpret_cast<double*>(ws + L->off_w + i * round256(8 * Kc * S1));
        a->Z[i] = reinterpret_cast<double*>(ws + L->off_z + i * round256(8 * Kc * n));
    }
    a->G = reinterpret_cast<double*>(ws + L->off_g);
    a->part = reinterpret_cast<double*>(ws + L->off_part);
    a->r = reinterpret_cast<double*>(ws + L->off_r);
    a->loss_y = reinterpret_cast<double*>(ws + L->off_loss);
    a->loss_n = reinterpret_cast<double*>(ws + L->off_loss + round256(8 * n));
    a->bp = reinterpret_cast<double*>(ws + L->off_bp);
    return "";
}

template <int KT, int RB>
void sl_launch_iteration(const SlArgs& a, hipStream_t s, bool step_and_forward, int final) {
    const dim3 b(256);
    hipLaunchKernelGGL(sl_resid_kernel, dim3((unsigned)((a.n + 255) / 256)), b, 0, s, a);
    hipLaunchKernelGGL(sl_grad_kernel<KT>, dim3((unsigned)a.col_blocks, (unsigned)a.n_chunks), b, 0, s, a);
    hipLaunchKernelGGL(sl_step_kernel, dim3((unsigned)a.col_blocks), b, 0, s, a);
    if (step_and_forward) hipLaunchKernelGGL((sl_forward_kernel<KT, RB>), dim3((unsigned)((a.n + 4 * RB - 1) / (4 * RB))), b, 0, s, a);
    hipLaunchKernelGGL(sl_control_kernel, dim3(1), b, 0, s, a, final);
}

void sl_iteration(const SlArgs& a, hipStream_t s, bool fwd, int final) {
    if (a.Kc <= 1) sl_launch_iteration<1, 4>(a, s, fwd, final);
    else if (a.Kc <= 4) sl_launch_iteration<4, 4>(a, s, fwd, final);
    else if (a.Kc <= 16) sl_launch_iteration<16, 4>(a, s, fwd, final);
    else sl_launch_iteration<64, 1>(a, s, fwd, final);
}

}  // namespace

int64_t saev_pool_images_range(void) { return SL_POOL_RANGE; }

int saev_pool_images(const int64_t* indptr, const int32_t* indices, const float* data, int64_t nnz, int64_t n_images,
                     int64_t tokens_per_image, int64_t n_latents, int32_t agg, float* out, int32_t* err, void* stream) {
    if (n_images < 0 || tokens_per_image < 0 || n_latents < 0) return entry_refuse(SAEV_INVALID_ARG, "saev_pool_images", "negative size");
    if (n_images < 1 || tokens_per_image < 1 || n_latents < 1)
        return entry_refuse(SAEV_INVALID_ARG, "saev_pool_images", "n_images, tokens_per_image and n_latents must be at least 1");
    if (n_images > 0x7fffffffLL || tokens_per_image > 0x7fffffffLL || n_latents > 0x7fffffffLL || n_images * tokens_per_image > 0x7fffffffLL)
        return entry_refuse(SAEV_UNSUPPORTED, "saev_pool_images", "n_images * tokens_per_image and n_latents must stay below 2^31");
    if ((n_latents + SL_POOL_RANGE - 1) / SL_POOL_RANGE > 65535) return entry_refuse(SAEV_UNSUPPORTED, "saev_pool_images", "more than 65535 latent ranges");
    if (agg != SAEV_POOL_MAX && agg != SAEV_POOL_MEAN) return entry_refuse(SAEV_INVALID_ARG, "saev_pool_images", "agg is SAEV_POOL_MAX or SAEV_POOL_MEAN");
    if (nnz < 0) return entry_refuse(SAEV_INVALID_ARG, "saev_pool_images", "negative nnz");
    if (!indptr || !out || !err) return entry_refuse(SAEV_INVALID_ARG, "saev_pool_images", "indptr, out and err must not be NULL");
    if (nnz > 0 && (!indices || !data)) return entry_refuse(SAEV_INVALID_ARG, "saev_pool_images", "indices and data come with nnz > 0");
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(err, 0, 4, s) != hipSuccess) return entry_refuse(SAEV_HIP_ERROR, "saev_pool_images", "hipMemsetAsync failed");
    const dim3 grid((unsigned)n_images, (unsigned)((n_latents + SL_POOL_RANGE - 1) / SL_POOL_RANGE));
    if (agg == SAEV_POOL_MEAN)
        hipLaunchKernelGGL(sl_pool_kernel<1>, grid, dim3(256), 0, s, indptr, indices, data, nnz, (int)tokens_per_image, (int)n_latents, out, err);
    else
        hipLaunchKernelGGL(sl_pool_kernel<0>, grid, dim3(256), 0, s, indptr, indices, data, nnz, (int)tokens_per_image, (int)n_latents, out, err);
    if (hipGetLastError() != hipSuccess) return entry_refuse(SAEV_HIP_ERROR, "saev_pool_images", "kernel launch failed");
    return SAEV_OK;
}

int64_t saev_l1_logistic_workspace_bytes(int64_t n, int64_t S, int64_t K) {
    if (!sl_shape_ok(n, S, K)) return -1;
    saev_l1_logistic_layout L;
    sl_layout(n, S, K, &L);
    return L.total_bytes;
}

int saev_l1_logistic_layout_of(int64_t n, int64_t S, int64_t K, saev_l1_logistic_layout* out) {
    if (!out) return entry_refuse(SAEV_INVALID_ARG, "saev_l1_logistic_layout_of", "no saev_l1_logistic_layout");
    if (!sl_shape_ok(n, S, K)) return entry_refuse(SAEV_UNSUPPORTED, "saev_l1_logistic_layout_of", "1 <= n < 2^31, 1 <= S <= 2^30, 2 <= K <= 64");
    sl_layout(n, S, K, out);
    return SAEV_OK;
}

#define SL_ENTRY(name)                                                                                                            \
    SlArgs a;                                                                                                                     \
    saev_l1_logistic_layout L;                                                                                                    \
    {                                                                                                                             \
        const char* why = sl_args(&a, X, y, n, S, K, C, kkt_tol, workspace, workspace_bytes, &L);                                 \
        if (!why) return entry_refuse(SAEV_UNSUPPORTED, name, "1 <= n < 2^31, 1 <= S <= 2^30, 2 <= K <= 64");                     \
        if (why[0]) return entry_refuse(SAEV_INVALID_ARG, name, why);                                                             \
    }                                                                                                                             \
    hipStream_t s = (hipStream_t)stream;

int saev_l1_logistic_init(const float* X, const int32_t* y, int64_t n, int64_t S, int64_t K, double C, double kkt_tol, void* workspace,
                          int64_t workspace_bytes, void* stream) {
    SL_ENTRY("saev_l1_logistic_init")
    // everything starts at 0: w = 0, so the logits are 0 and F = C n log(classes)
    if (hipMemsetAsync(workspace, 0, (size_t)L.off_g, s) != hipSuccess) return entry_refuse(SAEV_HIP_ERROR, "saev_l1_logistic_init", "hipMemsetAsync failed");
    hipLaunchKernelGGL(sl_init_kernel, dim3(1), dim3(64), 0, s, a.state, C * (double)n * std::log((double)K));
    const size_t total = (size_t)n * (size_t)S;
    const unsigned grid = (unsigned)std::min<size_t>((total + 255) / 256, 8192);
    hipLaunchKernelGGL(sl_check_kernel, dim3(grid), dim3(256), 0, s, X, total, y, n, (int)K, a.err);
    if (hipGetLastError() != hipSuccess) return entry_refuse(SAEV_HIP_ERROR, "saev_l1_logistic_init", "kernel launch failed");
    return SAEV_OK;
}

int saev_l1_logistic_iterate(const float* X, const int32_t* y, int64_t n, int64_t S, int64_t K, double C, double kkt_tol, int32_t n_iters,
                             void* workspace, int64_t workspace_bytes, void* stream) {
    SL_ENTRY("saev_l1_logistic_iterate")
    if (n_iters < 0) return entry_refuse(SAEV_INVALID_ARG, "saev_l1_logistic_iterate", "negative n_iters");
    for (int it = 0; it < n_iters; ++it) sl_iteration(a, s, true, 0);
    if (hipGetLastError() != hipSuccess) return entry_refuse(SAEV_HIP_ERROR, "saev_l1_logistic_iterate", "kernel launch failed");
    return SAEV_OK;
}

int saev_l1_logistic_result(const float* X, const int32_t* y, int64_t n, int64_t S, int64_t K, double C, double kkt_tol, double* coef,
                            double* intercept, double* scalars, void* workspace, int64_t workspace_bytes, void* stream) {
    SL_ENTRY("saev_l1_logistic_result")
    if (!coef || !intercept || !scalars) return entry_refuse(SAEV_INVALID_ARG, "saev_l1_logistic_result", "coef, intercept and scalars must not be NULL");
    // a fit that is not done gives up its momentum: the residual and the objective are then those of the iterate itself
    hipLaunchKernelGGL(sl_unmomentum_kernel, dim3(1), dim3(1), 0, s, a.state);
    sl_iteration(a, s, false, 1);
    const size_t total = (size_t)a.Kc * (size_t)S;
    hipLaunchKernelGGL(sl_out_kernel, dim3((unsigned)std::min<size_t>((total + 255) / 256, 4096)), dim3(256), 0, s, a, coef, intercept, scalars);
    if (hipGetLastError() != hipSuccess) return entry_refuse(SAEV_HIP_ERROR, "saev_l1_logistic_result", "kernel launch failed");
    return SAEV_OK;
}
