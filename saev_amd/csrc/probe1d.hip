// Per-latent logistic probes on sparse codes (include/saev_amd.h: PROBE1D): for each of the S x C (latent, class)
// pairs a two-parameter logistic regression y_c ~ sigma(b + w x_j), fitted by damped Newton (Levenberg-Marquardt) steps whose
// sums run over the latent's stored entries only -- the rows where the latent is zero enter in closed form.
//
//   prepare  the events latent-major: a stable counting sort of the CSR entries by latent, the regroup of DESIGN.md 3.22 in
//            this unit's own kernels, under the rule "every entry of a latent in [0, S)"; the part rule (lm_parts, lm_part_len,
//            LM_PARTS) is entry_util.h's, shared with latent_major.h.  The entries are cut into up to
//            LM_PARTS contiguous parts; integer atomics count every (part, latent); a pass per latent turns the counts into the
//            parts' offsets inside the latent's segment; a scan over the latents gives `starts` and the chunk list; then ONE WAVE
//            PER PART walks its entries in order, 64 at a time, and places each behind the earlier ones of its latent (the rank
//            inside the group of 64 by comparing lanes, the group's base by one integer atomic of the latent's first lane on a
//            cursor only this wave touches).  Rows ascend inside a part and parts are in row order, so every segment ends up in
//            ascending row order whatever the timing.  Then qx per latent (fp64, lanes strided, a fixed shuffle tree), the label
//            bits and the class counts (integer atomics).
//   events   the hot kernel, lane = class: a wave owns one chunk (P1_CHUNK events) of one latent and up to 64 classes; (row, v) of
//            an event is the same in every lane, the row's label bits are one word per lane; each lane keeps (b, w) of its pair and
//            its accumulators in registers.  A chunk is eight sub-chunks of 64 events, each summed from zero in event order and
//            added to the chunk's sums in sub-chunk order.  With at most 32 classes 2, 4 or 8 sub-chunks run side by side in the
//            lanes a single class group leaves idle and are added in the same order through lane shuffles: the sums of a pair do
//            not depend on how many classes there are.  A latent of one chunk stores its sums; a cut latent stores chunk partials
//            that p1_reduce_kernel adds in chunk order.  Every operation is written out (no contraction left to the compiler).
//   update   one thread per pair: gradient, curvature and loss from the sums and the closed-form share of the zero rows, the rho
//            rule on the damping, up to five damped 2 x 2 solves, the fallback step; state in place.  The slab's largest scaled
//            gradient is an integer max on the bits of a non-negative double; p1_slab_kernel turns it into the slab's done flag.
//   evaluate the events pass with other accumulators (loss and three exact counts), then the closed form per pair.
//
// No floating-point atomic, no (nnz, C) temporary; nothing is read back except the optional poll of the done counter in fit.
#include "entry_util.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace {

constexpr int P1_SUB = 64;                      // events per sub-chunk
constexpr int P1_NSUBCHUNK = P1_CHUNK / P1_SUB;  // 8
constexpr int P1_SCAN_THREADS = 1024;

void p1_layout(int64_t N, int64_t S, int64_t C, int64_t nnz, saev_probe1d_layout* L) {
    std::memset(L, 0, sizeof *L);
    L->struct_size = (int32_t)sizeof *L;
    L->chunk = P1_CHUNK;
    L->words = (C + 31) / 32;
    L->max_chunks = nnz / P1_CHUNK + S;
    L->parts = lm_parts(S, nnz);
    WsCarve ws;
    const int64_t pairs = S * C;
    L->off_err = ws.take(64);
    L->off_starts = ws.take(8 * (S + 1));
    L->off_chunk_starts = ws.take(4 * (S + 1));
    L->off_row = ws.take(4 * nnz);
    L->off_val = ws.take(4 * nnz);
    L->off_qx = ws.take(8 * S);
    L->off_ybits = ws.take(4 * N * L->words);
    L->off_pos = ws.take(8 * C);
    L->off_cnt = ws.take(4 * (int64_t)L->parts * S);
    L->off_tot = ws.take(4 * S);
    L->off_b = ws.take(8 * pairs);
    L->off_w = ws.take(8 * pairs);
    L->off_lam = ws.take(8 * pairs);
    L->off_prev_pred = ws.take(8 * pairs);
    L->off_prev_loss = ws.take(8 * pairs);
    L->off_clipped = ws.take(4 * pairs);
    L->off_sums = ws.take(8 * 7 * pairs);
    L->off_part = ws.take(8 * 7 * C * L->max_chunks);
    L->off_gmax = ws.take(8 * C);
    L->off_done = ws.take(4 * C);
    L->off_n_iter = ws.take(4 * C);
    L->off_active = ws.take(64);
    L->total_bytes = ws.at;
}

// ---------------------------------------------------------------- prepare ----------------------------------------------------------------

__global__ __launch_bounds__(256) void p1_count_kernel(const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ indices, long nnz, int S,
                                                       long part_len, int32_t* __restrict__ cnt, int32_t* __restrict__ err) {
    const int64_t p0 = row_ptr[0];
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < nnz; e += (long)gridDim.x * 256) {
        const int col = indices[p0 + e];
        if (col < 0 || col >= S) { atomicMax(err, SAEV_PROBE1D_ERR_LATENT); continue; }
        atomicAdd(cnt + (e / part_len) * S + col, 1);
    }
}

// cnt[p][l] -> the entries of latent l in parts before p; tot[l] = all of them
__global__ __launch_bounds__(256) void p1_parts_kernel(int32_t* __restrict__ cnt, int parts, int S, int32_t* __restrict__ tot) {
    const long l = (long)blockIdx.x * 256 + threadIdx.x;
    if (l >= S) return;
    int run = 0;
    for (int p = 0; p < parts; ++p) {
        const int t = cnt[(size_t)p * S + l];
        cnt[(size_t)p * S + l] = run;
        run += t;
    }
    tot[l] = run;
}

// starts[l] = sum of tot[0 .. l), chunk_starts[l] = sum of ceil(tot / P1_CHUNK) over the same: one workgroup, both sums in the two
// halves of one 64-bit word (each stays below 2^31)
__global__ __launch_bounds__(P1_SCAN_THREADS) void p1_scan_kernel(const int32_t* __restrict__ tot, int S, int64_t* __restrict__ starts,
                                                                  int32_t* __restrict__ chunk_starts) {
    typedef unsigned long long u64;
    const u64 end = block_scan_rounds<P1_SCAN_THREADS, u64, long>(
        S,
        [&](long l) {
            const unsigned n = (unsigned)tot[l];
            return ((u64)((n + P1_CHUNK - 1) / P1_CHUNK) << 32) | n;
        },
        [&](long l, u64 start) { starts[l] = (int64_t)(start & 0xffffffffull); chunk_starts[l] = (int32_t)(start >> 32); });
    if (threadIdx.x == 0) { starts[S] = (int64_t)(end & 0xffffffffull); chunk_starts[S] = (int32_t)(end >> 32); }
}

// one wave per part (see the head of the file)
__global__ __launch_bounds__(64) void p1_place_kernel(const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ indices,
                                                      const float* __restrict__ data, long nnz, int N, int S, long part_len,
                                                      const int64_t* __restrict__ starts, int32_t* __restrict__ cnt,
                                                      int32_t* __restrict__ row_out, float* __restrict__ val_out) {
    const int lane = threadIdx.x;
    const long part = blockIdx.x;
    const long first = part * part_len, last = min(first + part_len, nnz);
    int32_t* cur = cnt + (size_t)part * S;
    for (long g = first; g < last; g += 64) {
        const long e = g + lane;
        int col = -1, row = 0;
        float v = 0.f;
        if (e < last) {
            const int64_t p = row_ptr[0] + e;
            col = indices[p];
            if (col < 0 || col >= S) col = -1;  // (reported by the count pass)
            row = csr_row_of(row_ptr, N, p);
            v = data[p];
        }
        int rank = 0, same = 0, leader = 64;
        for (int i = 0; i < 64; ++i) {
            const int o = __shfl(col, i, 64);
            if (col >= 0 && o == col) {
                ++same;
                if (i < lane) ++rank;
                if (leader == 64) leader = i;
            }
        }
        int base = 0;
        if (col >= 0 && leader == lane) base = atomicAdd(cur + col, same);
        base = __shfl(base, leader & 63, 64);
        if (col >= 0) {
            const int64_t at = starts[col] + base + rank;
            if (at >= 0 && at < nnz) { row_out[at] = row; val_out[at] = v; }  // (always: the segments partition the entries)
        }
    }
}

// qx[l] = max(sqrt(sum v^2 / n_l), 1e-6), 1 for a latent without entries: squares and sums in fp64, lane i takes entries i, i + 64, ...
__global__ __launch_bounds__(256) void p1_qx_kernel(const int64_t* __restrict__ starts, const float* __restrict__ val, int S, double* __restrict__ qx) {
    const int lane = threadIdx.x & 63;
    const long l = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (l >= S) return;
    const int64_t s0 = starts[l], s1 = starts[l + 1];
    double acc = 0.0;
    for (int64_t e = s0 + lane; e < s1; e += 64) { const double v = (double)val[e]; acc = fma(v, v, acc); }
    acc = wave_sum_d(acc);
    if (lane == 0) qx[l] = s1 > s0 ? fmax(sqrt(acc / (double)(s1 - s0)), 1e-6) : 1.0;
}

__global__ __launch_bounds__(256) void p1_labels_ids_kernel(const uint8_t* __restrict__ ids8, const int32_t* __restrict__ ids32, int N, int C, int W,
                                                            uint32_t* __restrict__ ybits, unsigned long long* __restrict__ pos, int32_t* __restrict__ err) {
    const long r = (long)blockIdx.x * 256 + threadIdx.x;
    if (r >= N) return;
    int cls = ids8 ? (int)ids8[r] : ids32[r];
    if (cls < 0 || cls >= C) { atomicMax(err, SAEV_PROBE1D_ERR_CLASS); cls = -1; }
    for (int wi = 0; wi < W; ++wi) ybits[(size_t)r * W + wi] = (cls >= 0 && (cls >> 5) == wi) ? (1u << (cls & 31)) : 0u;
    if (cls >= 0) atomicAdd(pos + cls, 1ull);
}

__global__ __launch_bounds__(256) void p1_labels_matrix_kernel(const uint8_t* __restrict__ y, int N, int C, int W, uint32_t* __restrict__ ybits,
                                                               unsigned long long* __restrict__ pos, int32_t* __restrict__ err) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long)N * W) return;
    const long r = t / W;
    const int wi = (int)(t - r * W);
    uint32_t bits = 0;
    for (int j = 0; j < 32; ++j) {
        const int c = wi * 32 + j;
        if (c >= C) break;
        const uint8_t yv = y[(size_t)r * C + c];
        if (yv > 1) atomicMax(err, SAEV_PROBE1D_ERR_LABEL);
        if (yv == 1) { bits |= 1u << j; atomicAdd(pos + c, 1ull); }
    }
    ybits[t] = bits;
}

// ---------------------------------------------------------------- events -----------------------------------------------------------------

struct P1Ev {
    const int64_t* starts;
    const int32_t* chunk_starts;
    const int32_t* row;
    const float* val;
    const uint32_t* ybits;
    const double* b;
    const double* w;
    const int32_t* done;  // per slab, or NULL
    double* sums;         // (S, 7, C)
    double* part;         // (chunks, 7, C)
    double threshold;     // evaluate
    int S, C, W, slab;
};

// sigma(|z|), sigma(-|z|) and log1p(exp(-|z|)): every term of an event is a product or sum of these, none by cancellation
__device__ __forceinline__ void p1_sigmoid(double z, double* hi, double* lo, double* l1p) {
    const double e = exp(-fabs(z));
    const double inv = 1.0 / __dadd_rn(1.0, e);
    *hi = inv;
    *lo = __dmul_rn(e, inv);
    *l1p = log1p(e);
}

template <bool EVAL>
__device__ __forceinline__ void p1_event(double b, double w, float vf, bool y, double thr, double (&acc)[EVAL ? 4 : 7]) {
    const double v = (double)vf;
    const double z = __dadd_rn(b, __dmul_rn(w, v));
    double hi, lo, l1p;
    p1_sigmoid(z, &hi, &lo, &l1p);
    const bool up = z >= 0.0;
    const double mu = up ? hi : lo;
    const double loss = __dadd_rn(y ? fmax(-z, 0.0) : fmax(z, 0.0), l1p);
    if constexpr (EVAL) {
        const bool pred = mu > thr;
        acc[0] = __dadd_rn(acc[0], loss);
        acc[1] = __dadd_rn(acc[1], y ? 1.0 : 0.0);
        acc[2] = __dadd_rn(acc[2], (pred && y) ? 1.0 : 0.0);
        acc[3] = __dadd_rn(acc[3], (pred && !y) ? 1.0 : 0.0);
    } else {
        const double om = up ? lo : hi;  // 1 - mu
        const double s = __dmul_rn(hi, lo);
        const double r = y ? -om : mu;   // mu - y
        const double sv = __dmul_rn(s, v);
        acc[0] = __dadd_rn(acc[0], mu);
        acc[1] = fma(r, v, acc[1]);
        acc[2] = __dadd_rn(acc[2], s);
        acc[3] = __dadd_rn(acc[3], sv);
        acc[4] = fma(sv, v, acc[4]);
        acc[5] = __dadd_rn(acc[5], loss);
        acc[6] = __dadd_rn(acc[6], y ? 1.0 : 0.0);
    }
}

// NSUB sub-chunks side by side: 64 / NSUB lanes (classes) each.  grid: (ceil(max chunks / 4), class groups of 64 / NSUB)
template <int NSUB, bool EVAL>
__global__ __launch_bounds__(256) void p1_events_kernel(P1Ev a) {
    constexpr int NACC = EVAL ? 4 : 7;
    constexpr int CP = 64 / NSUB;
    const int lane = threadIdx.x & 63;
    const long chunk = (long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (chunk >= a.chunk_starts[a.S]) return;
    int llo = 0, lhi = a.S;  // the latent l with chunk_starts[l] <= chunk < chunk_starts[l + 1]
    while (lhi - llo > 1) {
        const int mid = llo + ((lhi - llo) >> 1);
        if (a.chunk_starts[mid] <= chunk) llo = mid; else lhi = mid;
    }
    const int l = llo;
    const int nch = a.chunk_starts[l + 1] - a.chunk_starts[l];
    const int64_t e0 = a.starts[l] + (int64_t)(chunk - a.chunk_starts[l]) * P1_CHUNK;
    const int64_t e1 = min(e0 + (int64_t)P1_CHUNK, a.starts[l + 1]);
    const int sub = lane / CP, cl = lane - sub * CP;
    const int c = blockIdx.y * CP + cl;
    const bool active = c < a.C && (a.done == nullptr || a.done[c / a.slab] == 0);
    if (!__any(active)) return;
    const double b = active ? a.b[(size_t)l * a.C + c] : 0.0;
    const double w = active ? a.w[(size_t)l * a.C + c] : 0.0;
    const int wi = active ? (c >> 5) : 0, bit = c & 31;

    double tot[NACC];
#pragma unroll
    for (int k = 0; k < NACC; ++k) tot[k] = 0.0;
    for (int r = 0; r < P1_NSUBCHUNK / NSUB; ++r) {
        const int64_t s0 = e0 + (int64_t)(r * NSUB + sub) * P1_SUB;
        const int64_t s1 = min(s0 + (int64_t)P1_SUB, e1);
        double acc[NACC];
#pragma unroll
        for (int k = 0; k < NACC; ++k) acc[k] = 0.0;
        if (active) {
            for (int64_t e = s0; e < s1; ++e) {
                const int row = a.row[e];
                const float v = a.val[e];
                const uint32_t bits = a.ybits[(size_t)row * a.W + wi];
                p1_event<EVAL>(b, w, v, ((bits >> bit) & 1u) != 0u, a.threshold, acc);
            }
        }
        if constexpr (NSUB == 1) {
#pragma unroll
            for (int k = 0; k < NACC; ++k) tot[k] = __dadd_rn(tot[k], acc[k]);
        } else {
#pragma unroll
            for (int s = 0; s < NSUB; ++s)
#pragma unroll
                for (int k = 0; k < NACC; ++k) tot[k] = __dadd_rn(tot[k], __shfl(acc[k], s * CP + cl, 64));
        }
        if (e0 + (int64_t)(r + 1) * NSUB * P1_SUB >= e1) break;  // (the sub-chunks left are empty: they would add zeros)
    }
    if (active && sub == 0) {
        double* dst = nch == 1 ? a.sums + (size_t)l * 7 * a.C : a.part + (size_t)chunk * 7 * a.C;
#pragma unroll
        for (int k = 0; k < NACC; ++k) dst[(size_t)k * a.C + c] = tot[k];
    }
}

// sums of the cut latents: chunk partials added in chunk order; a latent without events gets zeros.  grid: (S, ceil(nacc C / 256))
__global__ __launch_bounds__(256) void p1_reduce_kernel(const int32_t* __restrict__ chunk_starts, const double* __restrict__ part,
                                                        const int32_t* __restrict__ done, int C, int slab, int nacc, double* __restrict__ sums) {
    const int l = blockIdx.x;
    const int c0 = chunk_starts[l], c1 = chunk_starts[l + 1];
    if (c1 - c0 == 1) return;
    const int t = blockIdx.y * 256 + threadIdx.x;
    if (t >= nacc * C) return;
    const int c = t % C;
    if (done != nullptr && done[c / slab] != 0) return;
    double acc = 0.0;
    for (int ch = c0; ch < c1; ++ch) acc = __dadd_rn(acc, part[(size_t)ch * 7 * C + t]);
    sums[(size_t)l * 7 * C + t] = acc;
}

// ---------------------------------------------------------------- update -----------------------------------------------------------------

struct P1Cfg {
    double ridge, tol, lam_init, lam_shrink, lam_grow, delta_logit;
};
constexpr double P1_EPS = 1e-8, P1_LAM_MIN = 1e-12, P1_LAM_MAX = 1e12, P1_FALLBACK = 1e-3;

__device__ __forceinline__ double p1_clamp(double x, double lo, double hi) { return fmin(fmax(x, lo), hi); }
__device__ __forceinline__ double p1_base(double pi) {
    const double p = p1_clamp(pi, P1_EPS, 1.0 - P1_EPS);
    return log(p / (1.0 - p));
}
__device__ __forceinline__ double p1_sigma(double z) {
    const double e = exp(-fabs(z));
    const double inv = 1.0 / (1.0 + e);
    return z >= 0.0 ? inv : e * inv;
}

struct P1Upd {
    const double* sums;
    double *b, *w, *lam, *prev_pred, *prev_loss;
    int32_t* clipped;
    const int64_t* starts;
    const double* qx;
    const unsigned long long* pos;
    unsigned long long* gmax;
    const int32_t* done;
    double* step_out;    // optional (pairs, 4): db, dw, pred, lam after the step
    int32_t* flags_out;  // optional (pairs): SAEV_PROBE1D_STEP_* bits | tries << 8
    long pairs;
    int C, slab;
    double n;
    P1Cfg cfg;
};

__global__ __launch_bounds__(256) void p1_update_kernel(P1Upd a) {
#pragma clang fp contract(off)
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.pairs) return;
    const long l = i / a.C;
    const int c = (int)(i - l * a.C);
    const int sl = c / a.slab;
    if (a.done[sl] != 0) return;
    const P1Cfg& g = a.cfg;
    const double n = a.n;
    const double* s = a.sums + (size_t)l * 7 * a.C + c;
    const double S_mu = s[0], S_g1 = s[(size_t)a.C], S_h0 = s[(size_t)2 * a.C], S_h1 = s[(size_t)3 * a.C], S_h2 = s[(size_t)4 * a.C],
                 S_loss = s[(size_t)5 * a.C], S_y = s[(size_t)6 * a.C];
    const double nnz = (double)(a.starts[l + 1] - a.starts[l]);
    const bool empty = nnz == 0.0;
    const double pi = (double)a.pos[c] / n;
    const double base = p1_base(pi);
    double b = a.b[i], w = a.w[i], lam = a.lam[i];
    const double pp = a.prev_pred[i], pl = a.prev_loss[i];
    const bool pclip = a.clipped[i] != 0;
    const double qx = a.qx[l], qx_sq = qx * qx;

    const double mu0 = p1_clamp(p1_sigma(b), P1_EPS, 1.0 - P1_EPS);
    const double s0 = mu0 * (1.0 - mu0);
    const double zf = fmax(n - nnz, 0.0) / n;
    double g0 = S_mu / n + zf * mu0 - pi;
    g0 = g0 + g.ridge * (b - base);
    double g1 = S_g1 / n + g.ridge * w;
    const double h0 = S_h0 / n + zf * s0 + g.ridge;
    const double h1 = S_h1 / n;
    const double h2 = S_h2 / n + g.ridge;
    const double pos_zero = fmin(fmax(pi - S_y / n, 0.0), zf);
    const double neg_zero = zf - pos_zero;
    const double zero_loss = -(pos_zero * log(mu0) + neg_zero * log1p(-fmin(mu0, 1.0 - P1_EPS)));
    const double loss = S_loss / n + zero_loss + 0.5 * g.ridge * (w * w + (b - base) * (b - base));
    if (empty) { g0 = 0.0; g1 = 0.0; lam = g.lam_init; }

    int flags = 0;
    if (isfinite(pp) && isfinite(pl)) {  // the rho rule, before the step
        const double rho = (pl - loss) / fmax(pp, 1e-18);
        const bool grow = rho <= 0.25 || pclip;
        const bool shrink = rho >= 0.75 && !pclip;
        if (shrink) { lam = lam * g.lam_shrink; flags |= SAEV_PROBE1D_STEP_SHRUNK; }
        if (grow) { lam = lam * g.lam_grow; flags |= SAEV_PROBE1D_STEP_GROWN; }
        lam = p1_clamp(lam, P1_LAM_MIN, P1_LAM_MAX);
    }

    double db = 0.0, dw = 0.0, pred = 0.0;
    bool clipped = false, success = fmax(fabs(g0), fabs(g1)) <= g.tol;
    const double qxr = sqrt(qx_sq);
    int tries = 0;
    if (success) flags |= SAEV_PROBE1D_STEP_INACTIVE;
    for (int t = 0; t < 5 && !success; ++t) {
        ++tries;
        const double h0e = h0 + lam, h2e = h2 + lam * qx_sq;
        const double det = h0e * h2e - h1 * h1;
        const bool valid = fabs(det) > 1e-18;
        const double ds = valid ? det : 1.0;
        double dbt = (h2e * g0 - h1 * g1) / ds, dwt = (h0e * g1 - h1 * g0) / ds;
        if (!valid) { dbt = 0.0; dwt = 0.0; flags |= SAEV_PROBE1D_STEP_SINGULAR; }
        const double qd = qxr * dwt;
        const double norm = sqrt(dbt * dbt + qd * qd);
        const bool clip = norm > g.delta_logit;
        const double scale = clip ? g.delta_logit / (norm + 1e-18) : 1.0;
        dbt = dbt * scale;
        dwt = dwt * scale;
        const double predt = g0 * dbt + g1 * dwt - 0.5 * (h0 * (dbt * dbt) + 2.0 * h1 * dbt * dwt + h2 * (dwt * dwt));
        if (isfinite(predt) && predt > 0.0) {
            db = dbt; dw = dwt; pred = predt; clipped = clip; success = true;
        } else {
            lam = p1_clamp(lam * g.lam_grow, P1_LAM_MIN, P1_LAM_MAX);
        }
    }
    if (!success) {  // five failures: a step of norm 1e-3 delta_logit along the gradient, as the reference takes it
        const double qs = fmax(qxr, 1e-12);
        const double qg = qs * g1;
        const double gs = sqrt(g0 * g0 + qg * qg);
        const double alpha = gs > 0.0 ? (P1_FALLBACK * g.delta_logit) / (gs + 1e-18) : 0.0;
        db = -alpha * g0;
        dw = -alpha * g1;
        pred = __builtin_nan("");
        clipped = true;
        flags |= SAEV_PROBE1D_STEP_FALLBACK;
    }
    lam = p1_clamp(lam, P1_LAM_MIN, P1_LAM_MAX);
    if (clipped) flags |= SAEV_PROBE1D_STEP_CLIPPED;
    b = b - db;
    w = w - dw;
    if (empty) {
        b = base; w = 0.0; lam = g.lam_init; db = 0.0; dw = 0.0; pred = __builtin_nan(""); clipped = false;
        flags |= SAEV_PROBE1D_STEP_EMPTY;
    }
    a.b[i] = b;
    a.w[i] = w;
    a.lam[i] = lam;
    a.prev_pred[i] = pred;
    a.prev_loss[i] = loss;
    a.clipped[i] = clipped ? 1 : 0;
    if (a.step_out) {
        a.step_out[4 * i] = db; a.step_out[4 * i + 1] = dw; a.step_out[4 * i + 2] = pred; a.step_out[4 * i + 3] = lam;
    }
    if (a.flags_out) a.flags_out[i] = flags | (tries << 8);
    // the slab's termination measure: max(|g0|, |g1 / qx|) -- non-negative doubles order as their bit patterns (NaN above all)
    const double ga = fmax(fabs(g0), fabs(g1 / fmax(qxr, 1e-12)));
    const double key = (g0 != g0 || g1 != g1) ? __builtin_nan("") : ga;
    atomicMax(a.gmax + sl, (unsigned long long)__double_as_longlong(fabs(key)));
}

// per slab: count the iteration, stop after the first one whose largest scaled gradient is <= tol; *n_active = slabs still running
__global__ __launch_bounds__(256) void p1_slab_kernel(unsigned long long* __restrict__ gmax, int32_t* __restrict__ done, int32_t* __restrict__ n_iter,
                                                      int n_slabs, double tol, int32_t* __restrict__ n_active) {
    __shared__ int live;
    if (threadIdx.x == 0) live = 0;
    __syncthreads();
    int mine = 0;
    for (int s = threadIdx.x; s < n_slabs; s += 256) {
        if (done[s] != 0) continue;
        n_iter[s] += 1;
        const double m = __longlong_as_double((long long)gmax[s]);
        if (m <= tol) done[s] = 1; else ++mine;
        gmax[s] = 0ull;
    }
    if (mine) atomicAdd(&live, mine);
    __syncthreads();
    if (threadIdx.x == 0) *n_active = live;
}

__global__ __launch_bounds__(256) void p1_init_kernel(double* b, double* w, double* lam, double* pp, double* pl, int32_t* clipped,
                                                      const unsigned long long* __restrict__ pos, long pairs, int C, double n, double lam_init,
                                                      unsigned long long* gmax, int32_t* done, int32_t* n_iter, int32_t* n_active, int n_slabs) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < C) { gmax[i] = 0ull; done[i] = i < n_slabs ? 0 : 1; n_iter[i] = 0; }
    if (i == 0) *n_active = n_slabs;
    if (i >= pairs) return;
    const int c = (int)(i % C);
    b[i] = p1_base((double)pos[c] / n);
    w[i] = 0.0;
    lam[i] = lam_init;
    pp[i] = __builtin_nan("");
    pl[i] = __builtin_nan("");
    clipped[i] = 0;
}

template <typename T>
__global__ __launch_bounds__(256) void p1_export_kernel(const double* __restrict__ b, const double* __restrict__ w, long pairs, T* __restrict__ coef,
                                                        T* __restrict__ intercept, const int32_t* __restrict__ n_iter, int C, int slab,
                                                        int32_t* __restrict__ n_iter_out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < C && n_iter_out) n_iter_out[i] = n_iter[i / slab];
    if (i >= pairs) return;
    if (coef) coef[i] = (T)w[i];
    if (intercept) intercept[i] = (T)b[i];
}

// ---------------------------------------------------------------- evaluate ---------------------------------------------------------------

__device__ __forceinline__ double p1_softplus(double x) { return fmax(x, 0.0) + log1p(exp(-fabs(x))); }

template <typename T>
__global__ __launch_bounds__(256) void p1_eval_finish_kernel(const double* __restrict__ sums, const double* __restrict__ b, const int64_t* __restrict__ starts,
                                                             const unsigned long long* __restrict__ pos, long pairs, int C, double n, double thr,
                                                             T* loss, T* tp, T* fp, T* tn, T* fn) {
#pragma clang fp contract(off)
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= pairs) return;
    const long l = i / C;
    const int c = (int)(i - l * C);
    const double* s = sums + (size_t)l * 7 * C + c;
    const double loss_nz = s[0], pos_nz = s[(size_t)C], tp_nz = s[(size_t)2 * C], fp_nz = s[(size_t)3 * C];
    const double nnz = (double)(starts[l + 1] - starts[l]);
    const double n_zero = n - nnz;
    const double pos_zero = fmin(fmax((double)pos[c] - pos_nz, 0.0), n_zero);
    const double neg_zero = n_zero - pos_zero;
    const double bb = b[i];
    const bool pz = p1_sigma(bb) > thr;
    if (loss) loss[i] = (T)((loss_nz + pos_zero * p1_softplus(-bb) + neg_zero * p1_softplus(bb)) / n);
    if (tp) tp[i] = (T)(tp_nz + (pz ? pos_zero : 0.0));
    if (fp) fp[i] = (T)(fp_nz + (pz ? neg_zero : 0.0));
    if (fn) fn[i] = (T)((pos_nz - tp_nz) + (pz ? 0.0 : pos_zero));
    if (tn) tn[i] = (T)((nnz - pos_nz - fp_nz) + (pz ? 0.0 : neg_zero));
}

// ---------------------------------------------------------------- host -------------------------------------------------------------------

struct P1Ws {
    saev_probe1d_layout L;
    uint8_t* p;
    template <typename T> T* at(int64_t off) const { return reinterpret_cast<T*>(p + off); }
};

int p1_open(const char* who, int64_t N, int64_t S, int64_t C, int64_t nnz, void* ws, int64_t ws_bytes, P1Ws* out) {
    if (const int rc = entry_check_shape(who, N, S, C, nnz)) return rc;
    p1_layout(N, S, C, nnz, &out->L);
    if (const int rc = entry_check_workspace(who, ws, ws_bytes, out->L.total_bytes, "workspace smaller than saev_probe1d_workspace_bytes(N, S, C, nnz)")) return rc;
    out->p = static_cast<uint8_t*>(ws);
    return SAEV_OK;
}

int p1_cfg(const char* who, const saev_probe1d_cfg* cfg, saev_probe1d_cfg* c) {
    if (!cfg || cfg->struct_size < (int32_t)(2 * sizeof(int32_t))) return entry_refuse(SAEV_INVALID_ARG, who, "no saev_probe1d_cfg (or its struct_size is unset)");
    std::memset(c, 0, sizeof *c);
    std::memcpy(c, cfg, std::min<size_t>(sizeof *c, (size_t)cfg->struct_size));
    if (c->max_iter < 0) return entry_refuse(SAEV_INVALID_ARG, who, "max_iter must be >= 0");
    if (c->class_slab_size < 1) return entry_refuse(SAEV_INVALID_ARG, who, "class_slab_size must be >= 1");
    if (c->poll_every < 0) return entry_refuse(SAEV_INVALID_ARG, who, "poll_every must be >= 0");
    if (c->out_dtype != SAEV_PROBE1D_F32 && c->out_dtype != SAEV_PROBE1D_F64) return entry_refuse(SAEV_INVALID_ARG, who, "out_dtype must be SAEV_PROBE1D_F32 or SAEV_PROBE1D_F64");
    if (!(c->lam_shrink > 0.0 && c->lam_shrink < 1.0)) return entry_refuse(SAEV_INVALID_ARG, who, "lam_shrink must lie in (0, 1)");
    if (!(c->lam_grow > 1.0)) return entry_refuse(SAEV_INVALID_ARG, who, "lam_grow must be > 1");
    if (!(c->delta_logit > 0.0)) return entry_refuse(SAEV_INVALID_ARG, who, "delta_logit must be > 0");
    if (!(c->ridge >= 0.0) || !(c->tol >= 0.0) || !(c->lam_init > 0.0)) return entry_refuse(SAEV_INVALID_ARG, who, "ridge and tol must be >= 0 and lam_init > 0");
    return SAEV_OK;
}

template <bool EVAL>
void p1_launch_events(const P1Ws& W, int64_t S, int64_t C, const double* b, const double* w, const int32_t* done, int slab, double thr, double* sums,
                      hipStream_t s) {
    P1Ev a{W.at<int64_t>(W.L.off_starts), W.at<int32_t>(W.L.off_chunk_starts), W.at<int32_t>(W.L.off_row), W.at<float>(W.L.off_val),
           W.at<uint32_t>(W.L.off_ybits), b, w, done, sums, W.at<double>(W.L.off_part), thr, (int)S, (int)C, (int)W.L.words, slab};
    const unsigned gx = (unsigned)((W.L.max_chunks + 3) / 4);
    if (C <= 8) hipLaunchKernelGGL((p1_events_kernel<8, EVAL>), dim3(gx, 1), dim3(256), 0, s, a);
    else if (C <= 16) hipLaunchKernelGGL((p1_events_kernel<4, EVAL>), dim3(gx, 1), dim3(256), 0, s, a);
    else if (C <= 32) hipLaunchKernelGGL((p1_events_kernel<2, EVAL>), dim3(gx, 1), dim3(256), 0, s, a);
    else hipLaunchKernelGGL((p1_events_kernel<1, EVAL>), dim3(gx, (unsigned)((C + 63) / 64)), dim3(256), 0, s, a);
    const int nacc = EVAL ? 4 : 7;
    hipLaunchKernelGGL(p1_reduce_kernel, dim3((unsigned)S, (unsigned)((nacc * C + 255) / 256)), dim3(256), 0, s, a.chunk_starts, a.part, done, (int)C,
                       slab, nacc, sums);
}

void p1_launch_update(const P1Ws& W, int64_t N, int64_t S, int64_t C, const saev_probe1d_cfg& c, const double* sums, double* step_out,
                      int32_t* flags_out, hipStream_t s) {
    P1Upd u{sums, W.at<double>(W.L.off_b), W.at<double>(W.L.off_w), W.at<double>(W.L.off_lam), W.at<double>(W.L.off_prev_pred),
            W.at<double>(W.L.off_prev_loss), W.at<int32_t>(W.L.off_clipped), W.at<int64_t>(W.L.off_starts), W.at<double>(W.L.off_qx),
            W.at<unsigned long long>(W.L.off_pos), W.at<unsigned long long>(W.L.off_gmax), W.at<int32_t>(W.L.off_done), step_out, flags_out,
            (long)(S * C), (int)C, c.class_slab_size, (double)N, P1Cfg{c.ridge, c.tol, c.lam_init, c.lam_shrink, c.lam_grow, c.delta_logit}};
    const int n_slabs = (int)((C + c.class_slab_size - 1) / c.class_slab_size);
    hipLaunchKernelGGL(p1_update_kernel, dim3((unsigned)((S * C + 255) / 256)), dim3(256), 0, s, u);
    hipLaunchKernelGGL(p1_slab_kernel, dim3(1), dim3(256), 0, s, u.gmax, W.at<int32_t>(W.L.off_done), W.at<int32_t>(W.L.off_n_iter), n_slabs, c.tol,
                       W.at<int32_t>(W.L.off_active));
}

void p1_launch_init(const P1Ws& W, int64_t N, int64_t S, int64_t C, const saev_probe1d_cfg& c, hipStream_t s) {
    const int n_slabs = (int)((C + c.class_slab_size - 1) / c.class_slab_size);
    const long pairs = (long)(S * C);
    hipLaunchKernelGGL(p1_init_kernel, dim3((unsigned)((std::max<long>(pairs, C) + 255) / 256)), dim3(256), 0, s, W.at<double>(W.L.off_b),
                       W.at<double>(W.L.off_w), W.at<double>(W.L.off_lam), W.at<double>(W.L.off_prev_pred), W.at<double>(W.L.off_prev_loss),
                       W.at<int32_t>(W.L.off_clipped), W.at<unsigned long long>(W.L.off_pos), pairs, (int)C, (double)N, c.lam_init,
                       W.at<unsigned long long>(W.L.off_gmax), W.at<int32_t>(W.L.off_done), W.at<int32_t>(W.L.off_n_iter),
                       W.at<int32_t>(W.L.off_active), n_slabs);
}

}  // namespace

int64_t saev_probe1d_workspace_bytes(int64_t N, int64_t S, int64_t C, int64_t nnz) {
    if (!entry_shape_ok(N, S, C, nnz)) return -1;
    saev_probe1d_layout L;
    p1_layout(N, S, C, nnz, &L);
    return L.total_bytes;
}

int saev_probe1d_layout_of(int64_t N, int64_t S, int64_t C, int64_t nnz, saev_probe1d_layout* out) {
    if (!out) return entry_refuse(SAEV_INVALID_ARG, "saev_probe1d_layout_of", "no saev_probe1d_layout");
    if (!entry_shape_ok(N, S, C, nnz)) return entry_refuse(SAEV_UNSUPPORTED, "saev_probe1d_layout_of", "1 <= N, S < 2^31, 1 <= C <= 4096, 0 <= nnz < 2^31");
    p1_layout(N, S, C, nnz, out);
    return SAEV_OK;
}

int saev_probe1d_prepare(const int64_t* row_ptr, const int32_t* indices, const float* data, int64_t nnz, int64_t N, int64_t S, int64_t C,
                         const uint8_t* class_u8, const int32_t* class_i32, const uint8_t* y_matrix, void* workspace, int64_t workspace_bytes,
                         void* stream) {
    P1Ws W;
    if (const int rc = p1_open("saev_probe1d_prepare", N, S, C, nnz, workspace, workspace_bytes, &W)) return rc;
    if (!row_ptr) return entry_refuse(SAEV_INVALID_ARG, "saev_probe1d_prepare", "row_ptr is NULL");
    if (nnz > 0 && (!indices || !data)) return entry_refuse(SAEV_INVALID_ARG, "saev_probe1d_prepare", "indices and data come with nnz > 0");
    const int forms = (class_u8 != nullptr) + (class_i32 != nullptr) + (y_matrix != nullptr);
    if (forms != 1) return entry_refuse(SAEV_INVALID_ARG, "saev_probe1d_prepare", "give the labels as class ids (uint8 or int32) or as an N x C 0/1 matrix, one of the three");
    if (class_u8 && C > 256) return entry_refuse(SAEV_INVALID_ARG, "saev_probe1d_prepare", "uint8 class ids cannot name more than 256 classes");

    hipStream_t s = (hipStream_t)stream;
    const saev_probe1d_layout& L = W.L;
    int32_t* err = W.at<int32_t>(L.off_err);
    int32_t* cnt = W.at<int32_t>(L.off_cnt);
    int64_t* starts = W.at<int64_t>(L.off_starts);
    const long part_len = (long)lm_part_len(nnz, (int)L.parts);
    bool ok = hipMemsetAsync(err, 0, 64, s) == hipSuccess;
    ok = ok && hipMemsetAsync(cnt, 0, (size_t)(4 * L.parts * S), s) == hipSuccess;
    ok = ok && hipMemsetAsync(W.at<uint8_t>(L.off_pos), 0, (size_t)(8 * C), s) == hipSuccess;
    if (!ok) return entry_refuse(SAEV_HIP_ERROR, "saev_probe1d_prepare", "hipMemsetAsync failed");
    if (nnz > 0) {
        const int grid = (int)std::min<int64_t>((nnz + 255) / 256, 8192);
        hipLaunchKernelGGL(p1_count_kernel, dim3(grid), dim3(256), 0, s, row_ptr, indices, (long)nnz, (int)S, part_len, cnt, err);
    }
    hipLaunchKernelGGL(p1_parts_kernel, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, s, cnt, (int)L.parts, (int)S, W.at<int32_t>(L.off_tot));
    hipLaunchKernelGGL(p1_scan_kernel, dim3(1), dim3(P1_SCAN_THREADS), 0, s, W.at<int32_t>(L.off_tot), (int)S, starts, W.at<int32_t>(L.off_chunk_starts));
    if (nnz > 0) {
        const unsigned used = (unsigned)((nnz + part_len - 1) / part_len);
        hipLaunchKernelGGL(p1_place_kernel, dim3(used), dim3(64), 0, s, row_ptr, indices, data, (long)nnz, (int)N, (int)S, part_len, starts, cnt,
                           W.at<int32_t>(L.off_row), W.at<float>(L.off_val));
    }
    hipLaunchKernelGGL(p1_qx_kernel, dim3((unsigned)((S + 3) / 4)), dim3(256), 0, s, starts, W.at<float>(L.off_val), (int)S, W.at<double>(L.off_qx));
    uint32_t* ybits = W.at<uint32_t>(L.off_ybits);
    unsigned long long* pos = W.at<unsigned long long>(L.off_pos);
    if (y_matrix)
        hipLaunchKernelGGL(p1_labels_matrix_kernel, dim3((unsigned)((N * L.words + 255) / 256)), dim3(256), 0, s, y_matrix, (int)N, (int)C, (int)L.words,
                           ybits, pos, err);
    else
        hipLaunchKernelGGL(p1_labels_ids_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, class_u8, class_i32, (int)N, (int)C, (int)L.words,
                           ybits, pos, err);
    if (hipGetLastError() != hipSuccess) return entry_refuse(SAEV_HIP_ERROR, "saev_probe1d_prepare", "kernel launch failed");
    return SAEV_OK;
}

int saev_probe1d_stats(int64_t N, int64_t S, int64_t C, int64_t nnz, const double* b, const double* w, double* sums_out, void* workspace,
                       int64_t workspace_bytes, void* stream) {
    P1Ws W;
    if (const int rc = p1_open("saev_probe1d_stats", N, S, C, nnz, workspace, workspace_bytes, &W)) return rc;
    if (!b || !w || !sums_out) return entry_refuse(SAEV_INVALID_ARG, "saev_probe1d_stats", "b, w and sums_out must not be NULL");
    p1_launch_events<false>(W, S, C, b, w, nullptr, 1, 0.0, sums_out, (hipStream_t)stream);
    if (hipGetLastError() != hipSuccess) return entry_refuse(SAEV_HIP_ERROR, "saev_probe1d_stats", "kernel launch failed");
    return SAEV_OK;
}

int saev_probe1d_init(int64_t N, int64_t S, int64_t C, int64_t nnz, const saev_probe1d_cfg* cfg, void* workspace, int64_t workspace_bytes,
                      void* stream) {
    P1Ws W;
    saev_probe1d_cfg c;
    if (const int rc = p1_open("saev_probe1d_init", N, S, C, nnz, workspace, workspace_bytes, &W)) return rc;
    if (const int rc = p1_cfg("saev_probe1d_init", cfg, &c)) return rc;
    p1_launch_init(W, N, S, C, c, (hipStream_t)stream);
    if (hipGetLastError() != hipSuccess) return entry_refuse(SAEV_HIP_ERROR, "saev_probe1d_init", "kernel launch failed");
    return SAEV_OK;
}

int saev_probe1d_update(int64_t N, int64_t S, int64_t C, int64_t nnz, const saev_probe1d_cfg* cfg, const double* sums, double* step_out,
                        int32_t* flags_out, void* workspace, int64_t workspace_bytes, void* stream) {
    P1Ws W;
    saev_probe1d_cfg c;
    if (const int rc = p1_open("saev_probe1d_update", N, S, C, nnz, workspace, workspace_bytes, &W)) return rc;
    if (const int rc = p1_cfg("saev_probe1d_update", cfg, &c)) return rc;
    p1_launch_update(W, N, S, C, c, sums ? sums : W.at<double>(W.L.off_sums), step_out, flags_out, (hipStream_t)stream);
    if (hipGetLastError() != hipSuccess) return entry_refuse(SAEV_HIP_ERROR, "saev_probe1d_update", "kernel launch failed");
    return SAEV_OK;
}

int saev_probe1d_fit(int64_t N, int64_t S, int64_t C, int64_t nnz, const saev_probe1d_cfg* cfg, void* coef_out, void* intercept_out,
                     int32_t* n_iter_out, void* workspace, int64_t workspace_bytes, void* stream) {
    P1Ws W;
    saev_probe1d_cfg c;
    if (const int rc = p1_open("saev_probe1d_fit", N, S, C, nnz, workspace, workspace_bytes, &W)) return rc;
    if (const int rc = p1_cfg("saev_probe1d_fit", cfg, &c)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const saev_probe1d_layout& L = W.L;
    p1_launch_init(W, N, S, C, c, s);
    double* sums = W.at<double>(L.off_sums);
    for (int it = 0; it < c.max_iter; ++it) {
        p1_launch_events<false>(W, S, C, W.at<double>(L.off_b), W.at<double>(L.off_w), W.at<int32_t>(L.off_done), c.class_slab_size, 0.0, sums, s);
        p1_launch_update(W, N, S, C, c, sums, nullptr, nullptr, s);
        if (c.poll_every > 0 && (it + 1) % c.poll_every == 0 && it + 1 < c.max_iter) {
            // the one optional read-back: how many slabs still run.  Stopped slabs are skipped on the device either way, so the
            // results do not depend on whether or when the host looks
            int32_t live = 1;
            if (hipMemcpyAsync(&live, W.at<int32_t>(L.off_active), 4, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
                return entry_refuse(SAEV_HIP_ERROR, "saev_probe1d_fit", "reading the done counter failed");
            if (live == 0) break;
        }
    }
    const unsigned grid = (unsigned)((std::max<int64_t>(S * C, C) + 255) / 256);
    if (c.out_dtype == SAEV_PROBE1D_F64)
        hipLaunchKernelGGL(p1_export_kernel<double>, dim3(grid), dim3(256), 0, s, W.at<double>(L.off_b), W.at<double>(L.off_w), (long)(S * C),
                           (double*)coef_out, (double*)intercept_out, W.at<int32_t>(L.off_n_iter), (int)C, c.class_slab_size, n_iter_out);
    else
        hipLaunchKernelGGL(p1_export_kernel<float>, dim3(grid), dim3(256), 0, s, W.at<double>(L.off_b), W.at<double>(L.off_w), (long)(S * C),
                           (float*)coef_out, (float*)intercept_out, W.at<int32_t>(L.off_n_iter), (int)C, c.class_slab_size, n_iter_out);
    if (hipGetLastError() != hipSuccess) return entry_refuse(SAEV_HIP_ERROR, "saev_probe1d_fit", "kernel launch failed");
    return SAEV_OK;
}

int saev_probe1d_evaluate(int64_t N, int64_t S, int64_t C, int64_t nnz, const double* b, const double* w, double threshold, int32_t out_dtype,
                          void* loss, void* tp, void* fp, void* tn, void* fn, void* workspace, int64_t workspace_bytes, void* stream) {
    P1Ws W;
    if (const int rc = p1_open("saev_probe1d_evaluate", N, S, C, nnz, workspace, workspace_bytes, &W)) return rc;
    if (!b || !w) return entry_refuse(SAEV_INVALID_ARG, "saev_probe1d_evaluate", "b and w must not be NULL");
    if (!(threshold > 0.0 && threshold < 1.0)) return entry_refuse(SAEV_INVALID_ARG, "saev_probe1d_evaluate", "threshold must lie in (0, 1)");
    if (out_dtype != SAEV_PROBE1D_F32 && out_dtype != SAEV_PROBE1D_F64) return entry_refuse(SAEV_INVALID_ARG, "saev_probe1d_evaluate", "out_dtype must be SAEV_PROBE1D_F32 or SAEV_PROBE1D_F64");
    hipStream_t s = (hipStream_t)stream;
    const saev_probe1d_layout& L = W.L;
    double* sums = W.at<double>(L.off_sums);
    p1_launch_events<true>(W, S, C, b, w, nullptr, 1, threshold, sums, s);
    const unsigned grid = (unsigned)((S * C + 255) / 256);
    if (out_dtype == SAEV_PROBE1D_F64)
        hipLaunchKernelGGL(p1_eval_finish_kernel<double>, dim3(grid), dim3(256), 0, s, sums, b, W.at<int64_t>(L.off_starts),
                           W.at<unsigned long long>(L.off_pos), (long)(S * C), (int)C, (double)N, threshold, (double*)loss, (double*)tp, (double*)fp,
                           (double*)tn, (double*)fn);
    else
        hipLaunchKernelGGL(p1_eval_finish_kernel<float>, dim3(grid), dim3(256), 0, s, sums, b, W.at<int64_t>(L.off_starts),
                           W.at<unsigned long long>(L.off_pos), (long)(S * C), (int)C, (double)N, threshold, (float*)loss, (float*)tp, (float*)fp,
                           (float*)tn, (float*)fn);
    if (hipGetLastError() != hipSuccess) return entry_refuse(SAEV_HIP_ERROR, "saev_probe1d_evaluate", "kernel launch failed");
    return SAEV_OK;
}
