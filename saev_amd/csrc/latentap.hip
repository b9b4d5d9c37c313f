// Exact tie-aware average precision of every latent against every class on sparse codes (include/saev_amd.h: LATENT AP;
// DESIGN.md 3.19): AP[j, c] of latent j's activation as a detector of class c, the expectation over all orders of tied scores
// (McSherry and Najork), with the latent's zero rows as ONE tie group in closed form.
//
//   sort     the stored entries by (latent, value descending, row ascending): a stable LSD radix sort, 8 bits a pass, four passes
//            over the order-reversing 32-bit image of the value and one to four over the latent (as many bytes as S needs).  An
//            entry that is no event (+-0.0, a latent outside [0, S)) gets the latent S and so ends up behind every event.  The
//            entries are cut into up to LA_MAX_PARTS contiguous parts; per pass a wave per part counts its digits in LDS (integer
//            atomics), a workgroup per digit scans its row of the (digit, part) table and leaves the digit's total, and a wave per part
//            (its cursors: the smaller digits' totals plus its own row prefix) walks its entries in order, 64 at a time:
//            the lanes of equal digit find each other with eight ballots, the rank inside the 64 is a population count and the
//            base a cursor in LDS that only this wave touches -- stable whatever the timing.  The key is a total order (entries
//            come in ascending row order), so the sorted arrays have one answer.  starts[j] is a lower bound in the sorted latents.
//   terms    lane = class: a wave owns one latent and up to 64 classes and walks the latent's events in rank order, 64 loaded at a
//            time and handed round by lane shuffles.  The value image and the row's class are the same in every lane; each lane
//            keeps r (rows of its class in the running group), R (in earlier groups) and the pair's sum in registers.  When the
//            value changes the group is closed: its term is added, R += r, t += n.  The zero group is put between the last
//            positive and the first negative event; a latent with negative events is walked once before to count each pair's
//            events (the zero group's r is pos_c minus that count).  A pair without events gets the zero group's term alone.
//            Groups of at most LA_DIRECT_MAX rows are summed term by term, larger ones use the closed form with
//            H_{t+n} - H_t from log1p and the differences of the asymptotic terms (la_dh).  No regrouping by class: no second
//            sort, no array per (event, class), and a pair's sum is a plain left-to-right sum in group order.
//   best     a wave per latent: the row maximum of ap and the lowest column that attains it.
//
// PROBE AP (include/saev_amd.h: PROBE AP) shares the sort (la_sort) and ranks by the per-pair score fl(fl(w a) + b):
//   probe    lane = class as above, but every lane has its own w and b and so its own tie groups: a group is closed per lane, with
//            no cross-lane operation under that branch (the shuffles that hand the 64 loaded events round stay at the top level of
//            the loop).  The events are walked by descending value for the lanes with w >= 0 and by ascending value for those with
//            w < 0 -- a direction no lane of the wave needs is skipped -- and the zero rows enter at a = 0 as one block that merges
//            with the neighbours whose rounded score equals b.
//   top rows a gather from row and starts.
//
// LATENT AUROC (include/saev_amd.h: LATENT AUROC) shares the sort too and walks lane = task; its kernels (au_*) carry
// their own description further down.  LATENT OPERATING POINTS (include/saev_amd.h: LATENT OPERATING POINTS) walks the
// same sorted events with the same role table (op_walk_kernel) and may take both from a workspace a call before it has filled.
//
// Integer atomics only (digit counts in LDS, class counts, the error word); nothing is read back, nothing synchronises.
#include "entry_util.h"

#include <algorithm>
#include <cstring>

namespace {

constexpr int LA_H_SMALL = 32;        // below this t the first terms of H_{t+n} - H_t are added directly
constexpr int LA_MAX_PARTS = 2048;
constexpr int LA_SCAN_THREADS = 256;

int la_latent_passes(int64_t S) { return S < (1 << 8) ? 1 : S < (1 << 16) ? 2 : S < (1 << 24) ? 3 : 4; }  // bytes that hold the value S

void la_layout(int64_t S, int64_t C, int64_t nnz, saev_latent_ap_layout* L) {
    std::memset(L, 0, sizeof *L);
    L->struct_size = (int32_t)sizeof *L;
    L->direct_max = LA_DIRECT_MAX;
    L->parts = std::max<int64_t>(1, std::min<int64_t>(LA_MAX_PARTS, (nnz + 63) / 64));
    L->part_len = std::max<int64_t>(64, ((nnz + L->parts - 1) / L->parts + 63) / 64 * 64);
    L->passes = 4 + la_latent_passes(S);
    WsCarve ws;
    L->off_err = ws.take(64);
    L->off_starts = ws.take(8 * (S + 1));
    L->off_hist = ws.take(4 * 256 * (L->parts + 1));  // the (digit, part) table and the 256 digit totals behind it
    L->off_key = ws.take(4 * nnz);
    L->off_latent = ws.take(4 * nnz);
    L->off_row = ws.take(4 * nnz);
    L->off_key2 = ws.take(4 * nnz);
    L->off_latent2 = ws.take(4 * nnz);
    L->off_row2 = ws.take(4 * nnz);
    L->total_bytes = ws.at;
    (void)C;
}

// ---------------------------------------------------------------- labels -----------------------------------------------------------------

__device__ __forceinline__ int la_raw_class(const uint8_t* __restrict__ u8, const int32_t* __restrict__ remap, const int32_t* __restrict__ i32,
                                            long row) {
    if (u8 == nullptr) return i32[row];
    const int b = (int)u8[row];
    return remap ? remap[b] : b;
}
// the column of a row, -1 for a row without a class (or with an id the count pass has reported)
__device__ __forceinline__ int la_class(const uint8_t* __restrict__ u8, const int32_t* __restrict__ remap, const int32_t* __restrict__ i32, long row,
                                        int C) {
    const int c = la_raw_class(u8, remap, i32, row);
    return (c >= 0 && c < C) ? c : -1;
}

__global__ __launch_bounds__(256) void la_labels_kernel(const uint8_t* __restrict__ u8, const int32_t* __restrict__ remap,
                                                        const int32_t* __restrict__ i32, int N, int C, unsigned long long* __restrict__ pos,
                                                        int32_t* __restrict__ err) {
    const long r = (long)blockIdx.x * 256 + threadIdx.x;
    if (r >= N) return;
    const int c = la_raw_class(u8, remap, i32, r);
    if (c < -1 || c >= C) { atomicMax(err, SAEV_LATENT_AP_ERR_CLASS); return; }
    if (c >= 0) atomicAdd(pos + c, 1ull);
}

// ---------------------------------------------------------------- sort -------------------------------------------------------------------

// ascending key = descending value: positive events below 0x7fffffff, negative ones above 0x80000000
__device__ __forceinline__ uint32_t la_key(float v) { return ~f2ukey(v); }

__global__ __launch_bounds__(256) void la_init_kernel(const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ indices,
                                                      const float* __restrict__ data, long nnz, int N, int S, uint32_t* __restrict__ key,
                                                      uint32_t* __restrict__ latent, int32_t* __restrict__ row, int32_t* __restrict__ err) {
    const int64_t p0 = row_ptr[0];
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < nnz; e += (long)gridDim.x * 256) {
        const int64_t p = p0 + e;
        const int col = indices[p];
        const float v = data[p];
        const bool ok = col >= 0 && col < S;
        if (!ok) atomicMax(err, SAEV_LATENT_AP_ERR_LATENT);
        const int r = csr_row_of(row_ptr, N, p);
        key[e] = la_key(v);
        latent[e] = (ok && v != 0.f) ? (uint32_t)col : (uint32_t)S;
        row[e] = r;
    }
}

// one wave per part: hist[digit][part] = entries of the part with that digit
__global__ __launch_bounds__(64) void la_hist_kernel(const uint32_t* __restrict__ src, long nnz, long part_len, int shift, int parts,
                                                     int32_t* __restrict__ hist) {
    __shared__ int h[256];
    const int lane = threadIdx.x;
    const long part = blockIdx.x;
    for (int d = lane; d < 256; d += 64) h[d] = 0;
    __syncthreads();
    const long first = part * part_len, last = min(first + part_len, nnz);
    for (long e = first + lane; e < last; e += 64) atomicAdd(&h[(src[e] >> shift) & 255u], 1);
    __syncthreads();
    for (int d = lane; d < 256; d += 64) hist[(size_t)d * parts + part] = h[d];
}

// per digit (one workgroup each): hist[digit][.] -> the exclusive prefix over the parts, total[digit] = the row's sum.  A thread sums
// a contiguous piece, the pieces are scanned, then placed
__global__ __launch_bounds__(LA_SCAN_THREADS) void la_scan_kernel(int32_t* __restrict__ hist, int parts, int32_t* __restrict__ total) {
    __shared__ int sw[LA_SCAN_THREADS / 64];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    int32_t* row = hist + (size_t)blockIdx.x * parts;
    const int per = (parts + LA_SCAN_THREADS - 1) / LA_SCAN_THREADS;
    const int lo = min(t * per, parts), hi = min(lo + per, parts);
    int sum = 0;
    for (int i = lo; i < hi; ++i) sum += row[i];
    const int inc = wave_scan_incl(sum, lane);
    if (lane == 63) sw[w] = inc;
    __syncthreads();
    int run = inc - sum;
    for (int q = 0; q < w; ++q) run += sw[q];
    for (int i = lo; i < hi; ++i) {
        const int v = row[i];
        row[i] = run;
        run += v;
    }
    if (t == LA_SCAN_THREADS - 1) total[blockIdx.x] = run;
}

// one wave per part (see the head of the file); `by_latent` picks the array the digit is taken from
__global__ __launch_bounds__(64) void la_scatter_kernel(const uint32_t* __restrict__ key_in, const uint32_t* __restrict__ lat_in,
                                                        const int32_t* __restrict__ row_in, uint32_t* __restrict__ key_out,
                                                        uint32_t* __restrict__ lat_out, int32_t* __restrict__ row_out, long nnz, long part_len,
                                                        int shift, int by_latent, int parts, const int32_t* __restrict__ hist,
                                                        const int32_t* __restrict__ total) {
    __shared__ int cur[256];
    const int lane = threadIdx.x;
    const long part = blockIdx.x;
    {  // cursor of digit d = the entries of smaller digits (an exclusive scan of total, four digits a lane) + those of d in earlier parts
        int v[4], sum = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) { v[k] = total[lane * 4 + k]; sum += v[k]; }
        int run = wave_scan_incl(sum, lane) - sum;
#pragma unroll
        for (int k = 0; k < 4; ++k) { cur[lane * 4 + k] = run + hist[(size_t)(lane * 4 + k) * parts + part]; run += v[k]; }
    }
    __syncthreads();
    const long first = part * part_len, last = min(first + part_len, nnz);
    const unsigned long long below = (1ull << lane) - 1ull;
    for (long g = first; g < last; g += 64) {
        const long e = g + lane;
        const bool active = e < last;
        uint32_t k = 0, l = 0;
        int r = 0;
        if (active) { k = key_in[e]; l = lat_in[e]; r = row_in[e]; }
        const unsigned digit = ((by_latent ? l : k) >> shift) & 255u;
        unsigned long long peers = __ballot(active);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = ((digit >> b) & 1u) != 0u;
            const unsigned long long m = __ballot(active && bit);
            peers &= bit ? m : ~m;
        }
        const int rank = __popcll(peers & below), same = __popcll(peers);
        const int leader = __ffsll((long long)peers) - 1;
        const int old = active ? cur[digit] : 0;
        __syncthreads();
        if (active && lane == leader) cur[digit] = old + same;
        __syncthreads();
        if (active) {
            const long at = (long)old + rank;
            if (at >= 0 && at < nnz) { key_out[at] = k; lat_out[at] = l; row_out[at] = r; }  // (always: the digits partition the entries)
        }
    }
}

// starts[l] = the first sorted entry whose latent is >= l, for l = 0 .. S (starts[S] = the number of events)
__global__ __launch_bounds__(256) void la_starts_kernel(const uint32_t* __restrict__ latent, long nnz, int S, int64_t* __restrict__ starts) {
    const long l = (long)blockIdx.x * 256 + threadIdx.x;
    if (l > S) return;
    long lo = 0, hi = nnz;  // the first position with latent[pos] >= l
    while (lo < hi) {
        const long mid = lo + ((hi - lo) >> 1);
        if (latent[mid] < (uint32_t)l) lo = mid + 1; else hi = mid;
    }
    starts[l] = lo;
}

// ---------------------------------------------------------------- terms ------------------------------------------------------------------

// H_{t+n} - H_t for t >= LA_H_SMALL, from H_m = ln m + gamma + 1/(2m) - 1/(12m^2) + 1/(120m^4) - 1/(252m^6) + 1/(240m^8) - 1/(132m^10):
// the logarithms as log1p(n / t), the two leading corrections as exact differences, the rest (below 1e-8 of the result) subtracted
__device__ __forceinline__ double la_dh_asym(double t, double n) {
#pragma clang fp contract(off)
    const double m = t + n;
    const double it = 1.0 / t, im = 1.0 / m;
    const double it2 = it * it, im2 = im * im, it4 = it2 * it2, im4 = im2 * im2;
    double corr = -((im4 * im4) * im2 - (it4 * it4) * it2) / 132.0;
    corr = corr + (im4 * im4 - it4 * it4) / 240.0;
    corr = corr - (im4 * im2 - it4 * it2) / 252.0;
    corr = corr + (im4 - it4) / 120.0;
    corr = corr + (n * (t + m)) * (it2 * im2) / 12.0;
    corr = corr - n / ((2.0 * t) * m);
    return log1p(n / t) + corr;
}

// H_{t+n} - H_t, n >= 1: below LA_H_SMALL the terms 1 / p, p = min(t + n, LA_H_SMALL) down to t + 1, added in that order; the rest from
// la_dh_asym(LA_H_SMALL, .), the two added last
__device__ __forceinline__ double la_dh(long t, long n) {
#pragma clang fp contract(off)
    const long hi = t + n;
    if (t >= LA_H_SMALL) return la_dh_asym((double)t, (double)n);
    double direct = 0.0;
    for (long p = min(hi, (long)LA_H_SMALL); p > t; --p) direct = direct + 1.0 / (double)p;
    if (hi <= LA_H_SMALL) return direct;
    return direct + la_dh_asym((double)LA_H_SMALL, (double)(hi - LA_H_SMALL));
}

// term(g, c) of include/saev_amd.h; dh = H_{t+n} - H_t (read when n > LA_DIRECT_MAX only)
__device__ __forceinline__ double la_term(long t, long n, long R, long r, double dh) {
#pragma clang fp contract(off)
    if (r == 0) return 0.0;
    if (n == 1) return (double)(r * (R + 1)) / (double)(t + 1);
    const double rn = (double)r / (double)n;
    const double a = (double)(r - 1) / (double)(n - 1);
    const double R1 = (double)(R + 1);
    if (n <= LA_DIRECT_MAX) {
        double s = 0.0;
        for (long q = 0; q < n; ++q) s = s + (rn * (R1 + (double)q * a)) / (double)(t + 1 + q);
        return s;
    }
    return rn * ((R1 - a * (double)(t + 1)) * dh + a * (double)n);
}

struct LaTerms {
    const int64_t* starts;
    const uint32_t* key;
    const int32_t* row;
    const uint8_t* u8;
    const int32_t* remap;
    const int32_t* i32;
    const unsigned long long* pos;
    double* ap;
    int N, S, C;
};

// a wave per (latent, 64 classes).  grid: (ceil(S / 4), ceil(C / 64))
__global__ __launch_bounds__(256) void la_terms_kernel(LaTerms a) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const long j = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= a.S) return;
    const int c = blockIdx.y * 64 + lane;
    const bool active = c < a.C;
    const int64_t s0 = a.starts[j], s1 = a.starts[j + 1];
    const long Z = (long)a.N - (long)(s1 - s0);
    const long posc = active ? (long)a.pos[c] : 0;

    // with negative events the zero group sits inside the walk: count the pair's events first
    const bool has_neg = s1 > s0 && a.key[s1 - 1] >= 0x80000000u;
    long mine = 0;
    if (has_neg) {
        for (int64_t base = s0; base < s1; base += 64) {
            const int64_t e = base + lane;
            const int cl = e < s1 ? la_class(a.u8, a.remap, a.i32, a.row[e], a.C) : -1;
            const int cnt = (int)min((int64_t)64, s1 - base);
            for (int i = 0; i < cnt; ++i) {
                const int ci = __shfl(cl, i, 64);  // (every lane takes part: lane i may belong to no class of this group)
                mine += (active && ci == c) ? 1 : 0;
            }
        }
    }

    double acc = 0.0;
    long t = 0, n = 0, R = 0, r = 0;
    uint32_t curk = 0;
    bool zero_done = false;
    const auto close_group = [&]() {  // (n > 0)
        const double dh = (n > LA_DIRECT_MAX && __any(r > 0)) ? la_dh(t, n) : 0.0;
        if (r > 0) acc = acc + la_term(t, n, R, r, dh);
        R += r;
        t += n;
        r = 0;
        n = 0;
    };
    const auto zero_group = [&]() {
        zero_done = true;
        if (Z <= 0) return;
        const long rz = min(max(posc - (has_neg ? mine : R), 0L), Z);
        const double dh = (Z > LA_DIRECT_MAX && __any(rz > 0)) ? la_dh(t, Z) : 0.0;
        if (rz > 0) acc = acc + la_term(t, Z, R, rz, dh);
        R += rz;
        t += Z;
    };
    for (int64_t base = s0; base < s1; base += 64) {
        const int64_t e = base + lane;
        uint32_t myk = 0;
        int mycl = -1;
        if (e < s1) { myk = a.key[e]; mycl = la_class(a.u8, a.remap, a.i32, a.row[e], a.C); }
        const int cnt = (int)min((int64_t)64, s1 - base);
        for (int i = 0; i < cnt; ++i) {
            const uint32_t k = __shfl(myk, i, 64);
            const int cl = __shfl(mycl, i, 64);
            if (n > 0 && k != curk) close_group();
            if (!zero_done && k >= 0x80000000u) zero_group();  // (a negative key differs from every positive one: the group is closed)
            curk = k;
            n += 1;
            if (active && cl == c) r += 1;
        }
    }
    if (n > 0) close_group();
    if (!zero_done) zero_group();
    if (active) a.ap[(size_t)j * a.C + c] = posc > 0 ? acc / (double)posc : 0.0;
}

// a wave per latent: the largest ap of the row and the lowest column that has it
__global__ __launch_bounds__(256) void la_best_kernel(const double* __restrict__ ap, int S, int C, double* __restrict__ best_ap,
                                                      int32_t* __restrict__ best_class) {
    const int lane = threadIdx.x & 63;
    const long j = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= S) return;
    double best = -1.0;
    int bi = 0x7fffffff;
    for (int c = lane; c < C; c += 64) {
        const double v = ap[(size_t)j * C + c];
        if (v > best) { best = v; bi = c; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ob = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
    }
    if (lane == 0) {
        if (best_ap) best_ap[j] = best;
        if (best_class) best_class[j] = bi;
    }
}

// the sorted events of a workspace: what la_sort leaves at off_starts, off_key and off_row
struct LaSorted {
    const int64_t* starts;
    const uint32_t* key;
    const int32_t* row;
};

// init, the radix passes and starts, enqueued on s: both entries sort with this
LaSorted la_sort(const saev_latent_ap_layout& L, uint8_t* ws, const int64_t* row_ptr, const int32_t* indices, const float* data, int64_t nnz,
                 int64_t N, int64_t S, hipStream_t s) {
    int32_t* err = reinterpret_cast<int32_t*>(ws + L.off_err);
    int64_t* starts = reinterpret_cast<int64_t*>(ws + L.off_starts);
    int32_t* hist = reinterpret_cast<int32_t*>(ws + L.off_hist);
    int32_t* total = hist + 256 * L.parts;
    // the sort ends in (key, latent, row); it starts there when the number of passes is even
    uint32_t* key[2] = {reinterpret_cast<uint32_t*>(ws + L.off_key), reinterpret_cast<uint32_t*>(ws + L.off_key2)};
    uint32_t* lat[2] = {reinterpret_cast<uint32_t*>(ws + L.off_latent), reinterpret_cast<uint32_t*>(ws + L.off_latent2)};
    int32_t* row[2] = {reinterpret_cast<int32_t*>(ws + L.off_row), reinterpret_cast<int32_t*>(ws + L.off_row2)};
    int at = (int)(L.passes & 1);
    if (nnz > 0) {
        const int parts = (int)((nnz + L.part_len - 1) / L.part_len);
        const int grid = (int)std::min<int64_t>((nnz + 255) / 256, 8192);
        hipLaunchKernelGGL(la_init_kernel, dim3(grid), dim3(256), 0, s, row_ptr, indices, data, (long)nnz, (int)N, (int)S, key[at], lat[at], row[at],
                           err);
        for (int p = 0; p < (int)L.passes; ++p) {
            const int by_latent = p >= 4 ? 1 : 0, shift = 8 * (by_latent ? p - 4 : p);
            hipLaunchKernelGGL(la_hist_kernel, dim3(parts), dim3(64), 0, s, by_latent ? lat[at] : key[at], (long)nnz, (long)L.part_len, shift, parts,
                               hist);
            hipLaunchKernelGGL(la_scan_kernel, dim3(256), dim3(LA_SCAN_THREADS), 0, s, hist, parts, total);
            hipLaunchKernelGGL(la_scatter_kernel, dim3(parts), dim3(64), 0, s, key[at], lat[at], row[at], key[at ^ 1], lat[at ^ 1], row[at ^ 1],
                               (long)nnz, (long)L.part_len, shift, by_latent, parts, hist, total);
            at ^= 1;
        }
    }
    hipLaunchKernelGGL(la_starts_kernel, dim3((unsigned)((S + 1 + 255) / 256)), dim3(256), 0, s, lat[0], (long)nnz, (int)S, starts);
    return LaSorted{starts, key[0], row[0]};
}

// ---------------------------------------------------------------- probe ------------------------------------------------------------------

// s(a) = fl(fl(w a) + b) in the score's arithmetic, each operation rounded on its own (a fused multiply-add changes which scores tie)
__device__ __forceinline__ float pa_score(float w, float a, float b) { return __fadd_rn(__fmul_rn(w, a), b); }
__device__ __forceinline__ double pa_score(double w, float a, double b) { return __dadd_rn(__dmul_rn(w, (double)a), b); }

__global__ __launch_bounds__(256) void pa_values_kernel(const int64_t* __restrict__ row_ptr, const float* __restrict__ data, long nnz,
                                                        int32_t* __restrict__ err) {
    const int64_t p0 = row_ptr[0];
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < nnz; e += (long)gridDim.x * 256)
        if (!isfinite(data[p0 + e])) atomicMax(err, SAEV_PROBE_AP_ERR_VALUE);
}

struct PaTerms {
    LaTerms la;
    const void* w;
    const void* b;
    long long* tp;
    long long* pred_pos;
};

// a wave per (latent, 64 classes), lane = class = pair.  grid: (ceil(S / 4), ceil(C / 64))
template <typename T>
__global__ __launch_bounds__(256) void pa_terms_kernel(PaTerms p) {
#pragma clang fp contract(off)
    const LaTerms& a = p.la;
    const int lane = threadIdx.x & 63;
    const long j = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= a.S) return;
    const int c = blockIdx.y * 64 + lane;
    const bool active = c < a.C;
    const int64_t s0 = a.starts[j], s1 = a.starts[j + 1];
    const long Z = (long)a.N - (long)(s1 - s0);
    const long posc = active ? (long)a.pos[c] : 0;
    T w = (T)0, b = (T)0;
    if (active) {
        w = static_cast<const T*>(p.w)[(size_t)j * a.C + c];
        b = static_cast<const T*>(p.b)[(size_t)j * a.C + c];
    }
    const bool live = active && isfinite(w) && isfinite(b);  // (a void pair walks nothing)
    const bool fwd = live && w >= (T)0, bwd = live && w < (T)0;
    const bool any_fwd = __any(fwd), any_bwd = __any(bwd);

    // the zero block's r is pos_c minus the pair's events; it is needed before the walk unless the block comes last in it: in the
    // descending walk of a latent with negative events, and in every ascending walk.  The lanes that walk ascending count while the
    // others walk descending; a pass of its own is made only where that is too late or does not happen
    const bool has_neg = s1 > s0 && a.key[s1 - 1] >= 0x80000000u;
    const bool count_first = has_neg || (any_bwd && !any_fwd);
    const bool counted = bwd || count_first;
    long mine = 0;
    if (count_first) {
        for (int64_t base = s0; base < s1; base += 64) {
            const int64_t e = base + lane;
            const int cl = e < s1 ? la_class(a.u8, a.remap, a.i32, a.row[e], a.C) : -1;
            const int cnt = (int)min((int64_t)64, s1 - base);
            for (int i = 0; i < cnt; ++i) {
                const int ci = __shfl(cl, i, 64);
                mine += (active && ci == c) ? 1 : 0;
            }
        }
    }

    // everything below the shuffles is per lane: a lane closes its groups where ITS score changes
    double acc = 0.0;
    long t = 0, n = 0, R = 0, r = 0, hit = 0, pred = 0;
    T curs = (T)0;
    bool zero_done = false;
    const auto close_group = [&]() {  // (n > 0)
        if (r > 0) acc = acc + la_term(t, n, R, r, n > LA_DIRECT_MAX ? la_dh(t, n) : 0.0);
        R += r;
        t += n;
        r = 0;
        n = 0;
    };
    const auto feed = [&](T s, long rows, long of_class) {
        if (n > 0 && s != curs) close_group();
        curs = s;
        n += rows;
        r += of_class;
        if (s > (T)0) { pred += rows; hit += of_class; }
    };
    const auto zero_block = [&]() {  // the Z rows without an event, at a = 0; it joins the open group when the scores are equal
        zero_done = true;
        if (Z <= 0) return;
        feed(pa_score(w, 0.f, b), Z, min(max(posc - (counted ? mine : R + r), 0L), Z));
    };

    if (any_fwd) {  // by descending value: the positive events, the zero block, the negative events
        for (int64_t base = s0; base < s1; base += 64) {
            const int64_t e = base + lane;
            float myv = 0.f;
            int mycl = -1;
            if (e < s1) { myv = ukey2f(~a.key[e]); mycl = la_class(a.u8, a.remap, a.i32, a.row[e], a.C); }
            const int cnt = (int)min((int64_t)64, s1 - base);
            for (int i = 0; i < cnt; ++i) {
                const float v = __shfl(myv, i, 64);
                const int cl = __shfl(mycl, i, 64);
                if (fwd) {
                    if (!zero_done && !(v > 0.f)) zero_block();
                    feed(pa_score(w, v, b), 1, cl == c ? 1 : 0);
                } else if (bwd && !count_first) {
                    mine += cl == c ? 1 : 0;
                }
            }
        }
        if (fwd && !zero_done) zero_block();
    }
    if (any_bwd) {  // by ascending value: the same events from the far end, in chunks [top - 64, top) that end at s0
        for (int64_t top = s1; top > s0; top -= 64) {
            const int64_t base = max(s0, top - 64);
            const int cnt = (int)(top - base);
            float myv = 0.f;
            int mycl = -1;
            if (lane < cnt) { myv = ukey2f(~a.key[base + lane]); mycl = la_class(a.u8, a.remap, a.i32, a.row[base + lane], a.C); }
            for (int i = cnt - 1; i >= 0; --i) {
                const float v = __shfl(myv, i, 64);
                const int cl = __shfl(mycl, i, 64);
                if (bwd) {
                    if (!zero_done && !(v < 0.f)) zero_block();
                    feed(pa_score(w, v, b), 1, cl == c ? 1 : 0);
                }
            }
        }
        if (bwd && !zero_done) zero_block();
    }
    if (n > 0) close_group();
    if (active) {
        const size_t at = (size_t)j * a.C + c;
        a.ap[at] = !live ? __longlong_as_double(0x7ff8000000000000LL) : posc > 0 ? acc / (double)posc : 0.0;
        p.tp[at] = hit;
        p.pred_pos[at] = pred;
    }
}

// top_row[j][i] = the row of latent j's i-th event, 0 behind its last
__global__ __launch_bounds__(256) void pa_top_rows_kernel(const int64_t* __restrict__ starts, const int32_t* __restrict__ row, long S, int top_k,
                                                          long long* __restrict__ top_row) {
    const long total = S * (long)top_k;
    for (long at = (long)blockIdx.x * 256 + threadIdx.x; at < total; at += (long)gridDim.x * 256) {
        const long j = at / top_k;
        const int i = (int)(at - j * top_k);
        const int64_t e = starts[j] + i;
        top_row[at] = e < starts[j + 1] ? (long long)row[e] : 0ll;
    }
}

// ---------------------------------------------------------------- auroc ------------------------------------------------------------------

// LATENT AUROC (include/saev_amd.h: LATENT AUROC) shares the sort as well and walks lane = task:
//   roles    the T x C role matrix turned class-major: row c + 1 of the table holds class c's role in every task (row 0, zeros, is
//            class -1), Tp = 64 ceil(T / 64) bytes a row, so that the 64 lanes of a wave read 64 consecutive bytes per event.
//   counts   n_pos / n_neg of a task = the class counts la_open enqueues, summed over the classes of role 2 / 1.
//   walk     a wave per (latent, 64 tasks).  The key and the row's class are the same in every lane; a lane keeps its task's p, q of
//            the open group, P, the event counters, U2 and the two fp64 sums in registers.  A group closes when the key changes
//            (for every lane at once).  The rows without an event enter in closed form behind the walk.  The role bytes of eight
//            events are fetched before the eight are worked through, from a copy of the task group's (C + 1) x 64 slice in LDS
//            when that is at most AU_LDS_MAX_BYTES, from the table (L2) otherwise.
#ifndef AU_LDS_MAX_BYTES
#define AU_LDS_MAX_BYTES 16384
#endif
constexpr int AU_MAX_T = 4096;
constexpr int AU_BATCH = 8;

static inline int64_t au_tp(int64_t T) { return (T + 63) / 64 * 64; }

// grid: (Tp / 64, C + 1), 64 threads
__global__ __launch_bounds__(64) void au_roles_kernel(const uint8_t* __restrict__ role, int C, int T, int Tp, uint8_t* __restrict__ table,
                                                      int32_t* __restrict__ err) {
    const int t = blockIdx.x * 64 + threadIdx.x, r = blockIdx.y;  // (t < Tp, r <= C)
    uint8_t v = 0;
    if (r > 0 && t < T) {
        v = role[(size_t)t * C + (r - 1)];
        if (v > 2) { atomicMax(err, SAEV_LATENT_AUROC_ERR_ROLE); v = 0; }
    }
    table[(size_t)r * Tp + t] = v;
}

// a thread per task.  grid: ceil(T / 256)
__global__ __launch_bounds__(256) void au_counts_kernel(const uint8_t* __restrict__ table, const unsigned long long* __restrict__ pos, int C, int T,
                                                        int Tp, long long* __restrict__ n_pos, long long* __restrict__ n_neg) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    long long np = 0, nn = 0;
    for (int c = 0; c < C; ++c) {
        const int r = table[(size_t)(c + 1) * Tp + t];
        const long long n = (long long)pos[c];
        np += r == 2 ? n : 0;
        nn += r == 1 ? n : 0;
    }
    n_pos[t] = np;
    n_neg[t] = nn;
}

struct AuWalk {
    const int64_t* starts;
    const uint32_t* key;
    const int32_t* row;
    const uint8_t* u8;
    const int32_t* remap;
    const int32_t* i32;
    const uint8_t* table;
    const long long* n_pos;
    const long long* n_neg;
    double* auroc;
    long long* u2;
    long long* fire_pos;
    long long* fire_neg;
    double* sum_pos;
    double* sum_neg;
    int N, S, C, T, Tp;
};

// a wave per (latent, 64 tasks), lane = task.  grid: (ceil(S / 4), Tp / 64); LDS: (C + 1) x 64 bytes of dynamic LDS
template <bool LDS>
__global__ __launch_bounds__(256) void au_walk_kernel(AuWalk a) {
#pragma clang fp contract(off)
    extern __shared__ uint8_t au_slice[];
    const int lane = threadIdx.x & 63;
    const long j = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int t = blockIdx.y * 64 + lane;  // (< Tp)
    if (LDS) {  // the four waves share the task group: its slice of the table, a 64-byte row as 16 words
        const int words = (a.C + 1) * 16;
        for (int w = threadIdx.x; w < words; w += 256)
            reinterpret_cast<uint32_t*>(au_slice)[w] =
                *reinterpret_cast<const uint32_t*>(a.table + (size_t)(w >> 4) * a.Tp + (size_t)blockIdx.y * 64 + (size_t)(w & 15) * 4);
        __syncthreads();
    }
    if (j >= a.S) return;
    const bool active = t < a.T;
    const uint8_t* mine = LDS ? au_slice + lane : a.table + t;  // + (class + 1) * stride: this lane's role of a class
    const size_t stride = LDS ? 64 : (size_t)a.Tp;
    const int64_t s0 = a.starts[j], s1 = a.starts[j + 1];

    long long p = 0, q = 0, P = 0, Qev = 0, Ppos = 0, Qneg = 0, U2 = 0;
    double sp = 0.0, sn = 0.0;
    uint32_t curk = 0;
    bool open = false;
    for (int64_t base = s0; base < s1; base += 64) {
        const int64_t e = base + lane;
        uint32_t myk = 0;
        int mycl = -1;
        if (e < s1) { myk = a.key[e]; mycl = la_class(a.u8, a.remap, a.i32, a.row[e], a.C); }
        const int cnt = (int)min((int64_t)64, s1 - base);
        for (int i0 = 0; i0 < cnt; i0 += AU_BATCH) {
            uint32_t ks[AU_BATCH];
            int rs[AU_BATCH];
#pragma unroll
            for (int u = 0; u < AU_BATCH; ++u) {  // (behind cnt: class -1, the table's row of zeros)
                ks[u] = __shfl(myk, i0 + u, 64);
                rs[u] = mine[(size_t)(__shfl(mycl, i0 + u, 64) + 1) * stride];
            }
#pragma unroll
            for (int u = 0; u < AU_BATCH; ++u) {
                if (i0 + u < cnt) {
                    const uint32_t k = ks[u];
                    if (open && k != curk) {  // the group is closed, for every lane
                        U2 += q * (2 * P + p);
                        P += p;
                        p = 0;
                        q = 0;
                    }
                    curk = k;
                    open = true;
                    const float v = ukey2f(~k);
                    const double dv = (double)v;
                    const long long isp = rs[u] == 2 ? 1 : 0, isn = rs[u] == 1 ? 1 : 0;
                    p += isp;
                    q += isn;
                    Qev += isn;
                    if (v > 0.f) Ppos += isp; else Qneg += isn;
                    if (isp) sp = sp + dv;
                    if (isn) sn = sn + dv;
                }
            }
        }
    }
    if (open) {
        U2 += q * (2 * P + p);
        P += p;
    }
    if (!active) return;
    const long long np = a.n_pos[t], nn = a.n_neg[t];
    const long long p0 = np - P, q0 = nn - Qev;  // the rows without an event: one group between the positive and the negative values
    U2 += 2 * q0 * Ppos + p0 * q0 + 2 * p0 * Qneg;
    const size_t at = (size_t)j * a.T + t;
    a.u2[at] = U2;
    a.auroc[at] = (np > 0 && nn > 0) ? (double)U2 / ((2.0 * (double)np) * (double)nn) : __longlong_as_double(0x7ff8000000000000LL);
    a.fire_pos[at] = Ppos;
    a.fire_neg[at] = Qev - Qneg;
    a.sum_pos[at] = sp;
    a.sum_neg[at] = sn;
}

// ---------------------------------------------------------------- operating points -------------------------------------------------------

// LATENT OPERATING POINTS (include/saev_amd.h: LATENT OPERATING POINTS): per (latent, task) the threshold at which
// "a >= theta => positive" has the best F1 and the one with the best Youden J, with the confusion counts there, decided on integers.
//   walk     a wave per (latent, 64 tasks), lane = task, over the events la_sort left, with au_walk_kernel's role table, its LDS / L2
//            choice and its batches of eight role bytes.  A lane keeps the running TP, FP and J2 = TP n_neg - FP n_pos (an addition per
//            event, no product) and its two best candidates in registers.  A tie group closes where the key changes, for every lane at
//            once, and every close is a candidate; a later (lower) candidate replaces the best only when it is STRICTLY better, which
//            is the tie rule, and a group that changed neither count of a lane compares equal and so never wins there.  The F1
//            comparison is two 32 x 32 -> 64 products (TP and TP + FP + n_pos stay below 2^32).
//   zero     the rows without an event are one candidate at theta = 0 between the last positive and the first negative event: its
//            counts are n_pos / n_neg minus ALL of the lane's events of that role.  A latent without negative events meets the block
//            behind its last event, where the running counts are those totals; one with negative events (the last sorted key says
//            so) is walked once before to count them, as la_terms_kernel does.
struct OpWalk {
    const int64_t* starts;
    const uint32_t* key;
    const int32_t* row;
    const uint8_t* u8;
    const int32_t* remap;
    const int32_t* i32;
    const uint8_t* table;
    const long long* n_pos;
    const long long* n_neg;
    double* f1;
    float* f1_thr;
    long long* f1_tp;
    long long* f1_fp;
    long long* j2;
    double* youden;
    float* j_thr;
    long long* j_tp;
    long long* j_fp;
    int N, S, C, T, Tp;
};

// a wave per (latent, 64 tasks), lane = task.  grid: (ceil(S / 4), Tp / 64); LDS: (C + 1) x 64 bytes of dynamic LDS
template <bool LDS>
__global__ __launch_bounds__(256) void op_walk_kernel(OpWalk a) {
#pragma clang fp contract(off)
    extern __shared__ uint8_t op_slice[];
    const int lane = threadIdx.x & 63;
    const long j = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int t = blockIdx.y * 64 + lane;  // (< Tp)
    if (LDS) {  // the four waves share the task group: its slice of the table, a 64-byte row as 16 words
        const int words = (a.C + 1) * 16;
        for (int w = threadIdx.x; w < words; w += 256)
            reinterpret_cast<uint32_t*>(op_slice)[w] =
                *reinterpret_cast<const uint32_t*>(a.table + (size_t)(w >> 4) * a.Tp + (size_t)blockIdx.y * 64 + (size_t)(w & 15) * 4);
        __syncthreads();
    }
    if (j >= a.S) return;
    const bool active = t < a.T;
    const uint8_t* mine = LDS ? op_slice + lane : a.table + t;  // + (class + 1) * stride: this lane's role of a class
    const size_t stride = LDS ? 64 : (size_t)a.Tp;
    const int64_t s0 = a.starts[j], s1 = a.starts[j + 1];
    const uint32_t np = active ? (uint32_t)a.n_pos[t] : 0u, nn = active ? (uint32_t)a.n_neg[t] : 0u;  // (both below 2^31)

    // with negative events the zero block sits inside the walk: count the lane's events of either role first
    const bool has_neg = s1 > s0 && a.key[s1 - 1] >= 0x80000000u;
    uint32_t Pev = 0, Qev = 0;
    if (has_neg) {
        for (int64_t base = s0; base < s1; base += 64) {
            const int64_t e = base + lane;
            const int mycl = e < s1 ? la_class(a.u8, a.remap, a.i32, a.row[e], a.C) : -1;  // (behind s1: class -1, the table's row of zeros)
            const int cnt = (int)min((int64_t)64, s1 - base);
            for (int i0 = 0; i0 < cnt; i0 += AU_BATCH) {
                int rs[AU_BATCH];
#pragma unroll
                for (int u = 0; u < AU_BATCH; ++u) rs[u] = mine[(size_t)(__shfl(mycl, i0 + u, 64) + 1) * stride];
#pragma unroll
                for (int u = 0; u < AU_BATCH; ++u) {
                    Pev += rs[u] == 2 ? 1u : 0u;
                    Qev += rs[u] == 1 ? 1u : 0u;
                }
            }
        }
    }

    const float inf = __uint_as_float(0x7f800000u);
    uint32_t TP = 0, FP = 0;
    long long J2 = 0;
    uint32_t fTP = 0, fD = np, fFP = 0;  // the best F1 so far: "predict nothing"
    float fthr = inf;
    long long bJ2 = 0;                   // the best J so far: "predict nothing"
    uint32_t jTP = 0, jFP = 0;
    float jthr = inf;
    uint32_t curk = 0;
    bool open = false, zero_done = false;
    const auto candidate = [&](float theta) {  // the rule "a >= theta" with the running counts; equality keeps the earlier, higher one
        const uint32_t D = TP + FP + np;
        if ((unsigned long long)TP * fD > (unsigned long long)fTP * D) { fTP = TP; fD = D; fFP = FP; fthr = theta; }
        if (J2 > bJ2) { bJ2 = J2; jTP = TP; jFP = FP; jthr = theta; }
    };
    const auto zero_block = [&]() {  // (no group is open)
        zero_done = true;
        const uint32_t p0 = np - (has_neg ? Pev : TP), q0 = nn - (has_neg ? Qev : FP);
        TP += p0;
        FP += q0;
        J2 += (long long)p0 * (long long)nn - (long long)q0 * (long long)np;
        candidate(0.f);
    };
    for (int64_t base = s0; base < s1; base += 64) {
        const int64_t e = base + lane;
        uint32_t myk = 0;
        int mycl = -1;
        if (e < s1) { myk = a.key[e]; mycl = la_class(a.u8, a.remap, a.i32, a.row[e], a.C); }
        const int cnt = (int)min((int64_t)64, s1 - base);
        for (int i0 = 0; i0 < cnt; i0 += AU_BATCH) {
            uint32_t ks[AU_BATCH];
            int rs[AU_BATCH];
#pragma unroll
            for (int u = 0; u < AU_BATCH; ++u) {  // (behind cnt: class -1, the table's row of zeros)
                ks[u] = __shfl(myk, i0 + u, 64);
                rs[u] = mine[(size_t)(__shfl(mycl, i0 + u, 64) + 1) * stride];
            }
#pragma unroll
            for (int u = 0; u < AU_BATCH; ++u) {
                if (i0 + u < cnt) {
                    const uint32_t k = ks[u];
                    if (open && k != curk) {  // the group is closed, for every lane
                        candidate(ukey2f(~curk));
                        open = false;
                    }
                    if (!zero_done && k >= 0x80000000u) zero_block();  // (a negative key differs from every positive one: no group is open)
                    curk = k;
                    open = true;
                    const bool isp = rs[u] == 2, isn = rs[u] == 1;
                    TP += isp ? 1u : 0u;
                    FP += isn ? 1u : 0u;
                    J2 += isp ? (long long)nn : 0ll;
                    J2 -= isn ? (long long)np : 0ll;
                }
            }
        }
    }
    if (open) candidate(ukey2f(~curk));
    if (!zero_done) zero_block();
    if (!active) return;
    const long long nan = 0x7ff8000000000000LL;
    const size_t at = (size_t)j * a.T + t;
    a.f1[at] = np > 0 ? (2.0 * (double)fTP) / (double)fD : __longlong_as_double(nan);
    a.f1_thr[at] = fthr;
    a.f1_tp[at] = (long long)fTP;
    a.f1_fp[at] = (long long)fFP;
    a.j2[at] = bJ2;
    a.youden[at] = (np > 0 && nn > 0) ? (double)bJ2 / ((double)np * (double)nn) : __longlong_as_double(nan);
    a.j_thr[at] = jthr;
    a.j_tp[at] = (long long)jTP;
    a.j_fp[at] = (long long)jFP;
}

// ---------------------------------------------------------------- host -------------------------------------------------------------------

// what la_open leaves for the rest of an entry
struct LaOpen {
    saev_latent_ap_layout L;
    uint8_t* ws;
    int32_t* err;
    unsigned long long* pos;
    hipStream_t s;
};

// the front half of both entries: the refusals they share, the layout, err and pos cleared and the class counts enqueued (la_sort
// is the back half).  `own` is the refusal of the entry's own arguments (NULL: none); it is raised where each entry has always made
// those checks, behind the label forms and before the workspace.  la_check is the refusals and the layout alone: what an entry that
// takes a sorted workspace over keeps of it
int la_check(const char* who, const int64_t* row_ptr, const int32_t* indices, const float* data, int64_t nnz, int64_t N, int64_t S, int64_t C,
             const uint8_t* class_u8, const int32_t* remap, const int32_t* class_i32, int64_t* pos, const char* own, void* workspace,
             int64_t workspace_bytes, void* stream, LaOpen* o) {
    if (const int rc = entry_check_shape(who, N, S, C, nnz)) return rc;
    if (!row_ptr) return entry_refuse(SAEV_INVALID_ARG, who, "row_ptr is NULL");
    if (nnz > 0 && (!indices || !data)) return entry_refuse(SAEV_INVALID_ARG, who, "indices and data come with nnz > 0");
    if ((class_u8 != nullptr) == (class_i32 != nullptr))
        return entry_refuse(SAEV_INVALID_ARG, who, "give the classes as class_u8 (with an optional remap) or as class_i32, one of the two");
    if (remap && !class_u8) return entry_refuse(SAEV_INVALID_ARG, who, "remap goes with class_u8");
    if (own) return entry_refuse(SAEV_INVALID_ARG, who, own);
    la_layout(S, C, nnz, &o->L);
    if (const int rc = entry_check_workspace(who, workspace, workspace_bytes, o->L.total_bytes, "workspace smaller than saev_latent_ap_workspace_bytes(N, S, C, nnz)"))
        return rc;
    o->s = (hipStream_t)stream;
    o->ws = static_cast<uint8_t*>(workspace);
    o->err = reinterpret_cast<int32_t*>(o->ws + o->L.off_err);
    o->pos = reinterpret_cast<unsigned long long*>(pos);
    return SAEV_OK;
}

int la_open(const char* who, const int64_t* row_ptr, const int32_t* indices, const float* data, int64_t nnz, int64_t N, int64_t S, int64_t C,
            const uint8_t* class_u8, const int32_t* remap, const int32_t* class_i32, int64_t* pos, const char* own, void* workspace,
            int64_t workspace_bytes, void* stream, LaOpen* o) {
    if (const int rc = la_check(who, row_ptr, indices, data, nnz, N, S, C, class_u8, remap, class_i32, pos, own, workspace, workspace_bytes, stream, o)) return rc;
    bool ok = hipMemsetAsync(o->err, 0, 64, o->s) == hipSuccess;
    ok = ok && hipMemsetAsync(pos, 0, (size_t)(8 * C), o->s) == hipSuccess;
    if (!ok) return entry_refuse(SAEV_HIP_ERROR, who, "hipMemsetAsync failed");
    hipLaunchKernelGGL(la_labels_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, o->s, class_u8, remap, class_i32, (int)N, (int)C, o->pos, o->err);
    return SAEV_OK;
}

}  // namespace

int64_t saev_latent_ap_workspace_bytes(int64_t N, int64_t S, int64_t C, int64_t nnz) {
    if (!entry_shape_ok(N, S, C, nnz)) return -1;
    saev_latent_ap_layout L;
    la_layout(S, C, nnz, &L);
    return L.total_bytes;
}

int saev_latent_ap_layout_of(int64_t N, int64_t S, int64_t C, int64_t nnz, saev_latent_ap_layout* out) {
    if (!out) return entry_refuse(SAEV_INVALID_ARG, "saev_latent_ap_layout_of", "no saev_latent_ap_layout");
    if (!entry_shape_ok(N, S, C, nnz)) return entry_refuse(SAEV_UNSUPPORTED, "saev_latent_ap_layout_of", "1 <= N, S < 2^31, 1 <= C <= 4096, 0 <= nnz < 2^31");
    la_layout(S, C, nnz, out);
    return SAEV_OK;
}

int saev_latent_ap(const int64_t* row_ptr, const int32_t* indices, const float* data, int64_t nnz, int64_t N, int64_t S, int64_t C,
                   const uint8_t* class_u8, const int32_t* remap, const int32_t* class_i32, double* ap, int64_t* pos, double* best_ap,
                   int32_t* best_class, void* workspace, int64_t workspace_bytes, void* stream) {
    const char* who = "saev_latent_ap";
    const char* own = (!ap || !pos) ? "ap and pos must not be NULL" : nullptr;
    LaOpen o;
    if (const int rc = la_open(who, row_ptr, indices, data, nnz, N, S, C, class_u8, remap, class_i32, pos, own, workspace, workspace_bytes, stream, &o))
        return rc;
    hipStream_t s = o.s;
    const LaSorted e = la_sort(o.L, o.ws, row_ptr, indices, data, nnz, N, S, s);
    LaTerms a{e.starts, e.key, e.row, class_u8, remap, class_i32, o.pos, ap, (int)N, (int)S, (int)C};
    hipLaunchKernelGGL(la_terms_kernel, dim3((unsigned)((S + 3) / 4), (unsigned)((C + 63) / 64)), dim3(256), 0, s, a);
    if (best_ap || best_class)
        hipLaunchKernelGGL(la_best_kernel, dim3((unsigned)((S + 3) / 4)), dim3(256), 0, s, ap, (int)S, (int)C, best_ap, best_class);
    if (hipGetLastError() != hipSuccess) return entry_refuse(SAEV_HIP_ERROR, who, "kernel launch failed");
    return SAEV_OK;
}

int saev_probe_ap(const int64_t* row_ptr, const int32_t* indices, const float* data, int64_t nnz, int64_t N, int64_t S, int64_t C,
                  const uint8_t* class_u8, const int32_t* remap, const int32_t* class_i32, const void* w, const void* b, int32_t score_dtype,
                  double* ap, int64_t* pos, int64_t* tp, int64_t* pred_pos, int32_t top_k, int64_t* top_row, void* workspace,
                  int64_t workspace_bytes, void* stream) {
    const char* who = "saev_probe_ap";
    const char* own = (!w || !b) ? "w and b must not be NULL"
        : (score_dtype != 0 && score_dtype != 1) ? "score_dtype is 0 (fp32) or 1 (fp64)"
        : (!ap || !pos || !tp || !pred_pos) ? "ap, pos, tp and pred_pos must not be NULL"
        : (top_k < 0 || (int64_t)top_k > N) ? "top_k must lie in [0, N]"
        : (top_k > 0 && !top_row) ? "top_row comes with top_k > 0"
        : nullptr;
    LaOpen o;
    if (const int rc = la_open(who, row_ptr, indices, data, nnz, N, S, C, class_u8, remap, class_i32, pos, own, workspace, workspace_bytes, stream, &o))
        return rc;
    hipStream_t s = o.s;
    if (nnz > 0)
        hipLaunchKernelGGL(pa_values_kernel, dim3((unsigned)std::min<int64_t>((nnz + 255) / 256, 8192)), dim3(256), 0, s, row_ptr, data, (long)nnz, o.err);
    const LaSorted e = la_sort(o.L, o.ws, row_ptr, indices, data, nnz, N, S, s);
    PaTerms a{{e.starts, e.key, e.row, class_u8, remap, class_i32, o.pos, ap, (int)N, (int)S, (int)C}, w, b, reinterpret_cast<long long*>(tp),
              reinterpret_cast<long long*>(pred_pos)};
    const dim3 grid((unsigned)((S + 3) / 4), (unsigned)((C + 63) / 64));
    if (score_dtype == 0) hipLaunchKernelGGL(pa_terms_kernel<float>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(pa_terms_kernel<double>, grid, dim3(256), 0, s, a);
    if (top_k > 0)
        hipLaunchKernelGGL(pa_top_rows_kernel, dim3((unsigned)std::min<int64_t>((S * (int64_t)top_k + 255) / 256, 8192)), dim3(256), 0, s, e.starts,
                           e.row, (long)S, (int)top_k, reinterpret_cast<long long*>(top_row));
    if (hipGetLastError() != hipSuccess) return entry_refuse(SAEV_HIP_ERROR, who, "kernel launch failed");
    return SAEV_OK;
}

int64_t saev_latent_auroc_workspace_bytes(int64_t N, int64_t S, int64_t C, int64_t T, int64_t nnz) {
    if (!entry_shape_ok(N, S, C, nnz) || T < 1 || T > AU_MAX_T) return -1;
    saev_latent_ap_layout L;
    la_layout(S, C, nnz, &L);
    return L.total_bytes + round256((C + 1) * au_tp(T));
}

int saev_latent_auroc(const int64_t* row_ptr, const int32_t* indices, const float* data, int64_t nnz, int64_t N, int64_t S, int64_t C,
                      const uint8_t* class_u8, const int32_t* remap, const int32_t* class_i32, const uint8_t* role, int64_t T, double* auroc,
                      int64_t* u2, int64_t* n_pos, int64_t* n_neg, int64_t* fire_pos, int64_t* fire_neg, double* sum_pos, double* sum_neg,
                      int64_t* pos, void* workspace, int64_t workspace_bytes, void* stream) {
    const char* who = "saev_latent_auroc";
    if (const int rc = entry_check_shape(who, N, S, C, nnz)) return rc;
    if (T < 1 || T > AU_MAX_T) return entry_refuse(SAEV_UNSUPPORTED, who, "the number of tasks must lie in [1, 4096]");
    // this entry's workspace is longer than la_open's: its size is checked where la_open checks its own, behind the entry's arguments
    const int64_t need = saev_latent_auroc_workspace_bytes(N, S, C, T, nnz);
    const char* own = !role ? "role must not be NULL"
        : (!auroc || !u2 || !n_pos || !n_neg || !fire_pos || !fire_neg || !sum_pos || !sum_neg || !pos)
            ? "auroc, u2, n_pos, n_neg, fire_pos, fire_neg, sum_pos, sum_neg and pos must not be NULL"
        : (!workspace || workspace_bytes < need) ? "workspace smaller than saev_latent_auroc_workspace_bytes(N, S, C, T, nnz)"
        : nullptr;
    LaOpen o;
    if (const int rc = la_open(who, row_ptr, indices, data, nnz, N, S, C, class_u8, remap, class_i32, pos, own, workspace, workspace_bytes, stream, &o))
        return rc;
    hipStream_t s = o.s;
    const int Tp = (int)au_tp(T);
    uint8_t* table = o.ws + o.L.total_bytes;
    long long* np = reinterpret_cast<long long*>(n_pos);
    long long* nn = reinterpret_cast<long long*>(n_neg);
    hipLaunchKernelGGL(au_roles_kernel, dim3((unsigned)(Tp / 64), (unsigned)(C + 1)), dim3(64), 0, s, role, (int)C, (int)T, Tp, table, o.err);
    hipLaunchKernelGGL(au_counts_kernel, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, s, table, o.pos, (int)C, (int)T, Tp, np, nn);
    const LaSorted e = la_sort(o.L, o.ws, row_ptr, indices, data, nnz, N, S, s);
    AuWalk a{e.starts, e.key, e.row, class_u8, remap, class_i32, table, np, nn, auroc, reinterpret_cast<long long*>(u2),
             reinterpret_cast<long long*>(fire_pos), reinterpret_cast<long long*>(fire_neg), sum_pos, sum_neg, (int)N, (int)S, (int)C, (int)T, Tp};
    const dim3 grid((unsigned)((S + 3) / 4), (unsigned)(Tp / 64));
    const size_t slice = (size_t)(C + 1) * 64;
    if (slice <= (size_t)AU_LDS_MAX_BYTES) hipLaunchKernelGGL(au_walk_kernel<true>, grid, dim3(256), slice, s, a);
    else hipLaunchKernelGGL(au_walk_kernel<false>, grid, dim3(256), 0, s, a);
    if (hipGetLastError() != hipSuccess) return entry_refuse(SAEV_HIP_ERROR, who, "kernel launch failed");
    return SAEV_OK;
}

int64_t saev_latent_operating_workspace_bytes(int64_t N, int64_t S, int64_t C, int64_t T, int64_t nnz) {
    return saev_latent_auroc_workspace_bytes(N, S, C, T, nnz);
}

int saev_latent_operating(const int64_t* row_ptr, const int32_t* indices, const float* data, int64_t nnz, int64_t N, int64_t S, int64_t C,
                          const uint8_t* class_u8, const int32_t* remap, const int32_t* class_i32, const uint8_t* role, int64_t T, int32_t flags,
                          double* f1, float* f1_thr, int64_t* f1_tp, int64_t* f1_fp, int64_t* j2, double* youden, float* j_thr, int64_t* j_tp,
                          int64_t* j_fp, int64_t* n_pos, int64_t* n_neg, int64_t* pos, void* workspace, int64_t workspace_bytes, void* stream) {
    const char* who = "saev_latent_operating";
    if (const int rc = entry_check_shape(who, N, S, C, nnz)) return rc;
    if (T < 1 || T > AU_MAX_T) return entry_refuse(SAEV_UNSUPPORTED, who, "the number of tasks must lie in [1, 4096]");
    const int64_t need = saev_latent_operating_workspace_bytes(N, S, C, T, nnz);
    const bool sorted = (flags & SAEV_OPERATING_SORTED) != 0;
    const char* own = !role ? "role must not be NULL"
        : (!f1 || !f1_thr || !f1_tp || !f1_fp || !j2 || !youden || !j_thr || !j_tp || !j_fp)
            ? "f1, f1_thr, f1_tp, f1_fp, j2, youden, j_thr, j_tp and j_fp must not be NULL"
        : (flags & ~SAEV_OPERATING_SORTED) ? "flags holds a bit other than SAEV_OPERATING_SORTED"
        : (sorted && (!n_pos || !n_neg || !pos)) ? "with SAEV_OPERATING_SORTED n_pos, n_neg and pos are inputs and must not be NULL"
        : (!n_pos || !n_neg || !pos) ? "n_pos, n_neg and pos must not be NULL"
        : (!workspace || workspace_bytes < need) ? "workspace smaller than saev_latent_operating_workspace_bytes(N, S, C, T, nnz)"
        : nullptr;
    LaOpen o;
    const int rc = sorted ? la_check(who, row_ptr, indices, data, nnz, N, S, C, class_u8, remap, class_i32, pos, own, workspace, workspace_bytes, stream, &o)
                          : la_open(who, row_ptr, indices, data, nnz, N, S, C, class_u8, remap, class_i32, pos, own, workspace, workspace_bytes, stream, &o);
    if (rc) return rc;
    hipStream_t s = o.s;
    const int Tp = (int)au_tp(T);
    uint8_t* table = o.ws + o.L.total_bytes;
    long long* np = reinterpret_cast<long long*>(n_pos);
    long long* nn = reinterpret_cast<long long*>(n_neg);
    LaSorted e{reinterpret_cast<const int64_t*>(o.ws + o.L.off_starts), reinterpret_cast<const uint32_t*>(o.ws + o.L.off_key),
               reinterpret_cast<const int32_t*>(o.ws + o.L.off_row)};  // (where la_sort leaves them)
    if (!sorted) {
        hipLaunchKernelGGL(au_roles_kernel, dim3((unsigned)(Tp / 64), (unsigned)(C + 1)), dim3(64), 0, s, role, (int)C, (int)T, Tp, table, o.err);
        hipLaunchKernelGGL(au_counts_kernel, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, s, table, o.pos, (int)C, (int)T, Tp, np, nn);
        e = la_sort(o.L, o.ws, row_ptr, indices, data, nnz, N, S, s);
    }
    OpWalk a{e.starts, e.key, e.row, class_u8, remap, class_i32, table, np, nn, f1, f1_thr, reinterpret_cast<long long*>(f1_tp),
             reinterpret_cast<long long*>(f1_fp), reinterpret_cast<long long*>(j2), youden, j_thr, reinterpret_cast<long long*>(j_tp),
             reinterpret_cast<long long*>(j_fp), (int)N, (int)S, (int)C, (int)T, Tp};
    const dim3 grid((unsigned)((S + 3) / 4), (unsigned)(Tp / 64));
    const size_t slice = (size_t)(C + 1) * 64;
    if (slice <= (size_t)AU_LDS_MAX_BYTES) hipLaunchKernelGGL(op_walk_kernel<true>, grid, dim3(256), slice, s, a);
    else hipLaunchKernelGGL(op_walk_kernel<false>, grid, dim3(256), 0, s, a);
    if (hipGetLastError() != hipSuccess) return entry_refuse(SAEV_HIP_ERROR, who, "kernel launch failed");
    return SAEV_OK;
}
