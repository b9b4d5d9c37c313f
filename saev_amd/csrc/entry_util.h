// What the context-free analysis entries share (latenttopk.hip, probe1d.hip, latentap.hip, sparselinear.hip): how a
// workspace is carved, how a call is refused, the refusals common to the (N, S, C, nnz) entries, and the device pieces the
// CSR-reading units need -- the row of a stored entry, the streamed accumulators' view of one batch of codes and the
// single-workgroup exclusive scan (the wave scan under it is wave_scan_incl of common.h, which kmeans.hip uses too).  The
// latent-major regroup built on these is latent_major.h.  Everything inlines: a unit's code
// objects are what they were when it carried its own copy.
#pragma once
#include "common.h"
#include "kernels.h"

#include <algorithm>
#include <cstdio>

// ---- host ------------------------------------------------------------------------------------------------------------------------

static inline int64_t round256(int64_t b) { return (b + 255) / 256 * 256; }

// offsets of a workspace's arrays, each on a 256-byte boundary; `at` ends as the workspace's size
struct WsCarve {
    int64_t at = 0;
    int64_t take(int64_t bytes) {
        const int64_t o = at;
        at += round256(std::max<int64_t>(bytes, 1));
        return o;
    }
};

// The part rule of the latent-major counting sorts (latent_major.h, probe1d.hip): the stored entries are cut into at most LM_PARTS
// contiguous parts (4 096 bought the place pass an eighth and cost 200 MB of count table: its stores are the floor), parts x S
// counters stay at or below 2^26, and a part is a whole number of 64-entry trips
constexpr int LM_PARTS = 1024;

static inline int lm_parts(int64_t S, int64_t nnz) {
    int64_t p = std::min<int64_t>(LM_PARTS, (nnz + 63) / 64);
    p = std::min<int64_t>(p, std::max<int64_t>(1, ((int64_t)1 << 26) / std::max<int64_t>(S, 1)));
    return (int)std::max<int64_t>(p, 1);
}
static inline int64_t lm_part_len(int64_t nnz, int parts) { return std::max<int64_t>(64, ((nnz + parts - 1) / parts + 63) / 64 * 64); }

// leaves "who: what" as the thread's last error (saev_last_error(NULL)) and returns `code`
static inline int entry_refuse(int code, const char* who, const char* what) {
    static thread_local char msg[192];
    std::snprintf(msg, sizeof msg, "%s: %s", who, what);
    return free_refuse(code, msg);
}

constexpr int ENTRY_MAX_C = 4096;

static inline bool entry_shape_ok(int64_t N, int64_t S, int64_t C, int64_t nnz) {
    return N >= 1 && N <= 0x7fffffffLL && S >= 1 && S <= 0x7fffffffLL && C >= 1 && C <= ENTRY_MAX_C && nnz >= 0 && nnz <= 0x7fffffffLL;
}

// the shape refusals of an (N, S, C, nnz) entry, in the order every such entry makes them; SAEV_OK when there is none
static inline int entry_check_shape(const char* who, int64_t N, int64_t S, int64_t C, int64_t nnz) {
    if (N < 0 || S < 0 || C < 0 || nnz < 0) return entry_refuse(SAEV_INVALID_ARG, who, "negative size");
    if (N > 0x7fffffffLL || S > 0x7fffffffLL || nnz > 0x7fffffffLL) return entry_refuse(SAEV_UNSUPPORTED, who, "N, S and nnz must stay below 2^31");
    if (N < 1 || S < 1) return entry_refuse(SAEV_INVALID_ARG, who, "N and S must be at least 1");
    if (C < 1 || C > ENTRY_MAX_C) return entry_refuse(SAEV_UNSUPPORTED, who, "the number of classes must lie in [1, 4096]");
    return SAEV_OK;
}

// the workspace refusals; `too_small` names the entry's own sizing function
static inline int entry_check_workspace(const char* who, const void* ws, int64_t ws_bytes, int64_t need, const char* too_small) {
    if (!ws || ws_bytes < need) return entry_refuse(SAEV_INVALID_ARG, who, too_small);
    if (((uintptr_t)ws & 255) != 0) return entry_refuse(SAEV_INVALID_ARG, who, "workspace must be 256-byte aligned");
    return SAEV_OK;
}

// ---- device ----------------------------------------------------------------------------------------------------------------------

// the row r with row_ptr[r] <= p < row_ptr[r + 1] of stored entry p (empty rows are stepped over).  p >= row_ptr[N] gives N - 1: a
// caller that can be handed such a p guards it itself
__device__ __forceinline__ int csr_row_of(const int64_t* row_ptr, int N, int64_t p) {
    int lo = 0, hi = N;
    while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        if (row_ptr[mid] <= p) lo = mid; else hi = mid;
    }
    return lo;
}

// one batch of codes in either form (padded rows: idx != nullptr; CSR: row_ptr != nullptr), as the streamed accumulators take it
// (latenttopk.hip, latenthist.hip)
struct BatchCodes {
    const int32_t* idx;
    const float* val;
    const int32_t* row_nnz;
    int cap;
    const int64_t* row_ptr;
    const int32_t* indices;
    const float* data;
    const uint8_t* keep;
    long total;  // code slots n cap, or stored entries
    int n, S;
};

// entry e of the batch: false when it is no entry (padding, masked row, zero, latent out of range).  Without WANT_ROW a CSR entry's
// row is bisected for only when rows are masked, and *row is left alone
template <bool WANT_ROW>
__device__ __forceinline__ bool batch_entry(const BatchCodes& c, long e, int* lat, float* x, int* row) {
    int r = 0, i;
    float v;
    if (c.idx != nullptr) {
        const long rr = e / c.cap;
        const int slot = (int)(e - rr * c.cap);
        r = (int)rr;
        if (c.keep != nullptr && c.keep[r] == 0) return false;
        if (c.row_nnz != nullptr && slot >= c.row_nnz[r]) return false;  // (a count above cap reads as cap: slot < cap always)
        i = c.idx[e];
        v = c.val[e];
    } else {
        const int64_t p = c.row_ptr[0] + e;
        if (p >= c.row_ptr[c.n]) return false;
        if (WANT_ROW || c.keep != nullptr) {
            r = csr_row_of(c.row_ptr, c.n, p);
            if (c.keep != nullptr && c.keep[r] == 0) return false;
        }
        i = c.indices[p];
        v = c.data[p];
    }
    if (i < 0 || i >= c.S) return false;
    if (v == 0.f) return false;  // zeros of both signs are not entries
    *lat = i;
    *x = v;
    if (WANT_ROW) *row = r;
    return true;
}

// Exclusive prefix sums of S elements by ONE workgroup of THREADS, THREADS elements a round so that every load and store is
// coalesced, the sum of the earlier rounds carried in LDS.  load(l) gives element l, store(l, start) takes the sum of the elements
// before it; the sum of all S is returned to every thread.  T is an integer type (int, or two sums packed in an unsigned long long),
// I the type the element index is held in: each kernel keeps the width it was written with, and so its registers
template <int THREADS, typename T, typename I, typename Load, typename Store>
__device__ __forceinline__ T block_scan_rounds(int S, Load load, Store store) {
    __shared__ T sw[THREADS / 64];
    __shared__ T carry_s;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    if (t == 0) carry_s = 0;
    __syncthreads();
    for (I base = 0; base < S; base += THREADS) {
        const I l = base + t;
        const T mine = l < S ? load(l) : (T)0;
        const T inc = wave_scan_incl(mine, lane);
        if (lane == 63) sw[w] = inc;
        __syncthreads();
        T before = carry_s;
        for (int q = 0; q < w; ++q) before += sw[q];
        const T start = before + inc - mine;
        if (l < S) store(l, start);
        __syncthreads();
        if (t == THREADS - 1) carry_s = before + inc;
        __syncthreads();
    }
    return carry_s;
}
