// Per-latent top-k activating tokens (include/saev_amd.h: LATENT TOP-K): for every latent the k largest codes
// seen so far and the rows they sit in, kept exactly and deterministically over a stream of batches.
//
// State (the caller's, latent-major): top_val (S x k), top_row (S x k), top_cnt (S).  A latent's list is sorted by
// (value descending, row ascending) after every update; slots past its count are never written.
//
//   count    one thread per code slot (padded rows) or per stored entry (CSR: the row by bisection of row_ptr).  An entry is a
//            CANDIDATE when its latent's list is not full or its value is >= the list's last value (equality passes: its row may
//            be the lower one).  Integer atomics count the candidates of every latent.  Once the lists have warmed up almost
//            nothing passes: an update is then two reads of the codes.
//   scan     one workgroup: exclusive prefix sums of the counts (segment starts) and a copy of them as placement cursors.
//   place    the count pass again, with the same predicate on the same (unchanged) state: a candidate takes the next slot of its
//            latent's segment (integer atomic on the cursor) and leaves (value, local row) there.  The order inside a segment is
//            arbitrary; the merge orders by the full key, so the result does not depend on it.
//   merge    one wave per latent with candidates, one entry per lane.  Keys are (valid, value as an order-preserving integer,
//            row): a total order, so the sort has one answer.  Candidates come in chunks of 64: a chunk none of whose entries
//            beats the full list's last entry is dropped; any other is sorted by a bitonic network over lane shuffles, merged with
//            the resident 64 (lane i takes the better of resident[i] and chunk[63 - i]: the best 64 of the 128, as a bitonic
//            sequence) and sorted again by the network's last six stages.  The first min(k, entries) lanes are the new list.
//
// No floating-point atomic, no n x S temporary, nothing read back, no synchronisation.
#include "entry_util.h"

#include <algorithm>
#include <cstring>

namespace {

constexpr int LT_MAX_K = 64;
constexpr int LT_SCAN_THREADS = 1024;

// entry e of the batch: false when it is no entry (batch_entry) or no candidate
__device__ __forceinline__ bool lt_candidate(const BatchCodes& c, int k, long e, const float* __restrict__ top_val,
                                             const int32_t* __restrict__ top_cnt, int* lat, float* v, int* row) {
    if (!batch_entry<true>(c, e, lat, v, row)) return false;
    return top_cnt[*lat] < k || *v >= top_val[(size_t)*lat * k + k - 1];
}

__global__ __launch_bounds__(256) void lt_count_kernel(BatchCodes c, int k, const float* __restrict__ top_val, const int32_t* __restrict__ top_cnt,
                                                       int32_t* __restrict__ cnt) {
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < c.total; e += (long)gridDim.x * 256) {
        int lat, row;
        float v;
        if (lt_candidate(c, k, e, top_val, top_cnt, &lat, &v, &row)) atomicAdd(cnt + lat, 1);
    }
}

// off[l] = cur[l] = sum of cnt[0 .. l): one workgroup, 1 024 latents per round, so that every load and store is coalesced.  Its
// time grows with S whatever the number of candidates (the fixed cost of an update)
__global__ __launch_bounds__(LT_SCAN_THREADS) void lt_scan_kernel(const int32_t* __restrict__ cnt, int S, int32_t* __restrict__ off,
                                                                  int32_t* __restrict__ cur) {
    block_scan_rounds<LT_SCAN_THREADS, int, int>(S, [&](int l) { return cnt[l]; }, [&](int l, int start) { off[l] = start; cur[l] = start; });
}

__global__ __launch_bounds__(256) void lt_place_kernel(BatchCodes c, int k, const float* __restrict__ top_val, const int32_t* __restrict__ top_cnt,
                                                       int32_t* __restrict__ cur, float* __restrict__ cand_val, int32_t* __restrict__ cand_row) {
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < c.total; e += (long)gridDim.x * 256) {
        int lat, row;
        float v;
        if (!lt_candidate(c, k, e, top_val, top_cnt, &lat, &v, &row)) continue;
        const int at = atomicAdd(cur + lat, 1);
        if (at < 0 || (long)at >= c.total) continue;  // (cannot happen: every segment was counted with this predicate)
        cand_val[at] = v;
        cand_row[at] = row;
    }
}

// key of an entry: hi = valid << 32 | order-preserving image of the value (larger is better), lo = row (smaller is better)
struct LtKey {
    unsigned long long hi;
    long long lo;
};
__device__ __forceinline__ bool lt_before(const LtKey& a, const LtKey& b) { return a.hi > b.hi || (a.hi == b.hi && a.lo < b.lo); }
__device__ __forceinline__ LtKey lt_shfl(const LtKey& a, int src) { return LtKey{__shfl(a.hi, src, 64), __shfl(a.lo, src, 64)}; }
__device__ __forceinline__ LtKey lt_shfl_xor(const LtKey& a, int m) { return LtKey{__shfl_xor(a.hi, m, 64), __shfl_xor(a.lo, m, 64)}; }

// stages j = first .. 1 of the bitonic network for blocks of `size` lanes; blocks alternate best-first / worst-first, the block of
// 64 is best-first
__device__ __forceinline__ void lt_bitonic_stages(LtKey& a, int lane, int size, int first) {
    for (int j = first; j > 0; j >>= 1) {
        const LtKey b = lt_shfl_xor(a, j);
        const bool best_first = (lane & size) == 0;
        const bool low = (lane & j) == 0;
        const bool take_better = low == best_first;
        const bool b_better = lt_before(b, a);
        if (b_better == take_better && (b.hi != a.hi || b.lo != a.lo)) a = b;
    }
}

__global__ __launch_bounds__(256) void lt_merge_kernel(const int32_t* __restrict__ cnt, const int32_t* __restrict__ off,
                                                       const float* __restrict__ cand_val, const int32_t* __restrict__ cand_row,
                                                       long total, int S, int k, long long row_base, float* __restrict__ top_val,
                                                       long long* __restrict__ top_row, int32_t* __restrict__ top_cnt) {
    const int lane = threadIdx.x & 63;
    const int l = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (l >= S) return;
    const int m = cnt[l];
    if (m <= 0) return;
    const long start = off[l];
    if (start < 0 || start + m > total) return;  // (cannot happen: the segments partition the candidates)
    const int have = min(top_cnt[l], k);
    LtKey res{0ull, 0ll};
    if (lane < have) {
        res.hi = (1ull << 32) | f2ukey(top_val[(size_t)l * k + lane]);
        res.lo = top_row[(size_t)l * k + lane];
    }
    for (long base = start; base < start + m; base += 64) {
        LtKey c{0ull, 0ll};
        if (base + lane < start + m) {
            c.hi = (1ull << 32) | f2ukey(cand_val[base + lane]);
            c.lo = row_base + (long long)cand_row[base + lane];
        }
        const LtKey last = lt_shfl(res, k - 1);  // invalid while the list is not full: every entry beats it
        if (__ballot(lt_before(c, last)) == 0ull) continue;
        for (int size = 2; size <= 64; size <<= 1) lt_bitonic_stages(c, lane, size, size >> 1);
        const LtKey rev = lt_shfl(c, 63 - lane);
        if (lt_before(rev, res)) res = rev;
        lt_bitonic_stages(res, lane, 64, 32);
    }
    const int valid = __popcll(__ballot((res.hi >> 32) != 0ull));
    const int now = min(valid, k);
    if (lane < now) {
        top_val[(size_t)l * k + lane] = ukey2f((uint32_t)res.hi);
        top_row[(size_t)l * k + lane] = res.lo;
    }
    if (lane == 0) top_cnt[l] = now;
}

}  // namespace

int64_t saev_latent_topk_workspace_bytes(int64_t n_entries, int64_t S) {
    if (n_entries < 0 || n_entries > 0x7fffffffLL || S < 0 || S > 0x7fffffffLL) return -1;
    return std::max<int64_t>(256, 3 * round256(4 * S) + 2 * round256(4 * n_entries));
}

int saev_latent_topk_update(const int32_t* idx, const float* val, const int32_t* row_nnz, int64_t cap, const int64_t* row_ptr,
                            const int32_t* indices, const float* data, int64_t nnz, const uint8_t* keep, int64_t n, int64_t S,
                            int64_t row_base, const saev_latent_topk_state* state, void* workspace, int64_t workspace_bytes,
                            void* stream) {
    const char* who = "saev_latent_topk_update";
    if (n < 0 || S < 0 || cap < 0 || nnz < 0) return entry_refuse(SAEV_INVALID_ARG, who, "negative size");
    if (n > 0x7fffffffLL || S > 0x7fffffffLL || cap > 0x7fffffffLL) return entry_refuse(SAEV_INVALID_ARG, who, "size above 2^31 - 1");
    if (!state || state->struct_size < (int32_t)(2 * sizeof(int32_t))) return entry_refuse(SAEV_INVALID_ARG, who, "no saev_latent_topk_state (or its struct_size is unset)");
    saev_latent_topk_state st;
    std::memset(&st, 0, sizeof st);
    std::memcpy(&st, state, std::min<size_t>(sizeof st, (size_t)state->struct_size));
    if (st.k < 1 || st.k > LT_MAX_K) return entry_refuse(SAEV_UNSUPPORTED, who, "k must lie in [1, 64]");
    if (!st.top_val || !st.top_row || !st.top_cnt) return entry_refuse(SAEV_INVALID_ARG, who, "a state pointer is NULL");
    if (n == 0) return SAEV_OK;
    const bool padded = idx || val, csr = row_ptr || indices || data;
    if (padded == csr) return entry_refuse(SAEV_INVALID_ARG, who, "give the codes as padded rows (idx, val) or as CSR (row_ptr, indices, data), one of the two");
    if (padded && (!idx || !val)) return entry_refuse(SAEV_INVALID_ARG, who, "idx and val come together");
    if (csr && (!row_ptr || !indices || !data)) return entry_refuse(SAEV_INVALID_ARG, who, "row_ptr, indices and data come together");
    if (csr && row_nnz) return entry_refuse(SAEV_INVALID_ARG, who, "row_nnz belongs to the padded form");
    if (row_base < 0 || row_base > 0x7fffffffffffffffLL - n) return entry_refuse(SAEV_INVALID_ARG, who, "row_base + n leaves int64");
    const int64_t total = padded ? n * cap : nnz;
    if (total > 0x7fffffffLL) return entry_refuse(SAEV_UNSUPPORTED, who, "more than 2^31 - 1 entries in one batch");
    const int64_t need = saev_latent_topk_workspace_bytes(total, S);
    if (const int rc = entry_check_workspace(who, workspace, workspace_bytes, need, "workspace smaller than saev_latent_topk_workspace_bytes(entries, S)")) return rc;
    if (total == 0 || S == 0) return SAEV_OK;

    hipStream_t s = (hipStream_t)stream;
    uint8_t* ws = static_cast<uint8_t*>(workspace);
    int32_t* cnt = reinterpret_cast<int32_t*>(ws);
    int32_t* off = reinterpret_cast<int32_t*>(ws + round256(4 * S));
    int32_t* cur = reinterpret_cast<int32_t*>(ws + 2 * round256(4 * S));
    float* cand_val = reinterpret_cast<float*>(ws + 3 * round256(4 * S));
    int32_t* cand_row = reinterpret_cast<int32_t*>(ws + 3 * round256(4 * S) + round256(4 * total));
    BatchCodes c{idx, val, row_nnz, (int)cap, row_ptr, indices, data, keep, (long)total, (int)n, (int)S};
    if (hipMemsetAsync(cnt, 0, (size_t)S * 4, s) != hipSuccess) return entry_refuse(SAEV_HIP_ERROR, who, "hipMemsetAsync failed");
    const int grid = (int)std::min<int64_t>((total + 255) / 256, 8192);
    hipLaunchKernelGGL(lt_count_kernel, dim3(grid), dim3(256), 0, s, c, st.k, st.top_val, st.top_cnt, cnt);
    hipLaunchKernelGGL(lt_scan_kernel, dim3(1), dim3(LT_SCAN_THREADS), 0, s, cnt, (int)S, off, cur);
    hipLaunchKernelGGL(lt_place_kernel, dim3(grid), dim3(256), 0, s, c, st.k, st.top_val, st.top_cnt, cur, cand_val, cand_row);
    hipLaunchKernelGGL(lt_merge_kernel, dim3((unsigned)((S + 3) / 4)), dim3(256), 0, s, cnt, off, cand_val, cand_row, (long)total, (int)S,
                       st.k, (long long)row_base, st.top_val, reinterpret_cast<long long*>(st.top_row), st.top_cnt);
    if (hipGetLastError() != hipSuccess) return entry_refuse(SAEV_HIP_ERROR, who, "kernel launch failed");
    return SAEV_OK;
}
