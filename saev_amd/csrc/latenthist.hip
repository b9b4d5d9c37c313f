// Per-latent activation histograms and exact quantiles (include/saev_amd.h: LATENT HISTOGRAM): for every latent
// the distribution of its codes over a stream of batches, as integer counts of the bits of the order-preserving key of a float
// (f2ukey of common.h), and any order statistic of it by a three-level radix select over the same stream.
//
//   key      k = f2ukey(v): strictly increasing in v, invertible.  Level 0 is k >> 20 (sign, exponent, three mantissa bits: 4 096
//            bins, eight to the octave), level 1 (k >> 10) & 1023, level 2 k & 1023.
//   update   one thread per code slot (padded rows) or stored entry (CSR: the row by bisection of row_ptr, only when rows are
//            masked).  At level 0 an entry increments counter (latent, level-0 bin); at levels 1 and 2 it reads its latent's 16
//            prefixes in one 64-byte line and, for every target whose prefix its key carries, increments counter
//            (latent, target, digit).  The increments of a workgroup meet in an LDS hash table first (open addressing, integer
//            atomics); the table lives across the workgroup's whole grid stride and is flushed -- one global integer atomic per
//            distinct counter -- only when the next 256 entries could fill it, and at the end.  A latent that fires on every row
//            at one value therefore reaches memory once per flush, not once per row.  Kept rows are counted on the side.
//   locate   one workgroup per latent, nothing read back.  Level 0: the exclusive sums of the 4 096 bins, the zero block of the
//            silent rows (over = rows) between bins 2 047 and 2 048, h = (M - 1) q in fp64, and for each of the 2 Q target ranks
//            floor(h), ceil(h) the bin that holds it and the rank left inside it.  Levels 1 and 2: the same on the target's own
//            1 024 counters.  After level 2 the 32 located bits go back through ukey2f: lower, higher, and
//            linear = lower + (h - floor(h)) (higher - lower) in fp64 without contraction.
//
// Integer atomics only, so the counts are exact and the same for every order of the batches; no floating-point atomic, no n x S
// temporary, nothing read back, no synchronisation.
#include "entry_util.h"

#include <algorithm>
#include <cstring>

namespace {

constexpr int LH_BINS0 = 4096;
constexpr int LH_BINS = 1024;                 // levels 1 and 2
constexpr int LH_MAX_Q = 8;
constexpr int LH_T_STRIDE = 2 * LH_MAX_Q;     // prefix / rank / resolved rows are 16 wide, the first T = 2 Q live
constexpr int LH_THREADS = 256;
constexpr int LH_GRID_CAP = 1024;             // workgroups of an update: each walks the entries with a stride of LH_GRID_CAP * 256
constexpr int LH_SLOTS = 4096;                // of the LDS hash table (power of two); 32 KB with the counts
constexpr int LH_FILL = 3584;                 // a step that could push the table past this many keys flushes first
constexpr uint32_t LH_EMPTY = 0xffffffffu;    // no counter has this index: the tables stay below 2^32 - 1 counters
constexpr uint32_t LH_NO_PREFIX = 0xffffffffu;  // a resolved target: no key carries it

// entry e of the batch, its value as the key: false when it is no entry (batch_entry; no row is asked for)
__device__ __forceinline__ bool lh_entry(const BatchCodes& c, long e, int* lat, uint32_t* key) {
    float x;
    if (!batch_entry<false>(c, e, lat, &x, nullptr)) return false;
    *key = f2ukey(x);
    return true;
}

// one increment of counter `at` into the workgroup's table; returns 1 when it took a fresh slot.  Terminates: a step starts with
// at most LH_FILL - (its own inserts) keys in LH_SLOTS > LH_FILL slots, or with an empty table and at most LH_SLOTS = 256 x 16 inserts
__device__ __forceinline__ int lh_insert(uint32_t* keys, uint32_t* cnts, uint32_t at) {
    uint32_t slot = (at * 2654435761u) >> 20;  // the top 12 bits: LH_SLOTS = 4096
    for (int probe = 0; probe < LH_SLOTS; ++probe) {
        const uint32_t prev = atomicCAS(keys + slot, LH_EMPTY, at);
        if (prev == LH_EMPTY || prev == at) {
            atomicAdd(cnts + slot, 1u);
            return prev == LH_EMPTY;
        }
        slot = (slot + 1) & (LH_SLOTS - 1);
    }
    return 0;  // (cannot happen: see above)
}

__device__ __forceinline__ void lh_flush(uint32_t* keys, uint32_t* cnts, uint32_t* __restrict__ counts) {
    for (int s = threadIdx.x; s < LH_SLOTS; s += LH_THREADS) {
        const uint32_t at = keys[s];
        if (at != LH_EMPTY) {
            atomicAdd(counts + at, cnts[s]);
            keys[s] = LH_EMPTY;
            cnts[s] = 0u;
        }
    }
}

// LEVEL 0, 1 or 2.  counts: S x 4096 at level 0, S x T x 1024 above; prefix: S x 16 (levels 1, 2).  batch_rows: the kept rows of
// this batch, summed into the workspace's first word
template <int LEVEL>
__global__ __launch_bounds__(LH_THREADS) void lh_update_kernel(BatchCodes c, int T, uint32_t* __restrict__ counts,
                                                               const uint32_t* __restrict__ prefix,
                                                               unsigned long long* __restrict__ batch_rows) {
    __shared__ uint32_t keys[LH_SLOTS];
    __shared__ uint32_t cnts[LH_SLOTS];
    const int t = threadIdx.x, lane = t & 63;
    for (int s = t; s < LH_SLOTS; s += LH_THREADS) {
        keys[s] = LH_EMPTY;
        cnts[s] = 0u;
    }
    __syncthreads();

    // the kept rows of the batch
    int rows = 0;
    for (long r = (long)blockIdx.x * LH_THREADS + t; r < c.n; r += (long)gridDim.x * LH_THREADS) rows += c.keep == nullptr || c.keep[r] != 0;
    rows = wave_sum_i(rows);
    if (lane == 0 && rows > 0) atomicAdd(batch_rows, (unsigned long long)rows);

    // an upper bound of the keys in the table, the same in every thread: it comes out of the barrier that ends a step
    const int per_entry = LEVEL == 0 ? 1 : T, step_max = LH_THREADS * per_entry;
    int occ = 0;
    for (long base = (long)blockIdx.x * LH_THREADS; base < c.total; base += (long)gridDim.x * LH_THREADS) {
        if (occ > 0 && occ + step_max > LH_FILL) {
            lh_flush(keys, cnts, counts);
            occ = 0;
            __syncthreads();
        }
        const long e = base + t;
        int lat, fresh = 0;
        uint32_t key;
        if (e < c.total && lh_entry(c, e, &lat, &key)) {
            if (LEVEL == 0) {
                fresh = lh_insert(keys, cnts, (uint32_t)lat * LH_BINS0 + (key >> 20));
            } else {
                const uint32_t mine = LEVEL == 1 ? key >> 20 : key >> 10;
                const uint32_t digit = LEVEL == 1 ? (key >> 10) & 1023u : key & 1023u;
                const uint4* row = reinterpret_cast<const uint4*>(prefix + (size_t)lat * LH_T_STRIDE);  // one 64-byte line
                const uint4 p0 = row[0], p1 = row[1], p2 = row[2], p3 = row[3];
                const uint32_t p[LH_T_STRIDE] = {p0.x, p0.y, p0.z, p0.w, p1.x, p1.y, p1.z, p1.w, p2.x, p2.y, p2.z, p2.w, p3.x, p3.y, p3.z, p3.w};
#pragma unroll
                for (int q = 0; q < LH_T_STRIDE; ++q)
                    if (q < T && p[q] == mine) fresh += lh_insert(keys, cnts, ((uint32_t)lat * (uint32_t)T + q) * LH_BINS + digit);
            }
        }
        occ += per_entry * __syncthreads_count(fresh > 0);
    }
    lh_flush(keys, cnts, counts);
}

// *n_rows += the batch's kept rows: one plain add an update, behind the update kernel on the stream
__global__ void lh_commit_rows_kernel(const unsigned long long* __restrict__ batch_rows, long long* __restrict__ n_rows) {
    if (threadIdx.x == 0 && blockIdx.x == 0) *n_rows += (long long)*batch_rows;
}

struct LhTargets {
    double q[LH_MAX_Q];
    int Q, over_rows, S;
    uint32_t* prefix;
    uint32_t* rank;
    int32_t* resolved;
    long long* count;
    float* lower;
    float* higher;
    double* linear;
};

// the ranks floor(h) and ceil(h) of h = (M - 1) q, as numpy forms them
__device__ __forceinline__ void lh_ranks(unsigned long long M, double q, unsigned long long* lo, unsigned long long* hi, double* frac) {
#pragma clang fp contract(off)
    const double h = (double)(M - 1) * q;
    const double f = floor(h);
    *lo = (unsigned long long)f;
    *hi = (unsigned long long)ceil(h);
    *frac = h - f;
}

// lower + frac (higher - lower), each operation rounded on its own (no fused multiply-add)
__device__ __forceinline__ double lh_lerp(double lo, double hi, double frac) {
#pragma clang fp contract(off)
    const double d = hi - lo;
    const double m = frac * d;
    return lo + m;
}

// exclusive sums over the workgroup of one value per thread; the total to every thread
__device__ __forceinline__ unsigned long long lh_block_scan(unsigned long long mine, unsigned long long* total) {
    __shared__ unsigned long long sw[LH_THREADS / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const unsigned long long inc = wave_scan_incl(mine, lane);
    __syncthreads();  // (the last call's readers are done)
    if (lane == 63) sw[w] = inc;
    __syncthreads();
    unsigned long long before = 0, all = 0;
    for (int q = 0; q < LH_THREADS / 64; ++q) {
        if (q < w) before += sw[q];
        all += sw[q];
    }
    *total = all;
    return before + inc - mine;
}

// LEVEL 0: one table of 4 096 bins serves the latent's 2 Q targets
__global__ __launch_bounds__(LH_THREADS) void lh_locate0_kernel(const uint32_t* __restrict__ counts, const long long* __restrict__ n_rows, LhTargets g) {
    constexpr int PER = LH_BINS0 / LH_THREADS;  // 16 bins a thread; thread 128 holds the first positive bin
    const int l = blockIdx.x, t = threadIdx.x;
    if (l >= g.S) return;
    uint32_t c[PER];
    const uint4* src = reinterpret_cast<const uint4*>(counts + (size_t)l * LH_BINS0 + (size_t)t * PER);
#pragma unroll
    for (int v = 0; v < PER / 4; ++v) {
        const uint4 x = src[v];
        c[4 * v] = x.x, c[4 * v + 1] = x.y, c[4 * v + 2] = x.z, c[4 * v + 3] = x.w;
    }
    unsigned long long mine = 0;
#pragma unroll
    for (int v = 0; v < PER; ++v) mine += c[v];
    unsigned long long entries;
    const unsigned long long start = lh_block_scan(mine, &entries);
    // the negatives are what the lower half of the threads hold: the start of thread 128
    __shared__ unsigned long long neg_s;
    if (t == LH_THREADS / 2) neg_s = start;
    __syncthreads();
    const unsigned long long n_neg = neg_s;
    unsigned long long zeros = 0;
    if (g.over_rows) {
        const long long N = *n_rows;
        zeros = N > 0 && (unsigned long long)N > entries ? (unsigned long long)N - entries : 0ull;
    }
    const unsigned long long M = entries + zeros;
    if (t == 0) g.count[l] = (long long)M;
    const unsigned long long first = t < LH_THREADS / 2 ? start : start + zeros;  // rank of this thread's first element
    for (int k = 0; k < 2 * g.Q; ++k) {
        const size_t at = (size_t)l * LH_T_STRIDE + k;
        if (M == 0) {
            if (t == 0) g.prefix[at] = LH_NO_PREFIX, g.rank[at] = 0u, g.resolved[at] = 2;
            continue;
        }
        unsigned long long lo, hi;
        double frac;
        lh_ranks(M, g.q[k >> 1], &lo, &hi, &frac);
        const unsigned long long r = (k & 1) ? hi : lo;
        if (r >= n_neg && r < n_neg + zeros) {  // inside the zero block: 0.0 at once
            if (t == 0) g.prefix[at] = LH_NO_PREFIX, g.rank[at] = 0u, g.resolved[at] = 1;
            continue;
        }
        if (r >= first && r < first + mine) {  // exactly one thread
            unsigned long long left = r - first;
            int b = 0;
#pragma unroll
            for (int v = 0; v < PER; ++v) {
                if (left >= c[v] && b == v) left -= c[v], b = v + 1;
            }
            g.prefix[at] = (uint32_t)(t * PER + b);
            g.rank[at] = (uint32_t)left;
            g.resolved[at] = 0;
        }
    }
}

// LEVELS 1 and 2: target k of latent l has its own 1 024 counters
template <int LEVEL>
__global__ __launch_bounds__(LH_THREADS) void lh_locate_kernel(const uint32_t* __restrict__ counts, LhTargets g) {
    constexpr int PER = LH_BINS / LH_THREADS;  // 4
    const int l = blockIdx.x, t = threadIdx.x;
    if (l >= g.S) return;
    const int T = 2 * g.Q;
    for (int k = 0; k < T; ++k) {
        const size_t at = (size_t)l * LH_T_STRIDE + k;
        if (g.resolved[at] != 0) continue;  // (the same in every thread)
        const uint4 x = *reinterpret_cast<const uint4*>(counts + ((size_t)l * T + k) * LH_BINS + (size_t)t * PER);
        const uint32_t c[PER] = {x.x, x.y, x.z, x.w};
        const unsigned long long mine = (unsigned long long)c[0] + c[1] + c[2] + c[3];
        unsigned long long all;
        const unsigned long long first = lh_block_scan(mine, &all);
        const unsigned long long r = g.rank[at];
        const uint32_t pre = g.prefix[at];
        __syncthreads();  // every thread has read the target before its owner rewrites it
        if (r >= first && r < first + mine) {
            unsigned long long left = r - first;
            int b = 0;
#pragma unroll
            for (int v = 0; v < PER; ++v) {
                if (left >= c[v] && b == v) left -= c[v], b = v + 1;
            }
            g.prefix[at] = (pre << 10) | (uint32_t)(t * PER + b);
            g.rank[at] = (uint32_t)left;
        }
    }
    if (LEVEL != 2) return;
    __syncthreads();
    // the 32 located bits back to floats: thread i < Q writes quantile i
    if (t < g.Q) {
        const size_t at = (size_t)l * LH_T_STRIDE + 2 * t, out = (size_t)l * g.Q + t;
        const int state = g.resolved[at];  // (an empty multiset resolves both targets)
        const unsigned long long M = (unsigned long long)g.count[l];
        if (state == 2 || M == 0) {
            g.lower[out] = __uint_as_float(0x7fc00000u);
            g.higher[out] = __uint_as_float(0x7fc00000u);
            g.linear[out] = __longlong_as_double(0x7ff8000000000000LL);
        } else {
            const float lo = g.resolved[at] == 1 ? 0.f : ukey2f(g.prefix[at]);
            const float hi = g.resolved[at + 1] == 1 ? 0.f : ukey2f(g.prefix[at + 1]);
            unsigned long long rl, rh;
            double frac;
            lh_ranks(M, g.q[t], &rl, &rh, &frac);
            g.lower[out] = lo;
            g.higher[out] = hi;
            g.linear[out] = lo == hi ? (double)lo : lh_lerp((double)lo, (double)hi, frac);
        }
    }
}

int64_t lh_table_counters(int level, int64_t S, int64_t T) { return level == 0 ? S * LH_BINS0 : S * T * LH_BINS; }

}  // namespace

int64_t saev_latent_hist_workspace_bytes(int64_t n_entries, int64_t S) {
    if (n_entries < 0 || n_entries > 0x7fffffffLL || S < 0 || S > 0x7fffffffLL) return -1;
    return 256;  // the batch's kept-row count
}

int saev_latent_hist_update(const int32_t* idx, const float* val, const int32_t* row_nnz, int64_t cap, const int64_t* row_ptr,
                            const int32_t* indices, const float* data, int64_t nnz, const uint8_t* keep, int64_t n, int64_t S,
                            const saev_latent_hist_state* state, void* workspace, int64_t workspace_bytes, void* stream) {
    const char* who = "saev_latent_hist_update";
    if (n < 0 || S < 0 || cap < 0 || nnz < 0) return entry_refuse(SAEV_INVALID_ARG, who, "negative size");
    if (n > 0x7fffffffLL || S > 0x7fffffffLL || cap > 0x7fffffffLL) return entry_refuse(SAEV_INVALID_ARG, who, "size above 2^31 - 1");
    if (!state || state->struct_size < (int32_t)(2 * sizeof(int32_t))) return entry_refuse(SAEV_INVALID_ARG, who, "no saev_latent_hist_state (or its struct_size is unset)");
    saev_latent_hist_state st;
    std::memset(&st, 0, sizeof st);
    std::memcpy(&st, state, std::min<size_t>(sizeof st, (size_t)state->struct_size));
    if (st.level < 0 || st.level > 2) return entry_refuse(SAEV_INVALID_ARG, who, "level must be 0, 1 or 2");
    if (st.level > 0 && (st.T < 1 || st.T > LH_T_STRIDE)) return entry_refuse(SAEV_UNSUPPORTED, who, "T must lie in [1, 16] at levels 1 and 2");
    if (!st.counts || !st.n_rows || (st.level > 0 && !st.prefix)) return entry_refuse(SAEV_INVALID_ARG, who, "a state pointer is NULL");
    if (((uintptr_t)st.counts & 15) != 0 || ((uintptr_t)st.prefix & 15) != 0) return entry_refuse(SAEV_INVALID_ARG, who, "the count and prefix tables must be 16-byte aligned");
    if (lh_table_counters(st.level, S, st.T) >= 0xffffffffLL) return entry_refuse(SAEV_UNSUPPORTED, who, "the count table must stay below 2^32 - 1 counters");
    if (n == 0) return SAEV_OK;
    const bool padded = idx || val, csr = row_ptr || indices || data;
    if (padded == csr) return entry_refuse(SAEV_INVALID_ARG, who, "give the codes as padded rows (idx, val) or as CSR (row_ptr, indices, data), one of the two");
    if (padded && (!idx || !val)) return entry_refuse(SAEV_INVALID_ARG, who, "idx and val come together");
    if (csr && (!row_ptr || !indices || !data)) return entry_refuse(SAEV_INVALID_ARG, who, "row_ptr, indices and data come together");
    if (csr && row_nnz) return entry_refuse(SAEV_INVALID_ARG, who, "row_nnz belongs to the padded form");
    const int64_t total = padded ? n * cap : nnz;
    if (total > 0x7fffffffLL) return entry_refuse(SAEV_UNSUPPORTED, who, "more than 2^31 - 1 entries in one batch");
    const int64_t need = saev_latent_hist_workspace_bytes(total, S);
    if (const int rc = entry_check_workspace(who, workspace, workspace_bytes, need, "workspace smaller than saev_latent_hist_workspace_bytes(entries, S)")) return rc;
    if (S == 0) return SAEV_OK;

    hipStream_t s = (hipStream_t)stream;
    unsigned long long* batch_rows = static_cast<unsigned long long*>(workspace);
    BatchCodes c{idx, val, row_nnz, (int)cap, row_ptr, indices, data, keep, (long)total, (int)n, (int)S};
    if (hipMemsetAsync(batch_rows, 0, 8, s) != hipSuccess) return entry_refuse(SAEV_HIP_ERROR, who, "hipMemsetAsync failed");
    const int64_t work = std::max<int64_t>(total, n);
    const int grid = (int)std::min<int64_t>((work + LH_THREADS - 1) / LH_THREADS, LH_GRID_CAP);
    if (st.level == 0)
        hipLaunchKernelGGL(lh_update_kernel<0>, dim3(grid), dim3(LH_THREADS), 0, s, c, 0, st.counts, (const uint32_t*)nullptr, batch_rows);
    else if (st.level == 1)
        hipLaunchKernelGGL(lh_update_kernel<1>, dim3(grid), dim3(LH_THREADS), 0, s, c, st.T, st.counts, (const uint32_t*)st.prefix, batch_rows);
    else
        hipLaunchKernelGGL(lh_update_kernel<2>, dim3(grid), dim3(LH_THREADS), 0, s, c, st.T, st.counts, (const uint32_t*)st.prefix, batch_rows);
    hipLaunchKernelGGL(lh_commit_rows_kernel, dim3(1), dim3(64), 0, s, batch_rows, reinterpret_cast<long long*>(st.n_rows));
    if (hipGetLastError() != hipSuccess) return entry_refuse(SAEV_HIP_ERROR, who, "kernel launch failed");
    return SAEV_OK;
}

int saev_latent_hist_locate(const saev_latent_hist_state* state, const saev_latent_hist_targets* targets, int64_t S, void* stream) {
    const char* who = "saev_latent_hist_locate";
    if (S < 0) return entry_refuse(SAEV_INVALID_ARG, who, "negative size");
    if (S > 0x7fffffffLL) return entry_refuse(SAEV_INVALID_ARG, who, "size above 2^31 - 1");
    if (!state || state->struct_size < (int32_t)(2 * sizeof(int32_t))) return entry_refuse(SAEV_INVALID_ARG, who, "no saev_latent_hist_state (or its struct_size is unset)");
    if (!targets || targets->struct_size < (int32_t)(2 * sizeof(int32_t))) return entry_refuse(SAEV_INVALID_ARG, who, "no saev_latent_hist_targets (or its struct_size is unset)");
    saev_latent_hist_state st;
    std::memset(&st, 0, sizeof st);
    std::memcpy(&st, state, std::min<size_t>(sizeof st, (size_t)state->struct_size));
    saev_latent_hist_targets tg;
    std::memset(&tg, 0, sizeof tg);
    std::memcpy(&tg, targets, std::min<size_t>(sizeof tg, (size_t)targets->struct_size));
    if (st.level < 0 || st.level > 2) return entry_refuse(SAEV_INVALID_ARG, who, "level must be 0, 1 or 2");
    if (tg.Q < 1 || tg.Q > LH_MAX_Q) return entry_refuse(SAEV_UNSUPPORTED, who, "Q must lie in [1, 8]");
    for (int i = 0; i < tg.Q; ++i)
        if (!(tg.q[i] >= 0.0 && tg.q[i] <= 1.0)) return entry_refuse(SAEV_INVALID_ARG, who, "every q must lie in [0, 1]");
    if (st.level > 0 && st.T != 2 * tg.Q) return entry_refuse(SAEV_INVALID_ARG, who, "the state's T must be 2 Q");
    if (!st.counts || (st.level == 0 && tg.over_rows && !st.n_rows)) return entry_refuse(SAEV_INVALID_ARG, who, "a state pointer is NULL");
    if (!tg.prefix || !tg.rank || !tg.resolved || !tg.count) return entry_refuse(SAEV_INVALID_ARG, who, "a target pointer is NULL");
    if (st.level == 2 && (!tg.lower || !tg.higher || !tg.linear)) return entry_refuse(SAEV_INVALID_ARG, who, "lower, higher and linear are written after level 2");
    if (((uintptr_t)st.counts & 15) != 0) return entry_refuse(SAEV_INVALID_ARG, who, "the count and prefix tables must be 16-byte aligned");
    if (lh_table_counters(st.level, S, 2 * tg.Q) >= 0xffffffffLL) return entry_refuse(SAEV_UNSUPPORTED, who, "the count table must stay below 2^32 - 1 counters");
    if (S == 0) return SAEV_OK;

    hipStream_t s = (hipStream_t)stream;
    LhTargets g;
    for (int i = 0; i < LH_MAX_Q; ++i) g.q[i] = i < tg.Q ? tg.q[i] : 0.0;
    g.Q = tg.Q, g.over_rows = tg.over_rows != 0, g.S = (int)S;
    g.prefix = tg.prefix, g.rank = tg.rank, g.resolved = tg.resolved, g.count = reinterpret_cast<long long*>(tg.count);
    g.lower = tg.lower, g.higher = tg.higher, g.linear = tg.linear;
    if (st.level == 0)
        hipLaunchKernelGGL(lh_locate0_kernel, dim3((unsigned)S), dim3(LH_THREADS), 0, s, (const uint32_t*)st.counts, reinterpret_cast<const long long*>(st.n_rows), g);
    else if (st.level == 1)
        hipLaunchKernelGGL(lh_locate_kernel<1>, dim3((unsigned)S), dim3(LH_THREADS), 0, s, (const uint32_t*)st.counts, g);
    else
        hipLaunchKernelGGL(lh_locate_kernel<2>, dim3((unsigned)S), dim3(LH_THREADS), 0, s, (const uint32_t*)st.counts, g);
    if (hipGetLastError() != hipSuccess) return entry_refuse(SAEV_HIP_ERROR, who, "kernel launch failed");
    return SAEV_OK;
}
