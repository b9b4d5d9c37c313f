// Latents matched by what they fire on (include/saev_amd.h: COACTIVATION): for every latent a of a CSR matrix A
// the top_m latents b of a CSR matrix B over the same rows, ranked by Jaccard similarity or containment of the two firing sets,
// without the Sa x Sb intersection matrix.  Everything is integer arithmetic: no float atomics, no order of summation to fix.
//
//   count    a lane group per row of A: the entries with value > thr_a are counted per latent with integer global atomics (n_a);
//            the same for B (n_b).  Every stored entry is checked here (column range, finite value, indptr).
//   scan     one workgroup: exclusive sums of n_a -> the offsets of the latent-major event list; latents with more than
//            COACT_CHUNK_ROWS rows are appended to the heavy list.
//   place    the count pass again, each firing entry's row written under its latent (the order inside a latent is free: everything
//            downstream is a count).
//   walk     a workgroup per latent a with at most COACT_CHUNK_ROWS rows, one uint32 counter per latent of a window of B in LDS.
//            For every row of a's list a lane group reads B's row and adds 1 to the counter of each firing entry inside the window
//            (LDS integer atomics).  Then every thread turns its share of the non-zero counters into keys (I, n_b, b) and keeps the
//            8 best in registers; Sb past the window takes further windows, the registers carrying over.  A workgroup-wide argmax
//            per output rank merges the threads' lists.
//   heavy    a latent with more rows is cut into chunks of COACT_CHUNK_ROWS rows, each walked by its own workgroup, the chunk's
//            counters added into a global int32 row of Sb counters (integer atomics: the order is free); a second kernel ranks the
//            row.  COACT_SLOTS such rows exist, so the heavy list is taken in rounds of that many latents; the chunks are a work list
//            that a few hundred persistent workgroups share out.
//
// Three instantiations of the walk, so that a CU holds several workgroups where Sb allows it: windows of 8192 counters (32 KB, 256
// threads) for Sb <= 8192, of 16384 (64 KB, 512 threads) for Sb <= 16384, and the full window of COACT_WINDOW = 32768 counters (128 KB
// of the CU's 160 KB, 1024 threads) above.
#include "entry_util.h"

#include <algorithm>

namespace {

constexpr int COACT_CHUNK_ROWS = 8192;
constexpr int COACT_WINDOW = 32768;
constexpr int COACT_SMALL_WINDOW = 8192;
constexpr int COACT_MID_WINDOW = 16384;
constexpr int COACT_SLOTS = 512;
constexpr int COACT_LIST = 8;  // the longest top_m

// ---------------------------------------------------------------- the order ---------------------------------------------------------

// a candidate partner: I rows in common, x = U = n_a + n_b - I (Jaccard) or x = n_b (containment), b its index.  An empty slot is
// {0, 1, INT_MAX}: it ranks after every candidate, for a candidate has I >= 1
struct Cand {
    uint32_t I, x;
    int b;
};

__device__ __forceinline__ Cand cand_none() { return Cand{0u, 1u, 0x7fffffff}; }

template <int MEASURE>
__device__ __forceinline__ bool cand_before(const Cand& p, const Cand& q) {
    if (MEASURE == SAEV_COACT_JACCARD) {
        const unsigned long long l = (unsigned long long)p.I * q.x, r = (unsigned long long)q.I * p.x;
        return l != r ? l > r : p.b < q.b;
    }
    if (p.I != q.I) return p.I > q.I;
    if (p.x != q.x) return p.x < q.x;
    return p.b < q.b;
}

// the thread's list stays sorted: the newcomer sinks through it by compare-and-swap, everything unrolled so that it lives in registers
template <int MEASURE>
__device__ __forceinline__ void cand_insert(Cand (&list)[COACT_LIST], Cand c) {
    if (!cand_before<MEASURE>(c, list[COACT_LIST - 1])) return;
#pragma unroll
    for (int j = 0; j < COACT_LIST; ++j) {
        if (cand_before<MEASURE>(c, list[j])) {
            const Cand t = list[j];
            list[j] = c;
            c = t;
        }
    }
}

template <int MEASURE>
__device__ __forceinline__ Cand cand_of(uint32_t I, uint32_t na, uint32_t nb, int b) {
    return Cand{I, MEASURE == SAEV_COACT_JACCARD ? na + nb - I : nb, b};
}

// The threads' sorted lists merged into the latent's top_m: per rank a workgroup-wide argmax of the lists' heads; the thread that
// held the winner (a b sits in one thread's list only) drops it.  Ranks past the last candidate are padded with -1 / 0
template <int MEASURE, int THREADS>
__device__ __forceinline__ void cand_merge_out(Cand (&list)[COACT_LIST], int top_m, int32_t* __restrict__ out_index, int32_t* __restrict__ out_inter) {
    __shared__ uint32_t head_I[THREADS / 64], head_x[THREADS / 64];
    __shared__ int head_b[THREADS / 64];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    for (int r = 0; r < top_m; ++r) {
        Cand best = list[0];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            Cand other;
            other.I = __shfl_xor(best.I, o, 64);
            other.x = __shfl_xor(best.x, o, 64);
            other.b = __shfl_xor(best.b, o, 64);
            if (cand_before<MEASURE>(other, best)) best = other;
        }
        if (lane == 0) { head_I[w] = best.I; head_x[w] = best.x; head_b[w] = best.b; }
        __syncthreads();
        best = Cand{head_I[0], head_x[0], head_b[0]};
        for (int q = 1; q < THREADS / 64; ++q) {
            const Cand other{head_I[q], head_x[q], head_b[q]};
            if (cand_before<MEASURE>(other, best)) best = other;
        }
        __syncthreads();
        if (best.I != 0 && list[0].I != 0 && list[0].b == best.b) {
#pragma unroll
            for (int j = 0; j + 1 < COACT_LIST; ++j) list[j] = list[j + 1];
            list[COACT_LIST - 1] = cand_none();
        }
        if (t == 0) {
            out_index[r] = best.I != 0 ? best.b : -1;
            out_inter[r] = (int32_t)best.I;
        }
    }
}

// ---------------------------------------------------------------- count, scan, place -----------------------------------------------

// lanes of a lane group for rows of `avg` stored entries: a power of two in [8, 64]
int lanes_for(int64_t nnz, int64_t n_rows) {
    const int64_t avg = nnz / std::max<int64_t>(n_rows, 1);
    return avg <= 8 ? 8 : avg <= 16 ? 16 : avg <= 32 ? 32 : 64;
}

// a lane group of G lanes per row.  PLACE == 0: cnt[col] += 1 for every entry with value > thr, and every stored entry is checked.
// PLACE == 1: the row is written at cursor[col]++ (cursor starts at the latent's offset; the counts of this call sized the list)
template <int PLACE>
__global__ __launch_bounds__(256) void coact_rows_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                                         const float* __restrict__ data, int64_t nnz, int N, int S, float thr, int G,
                                                         int32_t* __restrict__ cnt_or_cursor, int32_t* __restrict__ rows_out,
                                                         int32_t* __restrict__ err) {
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t groups = (int64_t)gridDim.x * 256 / G;
    const int sub = (int)(gid % G);
    int bad = 0;
    for (int64_t r = gid / G; r < N; r += groups) {
        const int64_t e0 = indptr[r], e1 = indptr[r + 1];
        if (e0 < 0 || e1 < e0 || e1 > nnz) { bad = SAEV_COACT_ERR_INDPTR; continue; }
        for (int64_t e = e0 + sub; e < e1; e += G) {
            const int col = indices[e];
            const float v = data[e];
            if ((unsigned)col >= (unsigned)S) { bad = max(bad, SAEV_COACT_ERR_COLUMN); continue; }
            if (!(fabsf(v) <= 3.402823466e38f)) { bad = max(bad, SAEV_COACT_ERR_VALUE); continue; }
            if (!(v > thr)) continue;
            if (PLACE) {
                // (an indptr that steps back makes rows overlap and the events outnumber nnz: reported by the count pass, kept in bounds here)
                const int at = atomicAdd(&cnt_or_cursor[col], 1);
                if (at >= 0 && at < nnz) rows_out[at] = (int32_t)r;
            }
            else atomicAdd(&cnt_or_cursor[col], 1);
        }
    }
    if (!PLACE && bad) atomicMax(err, bad);
}

// start[l] = the events of the latents before l (start[Sa] = all of them), cursor = a copy for the placement; the heavy list
// (heavy_count[0] latents) and its chunks (heavy_count[1] work items)
__global__ __launch_bounds__(1024) void coact_scan_kernel(const int32_t* __restrict__ n_a, int Sa, int32_t* __restrict__ start,
                                                          int32_t* __restrict__ cursor, int32_t* __restrict__ heavy_count,
                                                          int32_t* __restrict__ heavy_ids, int max_heavy, int2* __restrict__ items,
                                                          int max_items) {
    if (threadIdx.x == 0) { heavy_count[0] = 0; heavy_count[1] = 0; }
    __syncthreads();
    const int total = block_scan_rounds<1024, int, int>(
        Sa, [&](int l) { return n_a[l]; },
        [&](int l, int s) {
            start[l] = s;
            cursor[l] = s;
            if (n_a[l] > COACT_CHUNK_ROWS) {
                const int h = atomicAdd(heavy_count, 1);
                if (h < max_heavy) heavy_ids[h] = l;  // (always: the counts sum to at most nnz_a)
                // the latent's chunks join the work list of the heavy walk: {position in the heavy list, chunk}
                const int nc = (n_a[l] + COACT_CHUNK_ROWS - 1) / COACT_CHUNK_ROWS;
                const int at = atomicAdd(heavy_count + 1, nc);
                for (int c = 0; c < nc && at + c < max_items; ++c) items[at + c] = make_int2(h, c);
            }
        });
    if (threadIdx.x == 0) start[Sa] = total;
}

// ---------------------------------------------------------------- the walk ----------------------------------------------------------

struct CoactB {
    const int64_t* indptr;
    const int32_t* indices;
    const float* data;
    int64_t nnz;
    int S;
    float thr;
    int G;  // lanes per row of B
};

// how many of the n rows of a list that starts at `start` lie inside the event list of `cap` entries: all of them, unless the input was
// broken (overlapping rows: more events than stored entries, sums past 2^31)
__device__ __forceinline__ int coact_list_len(int64_t start, int64_t n, int64_t cap) {
    if (start < 0 || n <= 0 || start >= cap) return 0;
    return (int)min(n, cap - start);
}

// cnt[0, len) += the rows of `rows[0, n)` in which latent lo + i of B fires; the caller zeroed cnt and synchronises after
template <int THREADS>
__device__ __forceinline__ void coact_walk_rows(const CoactB& B, const int32_t* __restrict__ rows, int n, int lo, int len, uint32_t* cnt) {
    const int G = B.G;
    const int sub = threadIdx.x % G;
    for (int i = threadIdx.x / G; i < n; i += THREADS / G) {
        const int r = rows[i];
        const int64_t e0 = B.indptr[r], e1 = B.indptr[r + 1];
        if (e0 < 0 || e1 < e0 || e1 > B.nnz) continue;  // (the count pass has reported it)
        for (int64_t e = e0 + sub; e < e1; e += G) {
            const unsigned c = (unsigned)(B.indices[e] - lo);
            if (c < (unsigned)len && B.data[e] > B.thr) atomicAdd(&cnt[c], 1u);
        }
    }
}

// Light latents: workgroup a walks a's whole list, window after window, and ranks.  self: b == a is no partner
template <int MEASURE, int WIN, int THREADS>
__global__ __launch_bounds__(THREADS) void coact_walk_kernel(CoactB B, const int32_t* __restrict__ n_a, const int32_t* __restrict__ n_b,
                                                             const int32_t* __restrict__ start, const int32_t* __restrict__ rows,
                                                             int64_t list_cap, int Sa, int self, int top_m, int32_t* __restrict__ out_index,
                                                             int32_t* __restrict__ out_inter) {
    __shared__ uint32_t cnt[WIN];
    const int t = threadIdx.x;
    for (int64_t a64 = blockIdx.x; a64 < Sa; a64 += gridDim.x) {  // (every branch below is the whole workgroup's)
        const int a = (int)a64;
        const int na = n_a[a];
        if (na > COACT_CHUNK_ROWS) continue;  // the heavy route writes its outputs
        int32_t* oi = out_index + (size_t)a * top_m;
        int32_t* ox = out_inter + (size_t)a * top_m;
        const int n_rows = coact_list_len(start[a], na, list_cap);
        if (n_rows <= 0) {
            if (t < top_m) { oi[t] = -1; ox[t] = 0; }
            continue;
        }
        const int32_t* my_rows = rows + start[a];
        Cand list[COACT_LIST];
#pragma unroll
        for (int j = 0; j < COACT_LIST; ++j) list[j] = cand_none();
        for (int lo = 0; lo < B.S; lo += WIN) {
            const int len = min(WIN, B.S - lo);
            for (int i = t; i < len; i += THREADS) cnt[i] = 0u;
            __syncthreads();
            coact_walk_rows<THREADS>(B, my_rows, n_rows, lo, len, cnt);
            __syncthreads();
            for (int i = t; i < len; i += THREADS) {
                const uint32_t I = cnt[i];
                const int b = lo + i;
                if (I != 0 && !(self && b == a)) cand_insert<MEASURE>(list, cand_of<MEASURE>(I, (uint32_t)na, (uint32_t)n_b[b], b));
            }
            __syncthreads();
        }
        cand_merge_out<MEASURE, THREADS>(list, top_m, oi, ox);
    }
}

// Heavy latents, round `base / COACT_SLOTS`: slot y holds heavy latent base + y.  The slot's counter row is zeroed ...
__global__ __launch_bounds__(256) void coact_heavy_clear_kernel(const int32_t* __restrict__ heavy_count, int base, int Sb, int32_t* __restrict__ grow) {
    if (base + (int)blockIdx.y >= *heavy_count) return;
    int32_t* row = grow + (size_t)blockIdx.y * Sb;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < Sb; i += (int64_t)gridDim.x * 256) row[i] = 0;
}

// ... the workgroups share out the work items of the round's latents: a chunk of a list is walked and its counters added to the row ...
template <int WIN, int THREADS>
__global__ __launch_bounds__(THREADS) void coact_heavy_walk_kernel(CoactB B, const int32_t* __restrict__ n_a, const int32_t* __restrict__ start,
                                                                   const int32_t* __restrict__ rows, const int32_t* __restrict__ heavy_count,
                                                                   const int32_t* __restrict__ heavy_ids, const int2* __restrict__ items,
                                                                   int max_items, int base, int slots, int64_t list_cap, int32_t* __restrict__ grow) {
    __shared__ uint32_t cnt[WIN];
    const int t = threadIdx.x;
    const int n_items = min(heavy_count[1], max_items);
    for (int w = blockIdx.x; w < n_items; w += gridDim.x) {  // (every branch below is the whole workgroup's)
        const int2 item = items[w];
        const int slot = item.x - base;
        if (slot < 0 || slot >= slots) continue;
        const int a = heavy_ids[item.x];
        const int na = n_a[a];
        const int64_t first = (int64_t)item.y * COACT_CHUNK_ROWS;
        if (first >= na) continue;
        const int n = coact_list_len(start[a] + first, min((int64_t)COACT_CHUNK_ROWS, na - first), list_cap);
        if (n <= 0) continue;
        const int32_t* my_rows = rows + start[a] + first;
        int32_t* row = grow + (size_t)slot * B.S;
        for (int lo = 0; lo < B.S; lo += WIN) {
            const int len = min(WIN, B.S - lo);
            for (int i = t; i < len; i += THREADS) cnt[i] = 0u;
            __syncthreads();
            coact_walk_rows<THREADS>(B, my_rows, n, lo, len, cnt);
            __syncthreads();
            for (int i = t; i < len; i += THREADS) {
                const uint32_t I = cnt[i];
                if (I != 0) atomicAdd(&row[lo + i], (int32_t)I);
            }
            __syncthreads();
        }
    }
}

// ... and one workgroup per slot ranks the finished row
template <int MEASURE>
__global__ __launch_bounds__(256) void coact_heavy_rank_kernel(const int32_t* __restrict__ n_a, const int32_t* __restrict__ n_b, int Sb,
                                                               const int32_t* __restrict__ heavy_count, const int32_t* __restrict__ heavy_ids,
                                                               int base, const int32_t* __restrict__ grow, int self, int top_m,
                                                               int32_t* __restrict__ out_index, int32_t* __restrict__ out_inter) {
    if (base + (int)blockIdx.x >= *heavy_count) return;
    const int a = heavy_ids[base + blockIdx.x];
    const uint32_t na = (uint32_t)n_a[a];
    const int32_t* row = grow + (size_t)blockIdx.x * Sb;
    Cand list[COACT_LIST];
#pragma unroll
    for (int j = 0; j < COACT_LIST; ++j) list[j] = cand_none();
    for (int b = threadIdx.x; b < Sb; b += 256) {
        const uint32_t I = (uint32_t)row[b];
        if (I != 0 && !(self && b == a)) cand_insert<MEASURE>(list, cand_of<MEASURE>(I, na, (uint32_t)n_b[b], b));
    }
    cand_merge_out<MEASURE, 256>(list, top_m, out_index + (size_t)a * top_m, out_inter + (size_t)a * top_m);
}

// ---------------------------------------------------------------- host --------------------------------------------------------------

struct CoactLayout {
    int64_t off_start, off_cursor, off_rows, off_heavy_count, off_heavy_ids, off_items, off_grow, total;
    int64_t max_heavy, max_items, slots;
};

bool coact_shape_ok(int64_t N, int64_t Sa, int64_t Sb, int64_t nnz_a, int64_t nnz_b) {
    const int64_t top = 0x7fffffffLL;
    return N >= 1 && N <= top && Sa >= 1 && Sa <= top && Sb >= 1 && Sb <= top && nnz_a >= 0 && nnz_a <= top && nnz_b >= 0 && nnz_b <= top;
}

CoactLayout coact_layout(int64_t Sa, int64_t Sb, int64_t nnz_a) {
    CoactLayout L;
    // a heavy latent has more than COACT_CHUNK_ROWS firing entries, and all latents together at most nnz_a
    L.max_heavy = std::min<int64_t>(Sa, nnz_a / (COACT_CHUNK_ROWS + 1));
    L.slots = std::min<int64_t>(L.max_heavy, COACT_SLOTS);
    // the chunks of the heavy latents: sum of ceil(n / chunk) <= nnz_a / chunk + their number
    L.max_items = L.max_heavy == 0 ? 0 : nnz_a / COACT_CHUNK_ROWS + L.max_heavy;
    WsCarve c;
    L.off_start = c.take((Sa + 1) * 4);
    L.off_cursor = c.take(Sa * 4);
    L.off_rows = c.take(nnz_a * 4);
    L.off_heavy_count = c.take(8);
    L.off_heavy_ids = c.take(L.max_heavy * 4);
    L.off_items = c.take(L.max_items * 8);
    L.off_grow = c.take(L.slots * Sb * 4);
    L.total = c.at;
    return L;
}

template <int MEASURE, int WIN, int THREADS>
void coact_launch(const CoactB& B, int64_t N, int64_t Sa, int64_t nnz_a, const CoactLayout& L, char* ws, const int32_t* n_a, const int32_t* n_b,
                  int self, int top_m, int32_t* out_index, int32_t* out_inter, hipStream_t s) {
    const int32_t* start = (const int32_t*)(ws + L.off_start);
    const int32_t* rows = (const int32_t*)(ws + L.off_rows);
    const int32_t* heavy_count = (const int32_t*)(ws + L.off_heavy_count);
    const int32_t* heavy_ids = (const int32_t*)(ws + L.off_heavy_ids);
    int32_t* grow = (int32_t*)(ws + L.off_grow);
    hipLaunchKernelGGL((coact_walk_kernel<MEASURE, WIN, THREADS>), dim3((unsigned)std::min<int64_t>(Sa, 1 << 20)), dim3(THREADS), 0, s, B, n_a, n_b, start, rows,
                       nnz_a, (int)Sa, self, top_m,
                       out_index, out_inter);
    if (L.slots == 0) return;
    const int2* items = (const int2*)(ws + L.off_items);
    // persistent workgroups over the work list: a launch that finds no heavy latent costs its few hundred workgroups' start-up
    const unsigned walkers = (unsigned)std::min<int64_t>(L.max_items, 256 * (131072 / (WIN * 4)));
    const unsigned clear_x = (unsigned)std::min<int64_t>((B.S + 2047) / 2048, 1024);
    for (int64_t base = 0; base < L.max_heavy; base += L.slots) {
        const unsigned slots = (unsigned)std::min<int64_t>(L.slots, L.max_heavy - base);
        hipLaunchKernelGGL(coact_heavy_clear_kernel, dim3(clear_x, slots), dim3(256), 0, s, heavy_count, (int)base, B.S, grow);
        hipLaunchKernelGGL((coact_heavy_walk_kernel<WIN, THREADS>), dim3(walkers), dim3(THREADS), 0, s, B, n_a, start, rows, heavy_count,
                           heavy_ids, items, (int)L.max_items, (int)base, (int)slots, nnz_a, grow);
        hipLaunchKernelGGL(coact_heavy_rank_kernel<MEASURE>, dim3(slots), dim3(256), 0, s, n_a, n_b, B.S, heavy_count, heavy_ids, (int)base, grow,
                           self, top_m, out_index, out_inter);
    }
}

}  // namespace

int64_t saev_coactivation_chunk_rows(void) { return COACT_CHUNK_ROWS; }
int64_t saev_coactivation_window(void) { return COACT_WINDOW; }
int64_t saev_coactivation_slots(void) { return COACT_SLOTS; }

int64_t saev_coactivation_workspace_bytes(int64_t N, int64_t Sa, int64_t Sb, int64_t nnz_a, int64_t nnz_b) {
    if (!coact_shape_ok(N, Sa, Sb, nnz_a, nnz_b)) return -1;
    return coact_layout(Sa, Sb, nnz_a).total;
}

int saev_coactivation(const int64_t* a_indptr, const int32_t* a_indices, const float* a_data, int64_t nnz_a, int64_t Sa,
                      const int64_t* b_indptr, const int32_t* b_indices, const float* b_data, int64_t nnz_b, int64_t Sb, int64_t N,
                      float thr_a, float thr_b, int32_t measure, int32_t top_m, int32_t* n_a, int32_t* n_b, int32_t* out_index,
                      int32_t* out_inter, int32_t* err, void* workspace, int64_t workspace_bytes, void* stream) {
    const char* who = "saev_coactivation";
    const bool self = b_indptr == nullptr;
    if (self) { Sb = Sa; nnz_b = nnz_a; thr_b = thr_a; }
    if (N < 0 || Sa < 0 || Sb < 0 || nnz_a < 0 || nnz_b < 0) return entry_refuse(SAEV_INVALID_ARG, who, "negative size");
    const int64_t top = 0x7fffffffLL;
    if (N > top || Sa > top || Sb > top || nnz_a > top || nnz_b > top) return entry_refuse(SAEV_UNSUPPORTED, who, "N, Sa, Sb and both nnz must stay below 2^31");
    if (N < 1 || Sa < 1 || Sb < 1) return entry_refuse(SAEV_INVALID_ARG, who, "N, Sa and Sb must be at least 1");
    if (top_m < 1 || top_m > COACT_LIST) return entry_refuse(SAEV_INVALID_ARG, who, "top_m must lie in [1, 8]");
    if (measure != SAEV_COACT_JACCARD && measure != SAEV_COACT_CONTAINMENT)
        return entry_refuse(SAEV_INVALID_ARG, who, "measure is SAEV_COACT_JACCARD or SAEV_COACT_CONTAINMENT");
    if (!a_indptr || !n_a || !out_index || !out_inter || !err) return entry_refuse(SAEV_INVALID_ARG, who, "a_indptr, n_a, out_index, out_inter and err must not be NULL");
    if (nnz_a > 0 && (!a_indices || !a_data)) return entry_refuse(SAEV_INVALID_ARG, who, "a_indices and a_data come with nnz_a > 0");
    if (!self && !n_b) return entry_refuse(SAEV_INVALID_ARG, who, "n_b comes with B");
    if (!self && nnz_b > 0 && (!b_indices || !b_data)) return entry_refuse(SAEV_INVALID_ARG, who, "b_indices and b_data come with nnz_b > 0");
    const CoactLayout L = coact_layout(Sa, Sb, nnz_a);
    if (int rc = entry_check_workspace(who, workspace, workspace_bytes, L.total, "workspace smaller than saev_coactivation_workspace_bytes"); rc != SAEV_OK)
        return rc;

    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    int32_t* start = (int32_t*)(ws + L.off_start);
    int32_t* cursor = (int32_t*)(ws + L.off_cursor);
    int32_t* rows = (int32_t*)(ws + L.off_rows);
    if (hipMemsetAsync(err, 0, 4, s) != hipSuccess || hipMemsetAsync(n_a, 0, (size_t)Sa * 4, s) != hipSuccess ||
        (!self && hipMemsetAsync(n_b, 0, (size_t)Sb * 4, s) != hipSuccess))
        return entry_refuse(SAEV_HIP_ERROR, who, "hipMemsetAsync failed");
    const int Ga = lanes_for(nnz_a, N);
    const auto row_grid = [&](int G) { return dim3((unsigned)std::min<int64_t>((N * G + 255) / 256, 16384)); };
    hipLaunchKernelGGL(coact_rows_kernel<0>, row_grid(Ga), dim3(256), 0, s, a_indptr, a_indices, a_data, nnz_a, (int)N, (int)Sa, thr_a, Ga, n_a,
                       (int32_t*)nullptr, err);
    CoactB B{a_indptr, a_indices, a_data, nnz_a, (int)Sa, thr_a, Ga};
    if (!self) {
        const int Gb = lanes_for(nnz_b, N);
        hipLaunchKernelGGL(coact_rows_kernel<0>, row_grid(Gb), dim3(256), 0, s, b_indptr, b_indices, b_data, nnz_b, (int)N, (int)Sb, thr_b, Gb, n_b,
                           (int32_t*)nullptr, err);
        B = CoactB{b_indptr, b_indices, b_data, nnz_b, (int)Sb, thr_b, Gb};
    }
    hipLaunchKernelGGL(coact_scan_kernel, dim3(1), dim3(1024), 0, s, n_a, (int)Sa, start, cursor, (int32_t*)(ws + L.off_heavy_count),
                       (int32_t*)(ws + L.off_heavy_ids), (int)L.max_heavy, (int2*)(ws + L.off_items), (int)L.max_items);
    hipLaunchKernelGGL(coact_rows_kernel<1>, row_grid(Ga), dim3(256), 0, s, a_indptr, a_indices, a_data, nnz_a, (int)N, (int)Sa, thr_a, Ga, cursor,
                       rows, err);
    const int32_t* nb = self ? n_a : n_b;
#define COACT_GO(M)                                                                                                                       \
    do {                                                                                                                               \
        if (Sb <= COACT_SMALL_WINDOW) coact_launch<M, COACT_SMALL_WINDOW, 256>(B, N, Sa, nnz_a, L, ws, n_a, nb, self, top_m, out_index, out_inter, s); \
        else if (Sb <= COACT_MID_WINDOW) coact_launch<M, COACT_MID_WINDOW, 512>(B, N, Sa, nnz_a, L, ws, n_a, nb, self, top_m, out_index, out_inter, s); \
        else coact_launch<M, COACT_WINDOW, 1024>(B, N, Sa, nnz_a, L, ws, n_a, nb, self, top_m, out_index, out_inter, s);                \
    } while (0)
    if (measure == SAEV_COACT_JACCARD) COACT_GO(SAEV_COACT_JACCARD);
    else COACT_GO(SAEV_COACT_CONTAINMENT);
#undef COACT_GO
    if (hipGetLastError() != hipSuccess) return entry_refuse(SAEV_HIP_ERROR, who, "kernel launch failed");
    return SAEV_OK;
}
