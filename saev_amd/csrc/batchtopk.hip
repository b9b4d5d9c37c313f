// BatchTopK activation (reference nn/modeling.py:183-244): the batch-wide select over a dense h (n x S fp32) and the compaction of
// the kept entries into padded rows.  Everything is exact and deterministic: order-preserving unsigned keys (common.h: f2ukey, with
// -0 read as +0 so that equal VALUES have equal keys), integer counts, integer atomics only.
//
// SELECT: the exact key of the T-th largest entry, T = min(n top_k, n S).  An MSB radix select in three levels of 12 / 12 / 8 key bits,
// of which only the first reads h as a whole in the usual case:
//   btk_hist_kernel (level 0)   per-workgroup LDS histogram of the 12 high key bits, flushed with integer atomics
//   btk_scan_kernel             one workgroup: the bin that holds the T-th largest, the count above it, the rank left inside it
//   btk_gather_kernel           second pass over h: the KEYS of the cut bin's entries into a list (staged in LDS, one global atomic per
//                               flush).  The list has a fixed capacity; its counter keeps counting past it
//   btk_hist_kernel (1, 2)      the next 12 and the last 8 bits, over the list -- or, when the cut bin held more entries than the list
//                               does (values crowded into one eighth of an octave), over h again with the prefix as a filter: slower,
//                               never wrong.  The choice is made on the device from the counter
// It leaves {cut key, cut value, entries strictly above, tie quota = how many entries EQUAL to the cut are kept, entries equal to it}
// in the state words; nothing is read back.
//
// COMPACTION: one wave per row sweeps it in ascending 256-latent chunks, four coalesced dwords per lane; ballots give every kept entry
// its slot, so a row's entries come out in ascending latent order (the Matryoshka decode and the inference CSR rely on it).  Training
// mode keeps key >= cut and counts the row's ties; eval mode keeps h > threshold (h > 0 when threshold <= 0), strictly.  Counts run
// on past row_cap (only the first row_cap entries are stored) and the largest overflowing count is atomicMax'ed into a device word.
// Ties (training): lower flat index first.  btk_tie_scan_kernel turns the per-row tie counts into how many ties each row keeps (an
// exclusive scan over n rows against the quota), btk_tie_drop_kernel re-compacts the few rows that keep fewer than they hold, in their
// n x row_cap output, not in h.  Slots past a row's count hold idx = -1, val = 0.
// btk_ema_kernel: threshold <- (1 - m) threshold + m min{f > 0 kept}, rounded as torch's mul_ / add_ round it; skipped when nothing
// positive was kept, and when a row overflowed (the caller repeats such a forward with larger rows: the update then happens once).
#include <algorithm>

#include "common.h"
#include "kernels.h"

namespace {

constexpr int BTK_THREADS = 256;
constexpr int BTK_GBUF = 4096;  // staged keys per workgroup of the gather (a tile adds at most 1024)

__device__ __forceinline__ uint32_t btk_key(float f) {
    uint32_t b = __float_as_uint(f);
    if (b == 0x80000000u) b = 0u;  // -0 == +0
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// bits of the key a level histograms, and the prefix an entry must carry to belong to the level
__device__ __forceinline__ bool btk_level_bin(uint32_t key, int level, uint32_t prefix, uint32_t* bin) {
    if (level == 0) { *bin = key >> 20; return true; }
    if (level == 1) { *bin = (key >> 8) & 0xfffu; return (key >> 20) == prefix; }
    *bin = key & 0xffu;
    return (key >> 8) == prefix;
}

__global__ __launch_bounds__(BTK_THREADS) void btk_hist_kernel(const float* __restrict__ h, size_t n4, int level, const uint32_t* st,
                                                                const uint32_t* __restrict__ list, uint32_t list_cap, uint32_t* hist) {
    __shared__ uint32_t lh[BTK_BINS];
    const int tid = threadIdx.x;
    const int nb = level == 2 ? 256 : BTK_BINS;
    for (int i = tid; i < nb; i += BTK_THREADS) lh[i] = 0u;
    __syncthreads();
    const uint32_t prefix = level == 0 ? 0u : st[BTK_ST_PREFIX];
    const uint32_t n_list = level == 0 ? 0u : st[BTK_ST_LIST];
    if (level > 0 && n_list <= list_cap) {
        // every key of the list carries the level-1 prefix already
        for (size_t i = (size_t)blockIdx.x * BTK_THREADS + tid; i < n_list; i += (size_t)gridDim.x * BTK_THREADS) {
            uint32_t bin;
            if (btk_level_bin(list[i], level, prefix, &bin)) atomicAdd(&lh[bin], 1u);
        }
    } else {
        const f32x4* h4 = reinterpret_cast<const f32x4*>(h);
        for (size_t q = (size_t)blockIdx.x * BTK_THREADS + tid; q < n4; q += (size_t)gridDim.x * BTK_THREADS) {
            const f32x4 v = h4[q];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                uint32_t bin;
                if (btk_level_bin(btk_key(v[e]), level, prefix, &bin)) atomicAdd(&lh[bin], 1u);
            }
        }
    }
    __syncthreads();
    uint32_t* out = hist + (size_t)level * BTK_BINS;
    for (int i = tid; i < nb; i += BTK_THREADS)
        if (lh[i] != 0u) atomicAdd(&out[i], lh[i]);
}

// One workgroup of 1024 threads: thread t owns the four bins 4 (1023 - t) + 3 ... 4 (1023 - t), i.e. ascending t = descending keys.
// The bin b with  count(bins > b) < rank <= count(bins >= b)  holds the entry of that rank.
__global__ __launch_bounds__(1024) void btk_scan_kernel(int level, uint32_t* st, const uint32_t* hist, uint32_t target) {
    __shared__ uint32_t wave_tot[16];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const uint32_t* hl = hist + (size_t)level * BTK_BINS;
    const int top = 4 * (1023 - t) + 3;
    uint32_t c[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) c[j] = hl[top - j];
    const uint32_t tot = c[0] + c[1] + c[2] + c[3];
    uint32_t incl = tot;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t nbr = __shfl_up(incl, o, 64);
        if (lane >= o) incl += nbr;
    }
    if (lane == 63) wave_tot[w] = incl;
    __syncthreads();
    uint32_t off = 0;
    for (int j = 0; j < w; ++j) off += wave_tot[j];
    incl += off;
    const uint32_t excl = incl - tot;
    const uint32_t rank = level == 0 ? target : st[BTK_ST_RANK];  // (every thread reads it before the one below writes: see the barrier)
    __syncthreads();
    if (excl < rank && rank <= incl) {
        uint32_t run = excl;
        int bin = top;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (rank <= run + c[j]) { bin = top - j; break; }
            run += c[j];
        }
        const uint32_t bits = level == 2 ? 8u : 12u;
        const uint32_t prefix = level == 0 ? (uint32_t)bin : ((st[BTK_ST_PREFIX] << bits) | (uint32_t)bin);
        st[BTK_ST_PREFIX] = prefix;
        st[BTK_ST_ABOVE] = (level == 0 ? 0u : st[BTK_ST_ABOVE]) + run;
        st[BTK_ST_RANK] = rank - run;
        if (level == 0) { st[BTK_ST_LIST] = 0u; st[BTK_ST_MINPOS] = 0x7f800000u; }
        if (level == 2) {
            st[BTK_ST_TIES] = hl[bin];
            const uint32_t k = prefix;
            st[BTK_ST_CUT] = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;  // the cut VALUE's bits (ukey2f)
        }
    }
}

__global__ __launch_bounds__(BTK_THREADS) void btk_gather_kernel(const float* __restrict__ h, size_t n4, uint32_t* st, uint32_t* list,
                                                                  uint32_t list_cap) {
    __shared__ uint32_t buf[BTK_GBUF];
    __shared__ uint32_t cnt, base;
    const int tid = threadIdx.x;
    if (tid == 0) cnt = 0u;
    __syncthreads();
    const uint32_t prefix = st[BTK_ST_PREFIX];
    const f32x4* h4 = reinterpret_cast<const f32x4*>(h);
    auto flush = [&](uint32_t m) {  // (called by all threads at once with the same m = cnt)
        if (tid == 0 && m != 0u) base = atomicAdd(&st[BTK_ST_LIST], m);
        __syncthreads();
        for (uint32_t i = tid; i < m; i += BTK_THREADS)
            if (base + i < list_cap) list[base + i] = buf[i];
        __syncthreads();
        if (tid == 0) cnt = 0u;
        __syncthreads();
    };
    const size_t n_tiles = (n4 + BTK_THREADS - 1) / BTK_THREADS;
    for (size_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const size_t q = tile * BTK_THREADS + tid;
        if (q < n4) {
            const f32x4 v = h4[q];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const uint32_t key = btk_key(v[e]);
                if ((key >> 20) == prefix) buf[atomicAdd(&cnt, 1u)] = key;
            }
        }
        __syncthreads();
        const uint32_t m = cnt;
        __syncthreads();  // (nobody appends to the next tile before everybody has read the count)
        if (m > BTK_GBUF - 4 * BTK_THREADS) flush(m);
    }
    __syncthreads();
    flush(cnt);
}

// One wave per row.  Column of lane l, sub-load e of chunk c: 256 c + 64 e + l -- four coalesced dword loads per chunk; the slot of a
// kept entry is the row's running count + the kept entries of sub-loads before e + those of lower lanes in e.
__global__ __launch_bounds__(BTK_THREADS) void btk_compact_kernel(BtkCompactArgs a) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * (BTK_THREADS / 64) + (threadIdx.x >> 6);
    if (row >= a.n_rows) return;
    const int S = a.S, cap = a.row_cap;
    const float* hr = a.h + (size_t)row * S;
    int32_t* ir = a.idx_out + (size_t)row * cap;
    float* vr = a.val_out + (size_t)row * cap;
    const uint32_t cut = a.training ? a.st[BTK_ST_PREFIX] : 0u;
    float thr = 0.f;
    if (!a.training) { thr = *a.threshold; if (!(thr > 0.f)) thr = 0.f; }
    const unsigned long long lt = (1ull << lane) - 1ull;
    int run = 0, ties = 0;
    uint32_t minpos = 0x7f800000u;
    for (int c0 = 0; c0 < S; c0 += 256) {
        float v[4];
        bool keep[4];
        unsigned long long m[4];
        bool any = false;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int col = c0 + 64 * e + lane;
            v[e] = col < S ? hr[col] : 0.f;
            bool k, tie = false;
            if (a.training) { const uint32_t key = btk_key(v[e]); k = key >= cut; tie = key == cut; }
            else k = v[e] > thr;
            k = k && col < S;
            tie = tie && col < S;
            keep[e] = k;
            m[e] = __ballot(k);
            any = any || m[e] != 0ull;
            if (a.training) ties += __popcll(__ballot(tie));
        }
        if (!any) continue;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (keep[e]) {
                const int pos = run + __popcll(m[e] & lt);
                if (pos < cap) { ir[pos] = c0 + 64 * e + lane; vr[pos] = v[e]; }
                if (v[e] > 0.f) minpos = min(minpos, __float_as_uint(v[e]));
            }
            run += __popcll(m[e]);
        }
    }
    for (int j = min(run, cap) + lane; j < cap; j += 64) { ir[j] = -1; vr[j] = 0.f; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) minpos = min(minpos, (uint32_t)__shfl_xor((int)minpos, o, 64));
    if (lane == 0) {
        a.row_nnz_out[row] = run;  // (training: ties included until btk_tie_scan_kernel has its say)
        if (a.training) {
            a.row_ties[row] = ties;
            if (minpos != 0x7f800000u) atomicMin(&a.st[BTK_ST_MINPOS], minpos);
        }
        if (run > cap) atomicMax(a.overflow, run);
    }
}

// keep_ties[b] = clamp(quota - ties in rows before b, 0, ties[b]); row_nnz[b] -= ties[b] - keep_ties[b].  One workgroup.
__global__ __launch_bounds__(1024) void btk_tie_scan_kernel(const uint32_t* st, int n_rows, const int32_t* row_ties, int32_t* keep_ties,
                                                            int32_t* row_nnz) {
    __shared__ uint32_t wave_tot[16];
    __shared__ uint32_t carry_s;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const uint32_t quota = st[BTK_ST_RANK];
    if (t == 0) carry_s = 0u;
    __syncthreads();
    for (int b0 = 0; b0 < n_rows; b0 += 1024) {
        const int b = b0 + t;
        const uint32_t c = b < n_rows ? (uint32_t)row_ties[b] : 0u;
        uint32_t incl = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t nbr = __shfl_up(incl, o, 64);
            if (lane >= o) incl += nbr;
        }
        if (lane == 63) wave_tot[w] = incl;
        __syncthreads();
        uint32_t off = carry_s;
        for (int j = 0; j < w; ++j) off += wave_tot[j];
        const uint32_t before = off + incl - c;
        if (b < n_rows) {
            const uint32_t keep = before >= quota ? 0u : min(c, quota - before);
            keep_ties[b] = (int32_t)keep;
            row_nnz[b] -= (int32_t)(c - keep);
        }
        __syncthreads();
        if (t == 1023) carry_s = off + incl;
        __syncthreads();
    }
}

// One wave per row: rows that keep all their ties (nearly all rows) return at once; the others drop every tie past the first
// keep_ties[b] from their stored entries, in place (a slot is written only after it has been read: output slots never run ahead).
__global__ __launch_bounds__(BTK_THREADS) void btk_tie_drop_kernel(const uint32_t* st, int n_rows, int row_cap, const int32_t* row_ties,
                                                                   const int32_t* keep_ties, const int32_t* row_nnz, int32_t* idx,
                                                                   float* val) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * (BTK_THREADS / 64) + (threadIdx.x >> 6);
    if (row >= n_rows) return;
    const int nt = row_ties[row], kt = keep_ties[row];
    if (kt == nt) return;
    const uint32_t cut = st[BTK_ST_PREFIX];
    const int stored = min(row_nnz[row] + (nt - kt), row_cap);  // what btk_compact_kernel stored of this row
    int32_t* ir = idx + (size_t)row * row_cap;
    float* vr = val + (size_t)row * row_cap;
    const unsigned long long lt = (1ull << lane) - 1ull;
    int out = 0, seen = 0;
    for (int j0 = 0; j0 < stored; j0 += 64) {
        const int j = j0 + lane;
        const bool have = j < stored;
        const int32_t i = have ? ir[j] : -1;
        const float v = have ? vr[j] : 0.f;
        const bool tie = have && btk_key(v) == cut;
        const unsigned long long tm = __ballot(tie);
        const bool keep = have && (!tie || seen + __popcll(tm & lt) < kt);
        const unsigned long long km = __ballot(keep);
        if (keep) { const int pos = out + __popcll(km & lt); ir[pos] = i; vr[pos] = v; }
        out += __popcll(km);
        seen += __popcll(tm);
    }
    for (int j = out + lane; j < stored; j += 64) { ir[j] = -1; vr[j] = 0.f; }
}

__global__ void btk_ema_kernel(const uint32_t* st, const int32_t* overflow, float* threshold, float one_minus_m, float m) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (*overflow != 0) return;                    // the caller repeats this forward: the update belongs to the repetition
    const uint32_t mp = st[BTK_ST_MINPOS];
    if (mp == 0x7f800000u) return;                 // nothing positive was kept: the threshold stays (the reference would raise)
    const float t1 = __fmul_rn(*threshold, one_minus_m);
    const float t2 = __fmul_rn(m, __uint_as_float(mp));
    *threshold = __fadd_rn(t1, t2);
}

}  // namespace

// the eval-mode compaction alone (h > max(*threshold, 0)) into rows of any capacity: a.training must be 0, a.st / a.row_ties are not read
hipError_t launch_threshold_compact(const BtkCompactArgs& a, hipStream_t s) {
    if (a.n_rows <= 0) return hipSuccess;
    if (a.training != 0) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(a.overflow, 0, sizeof(int32_t), s);
    if (e != hipSuccess) return e;
    const int row_blocks = (a.n_rows + BTK_THREADS / 64 - 1) / (BTK_THREADS / 64);
    hipLaunchKernelGGL(btk_compact_kernel, dim3(row_blocks), dim3(BTK_THREADS), 0, s, a);
    return hipGetLastError();
}

size_t btk_workspace_words(int max_rows) { return (size_t)BTK_ST_WORDS + 3 * BTK_BINS + BTK_LIST_CAP + 2 * (size_t)max_rows; }

hipError_t launch_batch_topk(const BtkArgs& a, hipStream_t s) {
    if (a.n_rows <= 0) return hipSuccess;
    uint32_t* st = a.ws;
    uint32_t* hist = a.ws + BTK_ST_WORDS;
    uint32_t* list = hist + 3 * BTK_BINS;
    int32_t* row_ties = reinterpret_cast<int32_t*>(list + BTK_LIST_CAP);
    int32_t* keep_ties = row_ties + a.max_rows;
    const size_t N = (size_t)a.n_rows * a.S, n4 = N / 4;  // (S % 4 == 0)
    hipError_t e = hipMemsetAsync(a.overflow, 0, sizeof(int32_t), s);
    if (e != hipSuccess) return e;
    BtkCompactArgs c{};
    c.h = a.h; c.n_rows = a.n_rows; c.S = a.S; c.row_cap = a.row_cap; c.training = a.training; c.st = st; c.threshold = a.threshold;
    c.idx_out = a.idx_out; c.val_out = a.val_out; c.row_nnz_out = a.row_nnz_out; c.row_ties = row_ties; c.overflow = a.overflow;
    const int row_blocks = (a.n_rows + BTK_THREADS / 64 - 1) / (BTK_THREADS / 64);
    if (a.training) {
        e = hipMemsetAsync(hist, 0, 3 * BTK_BINS * sizeof(uint32_t), s);
        if (e != hipSuccess) return e;
        const uint32_t cap = a.list_cap > 0 ? (uint32_t)std::min<long>(a.list_cap, BTK_LIST_CAP) : (uint32_t)BTK_LIST_CAP;
        const uint32_t target = (uint32_t)std::min<size_t>((size_t)a.n_rows * (size_t)a.top_k, N);
        const int grid = (int)std::min<size_t>((n4 + BTK_THREADS - 1) / BTK_THREADS, 2048);
        hipLaunchKernelGGL(btk_hist_kernel, dim3(grid), dim3(BTK_THREADS), 0, s, a.h, n4, 0, st, list, cap, hist);
        hipLaunchKernelGGL(btk_scan_kernel, dim3(1), dim3(1024), 0, s, 0, st, hist, target);
        hipLaunchKernelGGL(btk_gather_kernel, dim3(grid), dim3(BTK_THREADS), 0, s, a.h, n4, st, list, cap);
        for (int level = 1; level <= 2; ++level) {
            hipLaunchKernelGGL(btk_hist_kernel, dim3(grid), dim3(BTK_THREADS), 0, s, a.h, n4, level, st, list, cap, hist);
            hipLaunchKernelGGL(btk_scan_kernel, dim3(1), dim3(1024), 0, s, level, st, hist, target);
        }
        hipLaunchKernelGGL(btk_compact_kernel, dim3(row_blocks), dim3(BTK_THREADS), 0, s, c);
        hipLaunchKernelGGL(btk_tie_scan_kernel, dim3(1), dim3(1024), 0, s, st, a.n_rows, row_ties, keep_ties, a.row_nnz_out);
        hipLaunchKernelGGL(btk_tie_drop_kernel, dim3(row_blocks), dim3(BTK_THREADS), 0, s, st, a.n_rows, a.row_cap, row_ties, keep_ties,
                           a.row_nnz_out, a.idx_out, a.val_out);
        if (a.update_threshold)
            hipLaunchKernelGGL(btk_ema_kernel, dim3(1), dim3(64), 0, s, st, a.overflow, a.threshold, (float)(1.0 - a.momentum),
                               (float)a.momentum);
    } else {
        hipLaunchKernelGGL(btk_compact_kernel, dim3(row_blocks), dim3(BTK_THREADS), 0, s, c);
    }
    return hipGetLastError();
}
