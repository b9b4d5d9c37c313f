// The latent-major regroup that spatial.hip and exemplars.hip open with: the FIRING events of a token CSR -- a
// valid latent, the image's group in [0, G), value > thr -- as per-latent lists in ascending row order, by a stable counting sort.
// (probe1d.hip sorts every entry the same way with kernels of its own; the part rule all three cut the entries by is lm_parts and
// lm_part_len of entry_util.h.)
//
//   count   one pass over the stored entries finds the row of each, checks its latent and its image's group (the error word) and
//           keeps in fire_row the row of an entry that fires, or -1; integer atomics count every (part, latent), the entries
//           being cut into up to LM_PARTS contiguous parts.
//   parts   a thread per latent turns its counts into the parts' offsets inside the latent's segment.
//   scan    one workgroup: `starts`, the total at starts[S].
//   place   ONE WAVE PER PART walks its entries in order, 64 a trip, and places each event behind the earlier ones of its latent:
//           the rank inside the trip by comparing lanes, the trip's base by one integer atomic of the latent's first lane on a
//           cursor only this wave touches.  Rows ascend inside a part and parts are in row order, so every segment ends up in
//           ascending row order whatever the timing.
//
// The units' error codes are template arguments and every kernel is static: a unit's code objects hold its own instances.
#pragma once
#include "entry_util.h"

// ---- host ------------------------------------------------------------------------------------------------------------------------

constexpr int LM_SCAN_THREADS = 1024;

// the regroup's arrays as byte offsets into a workspace
struct LmLayout {
    int64_t parts, part_len;
    int64_t off_starts, off_tot, off_cnt, off_fire_row, off_row, off_val;
};

static inline void lm_carve(WsCarve& ws, int64_t S, int64_t nnz, LmLayout* L) {
    L->parts = lm_parts(S, nnz);
    L->part_len = lm_part_len(nnz, (int)L->parts);
    L->off_starts = ws.take(8 * (S + 1));
    L->off_tot = ws.take(4 * S);
    L->off_cnt = ws.take(4 * L->parts * S);
    L->off_fire_row = ws.take(4 * nnz);
    L->off_row = ws.take(4 * nnz);
    L->off_val = ws.take(4 * nnz);
}

// the same as pointers
struct LmLists {
    int64_t parts, part_len;
    int64_t* starts;
    int32_t *tot, *cnt, *fire_row, *row;
    float* val;
};

static inline LmLists lm_lists(uint8_t* ws, const LmLayout& L) {
    return LmLists{L.parts, L.part_len, reinterpret_cast<int64_t*>(ws + L.off_starts), reinterpret_cast<int32_t*>(ws + L.off_tot),
                   reinterpret_cast<int32_t*>(ws + L.off_cnt), reinterpret_cast<int32_t*>(ws + L.off_fire_row),
                   reinterpret_cast<int32_t*>(ws + L.off_row), reinterpret_cast<float*>(ws + L.off_val)};
}

// ---- kernels -----------------------------------------------------------------------------------------------------------------------

// n_group[g] = images of group g; a group id outside [-1, G) is reported
template <int ERR_GROUP>
static __global__ __launch_bounds__(256) void lm_groups_kernel(const int32_t* __restrict__ group, long n_images, int G, unsigned long long* __restrict__ n_group,
                                                               int32_t* __restrict__ err) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n_images; i += (long)gridDim.x * 256) {
        const int g = group[i];
        if (g < -1 || g >= G) atomicMax(err, ERR_GROUP);
        else if (g >= 0) atomicAdd(n_group + g, 1ull);
    }
}

// the first pass over the entries: fire_row[e] = the row of entry e when it is an event of a valid latent in an image (T rows each)
// of a group in [0, G), else -1; cnt[part][latent] counts the events
template <int ERR_LATENT, int ERR_GROUP>
static __global__ __launch_bounds__(256) void lm_count_kernel(const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ indices,
                                                              const float* __restrict__ data, const int32_t* __restrict__ group, long nnz, int N,
                                                              int S, int T, int G, float thr, long part_len, int32_t* __restrict__ fire_row,
                                                              int32_t* __restrict__ cnt, int32_t* __restrict__ err) {
    const int64_t p0 = row_ptr[0];
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < nnz; e += (long)gridDim.x * 256) {
        const int col = indices[p0 + e];
        const int row = csr_row_of(row_ptr, N, p0 + e);
        const int g = group[row / T];
        int keep = -1;
        if (col < 0 || col >= S) atomicMax(err, ERR_LATENT);
        else if (g < -1 || g >= G) atomicMax(err, ERR_GROUP);
        else if (g >= 0 && data[p0 + e] > thr) {  // NaN compares false
            keep = row;
            atomicAdd(cnt + (e / part_len) * S + col, 1);
        }
        fire_row[e] = keep;
    }
}

// cnt[p][l] -> the events of latent l in parts before p; tot[l] = all of them
static __global__ __launch_bounds__(256) void lm_parts_kernel(int32_t* __restrict__ cnt, int parts, int S, int32_t* __restrict__ tot) {
    const long l = (long)blockIdx.x * 256 + threadIdx.x;
    if (l >= S) return;
    int run = 0;
    for (int p = 0; p < parts; p += 8) {  // eight loads in flight: a store to cnt would otherwise hold back the next load
        int t[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) t[q] = p + q < parts ? cnt[(size_t)(p + q) * S + l] : 0;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            if (p + q < parts) cnt[(size_t)(p + q) * S + l] = run;
            run += t[q];
        }
    }
    tot[l] = run;
}

static __global__ __launch_bounds__(LM_SCAN_THREADS) void lm_scan_kernel(const int32_t* __restrict__ tot, int S, int64_t* __restrict__ starts) {
    const long long end = block_scan_rounds<LM_SCAN_THREADS, long long, long>(
        S, [&](long l) { return (long long)tot[l]; }, [&](long l, long long start) { starts[l] = start; });
    if (threadIdx.x == 0) starts[S] = end;
}

// one wave per part: the rank of an event among the 64 of its trip by comparing lanes, the trip's base by one integer atomic on a
// cursor only this wave touches
static __global__ __launch_bounds__(64) void lm_place_kernel(const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ indices,
                                                             const float* __restrict__ data, const int32_t* __restrict__ fire_row, long nnz, int S,
                                                             long part_len, const int64_t* __restrict__ starts, int32_t* __restrict__ cnt,
                                                             int32_t* __restrict__ row_out, float* __restrict__ val_out) {
    const int lane = threadIdx.x;
    const long part = blockIdx.x;
    const long first = part * part_len, last = min(first + part_len, nnz);
    const int64_t p0 = row_ptr[0];
    int32_t* cur = cnt + (size_t)part * S;
    // a trip's loads are issued one trip ahead: the atomic below returns a value, and nothing else hides its latency in a wave
    // that works alone
    int col_next = -1, row_next = -1;
    float v_next = 0.f;
    auto load = [&](long e) {
        col_next = row_next = -1;
        v_next = 0.f;
        if (e < last) {
            row_next = fire_row[e];
            col_next = indices[p0 + e];
            v_next = data[p0 + e];
            if (row_next < 0 || col_next < 0 || col_next >= S) col_next = -1;  // (a kept row has its latent inside [0, S))
        }
    };
    load(first + lane);
    for (long g = first; g < last; g += 64) {
        const int col = col_next, row = row_next;
        const float v = v_next;
        load(g + 64 + lane);
        const int64_t start = col >= 0 ? starts[col] : 0;
        int rank = 0, same = 0, leader = 64;
#pragma unroll 16
        for (int i = 0; i < 64; ++i) {
            const bool match = col >= 0 && __builtin_amdgcn_readlane(col, i) == col;
            same += match;
            rank += match && i < lane;
            leader = match && leader == 64 ? i : leader;
        }
        int base = 0;
        if (col >= 0 && leader == lane) base = atomicAdd(cur + col, same);
        base = __shfl(base, leader & 63, 64);
        if (col >= 0) {
            const int64_t at = start + base + rank;
            if (at >= 0 && at < nnz) { row_out[at] = row; val_out[at] = v; }  // (always: the segments partition the events)
        }
    }
}

// ---- the launches ------------------------------------------------------------------------------------------------------------------

// Clears err (64 bytes) and cnt, then groups -- the n_images images counted into n_group, which the caller has cleared --, count,
// parts, scan and place on stream s.  false: a memset failed and nothing was launched
template <int ERR_LATENT, int ERR_GROUP>
static inline bool lm_regroup(const int64_t* row_ptr, const int32_t* indices, const float* data, int64_t nnz, int64_t N, int64_t S,
                              const int32_t* group, int64_t n_images, int64_t T, int64_t G, float thr, int64_t* n_group, const LmLists& A,
                              int32_t* err, hipStream_t s) {
    if (hipMemsetAsync(err, 0, 64, s) != hipSuccess || hipMemsetAsync(A.cnt, 0, (size_t)(4 * A.parts * S), s) != hipSuccess) return false;
    hipLaunchKernelGGL(lm_groups_kernel<ERR_GROUP>, dim3((unsigned)std::min<int64_t>((n_images + 255) / 256, 1024)), dim3(256), 0, s, group,
                       (long)n_images, (int)G, reinterpret_cast<unsigned long long*>(n_group), err);
    if (nnz > 0)
        hipLaunchKernelGGL((lm_count_kernel<ERR_LATENT, ERR_GROUP>), dim3((unsigned)std::min<int64_t>((nnz + 255) / 256, 8192)), dim3(256), 0, s,
                           row_ptr, indices, data, group, (long)nnz, (int)N, (int)S, (int)T, (int)G, thr, (long)A.part_len, A.fire_row, A.cnt, err);
    hipLaunchKernelGGL(lm_parts_kernel, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, s, A.cnt, (int)A.parts, (int)S, A.tot);
    hipLaunchKernelGGL(lm_scan_kernel, dim3(1), dim3(LM_SCAN_THREADS), 0, s, A.tot, (int)S, A.starts);
    if (nnz > 0) {
        const unsigned used = (unsigned)((nnz + A.part_len - 1) / A.part_len);
        hipLaunchKernelGGL(lm_place_kernel, dim3(used), dim3(64), 0, s, row_ptr, indices, data, A.fire_row, (long)nnz, (int)S, (long)A.part_len,
                           A.starts, A.cnt, A.row, A.val);
    }
    return true;
}
