// Token codes pooled to an image-level CSR without the dense matrix (include/saev_amd.h: POOL CSR): entry (i, l) of
// the output exists iff some patch of image i stores a value of latent l above the latent's threshold; its value is the maximum of
// those values, its patch the lowest one that attains it, its count the stored entries that pass.
//
//   unit     one image and one range of POOL_CSR_RANGE consecutive latents; a workgroup per unit, units past the grid in rounds.  An
//            image's entries are ONE span of indices / data (indptr[i T] .. indptr[(i + 1) T]), walked 256 entries a trip however
//            long it is; the workgroup keeps the entries of its own range.
//   count    the qualifying latents are marked in an LDS bit set (64 words of 64 bits, bitwise OR: order-free); a pop-count of the
//            set is the unit's row length.  Three small kernels turn the units' lengths into their starts (sums of 4 096 units, one
//            workgroup's scan of those sums, a scan inside every 4 096) and write out_indptr on the way: no read-back.
//   fill     marks again, then the word prefix of the set (one wave) gives every latent its slot -- the prefix pop-count of the set,
//            so columns ascend without a sort.  The span is walked a second time: a qualifying entry offers the 64-bit key
//            (value bits, ~patch) to its SLOT's key in LDS by integer max and counts itself by integer add; only the n_set slots in
//            use are cleared.  Then slot s goes to output position start + s, coalesced, and the set's latents to out_indices.
//            The patch of an entry is bisected from the image's T + 1 row positions, staged in LDS while T <= 256.
//
// The key's value part is the float's plain bit pattern: only values above a threshold >= 0 enter, those are positive, and the bit
// patterns of positive floats order as unsigned integers (a negative entry of a threshold vector, which would let negative values in,
// is error 4 and voids the outputs).  No floating-point atomic; OR, integer max and integer add do not depend on order: two calls
// give the same bits.  Every output element below out_indptr[n_images] is written exactly once.
#include "entry_util.h"

#include <algorithm>
#include <cmath>

namespace {

constexpr int PC_THREADS = 256;
constexpr int PC_WORDS = POOL_CSR_RANGE / 64;  // one wave scans the set's words
constexpr int PC_STAGE_T = 256;                // row positions of an image kept in LDS (longer images bisect in global memory)
constexpr int PC_MAX_BLOCKS = 1 << 16;
constexpr int PC_SCAN_CHUNK = 4096;            // units per workgroup of the scan
static_assert(PC_WORDS == 64, "the word prefix is one wave's scan");

struct PcArgs {
    const int64_t* indptr;
    const int32_t* indices;
    const float* data;
    int64_t nnz;
    int n_images, T, S, R;
    float thr;
    const float* thr_vec;
    int64_t units;
    int64_t* start;  // units + 1: the unit's row length after the count pass, its first output position after the scan
    int32_t* err;
};

// the image's span (empty when its ends are no positions into indices) and the checks a unit makes besides those of its entries
__device__ __forceinline__ int pc_unit_checks(const PcArgs& a, int img, int r, int lo, int len, int64_t* e0, int64_t* e1) {
    int bad = 0;
    const int64_t row0 = (int64_t)img * a.T;
    int64_t b = a.indptr[row0], e = a.indptr[row0 + a.T];
    if (b < 0 || e < b || e > a.nnz) { bad = SAEV_POOL_CSR_ERR_INDPTR; b = e = 0; }  // (the same in every thread)
    *e0 = b;
    *e1 = e;
    if (r == 0)
        for (int p = threadIdx.x; p < a.T; p += PC_THREADS)
            if (a.indptr[row0 + p + 1] < a.indptr[row0 + p]) bad = SAEV_POOL_CSR_ERR_INDPTR;
    if (img == 0 && a.thr_vec != nullptr)
        for (int c = threadIdx.x; c < len; c += PC_THREADS)
            if (a.thr_vec[lo + c] < 0.f) bad = max(bad, SAEV_POOL_CSR_ERR_THRESHOLD);
    return bad;
}

// marks the unit's qualifying latents; the error code of the span's entries
__device__ __forceinline__ int pc_mark(const PcArgs& a, int64_t e0, int64_t e1, int lo, int len, unsigned long long* bits) {
    int bad = 0;
    for (int64_t e = e0 + threadIdx.x; e < e1; e += PC_THREADS) {
        const int col = a.indices[e];
        const float v = a.data[e];
        if ((unsigned)col >= (unsigned)a.S) { bad = max(bad, SAEV_POOL_CSR_ERR_COLUMN); continue; }
        if (!(fabsf(v) <= 3.402823466e38f)) bad = max(bad, SAEV_POOL_CSR_ERR_VALUE);
        const int c = col - lo;
        if (c < 0 || c >= len) continue;
        const float t = a.thr_vec != nullptr ? a.thr_vec[col] : a.thr;
        if (v > t) atomicOr(&bits[c >> 6], 1ull << (c & 63));  // (a NaN threshold passes nothing, +Inf neither)
    }
    return bad;
}

__global__ __launch_bounds__(PC_THREADS) void pc_count_kernel(PcArgs a) {
    __shared__ unsigned long long bits[PC_WORDS];
    const int t = threadIdx.x;
    for (int64_t u = blockIdx.x; u < a.units; u += gridDim.x) {
        const int img = (int)(u / a.R), r = (int)(u - (int64_t)img * a.R);
        const int lo = r * POOL_CSR_RANGE, len = min(POOL_CSR_RANGE, a.S - lo);
        if (t < PC_WORDS) bits[t] = 0ull;
        __syncthreads();
        int64_t e0, e1;
        int bad = pc_unit_checks(a, img, r, lo, len, &e0, &e1);
        bad = max(bad, pc_mark(a, e0, e1, lo, len, bits));
        if (bad) atomicMax(a.err, bad);
        __syncthreads();
        if (t < 64) {
            const int n = wave_sum_i(__popcll(bits[t]));
            if (t == 0) a.start[u] = n;
        }
        __syncthreads();  // the next unit clears the set
    }
}

template <typename Ptr>
__device__ __forceinline__ int pc_patch_of(Ptr rp, int T, int64_t e) {  // the p with rp[p] <= e < rp[p + 1]; always in [0, T)
    int lo = 0, hi = T;
    while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        if (rp[mid] <= e) lo = mid; else hi = mid;
    }
    return lo;
}

template <bool DETAILS>
__global__ __launch_bounds__(PC_THREADS) void pc_fill_kernel(PcArgs a, const int64_t* __restrict__ out_indptr, int32_t* __restrict__ out_indices,
                                                             float* __restrict__ out_data, int32_t* __restrict__ out_patch,
                                                             int32_t* __restrict__ out_count) {
    __shared__ unsigned long long bits[PC_WORDS];
    __shared__ int wpre[PC_WORDS];
    __shared__ int n_set_s;
    __shared__ unsigned long long key[POOL_CSR_RANGE];
    __shared__ int32_t cnt[DETAILS ? POOL_CSR_RANGE : 1];
    __shared__ int64_t rp[DETAILS ? PC_STAGE_T + 1 : 1];
    const int t = threadIdx.x;
    for (int64_t u = blockIdx.x; u < a.units; u += gridDim.x) {
        const int img = (int)(u / a.R), r = (int)(u - (int64_t)img * a.R);
        const int lo = r * POOL_CSR_RANGE, len = min(POOL_CSR_RANGE, a.S - lo);
        const int64_t* rows = a.indptr + (int64_t)img * a.T;
        const bool staged = DETAILS && a.T <= PC_STAGE_T;
        if (t < PC_WORDS) bits[t] = 0ull;
        if (staged)
            for (int p = t; p <= a.T; p += PC_THREADS) rp[p] = rows[p];
        __syncthreads();
        int64_t e0, e1;
        int bad = pc_unit_checks(a, img, r, lo, len, &e0, &e1);
        bad = max(bad, pc_mark(a, e0, e1, lo, len, bits));
        __syncthreads();
        if (t < 64) {
            const int pc = __popcll(bits[t]);
            const int inc = wave_scan_incl(pc, t);
            wpre[t] = inc - pc;
            if (t == 63) n_set_s = inc;
        }
        __syncthreads();
        const int n_set = n_set_s;  // at most len
        for (int s = t; s < n_set; s += PC_THREADS) {
            key[s] = 0ull;  // below every offered key: a qualifying value is positive, its bits are not 0
            if (DETAILS) cnt[s] = 0;
        }
        __syncthreads();
        for (int64_t e = e0 + t; e < e1; e += PC_THREADS) {
            const int col = a.indices[e];
            const float v = a.data[e];
            if ((unsigned)col >= (unsigned)a.S) continue;
            const int c = col - lo;
            if (c < 0 || c >= len) continue;
            const float th = a.thr_vec != nullptr ? a.thr_vec[col] : a.thr;
            if (!(v > th)) continue;
            const unsigned long long w = bits[c >> 6];
            const int slot = wpre[c >> 6] + __popcll(w & ((1ull << (c & 63)) - 1ull));  // < n_set: the entry's own bit is in the set
            unsigned low = 0xffffffffu;
            if (DETAILS) {
                const int p = staged ? pc_patch_of(rp, a.T, e) : pc_patch_of(rows, a.T, e);
                low = ~(unsigned)p;  // the larger key of equal values is the lower patch
                atomicAdd(&cnt[slot], 1);
            }
            atomicMax(&key[slot], ((unsigned long long)__float_as_uint(v) << 32) | low);
        }
        __syncthreads();
        const int64_t base = a.start[u];
        // (always, after a count pass over the same arrays: anything else writes nothing and is reported as a bad indptr)
        if (base < 0 || a.start[u + 1] - base != n_set || base + n_set > out_indptr[a.n_images]) bad = SAEV_POOL_CSR_ERR_INDPTR;
        else {
            for (int s = t; s < n_set; s += PC_THREADS) {
                const unsigned long long k = key[s];
                out_data[base + s] = __uint_as_float((unsigned)(k >> 32));
                if (DETAILS) {
                    if (out_patch != nullptr) out_patch[base + s] = (int32_t)~(unsigned)k;
                    if (out_count != nullptr) out_count[base + s] = cnt[s];
                }
            }
            for (int c = t; c < len; c += PC_THREADS) {
                const unsigned long long w = bits[c >> 6];
                if ((w >> (c & 63)) & 1ull) out_indices[base + wpre[c >> 6] + __popcll(w & ((1ull << (c & 63)) - 1ull))] = lo + c;
            }
        }
        if (bad) atomicMax(a.err, bad);
        __syncthreads();  // the next unit clears the set and the slots
    }
}

// ---------------------------------------------------------------- the scan over units -------------------------------------------------

__global__ __launch_bounds__(PC_THREADS) void pc_part_kernel(const int64_t* __restrict__ start, int64_t units, long long* __restrict__ part) {
    __shared__ long long sw[PC_THREADS / 64];
    const int t = threadIdx.x, lane = t & 63;
    const int64_t base = (int64_t)blockIdx.x * PC_SCAN_CHUNK;
    long long sum = 0;
    for (int i = t; i < PC_SCAN_CHUNK && base + i < units; i += PC_THREADS) sum += start[base + i];
    sum = wave_scan_incl(sum, lane);
    if (lane == 63) sw[t >> 6] = sum;
    __syncthreads();
    if (t == 0) part[blockIdx.x] = sw[0] + sw[1] + sw[2] + sw[3];
}

__global__ __launch_bounds__(PC_THREADS) void pc_part_scan_kernel(long long* __restrict__ part, int n_chunks) {
    block_scan_rounds<PC_THREADS, long long, int>(
        n_chunks, [&](int l) { return part[l]; }, [&](int l, long long before) { part[l] = before; });
}

__global__ __launch_bounds__(PC_THREADS) void pc_scan_kernel(int64_t* __restrict__ start, int64_t units, int R, int64_t n_images,
                                                             const long long* __restrict__ part, int64_t* __restrict__ out_indptr) {
    const int64_t base = (int64_t)blockIdx.x * PC_SCAN_CHUNK;
    const int n = units - base < PC_SCAN_CHUNK ? (int)(units - base) : PC_SCAN_CHUNK;
    const long long off = part[blockIdx.x];
    const long long total = block_scan_rounds<PC_THREADS, long long, int>(
        n, [&](int l) { return (long long)start[base + l]; },
        [&](int l, long long before) {
            const int64_t u = base + l;
            start[u] = off + before;
            if (u % R == 0) out_indptr[u / R] = off + before;
        });
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
        start[units] = off + total;
        out_indptr[n_images] = off + total;
    }
}

struct PcLayout {
    int64_t R, units, n_chunks, off_start, off_part, total_bytes;
};

bool pc_shape_ok(int64_t n_images, int64_t T, int64_t S, int64_t nnz) {
    if (n_images < 1 || T < 1 || S < 1 || nnz < 0) return false;
    if (n_images > 0x7fffffffLL || T > 0x7fffffffLL || S > 0x7fffffffLL || n_images * T > 0x7fffffffLL) return false;
    return n_images * ((S + POOL_CSR_RANGE - 1) / POOL_CSR_RANGE) <= 0x7fffffffLL;
}

void pc_layout(int64_t n_images, int64_t S, PcLayout* L) {
    L->R = (S + POOL_CSR_RANGE - 1) / POOL_CSR_RANGE;
    L->units = n_images * L->R;
    L->n_chunks = (L->units + PC_SCAN_CHUNK - 1) / PC_SCAN_CHUNK;
    WsCarve ws;
    L->off_start = ws.take(8 * (L->units + 1));
    L->off_part = ws.take(8 * L->n_chunks);
    L->total_bytes = ws.at;
}

// the refusals both entries share, in the header's order; the output pointers and the workspace follow in the entry
int pc_check(const char* who, const int64_t* indptr, const int32_t* indices, const float* data, int64_t nnz, int64_t n_images, int64_t T, int64_t S,
             float thr, const float* thr_vec) {
    if (n_images < 0 || T < 0 || S < 0 || nnz < 0) return entry_refuse(SAEV_INVALID_ARG, who, "negative size");
    if (n_images < 1 || T < 1 || S < 1) return entry_refuse(SAEV_INVALID_ARG, who, "n_images, tokens_per_image and n_latents must be at least 1");
    if (n_images > 0x7fffffffLL || T > 0x7fffffffLL || S > 0x7fffffffLL || n_images * T > 0x7fffffffLL)
        return entry_refuse(SAEV_UNSUPPORTED, who, "n_images * tokens_per_image and n_latents must stay below 2^31");
    if (!pc_shape_ok(n_images, T, S, nnz)) return entry_refuse(SAEV_UNSUPPORTED, who, "n_images * ceil(n_latents / 4096) must stay below 2^31");
    if (thr_vec == nullptr && !(thr >= 0.f && thr <= 3.402823466e38f))
        return entry_refuse(SAEV_INVALID_ARG, who, "a scalar threshold must be finite and at least 0");
    if (!indptr) return entry_refuse(SAEV_INVALID_ARG, who, "indptr is NULL");
    if (nnz > 0 && (!indices || !data)) return entry_refuse(SAEV_INVALID_ARG, who, "indices and data come with nnz > 0");
    return SAEV_OK;
}

PcArgs pc_args(const int64_t* indptr, const int32_t* indices, const float* data, int64_t nnz, int64_t n_images, int64_t T, int64_t S, float thr,
               const float* thr_vec, const PcLayout& L, void* ws, int32_t* err) {
    return PcArgs{indptr, indices, data, nnz, (int)n_images, (int)T, (int)S, (int)L.R, thr, thr_vec, L.units,
                  reinterpret_cast<int64_t*>(static_cast<uint8_t*>(ws) + L.off_start), err};
}

const char* const PC_TOO_SMALL = "workspace smaller than saev_pool_csr_workspace_bytes(n_images, tokens_per_image, n_latents, nnz)";

}  // namespace

// ---------------------------------------------------------------- C ABI ------------------------------------------------------------------

int64_t saev_pool_csr_range(void) { return POOL_CSR_RANGE; }

int64_t saev_pool_csr_workspace_bytes(int64_t n_images, int64_t tokens_per_image, int64_t n_latents, int64_t nnz) {
    if (!pc_shape_ok(n_images, tokens_per_image, n_latents, nnz)) return -1;
    PcLayout L;
    pc_layout(n_images, n_latents, &L);
    return L.total_bytes;
}

int saev_pool_csr_count(const int64_t* indptr, const int32_t* indices, const float* data, int64_t nnz, int64_t n_images, int64_t tokens_per_image,
                        int64_t n_latents, float thr, const float* thr_vec, int64_t* out_indptr, void* workspace, int64_t workspace_bytes,
                        int32_t* err, void* stream) {
    const char* who = "saev_pool_csr_count";
    if (const int rc = pc_check(who, indptr, indices, data, nnz, n_images, tokens_per_image, n_latents, thr, thr_vec)) return rc;
    if (!out_indptr || !err) return entry_refuse(SAEV_INVALID_ARG, who, "out_indptr and err must not be NULL");
    PcLayout L;
    pc_layout(n_images, n_latents, &L);
    if (const int rc = entry_check_workspace(who, workspace, workspace_bytes, L.total_bytes, PC_TOO_SMALL)) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(err, 0, 4, s) != hipSuccess) return entry_refuse(SAEV_HIP_ERROR, who, "hipMemsetAsync failed");
    const PcArgs a = pc_args(indptr, indices, data, nnz, n_images, tokens_per_image, n_latents, thr, thr_vec, L, workspace, err);
    long long* part = reinterpret_cast<long long*>(static_cast<uint8_t*>(workspace) + L.off_part);
    hipLaunchKernelGGL(pc_count_kernel, dim3((unsigned)std::min<int64_t>(L.units, PC_MAX_BLOCKS)), dim3(PC_THREADS), 0, s, a);
    hipLaunchKernelGGL(pc_part_kernel, dim3((unsigned)L.n_chunks), dim3(PC_THREADS), 0, s, a.start, L.units, part);
    hipLaunchKernelGGL(pc_part_scan_kernel, dim3(1), dim3(PC_THREADS), 0, s, part, (int)L.n_chunks);
    hipLaunchKernelGGL(pc_scan_kernel, dim3((unsigned)L.n_chunks), dim3(PC_THREADS), 0, s, a.start, L.units, (int)L.R, n_images, part, out_indptr);
    if (hipGetLastError() != hipSuccess) return entry_refuse(SAEV_HIP_ERROR, who, "kernel launch failed");
    return SAEV_OK;
}

int saev_pool_csr_fill(const int64_t* indptr, const int32_t* indices, const float* data, int64_t nnz, int64_t n_images, int64_t tokens_per_image,
                       int64_t n_latents, float thr, const float* thr_vec, const int64_t* out_indptr, int32_t* out_indices, float* out_data,
                       int32_t* out_patch, int32_t* out_count, void* workspace, int64_t workspace_bytes, int32_t* err, void* stream) {
    const char* who = "saev_pool_csr_fill";
    if (const int rc = pc_check(who, indptr, indices, data, nnz, n_images, tokens_per_image, n_latents, thr, thr_vec)) return rc;
    if (!out_indptr || !out_indices || !out_data || !err)
        return entry_refuse(SAEV_INVALID_ARG, who, "out_indptr, out_indices, out_data and err must not be NULL");
    PcLayout L;
    pc_layout(n_images, n_latents, &L);
    if (const int rc = entry_check_workspace(who, workspace, workspace_bytes, L.total_bytes, PC_TOO_SMALL)) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(err, 0, 4, s) != hipSuccess) return entry_refuse(SAEV_HIP_ERROR, who, "hipMemsetAsync failed");
    const PcArgs a = pc_args(indptr, indices, data, nnz, n_images, tokens_per_image, n_latents, thr, thr_vec, L, workspace, err);
    const dim3 grid((unsigned)std::min<int64_t>(L.units, PC_MAX_BLOCKS));
    if (out_patch || out_count)
        hipLaunchKernelGGL(pc_fill_kernel<true>, grid, dim3(PC_THREADS), 0, s, a, out_indptr, out_indices, out_data, out_patch, out_count);
    else
        hipLaunchKernelGGL(pc_fill_kernel<false>, grid, dim3(PC_THREADS), 0, s, a, out_indptr, out_indices, out_data, out_patch, out_count);
    if (hipGetLastError() != hipSuccess) return entry_refuse(SAEV_HIP_ERROR, who, "kernel launch failed");
    return SAEV_OK;
}
