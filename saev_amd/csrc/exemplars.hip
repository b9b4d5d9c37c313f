// Which images to look at (include/saev_amd.h: LATENT EXEMPLARS): per (latent, group of images) the k strongest
// firing images, the k weakest firing images and the first k silent ones, each firing image with its max-pooled value M and the
// lowest patch that attains it -- pooled on the fly from the token CSR, never through an n_images x S matrix -- and
// saev_latent_patch_rows, the gather of the stored patch vectors of chosen (latent, image) pairs.
//
//   prepare  the events latent-major in ascending row order: the regroup of latent_major.h with this entry's
//            error codes (a valid latent, the image's group in [0, G), value > thr).  Two small kernels also leave, for the silent lists,
//            n_group_images, the first slot of every group, each image's rank inside its group and the groups'
//            member lists in ascending image order: a stable counting sort of the n_images group ids, one wave per group, the rank
//            of an image among the 64 of a trip from a ballot.
//   walk     a wave per latent, 64 events a trip.  Lane = event first: a latent's rows ascend, so an image's events are consecutive;
//            a segmented scan by lane shuffles folds each run into (M, P), the EARLIER lane winning equal values (patches ascend
//            inside a run, so that is the lowest patch).  The run that reaches the trip's last lane is carried in scalars into the
//            next trip -- a run may be longer than a trip -- and the carry, being earlier, wins equal values too.  Then lane = group:
//            the finished runs are broadcast one at a time in list order (images ascend) and the lane that owns the record's group
//            counts it, moves its silent cursor (the members of rank cursor .. rank(i) - 1 did not fire and go to silent_img while
//            fewer than k are held) and offers it to its two k-lists.  The lists live in LDS, G x k x 2 x 12 bytes a wave, sorted at
//            all times by the total orders (M descending, image ascending) and (M ascending, image ascending); records arrive in
//            ascending image order, so a record goes behind every held one of equal M, and one that is not better than the k-th
//            held value -- a register -- costs two compares.  After the last trip the lanes flush the silent tails and the wave
//            copies the lists out, lane = slot.
//   rows     a workgroup per query, threads over the T rows of the image, each scanning its row's stored entries for the latent.
//
// The lanes of the walk exchange events through shuffles and lane reads only; a lane's lists in LDS are touched by that lane alone
// between the wave-wide fill before the first trip and the wave-wide copy after the last, and the wave's LDS stores are drained at
// both of those borders.  No floating-point atomic, no read-back.  A latent that fires on most rows is one wave's serial walk
// (DESIGN.md 7).
#include "latent_major.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace {

constexpr int EX_MAX_G = 64;
constexpr int EX_MAX_K = 32;
constexpr int EX_MAX_T = 4096;
constexpr int EX_ROWS_THREADS = 256;
constexpr int EX_ROWS_MAX_BLOCKS = 1 << 16;

// byte offsets into the workspace (all multiples of 256); the error word comes first
struct ExLayout {
    int64_t off_err;
    LmLayout lm;
    int64_t off_rank, off_members, off_gstart, total_bytes;
};

void ex_layout(int64_t nnz, int64_t S, int64_t n_images, ExLayout* L) {
    WsCarve ws;
    L->off_err = ws.take(64);
    lm_carve(ws, S, nnz, &L->lm);
    L->off_rank = ws.take(4 * n_images);
    L->off_members = ws.take(4 * n_images);
    L->off_gstart = ws.take(4 * (EX_MAX_G + 1));
    L->total_bytes = ws.at;
}

// ---------------------------------------------------------------- prepare ----------------------------------------------------------------

// one wave per group g: gstart[g] = the members of the groups before it (gstart[G] = all members, left by the last wave), and in
// ascending image order members[gstart[g] + r] = the r-th image of g, rank[that image] = r.  An image of no group keeps no rank: its
// events are no events, so nothing reads it
__global__ __launch_bounds__(64) void ex_members_kernel(const int32_t* __restrict__ group, int n_images, int G, const unsigned long long* __restrict__ n_group,
                                                        int32_t* __restrict__ gstart, int32_t* __restrict__ rank, int32_t* __restrict__ members) {
    const int lane = threadIdx.x, g = blockIdx.x;
    int start = 0;
    for (int q = 0; q < g; ++q) start += (int)n_group[q];
    if (lane == 0) {
        gstart[g] = start;
        if (g == G - 1) gstart[G] = start + (int)n_group[g];
    }
    int run = 0;
    for (int base = 0; base < n_images; base += 64) {
        const int i = base + lane;
        const bool mine = i < n_images && group[i] == g;
        const unsigned long long mask = __ballot(mine);
        if (mine) {
            const int r = run + __popcll(mask & ((1ull << lane) - 1ull));
            rank[i] = r;
            if (start + r < n_images) members[start + r] = i;  // (always: the groups partition at most n_images images)
        }
        run += __popcll(mask);
    }
}

// ---------------------------------------------------------------- walk -------------------------------------------------------------------

struct ExWalk {
    const int64_t* starts;
    const int32_t* row;
    const float* val;
    const int32_t* group;
    const int32_t *rank, *members, *gstart;
    int S, G, k, T, n_images;
    int32_t* n_fire;
    float* top_val;
    int32_t *top_img, *top_patch;
    float* bot_val;
    int32_t *bot_img, *bot_patch, *silent_img;
};

__device__ __forceinline__ float ex_lane_f(float x, int i) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), i)); }

// LDS of one wave: six arrays of G * k words -- top value, image, patch, then the same of the bottom list -- slot g * k + q
__global__ __launch_bounds__(256) void ex_walk_kernel(ExWalk a, int waves) {
    extern __shared__ int32_t ex_lds[];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long j = (long)blockIdx.x * waves + w;
    if (j >= a.S) return;  // no workgroup barrier below: a wave works alone
    const int G = a.G, k = a.k, T = a.T, slots = G * k;
    int32_t* mine = ex_lds + (size_t)w * 6 * slots;
    float* tv = reinterpret_cast<float*>(mine);
    int32_t *ti = mine + slots, *tp = mine + 2 * slots;
    float* bv = reinterpret_cast<float*>(mine + 3 * slots);
    int32_t *bi = mine + 4 * slots, *bp = mine + 5 * slots;
    for (int q = lane; q < slots; q += 64) {
        tv[q] = 0.f; ti[q] = -1; tp[q] = -1;
        bv[q] = 0.f; bi[q] = -1; bp[q] = -1;
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();

    const int lo = __builtin_amdgcn_readfirstlane((int)a.starts[j]), hi = __builtin_amdgcn_readfirstlane((int)a.starts[j + 1]);
    // lane = group state
    const bool own = lane < G;
    const int g0 = own ? a.gstart[lane] : 0, n_g = own ? a.gstart[lane + 1] - g0 : 0;
    const int lb = lane * k;  // the lane's slots (used only when own)
    int32_t* silent_out = a.silent_img + ((size_t)j * G + (own ? lane : 0)) * k;
    int nf = 0, cursor = 0, nsil = 0, tn = 0, bn = 0;
    float t_kth = 0.f, b_kth = 0.f;  // the k-th held value of a full list

    auto take = [&](int img, float v, int p, int g, int rk) {  // uniform arguments; the owner of g works
        if (lane != g) return;
        nf += 1;
        while (cursor < rk && nsil < k) silent_out[nsil++] = a.members[g0 + cursor++];
        cursor = rk + 1;
        if (tn < k || v > t_kth) {
            int q = tn < k ? tn : k - 1;
            while (q > 0 && tv[lb + q - 1] < v) {
                tv[lb + q] = tv[lb + q - 1]; ti[lb + q] = ti[lb + q - 1]; tp[lb + q] = tp[lb + q - 1];
                --q;
            }
            tv[lb + q] = v; ti[lb + q] = img; tp[lb + q] = p;
            tn += tn < k;
            if (tn == k) t_kth = tv[lb + k - 1];
        }
        if (bn < k || v < b_kth) {
            int q = bn < k ? bn : k - 1;
            while (q > 0 && bv[lb + q - 1] > v) {
                bv[lb + q] = bv[lb + q - 1]; bi[lb + q] = bi[lb + q - 1]; bp[lb + q] = bp[lb + q - 1];
                --q;
            }
            bv[lb + q] = v; bi[lb + q] = img; bp[lb + q] = p;
            bn += bn < k;
            if (bn == k) b_kth = bv[lb + k - 1];
        }
    };

    // the run that reached the last lane of the trip before (scalars); c_img = -1: none
    int c_img = -1, c_p = 0, c_g = 0, c_rk = 0;
    float c_v = 0.f;
    for (int base = lo; base < hi; base += 64) {
        const int e = base + lane;
        const int n = min(64, hi - base);  // scalar
        const bool valid = lane < n;
        int img = -2 - lane, p = 0;  // a lane without an event matches nobody, the carry neither
        float v = 0.f;
        if (valid) {
            const int row = a.row[e];
            v = a.val[e];
            img = row / T;
            p = row - img * T;
        }
        // the run's (M, P) so far in every lane: an inclusive segmented scan, the earlier lane keeping equal values
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int o_img = __shfl_up(img, d, 64), o_p = __shfl_up(p, d, 64);
            const float o_v = __shfl_up(v, d, 64);
            if (lane >= d && o_img == img && o_v >= v) { v = o_v; p = o_p; }
        }
        if (img == c_img && c_v >= v) { v = c_v; p = c_p; }
        const int next_img = __shfl_down(img, 1, 64);
        const bool tail = valid && (lane == n - 1 || next_img != img);
        int g = 0, rk = 0;
        if (tail) {
            const int at = min(max(img, 0), a.n_images - 1);  // (always img itself: an event's row lies in [0, n_images * T))
            g = a.group[at];  // in [0, G): prepare keeps no other event
            rk = a.rank[at];
        }
        if (c_img >= 0 && __builtin_amdgcn_readlane(img, 0) != c_img) take(c_img, c_v, c_p, c_g, c_rk);
        unsigned long long todo = __ballot(tail && lane < n - 1);
        while (todo) {
            const int i = __builtin_amdgcn_readfirstlane(__builtin_ctzll(todo));
            todo &= todo - 1;
            take(__builtin_amdgcn_readlane(img, i), ex_lane_f(v, i), __builtin_amdgcn_readlane(p, i), __builtin_amdgcn_readlane(g, i),
                 __builtin_amdgcn_readlane(rk, i));
        }
        const int last = __builtin_amdgcn_readfirstlane(n - 1);
        c_img = __builtin_amdgcn_readlane(img, last);
        c_v = ex_lane_f(v, last);
        c_p = __builtin_amdgcn_readlane(p, last);
        c_g = __builtin_amdgcn_readlane(g, last);
        c_rk = __builtin_amdgcn_readlane(rk, last);
    }
    if (c_img >= 0) take(c_img, c_v, c_p, c_g, c_rk);

    if (own) {
        while (cursor < n_g && nsil < k) silent_out[nsil++] = a.members[g0 + cursor++];
        while (nsil < k) silent_out[nsil++] = -1;
        a.n_fire[(size_t)j * G + lane] = nf;
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
    const size_t o = (size_t)j * slots;
    for (int q = lane; q < slots; q += 64) {
        a.top_val[o + q] = tv[q]; a.top_img[o + q] = ti[q]; a.top_patch[o + q] = tp[q];
        a.bot_val[o + q] = bv[q]; a.bot_img[o + q] = bi[q]; a.bot_patch[o + q] = bp[q];
    }
}

// ---------------------------------------------------------------- patch rows -------------------------------------------------------------

// out[q, p] = the stored value of q_latent[q] in row q_image[q] * T + p, or 0; a workgroup per query (queries past the grid in rounds)
__global__ __launch_bounds__(EX_ROWS_THREADS) void ex_rows_kernel(const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ indices,
                                                                  const float* __restrict__ data, long nnz, int n_images, int T, int S,
                                                                  const int32_t* __restrict__ q_latent, const int32_t* __restrict__ q_image, long Q,
                                                                  float* __restrict__ out, int32_t* __restrict__ err) {
    const int64_t p0 = row_ptr[0];
    for (long q = blockIdx.x; q < Q; q += gridDim.x) {
        const int j = q_latent[q], i = q_image[q];
        const bool bad = j < 0 || j >= S || i < -1 || i >= n_images;
        if (bad && threadIdx.x == 0) atomicMax(err, j < 0 || j >= S ? SAEV_LATENT_EXEMPLARS_ERR_LATENT : SAEV_LATENT_EXEMPLARS_ERR_IMAGE);
        for (int p = threadIdx.x; p < T; p += EX_ROWS_THREADS) {
            float v = 0.f;
            if (!bad && i >= 0) {
                const long row = (long)i * T + p;
                const int64_t first = row_ptr[row], last = row_ptr[row + 1], end = p0 + (int64_t)nnz;
                const int64_t lo = first < p0 ? p0 : first, hi = last > end ? end : last;  // (the row's own entries: a guard only)
                for (int64_t e = lo; e < hi; ++e)
                    if (indices[e] == j) {
                        v = data[e];
                        break;
                    }
            }
            out[(size_t)q * T + p] = v;
        }
    }
}

bool ex_shape_ok(int64_t nnz, int64_t S, int64_t n_images, int64_t G) {
    return entry_shape_ok(n_images, S, 1, nnz) && G >= 1 && G <= EX_MAX_G;
}

}  // namespace

// ---------------------------------------------------------------- C ABI ------------------------------------------------------------------

int64_t saev_latent_exemplars_workspace_bytes(int64_t nnz, int64_t S, int64_t n_images, int64_t G) {
    if (!ex_shape_ok(nnz, S, n_images, G)) return -1;
    ExLayout L;
    ex_layout(nnz, S, n_images, &L);
    return L.total_bytes;
}

int saev_latent_exemplars(const int64_t* row_ptr, const int32_t* indices, const float* data, int64_t nnz, const int32_t* group_i32, int64_t n_images,
                          int64_t T, int64_t S, int64_t G, int64_t k, float thr, const saev_latent_exemplars_out* out, void* workspace,
                          int64_t workspace_bytes, void* stream) {
    const char* who = "saev_latent_exemplars";
    if (const int rc = entry_check_shape(who, n_images, S, 1, nnz)) return rc;
    if (G < 1 || G > EX_MAX_G) return entry_refuse(SAEV_UNSUPPORTED, who, "the number of groups must lie in [1, 64]");
    if (k < 1 || k > EX_MAX_K) return entry_refuse(SAEV_UNSUPPORTED, who, "k must lie in [1, 32]");
    if (T < 1 || T > EX_MAX_T) return entry_refuse(SAEV_UNSUPPORTED, who, "T must lie in [1, 4096]");
    if (n_images * T > 0x7fffffffLL) return entry_refuse(SAEV_UNSUPPORTED, who, "n_images * T must stay below 2^31");
    if (S * G * k > 0x7fffffffLL) return entry_refuse(SAEV_UNSUPPORTED, who, "S * G * k must stay below 2^31");
    if (!(thr >= 0.f)) return entry_refuse(SAEV_INVALID_ARG, who, "thr must be at least 0");
    if (!row_ptr) return entry_refuse(SAEV_INVALID_ARG, who, "row_ptr is NULL");
    if (nnz > 0 && (!indices || !data)) return entry_refuse(SAEV_INVALID_ARG, who, "indices and data come with nnz > 0");
    if (!group_i32) return entry_refuse(SAEV_INVALID_ARG, who, "group_i32 must not be NULL");
    if (!out || out->struct_size < (int32_t)(2 * sizeof(int32_t)))
        return entry_refuse(SAEV_INVALID_ARG, who, "no saev_latent_exemplars_out (or its struct_size is unset)");
    saev_latent_exemplars_out o;
    std::memset(&o, 0, sizeof o);
    std::memcpy(&o, out, std::min<size_t>(sizeof o, (size_t)out->struct_size));
    if (!o.n_group_images || !o.n_fire || !o.top_val || !o.top_img || !o.top_patch || !o.bot_val || !o.bot_img || !o.bot_patch || !o.silent_img)
        return entry_refuse(SAEV_INVALID_ARG, who, "every output of saev_latent_exemplars_out must be set");
    ExLayout L;
    ex_layout(nnz, S, n_images, &L);
    if (const int rc = entry_check_workspace(who, workspace, workspace_bytes, L.total_bytes,
                                             "workspace smaller than saev_latent_exemplars_workspace_bytes(nnz, S, n_images, G)"))
        return rc;

    hipStream_t s = (hipStream_t)stream;
    uint8_t* ws = static_cast<uint8_t*>(workspace);
    const LmLists ev = lm_lists(ws, L.lm);
    int32_t* rank = reinterpret_cast<int32_t*>(ws + L.off_rank);
    int32_t* members = reinterpret_cast<int32_t*>(ws + L.off_members);
    int32_t* gstart = reinterpret_cast<int32_t*>(ws + L.off_gstart);
    bool ok = hipMemsetAsync(o.n_group_images, 0, (size_t)(8 * G), s) == hipSuccess;
    ok = ok && hipMemsetAsync(rank, 0, (size_t)(4 * n_images), s) == hipSuccess;
    ok = ok && lm_regroup<SAEV_LATENT_EXEMPLARS_ERR_LATENT, SAEV_LATENT_EXEMPLARS_ERR_GROUP>(
                    row_ptr, indices, data, nnz, n_images * T, S, group_i32, n_images, T, G, thr, o.n_group_images, ev,
                    reinterpret_cast<int32_t*>(ws + L.off_err), s);
    if (!ok) return entry_refuse(SAEV_HIP_ERROR, who, "hipMemsetAsync failed");
    hipLaunchKernelGGL(ex_members_kernel, dim3((unsigned)G), dim3(64), 0, s, group_i32, (int)n_images, (int)G,
                       reinterpret_cast<const unsigned long long*>(o.n_group_images), gstart, rank, members);
    ExWalk a{ev.starts, ev.row, ev.val, group_i32, rank, members, gstart, (int)S, (int)G, (int)k, (int)T, (int)n_images,
             o.n_fire, o.top_val, o.top_img, o.top_patch, o.bot_val, o.bot_img, o.bot_patch, o.silent_img};
    // the lists of a wave take G * k * 24 bytes of LDS: as many waves a workgroup (at most 4) as 64 KiB hold
    const int64_t wave_bytes = G * k * 24;
    const int waves = (int)std::max<int64_t>(1, std::min<int64_t>(4, (64 * 1024) / wave_bytes));
    hipLaunchKernelGGL(ex_walk_kernel, dim3((unsigned)((S + waves - 1) / waves)), dim3(64 * waves), (size_t)(waves * wave_bytes), s, a, waves);
    if (hipGetLastError() != hipSuccess) return entry_refuse(SAEV_HIP_ERROR, who, "kernel launch failed");
    return SAEV_OK;
}

int saev_latent_patch_rows(const int64_t* row_ptr, const int32_t* indices, const float* data, int64_t nnz, int64_t n_images, int64_t T, int64_t S,
                           const int32_t* q_latent, const int32_t* q_image, int64_t Q, float* out, int32_t* err, void* stream) {
    const char* who = "saev_latent_patch_rows";
    if (const int rc = entry_check_shape(who, n_images, S, 1, nnz)) return rc;
    if (T < 1 || T > EX_MAX_T) return entry_refuse(SAEV_UNSUPPORTED, who, "T must lie in [1, 4096]");
    if (n_images * T > 0x7fffffffLL) return entry_refuse(SAEV_UNSUPPORTED, who, "n_images * T must stay below 2^31");
    if (Q < 0) return entry_refuse(SAEV_INVALID_ARG, who, "negative size");
    if (Q > 0x7fffffffLL / T) return entry_refuse(SAEV_UNSUPPORTED, who, "Q * T must stay below 2^31");
    if (Q == 0) return SAEV_OK;
    if (!row_ptr) return entry_refuse(SAEV_INVALID_ARG, who, "row_ptr is NULL");
    if (nnz > 0 && (!indices || !data)) return entry_refuse(SAEV_INVALID_ARG, who, "indices and data come with nnz > 0");
    if (!q_latent || !q_image || !out || !err) return entry_refuse(SAEV_INVALID_ARG, who, "q_latent, q_image, out and err must not be NULL");
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(err, 0, 4, s) != hipSuccess) return entry_refuse(SAEV_HIP_ERROR, who, "hipMemsetAsync failed");
    hipLaunchKernelGGL(ex_rows_kernel, dim3((unsigned)std::min<int64_t>(Q, EX_ROWS_MAX_BLOCKS)), dim3(EX_ROWS_THREADS), 0, s, row_ptr, indices, data,
                       (long)nnz, (int)n_images, (int)T, (int)S, q_latent, q_image, (long)Q, out, err);
    if (hipGetLastError() != hipSuccess) return entry_refuse(SAEV_HIP_ERROR, who, "kernel launch failed");
    return SAEV_OK;
}
