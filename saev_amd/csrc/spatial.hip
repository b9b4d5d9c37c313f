// Where latents fire on the patch grid (include/saev_amd.h: LATENT SPATIAL): per (latent, group of images) the exact
// counts behind the spatial-coherence scores of saev_amd/spatial.py -- events, firing images, horizontal and vertical pairs of
// firing 4-neighbours, sum of m^2, the per-cell count map and its sum of squares -- and the activation-weighted moments and per-cell
// sums in a fixed order of addition.
//
//   prepare  the FIRING events latent-major in ascending row order: the regroup of latent_major.h: a valid
//            latent, the image's group in [0, G), value > thr.  Its first pass finds the row of each stored entry, checks
//            its latent and its image's group (the error word) and keeps the row of an entry that fires, or -1.
//   walk     a wave per latent, 64 events a trip.  Lane = event first: each lane loads its event and finds, by loads bounded to the
//            latent's own list, whether its right neighbour (the next element, row + 1, not past the grid row's end) and its lower
//            neighbour (row + gw, a binary search among the next gw elements, not past the image's end) fire, and -- at the first
//            event of an image -- m, the image's events (a binary search among the next T elements).  Then lane = group: the trip's
//            events are broadcast one at a time in list order and the lane that owns the event's group adds it to the integers and
//            to the five fp64 sums it keeps in registers, so every sum takes its terms in ascending row order.  The same loop
//            ranks each event among the trip's earlier events of the SAME MAP CELL; the cells are then updated by plain
//            read-modify-writes, lane = event, in rounds of equal rank with the wave's stores drained between rounds and between
//            trips: a cell takes its terms in ascending image order, and two lanes never update one cell at once.
//   overlap  a wave per (latent, group) squares and adds the cells of count_map.
//
// No floating-point atomic.  A latent that fires on most rows is one wave's serial walk.
#include "latent_major.h"

#include <algorithm>
#include <cmath>

namespace {

constexpr int SP_MAX_G = 64;
constexpr int SP_MAX_T = 4096;

bool sp_shape_ok(int64_t n_images, int64_t T, int64_t S, int64_t G, int64_t nnz) {
    if (n_images < 1 || T < 1 || T > SP_MAX_T || S < 1 || S > 0x7fffffffLL || G < 1 || G > SP_MAX_G || nnz < 0 || nnz > 0x7fffffffLL) return false;
    if (n_images > 0x7fffffffLL / T) return false;
    return S * G * T < ((int64_t)1 << 31);  // S * G * T < 2^31 * 2^18: no overflow
}

// byte offsets into the workspace (all multiples of 256); the error word comes first
struct SpLayout {
    int64_t off_err;
    LmLayout lm;
    int64_t total_bytes;
};

void sp_layout(int64_t S, int64_t nnz, SpLayout* L) {
    WsCarve ws;
    L->off_err = ws.take(64);
    lm_carve(ws, S, nnz, &L->lm);
    L->total_bytes = ws.at;
}

// ---------------------------------------------------------------- walk -------------------------------------------------------------------

struct SpWalk {
    const int64_t* starts;
    const int32_t* row;
    const float* val;
    const int32_t* group;
    int S, G, gh, gw, T;
    long long *n_events, *n_images_fire, *pairs_h, *pairs_v, *sum_m2;
    double* moments;
    int32_t* count_map;
    double* sum_map;
};

__global__ __launch_bounds__(256) void sp_walk_kernel(SpWalk a) {
    const int lane = threadIdx.x & 63;
    const long j = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= a.S) return;
    // the latent's segment, the same in every lane: held in scalars so that the broadcasts below read a lane by a scalar index
    const int lo = __builtin_amdgcn_readfirstlane((int)a.starts[j]), hi = __builtin_amdgcn_readfirstlane((int)a.starts[j + 1]);
    const int T = a.T, gw = a.gw, gh = a.gh;
    long long ne = 0, nf = 0, ph = 0, pv = 0, m2 = 0;
    double s_v = 0.0, s_vr = 0.0, s_vc = 0.0, s_vrr = 0.0, s_vcc = 0.0;
    for (int base = lo; base < hi; base += 64) {
        const int k = base + lane;
        const int n = min(64, hi - base);  // scalar
        int row = 0, g = SP_MAX_G, p = 0, r = 0, c = 0, right = 0, below = 0, m = 0;
        float v = 0.f;
        if (k < hi) {
            row = a.row[k];
            v = a.val[k];
            const int img = row / T;
            p = row - img * T;
            r = p / gw;
            c = p - r * gw;
            g = a.group[img];  // in [0, G): prepare keeps no other event
            if (c + 1 < gw && k + 1 < hi) right = a.row[k + 1] == row + 1;
            if (r + 1 < gh && k + 1 < hi) {  // rows ascend and differ: row + gw lies among the next gw elements or nowhere
                const int want = row + gw;
                int x = k + 1, y = min(k + gw, hi - 1);
                while (x < y) {
                    const int mid = x + ((y - x) >> 1);
                    if (a.row[mid] < want) x = mid + 1; else y = mid;
                }
                below = a.row[x] == want;
            }
            if (k == lo || a.row[k - 1] / T != img) {  // the image's first event: m = its events, at most T of them
                const long end_row = (long)(img + 1) * T;
                int x = k + 1, y = (int)min((long)k + T, (long)hi);
                while (x < y) {
                    const int mid = x + ((y - x) >> 1);
                    if (a.row[mid] < end_row) x = mid + 1; else y = mid;
                }
                m = x - k;
            }
        }
        const int cell = k < hi ? g * T + p : -1 - lane;  // below 2^18; a lane without an event matches nobody
        const int word = g | (right << 8) | (below << 9) | (m << 10), rc = r | (c << 16);
        int rank = 0;
        for (int i = 0; i < n; ++i) {
            const int word_i = __builtin_amdgcn_readlane(word, i), rc_i = __builtin_amdgcn_readlane(rc, i);
            const int cell_i = __builtin_amdgcn_readlane(cell, i);
            const double dv = (double)__int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), i));
            if (lane > i && cell == cell_i) ++rank;
            if (lane == (word_i & 0xff)) {
                const int m_i = word_i >> 10, r_i = rc_i & 0xffff, c_i = rc_i >> 16;
                ne += 1;
                ph += (word_i >> 8) & 1;
                pv += (word_i >> 9) & 1;
                if (m_i > 0) {
                    nf += 1;
                    m2 += (long long)m_i * m_i;
                }
                // the products are exact (24 bits by at most 24); every sum takes one term, in list order
                s_v = __dadd_rn(s_v, dv);
                s_vr = __dadd_rn(s_vr, __dmul_rn(dv, (double)r_i));
                s_vc = __dadd_rn(s_vc, __dmul_rn(dv, (double)c_i));
                s_vrr = __dadd_rn(s_vrr, __dmul_rn(dv, (double)(r_i * r_i)));
                s_vcc = __dadd_rn(s_vcc, __dmul_rn(dv, (double)(c_i * c_i)));
            }
        }
        // the maps: rounds of equal rank, the wave's stores drained before the next round's (and the next trip's) loads
        int rounds = rank;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) rounds = max(rounds, __shfl_xor(rounds, o, 64));
        rounds = __builtin_amdgcn_readfirstlane(rounds);
        for (int q = 0; q <= rounds; ++q) {
            if (k < hi && rank == q) {
                const size_t at = ((size_t)j * a.G + g) * T + p;
                a.count_map[at] += 1;
                if (a.sum_map) a.sum_map[at] = __dadd_rn(a.sum_map[at], (double)v);
            }
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        }
    }
    if (lane < a.G) {
        const size_t o = (size_t)j * a.G + lane;
        a.n_events[o] = ne;
        a.n_images_fire[o] = nf;
        a.pairs_h[o] = ph;
        a.pairs_v[o] = pv;
        a.sum_m2[o] = m2;
        a.moments[o * 5 + 0] = s_v;
        a.moments[o * 5 + 1] = s_vr;
        a.moments[o * 5 + 2] = s_vc;
        a.moments[o * 5 + 3] = s_vrr;
        a.moments[o * 5 + 4] = s_vcc;
    }
}

// overlap[j, g] = sum over p of count_map[j, g, p]^2: a wave per pair
__global__ __launch_bounds__(256) void sp_overlap_kernel(const int32_t* __restrict__ count_map, long pairs, int T, long long* __restrict__ overlap) {
    const int lane = threadIdx.x & 63;
    const long o = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (o >= pairs) return;
    long long sum = 0;
    for (int p = lane; p < T; p += 64) {
        const long long n = count_map[(size_t)o * T + p];
        sum += n * n;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) sum += __shfl_xor(sum, d, 64);
    if (lane == 0) overlap[o] = sum;
}

}  // namespace

// ---------------------------------------------------------------- C ABI ------------------------------------------------------------------

int64_t saev_latent_spatial_workspace_bytes(int64_t n_images, int64_t T, int64_t S, int64_t G, int64_t nnz) {
    if (!sp_shape_ok(n_images, T, S, G, nnz)) return -1;
    SpLayout L;
    sp_layout(S, nnz, &L);
    return L.total_bytes;
}

int saev_latent_spatial(const int64_t* row_ptr, const int32_t* indices, const float* data, int64_t nnz, int64_t N, int64_t n_images, int64_t gh,
                        int64_t gw, int64_t S, const int32_t* group_i32, int64_t G, float thr, int64_t* n_group_images, int64_t* n_events,
                        int64_t* n_images_fire, int64_t* pairs_h, int64_t* pairs_v, int64_t* sum_m2, int64_t* overlap, double* moments,
                        int32_t* count_map, double* sum_map, void* workspace, int64_t workspace_bytes, void* stream) {
    const char* who = "saev_latent_spatial";
    if (N < 0 || S < 0 || nnz < 0 || n_images < 0 || gh < 0 || gw < 0 || G < 0) return entry_refuse(SAEV_INVALID_ARG, who, "negative size");
    if (N > 0x7fffffffLL || S > 0x7fffffffLL || nnz > 0x7fffffffLL) return entry_refuse(SAEV_UNSUPPORTED, who, "N, S and nnz must stay below 2^31");
    if (N < 1 || S < 1) return entry_refuse(SAEV_INVALID_ARG, who, "N and S must be at least 1");
    if (G < 1 || G > SP_MAX_G) return entry_refuse(SAEV_UNSUPPORTED, who, "the number of groups must lie in [1, 64]");
    if (gh < 1 || gw < 1 || gh > SP_MAX_T || gw > SP_MAX_T || gh * gw > SP_MAX_T)
        return entry_refuse(SAEV_UNSUPPORTED, who, "the grid must have gh, gw >= 1 and at most 4096 positions");
    const int64_t T = gh * gw;
    if (n_images > 0x7fffffffLL || N != n_images * T) return entry_refuse(SAEV_INVALID_ARG, who, "N must equal n_images * gh * gw");
    if (S * G * T >= ((int64_t)1 << 31)) return entry_refuse(SAEV_UNSUPPORTED, who, "S * G * gh * gw must stay below 2^31");
    if (!(thr >= 0.f)) return entry_refuse(SAEV_INVALID_ARG, who, "thr must be at least 0");
    if (!row_ptr) return entry_refuse(SAEV_INVALID_ARG, who, "row_ptr is NULL");
    if (nnz > 0 && (!indices || !data)) return entry_refuse(SAEV_INVALID_ARG, who, "indices and data come with nnz > 0");
    if (!group_i32) return entry_refuse(SAEV_INVALID_ARG, who, "group_i32 must not be NULL");
    if (!n_group_images || !n_events || !n_images_fire || !pairs_h || !pairs_v || !sum_m2 || !overlap || !moments || !count_map)
        return entry_refuse(SAEV_INVALID_ARG, who,
                            "n_group_images, n_events, n_images_fire, pairs_h, pairs_v, sum_m2, overlap, moments and count_map must not be NULL");
    SpLayout L;
    sp_layout(S, nnz, &L);
    if (const int rc = entry_check_workspace(who, workspace, workspace_bytes, L.total_bytes,
                                             "workspace smaller than saev_latent_spatial_workspace_bytes(n_images, T, S, G, nnz)"))
        return rc;

    hipStream_t s = (hipStream_t)stream;
    uint8_t* ws = static_cast<uint8_t*>(workspace);
    const LmLists ev = lm_lists(ws, L.lm);
    const size_t cells = (size_t)(S * G * T);
    bool ok = hipMemsetAsync(n_group_images, 0, (size_t)(8 * G), s) == hipSuccess;
    ok = ok && hipMemsetAsync(count_map, 0, 4 * cells, s) == hipSuccess;
    if (sum_map) ok = ok && hipMemsetAsync(sum_map, 0, 8 * cells, s) == hipSuccess;
    ok = ok && lm_regroup<SAEV_LATENT_SPATIAL_ERR_LATENT, SAEV_LATENT_SPATIAL_ERR_GROUP>(
                    row_ptr, indices, data, nnz, N, S, group_i32, n_images, T, G, thr, n_group_images, ev, reinterpret_cast<int32_t*>(ws + L.off_err), s);
    if (!ok) return entry_refuse(SAEV_HIP_ERROR, who, "hipMemsetAsync failed");
    SpWalk a{ev.starts, ev.row, ev.val, group_i32, (int)S, (int)G, (int)gh, (int)gw, (int)T,
             reinterpret_cast<long long*>(n_events), reinterpret_cast<long long*>(n_images_fire), reinterpret_cast<long long*>(pairs_h),
             reinterpret_cast<long long*>(pairs_v), reinterpret_cast<long long*>(sum_m2), moments, count_map, sum_map};
    hipLaunchKernelGGL(sp_walk_kernel, dim3((unsigned)((S + 3) / 4)), dim3(256), 0, s, a);
    hipLaunchKernelGGL(sp_overlap_kernel, dim3((unsigned)((S * G + 3) / 4)), dim3(256), 0, s, count_map, (long)(S * G), (int)T,
                       reinterpret_cast<long long*>(overlap));
    if (hipGetLastError() != hipSuccess) return entry_refuse(SAEV_HIP_ERROR, who, "kernel launch failed");
    return SAEV_OK;
}
