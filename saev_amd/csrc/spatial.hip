// Where latents fire on the patch grid (include/saev_amd.h: LATENT SPATIAL): per (latent, group of images) the exact
// counts behind the spatial-coherence scores of saev_amd/spatial.py -- events, firing images, horizontal and vertical pairs of
// firing 4-neighbours, sum of m^2, the per-cell count map and its sum of squares -- and the activation-weighted moments and per-cell
// sums in a fixed order of addition.
//
//   prepare  the FIRING events latent-major in ascending row order, as probe1d.hip's prepare leaves its entries: one pass over the
//            stored entries finds the row of each, checks its latent and its image's group (the error word) and keeps the row of an
//            entry that fires (value > thr, group >= 0) or -1; integer atomics count every (part, latent); a pass per latent and
//            one scan give the segments; ONE WAVE PER PART places its entries in order (rows ascend inside a part, parts are in row
//            order, so every segment is in ascending row order whatever the timing).
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
// No floating-point atomic.  A latent that fires on most rows is one wave's serial walk.  The parts, scan and place
// kernels restate probe1d.hip's with the event rule in front of them; that unit is left as it is.
#include "entry_util.h"

#include <algorithm>
#include <cmath>

namespace {

constexpr int SP_MAX_G = 64;
constexpr int SP_MAX_T = 4096;
constexpr int SP_PARTS = 1024;  // at most this many contiguous parts of the stored entries in prepare's stable counting sort (4 096
                                // parts bought the place pass an eighth and cost 200 MB of count table: its stores are the floor)
constexpr int SP_SCAN_THREADS = 1024;

int sp_parts(int64_t S, int64_t nnz) {
    int64_t p = std::min<int64_t>(SP_PARTS, (nnz + 63) / 64);
    p = std::min<int64_t>(p, std::max<int64_t>(1, ((int64_t)1 << 26) / std::max<int64_t>(S, 1)));
    return (int)std::max<int64_t>(p, 1);
}
int64_t sp_part_len(int64_t nnz, int parts) { return std::max<int64_t>(64, ((nnz + parts - 1) / parts + 63) / 64 * 64); }

bool sp_shape_ok(int64_t n_images, int64_t T, int64_t S, int64_t G, int64_t nnz) {
    if (n_images < 1 || T < 1 || T > SP_MAX_T || S < 1 || S > 0x7fffffffLL || G < 1 || G > SP_MAX_G || nnz < 0 || nnz > 0x7fffffffLL) return false;
    if (n_images > 0x7fffffffLL / T) return false;
    return S * G * T < ((int64_t)1 << 31);  // S * G * T < 2^31 * 2^18: no overflow
}

// byte offsets into the workspace (all multiples of 256); the error word comes first
struct SpLayout {
    int64_t parts, part_len, total_bytes;
    int64_t off_err, off_starts, off_tot, off_cnt, off_fire_row, off_row, off_val;
};

void sp_layout(int64_t S, int64_t nnz, SpLayout* L) {
    *L = SpLayout{};
    L->parts = sp_parts(S, nnz);
    L->part_len = sp_part_len(nnz, (int)L->parts);
    WsCarve ws;
    L->off_err = ws.take(64);
    L->off_starts = ws.take(8 * (S + 1));
    L->off_tot = ws.take(4 * S);
    L->off_cnt = ws.take(4 * L->parts * S);
    L->off_fire_row = ws.take(4 * nnz);
    L->off_row = ws.take(4 * nnz);
    L->off_val = ws.take(4 * nnz);
    L->total_bytes = ws.at;
}

// ---------------------------------------------------------------- prepare ----------------------------------------------------------------

// n_group[g] = images of group g; a group id outside [-1, G) is reported
__global__ __launch_bounds__(256) void sp_groups_kernel(const int32_t* __restrict__ group, long n_images, int G, unsigned long long* __restrict__ n_group,
                                                        int32_t* __restrict__ err) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n_images; i += (long)gridDim.x * 256) {
        const int g = group[i];
        if (g < -1 || g >= G) atomicMax(err, SAEV_LATENT_SPATIAL_ERR_GROUP);
        else if (g >= 0) atomicAdd(n_group + g, 1ull);
    }
}

// the first pass over the entries: fire_row[e] = the row of entry e when it is an event of a valid latent in an image of a group in
// [0, G), else -1; cnt[part][latent] counts the events
__global__ __launch_bounds__(256) void sp_count_kernel(const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ indices,
                                                       const float* __restrict__ data, const int32_t* __restrict__ group, long nnz, int N, int S,
                                                       int T, int G, float thr, long part_len, int32_t* __restrict__ fire_row,
                                                       int32_t* __restrict__ cnt, int32_t* __restrict__ err) {
    const int64_t p0 = row_ptr[0];
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < nnz; e += (long)gridDim.x * 256) {
        const int col = indices[p0 + e];
        const int row = csr_row_of(row_ptr, N, p0 + e);
        const int g = group[row / T];
        int keep = -1;
        if (col < 0 || col >= S) atomicMax(err, SAEV_LATENT_SPATIAL_ERR_LATENT);
        else if (g < -1 || g >= G) atomicMax(err, SAEV_LATENT_SPATIAL_ERR_GROUP);
        else if (g >= 0 && data[p0 + e] > thr) {  // NaN compares false
            keep = row;
            atomicAdd(cnt + (e / part_len) * S + col, 1);
        }
        fire_row[e] = keep;
    }
}

// cnt[p][l] -> the events of latent l in parts before p; tot[l] = all of them
__global__ __launch_bounds__(256) void sp_parts_kernel(int32_t* __restrict__ cnt, int parts, int S, int32_t* __restrict__ tot) {
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

__global__ __launch_bounds__(SP_SCAN_THREADS) void sp_scan_kernel(const int32_t* __restrict__ tot, int S, int64_t* __restrict__ starts) {
    const long long end = block_scan_rounds<SP_SCAN_THREADS, long long, long>(
        S, [&](long l) { return (long long)tot[l]; }, [&](long l, long long start) { starts[l] = start; });
    if (threadIdx.x == 0) starts[S] = end;
}

// one wave per part (see the head of probe1d.hip): the rank of an event among the 64 of its trip by comparing lanes, the trip's base
// by one integer atomic on a cursor only this wave touches
__global__ __launch_bounds__(64) void sp_place_kernel(const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ indices, const float* __restrict__ data,
                                                      const int32_t* __restrict__ fire_row, long nnz, int S, long part_len,
                                                      const int64_t* __restrict__ starts, int32_t* __restrict__ cnt,
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
    int32_t* err = reinterpret_cast<int32_t*>(ws + L.off_err);
    int64_t* starts = reinterpret_cast<int64_t*>(ws + L.off_starts);
    int32_t* tot = reinterpret_cast<int32_t*>(ws + L.off_tot);
    int32_t* cnt = reinterpret_cast<int32_t*>(ws + L.off_cnt);
    int32_t* fire_row = reinterpret_cast<int32_t*>(ws + L.off_fire_row);
    int32_t* row = reinterpret_cast<int32_t*>(ws + L.off_row);
    float* val = reinterpret_cast<float*>(ws + L.off_val);
    const size_t cells = (size_t)(S * G * T);
    bool ok = hipMemsetAsync(err, 0, 64, s) == hipSuccess;
    ok = ok && hipMemsetAsync(cnt, 0, (size_t)(4 * L.parts * S), s) == hipSuccess;
    ok = ok && hipMemsetAsync(n_group_images, 0, (size_t)(8 * G), s) == hipSuccess;
    ok = ok && hipMemsetAsync(count_map, 0, 4 * cells, s) == hipSuccess;
    if (sum_map) ok = ok && hipMemsetAsync(sum_map, 0, 8 * cells, s) == hipSuccess;
    if (!ok) return entry_refuse(SAEV_HIP_ERROR, who, "hipMemsetAsync failed");
    hipLaunchKernelGGL(sp_groups_kernel, dim3((unsigned)std::min<int64_t>((n_images + 255) / 256, 1024)), dim3(256), 0, s, group_i32, (long)n_images,
                       (int)G, reinterpret_cast<unsigned long long*>(n_group_images), err);
    if (nnz > 0)
        hipLaunchKernelGGL(sp_count_kernel, dim3((unsigned)std::min<int64_t>((nnz + 255) / 256, 8192)), dim3(256), 0, s, row_ptr, indices, data, group_i32,
                           (long)nnz, (int)N, (int)S, (int)T, (int)G, thr, (long)L.part_len, fire_row, cnt, err);
    hipLaunchKernelGGL(sp_parts_kernel, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, s, cnt, (int)L.parts, (int)S, tot);
    hipLaunchKernelGGL(sp_scan_kernel, dim3(1), dim3(SP_SCAN_THREADS), 0, s, tot, (int)S, starts);
    if (nnz > 0) {
        const unsigned used = (unsigned)((nnz + L.part_len - 1) / L.part_len);
        hipLaunchKernelGGL(sp_place_kernel, dim3(used), dim3(64), 0, s, row_ptr, indices, data, fire_row, (long)nnz, (int)S, (long)L.part_len, starts,
                           cnt, row, val);
    }
    SpWalk a{starts, row, val, group_i32, (int)S, (int)G, (int)gh, (int)gw, (int)T,
             reinterpret_cast<long long*>(n_events), reinterpret_cast<long long*>(n_images_fire), reinterpret_cast<long long*>(pairs_h),
             reinterpret_cast<long long*>(pairs_v), reinterpret_cast<long long*>(sum_m2), moments, count_map, sum_map};
    hipLaunchKernelGGL(sp_walk_kernel, dim3((unsigned)((S + 3) / 4)), dim3(256), 0, s, a);
    hipLaunchKernelGGL(sp_overlap_kernel, dim3((unsigned)((S * G + 3) / 4)), dim3(256), 0, s, count_map, (long)(S * G), (int)T,
                       reinterpret_cast<long long*>(overlap));
    if (hipGetLastError() != hipSuccess) return entry_refuse(SAEV_HIP_ERROR, who, "kernel launch failed");
    return SAEV_OK;
}
