// Interventions on latents (include/saev_amd.h: LATENT EDITS and CLASS FIRING COUNTS), context-free.
//
// EDITS.  x' = (x - x_hat) + x_hat_mod = x + sum_e (t_e(f_l) - f_l) W_dec[l_e, :]: b_dec and every unedited latent cancel, so the
// reference's two dense decodes become one streaming pass over x with a few W_dec rows out of L2.
//
//   plan     (host) the caller's edits validated and regrouped: the global list, then each group's list, with a CSR over the
//            lists; a record is {latent, op, value, the caller's index of the edit}.
//   rows     one wave per row, four rows a workgroup.  Phase 1: the lanes hold the row's first 64 code slots in registers (later
//            slots are read 64 at a time), the applicable records are loaded 64 at a time and broadcast one by one; a ballot finds
//            the edit's latent among the slots, the coefficient c_e is formed from the ORIGINAL f, and the edits that remain
//            (c_e != 0) are appended to the wave's list in LDS.  Phase 2: float4 trips over D, four in flight; each starts from x
//            and takes one fmaf per remaining edit, in list order.  A row without a remaining edit is copied (or, in place, left
//            alone): its bits are x's.
//   counts   rows_changed through a 256-slot direct-mapped table in LDS keyed by the record's position in the plan: a workgroup
//            sums there first and adds each slot once at its end; a record that finds its slot taken by another adds directly.
//            Integer atomics only; every float is written once, by one lane, from operands that do not depend on the schedule.
//
// FIRING COUNTS.  One thread per code slot: m = #{t : v > thr_t} and, when m >= 1, one integer atomic on hist[label][m - 1][s]
// and one on pos[m - 1][s] (the suffix sums over the threshold bins are taken when F1 is formed).  Rows per class are summed in
// LDS by a second, small kernel.  F1 is one thread per (class, latent).
#include "entry_util.h"

#include <algorithm>
#include <cstring>
#include <vector>

namespace {

constexpr int IV_MAX_EDITS = 65536;
constexpr int IV_MAX_GROUPS = 65536;
constexpr int IV_MAX_LIST = 256;            // edits in one list; a row sees the global list and one group list
constexpr int IV_WAVES = 4;                 // rows per workgroup
constexpr int IV_ROW_EDITS = 2 * IV_MAX_LIST;
constexpr int IV_CNT_SLOTS = 256;
constexpr int IV_TRIPS = 4;                 // trips of a wave over D in flight
constexpr int IV_MAX_GRID = 2048;           // workgroups; the rows beyond are strided over (8 a CU: the residency of the kernel)

constexpr int CF_CODES_MAX_GRID = 8192;     // workgroups of 256 threads; the code slots, rows and (class, latent) pairs beyond are
constexpr int CF_ROWS_MAX_GRID = 1024;      // strided over
constexpr int CF_F1_MAX_GRID = 8192;

constexpr int OP_MASK = 3;

struct IvPlanLayout {
    int64_t off_ptr, off_rec, total;
};

// list 0 is the global list, list g + 1 group g's: ptr (G + 2 int32), then the records (16 bytes each)
IvPlanLayout iv_plan_layout(int64_t E, int64_t G) {
    WsCarve c;
    IvPlanLayout l;
    l.off_ptr = c.take(4 * (G + 2));
    l.off_rec = c.take(16 * E);
    l.total = c.at;
    return l;
}

struct IvArgs {
    const float* x;
    const float* W;
    const int32_t* idx;
    const float* val;
    const int32_t* row_nnz;
    const int32_t* ptr;       // G + 2
    const int4* rec;          // E
    const int32_t* row_group;
    const uint8_t* row_keep;
    float* out;
    unsigned long long* rows_changed;
    int n, D, S, cap, E, G;
};

__device__ __forceinline__ void iv_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// phase 2 on elements of type V (float4 or float): NV of them in a row, W rows NV apart
template <typename V>
__device__ __forceinline__ void iv_apply(const V* __restrict__ W, const V* xr, V* outr, int NV, int lane, int m, const int* s_lat,
                                         const float* s_c) {
    for (int q0 = lane; q0 < NV; q0 += 64 * IV_TRIPS) {
        V acc[IV_TRIPS];
#pragma unroll
        for (int u = 0; u < IV_TRIPS; ++u) {
            const int q = q0 + 64 * u;
            if (q < NV) acc[u] = xr[q];
        }
#pragma unroll 2
        for (int e = 0; e < m; ++e) {
            const float c = s_c[e];
            const V* wr = W + (size_t)s_lat[e] * NV;
            V w[IV_TRIPS];
#pragma unroll
            for (int u = 0; u < IV_TRIPS; ++u) {
                const int q = q0 + 64 * u;
                if (q < NV) w[u] = wr[q];
            }
#pragma unroll
            for (int u = 0; u < IV_TRIPS; ++u) {
                const int q = q0 + 64 * u;
                if (q < NV) {
                    if constexpr (sizeof(V) == 16) {
#pragma unroll
                        for (int i = 0; i < 4; ++i) acc[u][i] = __builtin_fmaf(c, w[u][i], acc[u][i]);
                    } else {
                        acc[u] = __builtin_fmaf(c, w[u], acc[u]);
                    }
                }
            }
        }
#pragma unroll
        for (int u = 0; u < IV_TRIPS; ++u) {
            const int q = q0 + 64 * u;
            if (q < NV) outr[q] = acc[u];
        }
    }
}

template <bool VEC>
__global__ __launch_bounds__(IV_WAVES * 64) void iv_rows_kernel(IvArgs a) {
    __shared__ int s_lat[IV_WAVES][IV_ROW_EDITS];
    __shared__ float s_c[IV_WAVES][IV_ROW_EDITS];
    __shared__ int s_tag[IV_CNT_SLOTS];
    __shared__ unsigned s_cnt[IV_CNT_SLOTS];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const bool counting = a.rows_changed != nullptr;
    if (counting) {
        for (int i = threadIdx.x; i < IV_CNT_SLOTS; i += IV_WAVES * 64) { s_tag[i] = -1; s_cnt[i] = 0u; }
        __syncthreads();
    }
    for (long b = (long)blockIdx.x * IV_WAVES + w; b < a.n; b += (long)gridDim.x * IV_WAVES) {
        // the lists of this row: [lo[0], hi[0]) global, [lo[1], hi[1]) its group's; every bound clamped to the plan
        int lo[2] = {0, 0}, hi[2] = {0, 0};
        if (a.E > 0 && (a.row_keep == nullptr || a.row_keep[b] != 0)) {
            lo[0] = 0;
            hi[0] = min(max(a.ptr[1], 0), a.E);
            const int g = a.row_group != nullptr ? a.row_group[b] : -1;
            if (g >= 0 && g < a.G) {
                lo[1] = min(max(a.ptr[g + 1], 0), a.E);
                hi[1] = min(max(a.ptr[g + 2], lo[1]), a.E);
                if (hi[1] - lo[1] > IV_MAX_LIST) hi[1] = lo[1] + IV_MAX_LIST;
            }
            if (hi[0] > IV_MAX_LIST) hi[0] = IV_MAX_LIST;
        }
        int m = 0;
        if (hi[0] + hi[1] - lo[1] > 0) {
            const int nnz = a.row_nnz != nullptr ? min(max(a.row_nnz[b], 0), a.cap) : a.cap;
            const int32_t* ir = a.idx + (size_t)b * a.cap;
            const float* vr = a.val + (size_t)b * a.cap;
            const int idx0 = lane < nnz ? ir[lane] : -1;
            const float val0 = lane < nnz ? vr[lane] : 0.f;
#pragma unroll
            for (int part = 0; part < 2; ++part) {
                for (int p0 = lo[part]; p0 < hi[part]; p0 += 64) {
                    const int cnt = min(64, hi[part] - p0);
                    int4 r = make_int4(-1, 0, 0, 0);
                    if (lane < cnt) r = a.rec[p0 + lane];
                    for (int j = 0; j < cnt; ++j) {
                        const int lat = __shfl(r.x, j, 64);
                        const int op = __shfl(r.y, j, 64);
                        const float value = __int_as_float(__shfl(r.z, j, 64));
                        const int orig = __shfl(r.w, j, 64);
                        if (lat < 0 || lat >= a.S || orig < 0 || orig >= a.E) continue;  // (cannot happen with a plan built for this S)
                        float f = 0.f;
                        unsigned long long hit = __ballot(idx0 == lat);
                        if (hit != 0ull) {
                            f = __shfl(val0, __ffsll((long long)hit) - 1, 64);
                        } else {
                            for (int base = 64; base < nnz; base += 64) {
                                const bool in = base + lane < nnz;
                                hit = __ballot(in && ir[base + lane] == lat);
                                if (hit != 0ull) {
                                    const int src = __ffsll((long long)hit) - 1;
                                    f = vr[base + src];
                                    break;
                                }
                            }
                        }
                        if ((op & SAEV_EDIT_IF_ACTIVE) != 0 && f == 0.f) continue;
                        float c;
                        switch (op & OP_MASK) {
                            case SAEV_EDIT_SET: c = value - f; break;
                            case SAEV_EDIT_SCALE: c = __builtin_fmaf(value, f, -f); break;
                            default: c = value; break;
                        }
                        if (c == 0.f) continue;
                        if (lane == 0) {
                            s_lat[w][m] = lat;
                            s_c[w][m] = c;
                            if (counting) {
                                const int p = p0 + j, slot = p & (IV_CNT_SLOTS - 1);
                                const int old = atomicCAS(&s_tag[slot], -1, p);
                                if (old == -1 || old == p) atomicAdd(&s_cnt[slot], 1u);
                                else atomicAdd(a.rows_changed + orig, 1ull);
                            }
                        }
                        ++m;
                    }
                }
            }
        }
        if (m == 0 && a.out == a.x) continue;
        iv_wave_sync();
        if constexpr (VEC) {
            iv_apply<f32x4>(reinterpret_cast<const f32x4*>(a.W), reinterpret_cast<const f32x4*>(a.x) + (size_t)b * (a.D / 4),
                            reinterpret_cast<f32x4*>(a.out) + (size_t)b * (a.D / 4), a.D / 4, lane, m, s_lat[w], s_c[w]);
        } else {
            iv_apply<float>(a.W, a.x + (size_t)b * a.D, a.out + (size_t)b * a.D, a.D, lane, m, s_lat[w], s_c[w]);
        }
        iv_wave_sync();
    }
    if (counting) {
        __syncthreads();
        for (int i = threadIdx.x; i < IV_CNT_SLOTS; i += IV_WAVES * 64) {
            const int p = s_tag[i];
            if (p >= 0 && p < a.E && s_cnt[i] != 0u) {
                const int orig = a.rec[p].w;
                if (orig >= 0 && orig < a.E) atomicAdd(a.rows_changed + orig, (unsigned long long)s_cnt[i]);
            }
        }
    }
}

// ---- firing counts ---------------------------------------------------------------------------------------------------------------

struct CfThr {
    float t[8];
};

__global__ __launch_bounds__(256) void cf_codes_kernel(const int32_t* __restrict__ idx, const float* __restrict__ val,
                                                       const int32_t* __restrict__ row_nnz, int cap, long total,
                                                       const int32_t* __restrict__ label, const uint8_t* __restrict__ keep, int S, int C,
                                                       CfThr thr, int T, unsigned* __restrict__ hist, unsigned* __restrict__ pos) {
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const long r = e / cap;
        const int slot = (int)(e - r * cap);
        if (keep != nullptr && keep[r] == 0) continue;
        const int c = label[r];
        if (c < 0 || c >= C) continue;
        if (row_nnz != nullptr && slot >= row_nnz[r]) continue;
        const int s = idx[e];
        if (s < 0 || s >= S) continue;
        const float v = val[e];
        int m = 0;
#pragma unroll
        for (int t = 0; t < 8; ++t) m += (t < T && v > thr.t[t]) ? 1 : 0;
        if (m == 0) continue;
        atomicAdd(hist + ((size_t)c * T + (m - 1)) * S + s, 1u);
        atomicAdd(pos + (size_t)(m - 1) * S + s, 1u);
    }
}

// rows per class: summed in LDS (C <= ENTRY_MAX_C counters), one atomic per class and workgroup
__global__ __launch_bounds__(256) void cf_rows_kernel(const int32_t* __restrict__ label, const uint8_t* __restrict__ keep, int n, int C,
                                                      unsigned long long* __restrict__ n_rows_c) {
    extern __shared__ unsigned cf_cnt[];
    for (int i = threadIdx.x; i < C; i += 256) cf_cnt[i] = 0u;
    __syncthreads();
    for (long r = (long)blockIdx.x * 256 + threadIdx.x; r < n; r += (long)gridDim.x * 256) {
        if (keep != nullptr && keep[r] == 0) continue;
        const int c = label[r];
        if (c >= 0 && c < C) atomicAdd(&cf_cnt[c], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < C; i += 256)
        if (cf_cnt[i] != 0u) atomicAdd(n_rows_c + i, (unsigned long long)cf_cnt[i]);
}

__global__ __launch_bounds__(256) void cf_f1_kernel(const unsigned* __restrict__ hist, const unsigned* __restrict__ pos,
                                                    const long long* __restrict__ n_rows_c, int S, int C, int T,
                                                    const uint8_t* __restrict__ mask, float* __restrict__ f1, uint8_t* __restrict__ best_t) {
    const long total = (long)C * S;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int c = (int)(i / S), s = (int)(i - (long)c * S);
        if (mask != nullptr && mask[s] == 0) {
            f1[i] = -1.f;
            best_t[i] = 0;
            continue;
        }
        const long long nc = n_rows_c[c];
        long long tp = 0, ps = 0;
        float best = -1.f;
        int bt = 0;
        for (int t = T - 1; t >= 0; --t) {  // suffix sums; ">=" hands a tie to the lower t
            tp += hist[((size_t)c * T + t) * S + s];
            ps += pos[(size_t)t * S + s];
            const long long fp = ps - tp, fn = nc - tp;
            const float v = (float)(2 * tp) / ((float)(2 * tp + fp + fn) + 1e-10f);
            if (v >= best) { best = v; bt = t; }
        }
        f1[i] = best;
        best_t[i] = (uint8_t)bt;
    }
}

bool overlaps(const void* a, int64_t a_bytes, const void* b, int64_t b_bytes) {
    if (!a || !b || a_bytes <= 0 || b_bytes <= 0) return false;
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + (uintptr_t)b_bytes && b0 < a0 + (uintptr_t)a_bytes;
}

}  // namespace

int64_t saev_edit_plan_bytes(int64_t n_edits, int64_t n_groups) {
    if (n_edits < 0 || n_edits > IV_MAX_EDITS || n_groups < 0 || n_groups > IV_MAX_GROUPS) return -1;
    return iv_plan_layout(n_edits, n_groups).total;
}

int saev_edit_plan_build(const saev_edit* edits_host, int64_t n_edits, int64_t n_groups, int64_t S, void* plan_dev, int64_t plan_bytes,
                         void* stream) {
    const char* who = "saev_edit_plan_build";
    // 1. sizes
    if (n_edits < 0 || n_groups < 0 || S < 0) return entry_refuse(SAEV_INVALID_ARG, who, "negative size");
    if (n_edits > IV_MAX_EDITS || n_groups > IV_MAX_GROUPS) return entry_refuse(SAEV_UNSUPPORTED, who, "at most 65536 edits and 65536 groups");
    if (S < 1 || S > 0x7fffffffLL) return entry_refuse(SAEV_INVALID_ARG, who, "S must lie in [1, 2^31)");
    if (n_edits > 0 && !edits_host) return entry_refuse(SAEV_INVALID_ARG, who, "edits is NULL");
    // 2. latents, 3. ops, 4. groups
    for (int64_t e = 0; e < n_edits; ++e)
        if (edits_host[e].latent < 0 || edits_host[e].latent >= S) return entry_refuse(SAEV_INVALID_ARG, who, "an edit's latent lies outside [0, S)");
    for (int64_t e = 0; e < n_edits; ++e) {
        const int32_t op = edits_host[e].op;
        if (op < 0 || (op & ~(OP_MASK | SAEV_EDIT_IF_ACTIVE)) != 0 || (op & OP_MASK) > SAEV_EDIT_ADD)
            return entry_refuse(SAEV_INVALID_ARG, who, "unknown op (SET, SCALE or ADD, with or without IF_ACTIVE)");
    }
    for (int64_t e = 0; e < n_edits; ++e)
        if (edits_host[e].group < -1 || edits_host[e].group >= n_groups) return entry_refuse(SAEV_INVALID_ARG, who, "an edit's group lies outside [-1, n_groups)");
    // 5. list lengths
    const IvPlanLayout lay = iv_plan_layout(n_edits, n_groups);
    std::vector<int32_t> ptr((size_t)n_groups + 2, 0);
    for (int64_t e = 0; e < n_edits; ++e) ++ptr[(size_t)edits_host[e].group + 2];  // (counts of list l at ptr[l + 1], shifted below)
    for (int64_t l = 0; l <= n_groups; ++l)
        if (ptr[(size_t)l + 1] > IV_MAX_LIST) return entry_refuse(SAEV_UNSUPPORTED, who, "more than 256 edits in the global list or in one group's list");
    for (int64_t l = 0; l <= n_groups; ++l) ptr[(size_t)l + 1] += ptr[(size_t)l];
    // the records grouped, the caller's order kept inside a list
    std::vector<int32_t> rec(4 * (size_t)std::max<int64_t>(n_edits, 1), 0);
    {
        std::vector<int32_t> cur(ptr.begin(), ptr.end() - 1);
        for (int64_t e = 0; e < n_edits; ++e) {
            const int32_t at = cur[(size_t)edits_host[e].group + 1]++;
            int32_t* r = rec.data() + 4 * (size_t)at;
            r[0] = edits_host[e].latent;
            r[1] = edits_host[e].op;
            std::memcpy(r + 2, &edits_host[e].value, 4);
            r[3] = (int32_t)e;
        }
    }
    // 6. a latent once per list, and not in both the global list and a group's
    {
        std::vector<int32_t> lats;
        auto sorted_list = [&](int64_t l) {
            lats.clear();
            for (int32_t p = ptr[(size_t)l]; p < ptr[(size_t)l + 1]; ++p) lats.push_back(rec[4 * (size_t)p]);
            std::sort(lats.begin(), lats.end());
        };
        sorted_list(0);
        const std::vector<int32_t> global = lats;
        for (int64_t l = 0; l <= n_groups; ++l) {
            sorted_list(l);
            if (std::adjacent_find(lats.begin(), lats.end()) != lats.end())
                return entry_refuse(SAEV_INVALID_ARG, who, "a latent is edited twice in one list (edits do not compose)");
            if (l == 0) continue;
            for (const int32_t x : lats)
                if (std::binary_search(global.begin(), global.end(), x))
                    return entry_refuse(SAEV_INVALID_ARG, who, "a latent is edited in the global list and in a group's list (edits do not compose)");
        }
    }
    if (!plan_dev && plan_bytes == 0) return SAEV_OK;  // validation alone
    if (!plan_dev || plan_bytes < lay.total) return entry_refuse(SAEV_INVALID_ARG, who, "plan smaller than saev_edit_plan_bytes(n_edits, n_groups)");
    if (((uintptr_t)plan_dev & 255) != 0) return entry_refuse(SAEV_INVALID_ARG, who, "plan must be 256-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    uint8_t* dev = static_cast<uint8_t*>(plan_dev);
    // the host images die with this call: the copies are waited for
    if (hipMemcpyAsync(dev + lay.off_ptr, ptr.data(), ptr.size() * 4, hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemcpyAsync(dev + lay.off_rec, rec.data(), rec.size() * 4, hipMemcpyHostToDevice, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
        return entry_refuse(SAEV_HIP_ERROR, who, "copy of the plan to the device failed");
    return SAEV_OK;
}

int saev_intervene_rows(const float* x, int64_t n_rows, int64_t D, const float* W_dec, int64_t S, const int32_t* idx, const float* val,
                        const int32_t* row_nnz, int64_t row_cap, const void* plan_dev, int64_t n_edits, int64_t n_groups,
                        const int32_t* row_group, const uint8_t* row_keep, float* out, int64_t* rows_changed, void* stream) {
    const char* who = "saev_intervene_rows";
    if (n_rows < 0 || D < 0 || S < 0 || row_cap < 0 || n_edits < 0 || n_groups < 0) return entry_refuse(SAEV_INVALID_ARG, who, "negative size");
    if (n_rows > 0x7fffffffLL || D > 0x7fffffffLL || S > 0x7fffffffLL || row_cap > 0x7fffffffLL)
        return entry_refuse(SAEV_UNSUPPORTED, who, "n_rows, D, S and row_cap must stay below 2^31");
    if (n_edits > IV_MAX_EDITS || n_groups > IV_MAX_GROUPS) return entry_refuse(SAEV_UNSUPPORTED, who, "at most 65536 edits and 65536 groups");
    if (D < 1 || S < 1) return entry_refuse(SAEV_INVALID_ARG, who, "D and S must be at least 1");
    if (n_rows == 0) return SAEV_OK;
    if (!x || !W_dec || !out) return entry_refuse(SAEV_INVALID_ARG, who, "x, W_dec or out is NULL");
    if (n_edits > 0 && !plan_dev) return entry_refuse(SAEV_INVALID_ARG, who, "edits without a plan");
    if (n_edits > 0 && row_cap > 0 && (!idx || !val)) return entry_refuse(SAEV_INVALID_ARG, who, "idx or val is NULL");
    const int64_t xb = 4 * n_rows * D;
    if (out != x && overlaps(out, xb, x, xb)) return entry_refuse(SAEV_INVALID_ARG, who, "out overlaps x without being x");
    if (overlaps(out, xb, W_dec, 4 * S * D) || overlaps(out, xb, idx, 4 * n_rows * row_cap) || overlaps(out, xb, val, 4 * n_rows * row_cap))
        return entry_refuse(SAEV_INVALID_ARG, who, "out overlaps W_dec or the codes");
    const IvPlanLayout lay = iv_plan_layout(n_edits, n_groups);
    const uint8_t* plan = static_cast<const uint8_t*>(plan_dev);
    IvArgs a;
    a.x = x; a.W = W_dec; a.idx = idx; a.val = val; a.row_nnz = row_nnz;
    a.ptr = plan ? reinterpret_cast<const int32_t*>(plan + lay.off_ptr) : nullptr;
    a.rec = plan ? reinterpret_cast<const int4*>(plan + lay.off_rec) : nullptr;
    a.row_group = row_group; a.row_keep = row_keep; a.out = out;
    a.rows_changed = reinterpret_cast<unsigned long long*>(rows_changed);
    a.n = (int)n_rows; a.D = (int)D; a.S = (int)S; a.cap = (int)row_cap; a.E = (int)n_edits; a.G = (int)n_groups;
    if (n_edits == 0 && out == x) return SAEV_OK;
    hipStream_t s = (hipStream_t)stream;
    const bool vec = D % 4 == 0 && (((uintptr_t)x | (uintptr_t)out | (uintptr_t)W_dec) & 15) == 0;
    const unsigned grid = (unsigned)std::min<int64_t>((n_rows + IV_WAVES - 1) / IV_WAVES, IV_MAX_GRID);
    if (vec) hipLaunchKernelGGL(iv_rows_kernel<true>, dim3(grid), dim3(IV_WAVES * 64), 0, s, a);
    else hipLaunchKernelGGL(iv_rows_kernel<false>, dim3(grid), dim3(IV_WAVES * 64), 0, s, a);
    if (hipGetLastError() != hipSuccess) return entry_refuse(SAEV_HIP_ERROR, who, "kernel launch failed");
    return SAEV_OK;
}

static int cf_check(const char* who, int64_t S, int64_t C, int32_t T) {
    if (S < 0 || C < 0 || T < 0) return entry_refuse(SAEV_INVALID_ARG, who, "negative size");
    if (S > 0x7fffffffLL) return entry_refuse(SAEV_UNSUPPORTED, who, "S must stay below 2^31");
    if (S < 1) return entry_refuse(SAEV_INVALID_ARG, who, "S must be at least 1");
    if (C < 1 || C > ENTRY_MAX_C) return entry_refuse(SAEV_UNSUPPORTED, who, "the number of classes must lie in [1, 4096]");
    if (T < 1 || T > 8) return entry_refuse(SAEV_UNSUPPORTED, who, "the number of thresholds must lie in [1, 8]");
    return SAEV_OK;
}

int saev_class_fire_counts(const int32_t* idx, const float* val, const int32_t* row_nnz, int64_t row_cap, int64_t n_rows,
                           const int32_t* label, const uint8_t* row_keep, int64_t S, int64_t C, const float* thr_host, int32_t T,
                           uint32_t* hist, uint32_t* pos, int64_t* n_rows_c, void* stream) {
    const char* who = "saev_class_fire_counts";
    if (row_cap < 0 || n_rows < 0) return entry_refuse(SAEV_INVALID_ARG, who, "negative size");
    if (const int rc = cf_check(who, S, C, T)) return rc;
    if (n_rows > 0x7fffffffLL || row_cap > 0x7fffffffLL || n_rows * row_cap > 0x7fffffffLL)
        return entry_refuse(SAEV_UNSUPPORTED, who, "n_rows, row_cap and n_rows * row_cap must stay below 2^31");
    if (!thr_host) return entry_refuse(SAEV_INVALID_ARG, who, "thr is NULL");
    CfThr thr;
    for (int t = 0; t < 8; ++t) thr.t[t] = 0.f;
    for (int t = 0; t < T; ++t) {
        if (!(thr_host[t] >= 0.f) || (t > 0 && !(thr_host[t] > thr_host[t - 1])))
            return entry_refuse(SAEV_INVALID_ARG, who, "thresholds must be >= 0 and strictly ascending");
        thr.t[t] = thr_host[t];
    }
    if (C * (int64_t)T * S >= 0x80000000LL) return entry_refuse(SAEV_UNSUPPORTED, who, "C * T * S must stay below 2^31");
    if (!hist || !pos || !n_rows_c) return entry_refuse(SAEV_INVALID_ARG, who, "hist, pos or n_rows_c is NULL");
    if (n_rows == 0) return SAEV_OK;
    if (!label) return entry_refuse(SAEV_INVALID_ARG, who, "label is NULL");
    if (row_cap > 0 && (!idx || !val)) return entry_refuse(SAEV_INVALID_ARG, who, "idx or val is NULL");
    hipStream_t s = (hipStream_t)stream;
    const int64_t total = n_rows * row_cap;
    if (total > 0)
        hipLaunchKernelGGL(cf_codes_kernel, dim3((unsigned)std::min<int64_t>((total + 255) / 256, CF_CODES_MAX_GRID)), dim3(256), 0, s, idx, val, row_nnz,
                           (int)row_cap, (long)total, label, row_keep, (int)S, (int)C, thr, (int)T, hist, pos);
    hipLaunchKernelGGL(cf_rows_kernel, dim3((unsigned)std::min<int64_t>((n_rows + 255) / 256, CF_ROWS_MAX_GRID)), dim3(256), (size_t)C * 4, s, label,
                       row_keep, (int)n_rows, (int)C, reinterpret_cast<unsigned long long*>(n_rows_c));
    if (hipGetLastError() != hipSuccess) return entry_refuse(SAEV_HIP_ERROR, who, "kernel launch failed");
    return SAEV_OK;
}

int saev_class_fire_f1(const uint32_t* hist, const uint32_t* pos, const int64_t* n_rows_c, int64_t S, int64_t C, int32_t T,
                       const uint8_t* latent_mask, float* f1, uint8_t* best_t, void* stream) {
    const char* who = "saev_class_fire_f1";
    if (const int rc = cf_check(who, S, C, T)) return rc;
    if (C * (int64_t)T * S >= 0x80000000LL) return entry_refuse(SAEV_UNSUPPORTED, who, "C * T * S must stay below 2^31");
    if (!hist || !pos || !n_rows_c || !f1 || !best_t) return entry_refuse(SAEV_INVALID_ARG, who, "hist, pos, n_rows_c, f1 or best_t is NULL");
    const int64_t total = C * S;
    hipLaunchKernelGGL(cf_f1_kernel, dim3((unsigned)std::min<int64_t>((total + 255) / 256, CF_F1_MAX_GRID)), dim3(256), 0, (hipStream_t)stream, hist, pos,
                       reinterpret_cast<const long long*>(n_rows_c), (int)S, (int)C, (int)T, latent_mask, f1, best_t);
    if (hipGetLastError() != hipSuccess) return entry_refuse(SAEV_HIP_ERROR, who, "kernel launch failed");
    return SAEV_OK;
}
