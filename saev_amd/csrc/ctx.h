// Private to the ctx*.hip units of libsaev_amd.so: the context behind the C ABI (include/saev_amd.h), what invalidates its caches,
// and the small helpers more than one of the units needs.  Host code only.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "kernels.h"

constexpr int AUX_KSPLIT_MAX = 16;
constexpr int CAND_CAP = 4096;
// Entries between the candidate lists of consecutive rows.  Not the capacity: with a 16 KB (power-of-two) row pitch the
// 32 rows a wave appends to at once fall on few memory channels, and how badly depends on which physical pages the
// allocation got -- the fused encoder then ran at 1.40 or 1.54 ms from one engine instance to the next
// (tools/experiments/bimodal_probe.py).  Measured pitches: +128 B 1.50 ms, +256 B / +512 B / +1 KB 1.41-1.42 ms, all
// stable; 1 KB it is.
constexpr int CAND_STRIDE = CAND_CAP + 256;
constexpr int TIMING_RING = 512;
// saev_step_dead decides between "nothing / a handful of dead latents" (kernels that take the count from the device) and
// "read the count back and run the dense algebra" from the record the device wrote DEAD_LAG steps earlier.
constexpr int DEAD_LAG = 4;
constexpr int DEAD_RING = 16;
enum { AUX_NONE = 0, AUX_SMALL_DEVICE = 1, AUX_SMALL_HOST = 2, AUX_DENSE = 3 };

struct saev_ctx {
    saev_cfg cfg{};
    saev_debug_cfg dbg{};  // route switches (saev_create_ex); all zero = shipped defaults
    int device = 0;
    std::string err;
    // bound buffers
    float* params = nullptr;
    float* grads = nullptr;
    float* adam_m = nullptr;
    float* adam_v = nullptr;
    // derived
    long n_params = 0;  // floats in each flat buffer, padding included
    long off_W_dec = 0, off_b_dec = 0, off_W_enc = 0, off_b_enc = 0;
    int shard_world = 1;
    long chunk_a = 0, chunk_b = 0;  // floats per rank of the [W_dec | b_dec] half and of the [W_enc | b_enc] half
    double* sumsq_bound = nullptr;  // caller-owned replacement of sumsq_total (so that a collective can reach it)
    hipEvent_t wdec_ready = nullptr;  // one-shot: the next forward waits for it before it touches W_dec
    hipEvent_t wenc_ready = nullptr;  // one-shot: ... before it touches W_enc / b_enc (the x-only preparation runs ahead of it)
    // scratch
    std::vector<void*> allocs;
    size_t scratch_bytes = 0, aux_bytes = 0;  // device memory the context owns: per-step scratch, AuxK dead-set buffers
    uint8_t* muon_ws = nullptr;  // Muon workspace (muon.hip: MuonLayout), allocated by the first saev_muon_tail
    size_t muon_bytes = 0;
    int cuts_last[MAX_PREFIXES] = {0};  // the cut points the forward in flight used (the backward must see the same)
    int32_t *cand_cnt = nullptr, *gmax = nullptr, *cand_idx = nullptr;
    int gmax_stride = 0;
    float* cand_val = nullptr;
    float* h_dense = nullptr;
    int32_t *idx = nullptr, *aux_idx = nullptr;
    float *val = nullptr, *aux_val = nullptr;
    float *x_hat = nullptr, *g = nullptr, *g_aux = nullptr;
    RowStats* rowstats = nullptr;
    uint32_t* bitmap = nullptr;
    int32_t* grp_prefix = nullptr;
    int32_t* scan_totals = nullptr;
    int32_t csc_epoch = 0;  // CscArgs::epoch of the last build
    int bitmap_words = 0;
    int back_rows = 0;  // max(max_batch, max_backward_rows): rows a (gathered) backward may cover
    int bitmap_words_last = 0;
    bool bitmap_clean = false;  // every word the next csc build will use is zero (the last full backward cleared behind itself)
    int bitmap_clean_words = 0; // ... for row pitches up to this many words
    int bitmap_prefill_words = 0, bitmap_prefill_rows = 0;  // the training decode in flight has set the bits of its codes at this pitch (0: no)
    bool last_backward_gathered = false;  // the previous backward ran over gathered rows (saev_backward_override): its forward's bits were wasted
    int32_t *counts = nullptr, *starts = nullptr;
    int2* pairs = nullptr;
    float* colsum_partials = nullptr;
    float* dval_pairs = nullptr;  // <g row, W_dec[latent]> per (row, latent) pair in CSC order (saev_backward_rows_part 1 -> 2)
    double *sumsq_partials = nullptr, *sumsq_total = nullptr;
    // squares of the W_enc gradient, taken by the transpose that ends the backward (saev_backward_end): valid until the
    // next backward; the tail uses them only when the caller vouches that nothing wrote the gradient since (trust_grads)
    bool wenc_sq_valid = false;
    // {projection coefficient, projected squares} of every decoder-gradient row, left by the kernels that wrote the rows
    // (DwRowsArgs::row_proj); valid after a one-pass backward over all latents, trusted like wenc_sq
    float2* row_proj = nullptr;
    float* enc_sq = nullptr;  // squares of the rows of the transposed W_enc gradient, from the same kernels
    bool row_proj_valid = false, tail_proj_in_adam = false;
    bool wenc_t_pending = false;  // saev_train_step: the W_enc gradient is still in dW_encT, the tail's Adam reads it there
    int64_t* toks = nullptr;
    int32_t *fired = nullptr, *dead = nullptr;
    int32_t* flags = nullptr;  // [0] need_dense_pre [1] need_dense [2] n_overflow [3] cand_max [4] n_dead [5] k_use [6,7,8] dead_update scratch
    int32_t *chunk_starts = nullptr, *part_starts = nullptr, *work_latent = nullptr;
    float *dW_encT = nullptr, *partials = nullptr, *db_partials = nullptr;
    // column-sliced weight gradients (launch_dw_slices; SAEV_AMD_DW=rows keeps dw_rows): slice-major copies of g and x left by
    // the decode, pair words / latents in pair order from the CSC build, the per-slice shares of dval
    bool dws_ok = false;         // geometry fits (d_model % 32 == 0, 32-bit offsets) and not switched off
    int dws_rows = 0;            // > 0: the copies describe the training forward in flight (that many rows)
    bool dws_pairs = false;      // the CSC build of this backward left pv / plat
    float *gS = nullptr, *xS = nullptr, *dvp = nullptr;
    // A gathered backward (saev_backward_override) of a context that LENDS its x-derived buffers (saev_share_x) must not write
    // the rows of all ranks over xS: its followers' forwards run after this backward and read xS as their own batch.  Such a
    // context gets a second slice-major buffer for the gathered rows, allocated at the first backward that needs it.
    float* xS_ov = nullptr;
    float* xS_bwd = nullptr;  // the slice-major x the backward in flight reads when it runs over gathered rows (xS or xS_ov)
    // dval[b][j] = <g_b, W_dec[idx[b][j]]> left by the decode itself (decode_q_kernel; kernels.h: DecodeArgs::dval_out): pass A of
    // the slices then forms dW_dec only.  dval_fwd: the forward in flight has left it (same condition as dws_rows, plus the shape)
    float* dval_rows = nullptr;
    bool dval_fwd = false;
    // the light finalize (kernels.h: DwSlicesArgs::wn2): ||w_i||^2 of the decoder rows as this step's normalize_rows wrote them
    float* wn2 = nullptr;
    float* sq_wave = nullptr;  // per-wave squares of the two passes (DwSlicesArgs::sq_wave_dec, then _enc: contiguous)
    int sq_wave_n = 0;         // > 0: the backward in flight left 2 x this many of them (the tail adds them to the clip norm)
    bool wn2_fresh = false;  // wn2 describes W_dec as it is now (set by the training forward, cleared by whatever writes W_dec)
    bool dval_pairs_ready = false;  // the CSC build of this backward has written pv2 from it
    bool fused_forward = false;     // saev_train_step's forward: Matryoshka G blocks past the first are not needed row-major
    // saev_train_step's plain forward on the slice route leaves dL/dx_hat slice-major alone (gS): its backward reads nothing else
    bool g_rows_valid = true;       // the row-major g describes the training forward in flight
    // exact refinement of the f16r encoder from 32-column slices (select.hip: refine_slices_kernel): split_f16r leaves x and
    // W_enc^T slice-major (xS; dW_encT in that layout), rs_part holds the per-slice shares of the survivors' dot products
    bool fwd_slices = false;     // geometry fits and not switched off (saev_debug_cfg.fwd_route)
    bool fwd_step = false;       // the forward in flight took that route: xS_c describes its batch, W_enc^T is slice-major
    float* rs_part = nullptr;
    float* xS_c = nullptr;       // the slice-major x of the step in flight (own xS, or the leader's: saev_share_x)
    int2 *pv = nullptr, *pv2 = nullptr;
    int32_t *plat = nullptr, *cut_lat = nullptr, *cut_list = nullptr;
    // saev_train_step: latents without pairs are flagged instead of having their dW_enc^T row zeroed (DwSlicesArgs::lat_unused)
    int32_t* lat_unused = nullptr;
    bool fused_step = false;     // inside saev_train_step: the transposed W_enc gradient is read by the fused Adam alone
    bool unused_valid = false;   // the backward in flight left lat_unused
    // Matryoshka prefixes of the step (P == 1: plain objective)
    int P = 1;
    int32_t cuts[MAX_PREFIXES] = {0};
    float* G = nullptr;  // (max_batch, P_cap, D)
    float* GS = nullptr; // slice-major copy of G for launch_dw_slices: [D / 32][P][rows][32] (with dws_ok)
    int P_cap = 0;
    // AuxK dense-over-dead-set path (auxk.hip)
    int n_dead_host = 0, k_use_host = 0;
    int64_t tokens_seen = 0;
    bool tracker_dirty = false;
    int nd_cap = 0;
    // per-step records of the dead set in pinned host memory (written by dead_update_kernel), one event per record
    DeadRecord* rec_host = nullptr;
    DeadRecord* rec_dev = nullptr;
    hipEvent_t dead_ev[DEAD_RING];
    bool dead_ev_created = false;
    int64_t dead_steps = 0;      // saev_step_dead calls so far (the current step's 1-based id during the call)
    int64_t rec_valid_from = 1;  // records of earlier steps predate a host write to the tracker
    int aux_route = AUX_NONE;    // what the step in flight does for the auxiliary loss
    int64_t n_readbacks = 0;     // blocking reads of n_dead so far (diagnostics: saev_dead_readbacks)
    std::vector<void*> aux_allocs;
    int32_t* dead_list = nullptr;
    float *Wenc_dead = nullptr, *Wdec_dead = nullptr, *H_dead = nullptr, *A_dead = nullptr, *dWd = nullptr, *dWe = nullptr,
          *dbe = nullptr, *aux_partials = nullptr, *WencT_dead = nullptr, *aux_small_part = nullptr, *aux_small_part2 = nullptr, *aux_small_partbe = nullptr;
    bool aux_dev_count = false;  // dense branch sized by a host-side BOUND of the dead count; the count itself stays on the device
    bool aux_small = false;  // this step's AuxK ran on the few-dead-latents path
    int aux_mfma_bound = 0;
    int aux_ndp = AUX_SMALL_MAX;  // row pitch of A / dA / the block partials of the few-dead-latents step in flight (AUX_MFMA_MAX beyond 64)
    int aux_mfma_cap = AUX_SMALL_MAX;  // largest bound the matrix-core kernels take in this context (its buffers decide)
    bool aux_mfma = false;   // ... in its fp32 matrix-core form (at most AUX_MFMA_MAX dead latents, d_model % 128 == 0: auxk.hip aux_mfma_*)
    bool aux_fused = false;  // ... in its one-pass form (at most AUX_FUSED_MAX dead latents: block partials instead of g_aux / A / dA)
    bool aux_all = false;    // dense branch with every dead latent selected (n_dead <= k_aux): no select, no mask
    uint8_t* A_mask = nullptr;
    // AuxK contractions on the f16x3 encoder kernel (F16X3 mode): operand images and compact vectors
    _Float16 *aux_ws1 = nullptr, *aux_ws2 = nullptr, *aux_xsA = nullptr, *aux_xsg = nullptr, *aux_kA = nullptr, *aux_kD = nullptr, *aux_kX = nullptr;
    bool aux_both = false;  // the dense route's forward has left the k-major images of A (aux_kA) and x (aux_kX) beside the row-form ones
    float* aux_parts = nullptr;
    int aux_kpad = 0;
    float *bias_dead = nullptr, *zero_bias = nullptr, *aux_scales = nullptr;  // aux_scales: {absmax, -, sA, 1, sg, 1}
    float* aux_sync = nullptr;     // per-workgroup maxima of the AuxK kernels that leave an operand scale behind (auxk.hip: pow2_parts_kernel)
    int aux_Dp2 = 0;
    // F16R: per-row candidate margins and the max encoder column norm (W_enc^T in fp32 lives in dW_encT during forward)
    float *row_margin = nullptr, *wnorm_scratch = nullptr, *surv_val = nullptr;
    int32_t *surv_idx = nullptr, *surv_cnt = nullptr, *surv_rng = nullptr;
    int rs_lat_range = 0, rs_n_ranges = 0;
    int32_t* tau_max = nullptr;   // (max_batch) largest predicted bound used per row
    float* heur_state = nullptr;  // [0] z  [1] failed predictions  [2] predicted-bound launches  [3] mean list length
    // norm-predicted bounds (bound_mode 2; kernels.h: RhoArgs): controller state, partials of the ratio reduction, the rows' bounds
    // and the exact k-th largest values of the last final select
    float *rho_state = nullptr, *rho_scratch = nullptr, *row_bound = nullptr, *kth_val = nullptr;
    bool rho_valid = false;       // the previous forward was a streamed training step of this mode that left rho_lo for this one
    int rho_n = 0;                // ... over this many rows
    int rho_step = 0;             // this forward: 0 not involved, 1 collects the ratios only, 2 predicts as well
    int32_t rho_serial_seen = 0;  // the controller's last pause the host has taken note of (pinned words stale_host[4], [5]) ...
    int rho_pause_left = 0;       // ... and how many of its steps are still to come
    float *f16r_scales = nullptr, *mu = nullptr, *xnorm = nullptr, *b_shift = nullptr, *dot_part = nullptr, *xabs_part = nullptr,
          *sq_part = nullptr, *wmax_prev = nullptr;
    bool wmax_known = false;
    bool mu_ready = false;  // the step already put the column means of x into mu
    // ---- the streamed f16r step: what a forward derives from x comes from ONE pass (xprep_kernel) centred, scaled
    // and normalised with what the previous batch left; what it derives from W_enc was left by the fused Adam of the previous step
    // (AdamImageArgs) -- or by this context's last full preparation, while W_enc has not moved since.
    bool stream_ok = false;       // mode and geometry allow it (f16r, slice route of the refinement, guaranteed bounds)
    float *WeS = nullptr;         // slice-major fp32 W_enc^T of its own (the gradient scratch dW_encT no longer doubles as it)
    float *xn_part = nullptr, *amax_part = nullptr, *cmax_part = nullptr;
    float* b_seen = nullptr;      // b_enc as bias_finish read it (the staleness samples of xprep_kernel compare against it)
    int32_t *stale_host = nullptr, *stale_dev = nullptr;  // pinned words: [0] a streamed step found the parameters changed behind its
                                                          // back before using its images (and took the exact route); [1] the fused
                                                          // Adam found W_enc tiles changed AFTER the step had used them (AdamImageArgs::chk)
    uint32_t* wchk = nullptr;     // two checksum words per 32 x 256 tile of W_enc, left by the fused Adam that wrote it
    // Several SAEs on the same batches (saev_share_x) with the streamed preparation: the lender streams as a context on its own does and
    // keeps what its followers need of the step's x side (XprepArgs::mu_keep / xside_keep); a follower's fused Adam leaves ITS W images
    // centred on the lender's next mu, so that from the third step of a group nobody prepares anything from scratch.
    float *mu_keep = nullptr, *xside_keep = nullptr;
    bool fwd_streamed = false;     // (lender) the forward that built the current x-derived buffers took the streamed preparation ...
    bool fwd_moves_mu = false;     // ... inside saev_train_step: its second launch has moved mu on to this batch's mean
    int64_t fwd_mu_serial = -1;    // ... with the centre of this serial
    bool borrow_streamed = false;  // (follower) the forward in flight borrowed the x side of a streamed step of its lender
    bool follow_stream = false;    // ... and runs on W images its own Adam left: no preparation at all
    bool wchk_valid = false;      // wchk describes W_enc as the library last wrote it, and only the library may have written it since
    bool fwd_reused_wimg = false; // the forward in flight ran on operand images a previous step's Adam left (their checksums are due)
    uint32_t stale_salt = 0;
    int scale_par = 0;            // which half of f16r_scales (2 x 8 floats) belongs to the step in flight
    bool prep_valid = false;      // mu and scales[par][0, 4] describe a previous batch of this context
    bool wimg_fresh = false;      // ws / WeS / dot_part / sq_part / b_shift / wnorm_scratch describe W_enc AS IT IS NOW ...
    int64_t mu_serial = 0, wimg_mu_serial = -1;  // ... centred on the mu of this version (mu_serial: bumped whenever mu is rewritten)
    bool wimg_bf16_fresh = false; // bf16 encoder: ws describes W_enc as it is now
    bool stream_step = false;     // the forward in flight took the streamed preparation
    bool stats_pending = false, stats_lists = false;  // the forward of a fused train step left its statistics to saev_step_dead's launch
    bool aux_stats_pending = false;  // ... and its one-pass AuxK forward left the auxiliary loss to the backward's ordered-sum launch
    bool dead_list_ready = false; // ... which also left the list of dead latents (if any are dead)
    bool train_fused = false;     // inside saev_train_step: the forward moves mu, the tail's Adam leaves the next images
    const float* gather_pool = nullptr;   // saev_train_step_gather: the batch is rows[0..n) of this pool, x is where it is written
    const int64_t* gather_rows = nullptr;
    // Where the step in flight finds what was derived from x alone: max|x|, the column means, the centred row norms, the
    // per-workgroup maxima behind the x scale, and the fp16 / bf16 images.  Its own buffers -- or those of the context it
    // shares a batch with (saev_share_x: several SAEs trained on the same batches form them once).
    float *upper_c = nullptr, *mu_c = nullptr, *xnorm_c = nullptr, *xabs_c = nullptr;
    _Float16* xs_c = nullptr;
    saev_ctx* leader = nullptr;
    void* comm = nullptr;        // ncclComm_t (saev_comm_init)
    int comm_rank = 0, comm_world = 0;
    std::vector<saev_ctx*> followers;  // contexts whose `leader` is this one (saev_destroy / a new link clears them)
    const float* xprep_x = nullptr;  // what this context's own x-derived buffers currently describe
    int xprep_n = 0;
    int64_t xprep_serial = 0;        // bumped every time they are rebuilt
    int64_t leader_serial_seen = 0;  // the leader's serial this context last borrowed
    // f16x3 encoder operands
    _Float16 *xs = nullptr, *ws = nullptr;
    int Dp = 0, S_pad = 0, MB_pad = 0;
    int max_work = 0, max_part = 0;
    float* upper = nullptr;
    saev_step_stats* stats = nullptr;
    double* stats_scratch = nullptr;  // per-workgroup partial sums + ticket of stats_reduce_kernel
    int* tickets = nullptr;           // arrival counters of "last workgroup finishes" kernels (zero between launches)
    // gathered backward (saev_backward_override): the (row, latent) pairs of ALL ranks' rows, set for one backward
    const float *ov_x = nullptr, *ov_g = nullptr, *ov_val = nullptr;
    const int32_t* ov_idx = nullptr;
    int ov_n = 0;
    float* db_aux = nullptr;       // the auxiliary term's share of db_dec, kept apart while an override is active
    bool trust_grads = false;      // the caller vouches that nothing touches the gradient between backward and tail
    // BatchTopK (include/saev_amd.h: BATCHTOPK; kernels in batchtopk.hip).  cfg.top_k of such a context is its ROW CAPACITY -- what
    // every buffer and loop a TopK context sizes by top_k goes by -- and btk_k the configured codes per row on average.
    bool btk = false;
    int btk_k = 0, btk_list_cap = 0;
    double btk_momentum = 0.1;
    float *threshold = nullptr, *threshold_own = nullptr;  // the word in use (own, or caller-bound: saev_bind_threshold)
    uint32_t* btk_ws = nullptr;       // select state, histograms, key list, per-row tie counters (btk_workspace_words)
    int32_t *row_nnz = nullptr, *btk_over = nullptr;  // of the last forward; the overflow word
    int btk_need = 0;                 // after SAEV_ROW_OVERFLOW: the largest row count met
    // ReLU training (include/saev_amd.h: RELU TRAINING; ctx_relu_train.hip, kernels in relu_train.hip): a context kind of its own
    // (saev_create_relu_train) with cfg.activation = SAEV_ACT_RELU.  f lives in h_dense, dH in rt_dA after the backward.
    bool relu_train = false;
    bool rt_fwd_live = false;         // a training forward's f images are in place: cleared by the backward, which overwrites them with dH's
    double rt_l1 = 0.0;               // the L1 coefficient (objectives.py: sparsity = coeff * l1)
    float* rt_dA = nullptr;           // (max_batch x d_sae) g W_dec^T, then dH in place
    float *rt_parts = nullptr, *rt_colpart = nullptr;  // per-workgroup maxima; column sums of dH per block of rows
    float* rt_scales = nullptr;       // operand scales {2^e, 1}: [0] f, [2] g, [4] dH, [6] x; saev_encode_dense (f16x3): [8] max |x|, [10] its pair
    int rt_Sp = 0, rt_kpad = 0;       // d_sae rounded up to 32; the batch axis padded for the split-K weight gradients
    _Float16 *rt_xsF = nullptr, *rt_xsG = nullptr;    // row-operand images of f (k = d_sae) and of g (k = d_model)
    _Float16 *rt_wsR = nullptr, *rt_wsK = nullptr;    // W_dec as "encoder" of dA (rows = latents) and of x_hat (rows = d_model columns)
    _Float16 *rt_kF = nullptr, *rt_kG = nullptr, *rt_kX = nullptr;  // k-major images (k = batch) of f / dH, of g and of x
    float* rt_wparts = nullptr;       // split-K partial products of a weight gradient
    // state of the step in flight
    const float* x_last = nullptr;
    int n_last = 0;
    int training_last = 0;
    int P_last = 1;
    // timing
    bool timing = false;
    hipEvent_t ev_start[TIMING_RING], ev_stop[TIMING_RING];
    bool ev_created = false;
    long ev_count = 0;
};

// ---- what makes the caches above stale: one name per event, so that a new writer cannot pick the wrong subset of flags ----
// The parameters moved (or may have: a new binding, a write the caller announces, an optimizer tail): nothing the context
// derived from W_enc / W_dec describes them any longer.  The fused Adam that leaves fresh images says so after this.
inline void params_moved(saev_ctx* c) {
    c->wn2_fresh = false;
    c->wimg_fresh = false;
    c->wimg_bf16_fresh = false;
    c->wchk_valid = false;
}
// The owner of the images' centre changed.  W images a context keeps are centred on a mu identified by a SERIAL of whoever owned
// that mu: its lender's while it follows, its own otherwise.  Serials of different contexts are unrelated numbers, so the images
// are dropped whenever the owner changes -- an equal number must never pass for an equal centre.
inline void centre_owner_changed(saev_ctx* c) {
    c->wimg_fresh = false;
    c->wchk_valid = false;
}

#define HIPCHK(ctx, expr)                                                                    \
    do {                                                                                     \
        hipError_t _e = (expr);                                                              \
        if (_e != hipSuccess) {                                                              \
            (ctx)->err = std::string(#expr) + ": " + hipGetErrorString(_e);                  \
            return SAEV_HIP_ERROR;                                                           \
        }                                                                                    \
    } while (0)

#define REQUIRE(ctx, cond, code, msg)                                                        \
    do {                                                                                     \
        if (!(cond)) {                                                                       \
            (ctx)->err = (msg);                                                              \
            return (code);                                                                   \
        }                                                                                    \
    } while (0)

template <typename T>
inline int alloc(saev_ctx* c, T** p, size_t count) {
    void* q = nullptr;
    if (count == 0) count = 1;
    hipError_t e = hipMalloc(&q, count * sizeof(T));
    if (e != hipSuccess) {
        c->err = std::string("hipMalloc failed: ") + hipGetErrorString(e);
        return SAEV_HIP_ERROR;
    }
    c->allocs.push_back(q);
    c->scratch_bytes += count * sizeof(T);
    *p = static_cast<T*>(q);
    return SAEV_OK;
}

// {x scale, W scale, x scale, 1, square normaliser, -, -, -} of the step in flight / of the next one (streamed f16r step)
inline float* scl(const saev_ctx* c) { return c->f16r_scales + 8 * c->scale_par; }
inline float* scl_next(const saev_ctx* c) { return c->f16r_scales + 8 * (c->scale_par ^ 1); }

// TopK bound of the fp16-image encoders: the minimum over 32 group maxima for top_k <= 32; 64 groups with the top_k-th
// largest of the group maxima for 32 < top_k <= 64.  The second variant for small k as well cut the candidates per row from
// ~980 to ~360 at config 2, but its bound phase (32 published maxima per lane, a bisection over packed 16-bit keys) cost more
// than the shorter lists saved (encoder 1.43-1.51 vs 1.35-1.38 ms).
inline int f16_ngroups(const saev_ctx* c) { return c->cfg.top_k > 32 ? 64 : 32; }

inline int encoder_splits(int n_rows, int S, int tile_rows, int tile_latents, int target_wgs) {
    const int nb = (n_rows + tile_rows - 1) / tile_rows;
    const int nst = (S + tile_latents - 1) / tile_latents;
    int sp = std::max(1, std::min((target_wgs + nb - 1) / nb, nst));
    // the fewest splits that keep the longest walk as short: 24 tiles over 16 splits are walks of 1 and 2 tiles -- as long as 12
    // splits of 2 each, with a third more workgroups paying a first tile's bound refresh and sharing the board's power
    // (configs[0]: encoder 92 -> 84 us, step 0.435 -> 0.415 ms; profiles/r06_c0_encoder_grid.txt)
    const int longest = (nst + sp - 1) / sp;
    return (nst + longest - 1) / longest;
}

inline bool fused_supported(const saev_cfg& c) { return c.top_k <= 64; }

// slices and padded length of the batch-long contraction of an R x C weight gradient on the split-fp16 kernel (a single slice would
// leave most CUs idle when R x C is only a few tiles): the k-major images of its operands are laid out for them
inline void ksplit_shape(int R, int C, int K, int* n_split_out, int* Kp_out) {
    const int R256 = (R + 255) / 256 * 256, C256 = (C + 255) / 256 * 256;
    const int tiles = (R256 / 256) * (C256 / 256);
    int n_split = 1;
    while (n_split < AUX_KSPLIT_MAX && tiles * n_split < 256) n_split *= 2;
    *n_split_out = n_split;
    *Kp_out = (K + 16 * n_split - 1) / (16 * n_split) * (16 * n_split);
}

// internal functions that cross a unit boundary
int create_context(const saev_cfg* cfg, const saev_debug_cfg* dbg, const saev_batch_topk_cfg* bt, const saev_relu_train_cfg* rt, int device,
                   saev_ctx** out);             // ctx.hip: what every saev_create_* ends in
int encode_dense_h(saev_ctx* c, const float* x, int n, hipStream_t s);  // ctx_forward.hip: h = x W_enc + b_enc into h_dense, exact fp32 (BatchTopK and ReLU steps)
int relu_train_alloc(saev_ctx* c);              // ctx_relu_train.hip: the dense step's scratch (create_context)
int relu_train_forward(saev_ctx* c, const float* x, int n, int64_t n_rows_global, int training, hipStream_t s);  // (saev_step_forward)
int relu_train_backward(saev_ctx* c, hipStream_t s);                                                              // (saev_step_backward)
int alloc_aux_buffers(saev_ctx* c, int cap);    // ctx_auxk.hip: the dead-set buffers (saev_create_*, and saev_step_dead grows them)
int auxk_backward(saev_ctx* c, hipStream_t s);  // ctx_auxk.hip: gradients of the auxiliary loss (saev_backward_begin)
int muon_cfg_check(const saev_muon_cfg& m, std::string* why);  // ctx.hip (saev_muon_newton_schulz, saev_muon_tail)

inline void timing_begin(saev_ctx* c, hipStream_t s) {
    if (c->timing) hipEventRecord(c->ev_start[c->ev_count % TIMING_RING], s);
}
inline void timing_end(saev_ctx* c, hipStream_t s) {
    if (c->timing) {
        hipEventRecord(c->ev_stop[c->ev_count % TIMING_RING], s);
        c->ev_count++;
    }
}
