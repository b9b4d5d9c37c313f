// The forward launch sequences behind the C ABI: operand preparation, encoder, select, the single-op entries and saev_step_forward.
#include "ctx.h"

extern "C" {

// ------------------------------------------------------------------------------------------
// single ops
// ------------------------------------------------------------------------------------------

int saev_normalize_w_dec(saev_ctx* c, void* stream) {
    if (!c) return SAEV_INVALID_ARG;
    REQUIRE(c, c->params, SAEV_NOT_BOUND, "parameters not bound");
    if (!c->cfg.normalize_w_dec) return SAEV_OK;
    HIPCHK(c, launch_normalize_rows(c->params + c->off_W_dec, c->cfg.d_sae, c->cfg.d_model, (hipStream_t)stream));
    return SAEV_OK;
}

// Points the *_c members at this context's own x-derived buffers, or at the leader's when they describe exactly this
// batch (same pointer, same row count, built since this context last borrowed them).  Returns true when borrowed.
static bool bind_x_sources(saev_ctx* c, const float* x, int n, bool allow_borrow) {
    saev_ctx* l = c->leader;
    const bool borrow = allow_borrow && l != nullptr && l->xprep_x == x && l->xprep_n == n && l->xprep_serial != c->leader_serial_seen;
    saev_ctx* src = borrow ? l : c;
    c->upper_c = src->upper; c->mu_c = src->mu; c->xnorm_c = src->xnorm; c->xabs_c = src->xabs_part; c->xs_c = src->xs;
    // (a streamed step of the lender has moved its mu on already: the centre of the images it lends is the copy it kept)
    c->borrow_streamed = borrow && l->fwd_streamed && l->mu_keep != nullptr;
    if (c->borrow_streamed) c->mu_c = l->mu_keep;
    // (the slice route of the refinement needs the source's slice-major x as well: a leader without it sends this step down
    // the row route)
    c->fwd_step = c->fwd_slices && (src == c || src->fwd_slices);
    c->xS_c = c->fwd_step ? src->xS : nullptr;
    if (borrow) c->leader_serial_seen = l->xprep_serial;
    return borrow;
}

// saev_wenc_ready_event: the encoder half of the parameters may still be arriving on another stream; everything that
// depends on x alone has been enqueued by the time this is called
static int wait_wenc(saev_ctx* c, hipStream_t s) {
    if (c->wenc_ready != nullptr) {
        hipEvent_t ev = c->wenc_ready;
        c->wenc_ready = nullptr;
        HIPCHK(c, hipStreamWaitEvent(s, ev, 0));
    }
    return SAEV_OK;
}

// operand preparation for the f16 encoders: x and W_enc^T rewritten as fp16 / bf16 images (no-op for the f32 encoder).
// `xmax_dev` = device scalar max|x| when the caller has it already (the step computes it for the MSE), else NULL.
static int prepare_encoder(saev_ctx* c, const float* x, int n, int32_t* pre_flag, hipStream_t s,
                           const float* xmax_dev = nullptr, bool x_borrowed = false, bool defer_margins = false) {
    if (c->cfg.encoder_mode == SAEV_ENCODER_F32) return SAEV_OK;
    const int D = c->cfg.d_model, S = c->cfg.d_sae;
    const bool bf = c->cfg.encoder_mode == SAEV_ENCODER_BF16;
    if (c->cfg.encoder_mode == SAEV_ENCODER_F16R) {
        // One pass over W_enc (split_wT) yields the fp16 images, W_enc^T in fp32 for the exact refinement (in the
        // gradient scratch dW_encT, free until the backward), mu W_enc and the column norms.  Its power-of-two scale
        // comes from the previous step's largest column norm; f16r_check sends the step down the dense route if the
        // current parameters do not fit that scale.  Only the first use needs a pass of its own for the norm.
        if (!c->wmax_known) {
            { int rcw = wait_wenc(c, s); if (rcw != SAEV_OK) return rcw; }
            HIPCHK(c, launch_transpose(c->params + c->off_W_enc, c->dW_encT, D, S, s));
            HIPCHK(c, launch_wnorm_max(c->dW_encT, S, D, c->wnorm_scratch, c->wmax_prev, s));
            c->wmax_known = true;
        }
        // centre the first pass on the batch's column mean: h = (x - mu) W + (mu W + b)
        // (mu = column sums / n, scaled in the same kernel so that every consumer sees the same fp32 values)
        if (!x_borrowed) {
            if (!c->mu_ready) { HIPCHK(c, launch_colsum(x, n, D, c->colsum_partials, c->mu, 0, nullptr, s, 0, 1.0f / (float)n)); c->mu_serial++; }
            HIPCHK(c, launch_center_stats(x, c->mu, n, D, c->xnorm, c->xabs_part, s, xmax_dev));
        }
        c->mu_ready = false;
        // (the x scale depends on x alone: a borrowing context recomputes the same value from the leader's maxima, next
        // to its own W scale.  Folding this reduction into center_stats_kernel's last workgroup was tried: a release fence
        // per workgroup of four rows took that kernel from 12 to 115 us)
        if (c->borrow_streamed)  // (the lender's images carry the scale of ITS previous batch, not this batch's maxima)
            HIPCHK(c, launch_follower_scales(c->leader->xside_keep, c->wmax_prev, scl(c), pre_flag != nullptr ? pre_flag : c->flags, 0, s));
        else
        HIPCHK(c, launch_f16r_scales(c->xabs_c, (n + 3) / 4, c->wmax_prev, scl(c), s));
        // (the slice-major W_enc^T: in the gradient scratch, free until the backward -- or, where the streamed step may follow, in a
        // buffer of its own, so that it survives the backward)
        float* const wt_out = (c->fwd_step && c->stream_ok) ? c->WeS : c->dW_encT;
        if (!x_borrowed && c->wenc_ready == nullptr) {
            // the usual case: nobody's parameter all-gather to wait for in between -- both image passes in one launch
            HIPCHK(c, launch_split_f16r(x, n, D, c->Dp, c->xs, scl(c), c->mu, c->params + c->off_W_enc, S, c->S_pad, c->ws,
                                        reinterpret_cast<double*>(c->dot_part), c->sq_part, wt_out, s, c->fwd_step ? c->xS : nullptr,
                                        c->fwd_step ? 1 : 0));
        } else {
            if (!x_borrowed) HIPCHK(c, launch_split_rows(x, n, D, c->Dp, c->xs, 2, s, 1.0f, scl(c), c->mu, c->fwd_step ? c->xS : nullptr));
            { int rcw = wait_wenc(c, s); if (rcw != SAEV_OK) return rcw; }  // x is prepared; from here on W_enc / b_enc are read
            HIPCHK(c, launch_split_wT(c->params + c->off_W_enc, D, S, c->S_pad, c->Dp, 1.0f, c->ws, 2, s, scl(c) + 1,
                                      c->mu_c, reinterpret_cast<double*>(c->dot_part), c->sq_part, wt_out, c->fwd_step ? 1 : 0));
        }
        // what this pass leaves describes W_enc as it is now, centred on this context's current mu: a streamed forward may follow
        // while neither moves (a borrowed centre belongs to the leader: no streamed step there)
        c->wimg_fresh = c->stream_ok && c->fwd_step && !x_borrowed && c->leader == nullptr;
        c->wimg_mu_serial = c->mu_serial;
        HIPCHK(c, launch_bias_finish(reinterpret_cast<const double*>(c->dot_part), c->sq_part, c->Dp, S, c->S_pad,
                                     scl(c) + 1, c->params + c->off_b_enc, c->b_shift, c->wnorm_scratch, s, c->b_seen));
        // (defer_margins: the caller's launch_pre_encode forms the margins together with the encoder's per-launch state)
        if (!defer_margins)
            HIPCHK(c, launch_row_margins(c->xnorm_c, n, D, c->wnorm_scratch, (S + 255) / 256, scl(c), pre_flag,
                                         c->wmax_prev, c->row_margin, s));
        return SAEV_OK;
    }
    if (!x_borrowed) HIPCHK(c, launch_split_rows(x, n, D, c->Dp, c->xs, bf ? 1 : 0, s));
    { int rcw = wait_wenc(c, s); if (rcw != SAEV_OK) return rcw; }
    // (bf16: the fused Adam of the previous step has left the images of the W_enc it wrote -- AdamImageArgs::mode 1 -- and nothing
    // has written the parameters since: include/saev_amd.h, PARAMETER OWNERSHIP)
    c->fwd_reused_wimg = bf && c->wimg_bf16_fresh;
    if (!(bf && c->wimg_bf16_fresh))
        HIPCHK(c, launch_split_wT(c->params + c->off_W_enc, D, S, c->S_pad, c->Dp, bf ? 1.0f : 256.0f, c->ws, bf ? 1 : 0, s));
    if (bf && c->dbg.prep_route == 0 && c->Dp == D && D % 32 == 0) c->wimg_bf16_fresh = true;  // (the images describe W_enc as it is)
    return SAEV_OK;
}

// The f16x3 images of a ReLU TRAINING context's dense h: x times the power of two that puts max |x| (absmax_dev, on the device)
// into [2^13, 2^14), written to pair = {2^e, 1} for the encoder to undo.  The other contexts' f16x3 images carry no
// data-dependent scale (|x| < 65 504, and small x loses the low half to fp16's subnormals); the dense step's mask is
// a comparison of h with zero and must hold at any activation scale, as its other four contractions do (rt_scales).
static int prepare_dense_scaled(saev_ctx* c, const float* x, int n, const float* absmax_dev, float* pair, hipStream_t s) {
    HIPCHK(c, launch_pow2_scale(absmax_dev, pair, s));
    HIPCHK(c, launch_split_rows(x, n, c->cfg.d_model, c->Dp, c->xs, 0, s, 1.0f, pair));
    { int rcw = wait_wenc(c, s); if (rcw != SAEV_OK) return rcw; }
    HIPCHK(c, launch_split_wT(c->params + c->off_W_enc, c->cfg.d_model, c->cfg.d_sae, c->S_pad, c->Dp, 256.0f, c->ws, 0, s));
    return SAEV_OK;
}

static int run_encoder(saev_ctx* c, const float* x, int n, int epi, float* h_out, const int32_t* flag, int when,
                       hipStream_t s, bool predicted = false, const float* x_scale = nullptr, bool norm_bounds = false) {
    // F16R: only the TopK pass is approximate-then-refined; a dense h must be exact, so it comes from the fp32 kernel
    const bool f16r = c->cfg.encoder_mode == SAEV_ENCODER_F16R;
    if (c->cfg.encoder_mode != SAEV_ENCODER_F32 && !(f16r && epi == EPI_DENSE)) {
        const bool bf = c->cfg.encoder_mode == SAEV_ENCODER_BF16;
        EncodeF16Args a{};
        a.xs = c->xs_c; a.ws = c->ws;
        a.b_enc = f16r ? c->b_shift : c->params + c->off_b_enc;  // f16r: images are centred, the bias carries mu W
        a.n_rows = n; a.Dp = c->Dp; a.S = c->cfg.d_sae; a.w_scale = (bf || f16r) ? 1.0f : 256.0f;
        a.scale_dev = f16r ? scl(c) : x_scale;  // (x_scale: prepare_dense_scaled's pair, f16x3 only)
        a.arith = bf ? 1 : (f16r ? 2 : 0);
        a.row_margin = f16r ? c->row_margin : nullptr;
        a.s_splits = encoder_splits(n, a.S, encode_f16x3_tile_rows(), encode_f16x3_tile_latents(), 256);  // (one workgroup per CU)
        a.h_out = h_out;
        a.ngroups = f16_ngroups(c); a.top_k = c->cfg.top_k;
        a.gmax = c->gmax; a.gmax_stride = c->gmax_stride; a.cand_cnt = c->cand_cnt; a.cand_val = c->cand_val; a.cand_idx = c->cand_idx;
        a.cand_cap = CAND_CAP; a.cand_stride = CAND_STRIDE;
        a.enable_flag = flag; a.enable_when = when;
        if (predicted) { a.heur_z = c->heur_state; a.tau_max = c->tau_max; }
        if (norm_bounds) a.row_bound = c->row_bound;  // (pre_encode2_kernel has formed them, and the keys the select stage verifies)
        // the 64-group variant (32 < k <= 64, e.g. 82 k latents at k = 64) refreshes on every tile: with twice the codes
        // per row and many more tiles per workgroup its lists would outgrow their 4 096 entries otherwise
        a.refresh_first = 8;
        a.refresh_every = a.ngroups > 32 ? 1 : 2;
        HIPCHK(c, launch_encode_f16x3(a, epi, s));
        return SAEV_OK;
    }
    EncodeArgs a{};
    a.x = x;
    a.W_enc = c->params + c->off_W_enc;
    a.b_enc = c->params + c->off_b_enc;
    a.n_rows = n;
    a.D = c->cfg.d_model;
    a.S = c->cfg.d_sae;
    a.s_splits = encoder_splits(n, a.S, encode_gemm_tile_rows(), encode_gemm_tile_latents(), 512);
    a.h_out = h_out;
    a.ngroups = c->cfg.top_k <= 32 ? 32 : 64;
    a.gmax = c->gmax;
    a.gmax_stride = c->gmax_stride;
    a.cand_cnt = c->cand_cnt;
    a.cand_val = c->cand_val;
    a.cand_idx = c->cand_idx;
    a.cand_cap = CAND_CAP; a.cand_stride = CAND_STRIDE;
    a.enable_flag = flag;
    a.enable_when = when;
    HIPCHK(c, launch_encode_gemm(a, epi, s));
    return SAEV_OK;
}

int saev_encode_dense(saev_ctx* c, const float* x, int32_t n, float* h_out, void* stream) {
    if (!c) return SAEV_INVALID_ARG;
    REQUIRE(c, c->params, SAEV_NOT_BOUND, "parameters not bound");
    REQUIRE(c, x && h_out && n > 0, SAEV_INVALID_ARG, "saev_encode_dense: bad arguments");
    REQUIRE(c, n <= c->cfg.max_batch || c->cfg.encoder_mode == SAEV_ENCODER_F32, SAEV_INVALID_ARG,
            "saev_encode_dense: n_rows > max_batch");
    bind_x_sources(c, x, n, false);
    c->xprep_x = nullptr;  // the images below are rebuilt for this call: nothing to lend
    if (c->relu_train && c->cfg.encoder_mode == SAEV_ENCODER_F16X3) {
        // the step's own h, bit for bit: the same scaled images from this x's own maximum (in words of rt_scales the step does not
        // use: a step between its forward and its backward keeps its `upper` and its scales)
        hipStream_t s = (hipStream_t)stream;
        HIPCHK(c, hipMemsetAsync(c->rt_scales + 8, 0, sizeof(float), s));
        HIPCHK(c, launch_absmax(x, (long)n * c->cfg.d_model, c->rt_scales + 8, s));
        int rc = prepare_dense_scaled(c, x, n, c->rt_scales + 8, c->rt_scales + 10, s);
        if (rc != SAEV_OK) return rc;
        return run_encoder(c, x, n, EPI_DENSE, h_out, nullptr, 0, s, false, c->rt_scales + 10);
    }
    if (c->cfg.encoder_mode != SAEV_ENCODER_F16R) {  // (f16r: a dense h comes from the fp32 kernel, no images needed)
        int rc = prepare_encoder(c, x, n, nullptr, (hipStream_t)stream);
        if (rc != SAEV_OK) return rc;
    }
    return run_encoder(c, x, n, EPI_DENSE, h_out, nullptr, 0, (hipStream_t)stream);
}

int saev_topk_dense(saev_ctx* c, const float* h, int32_t n, int32_t k, const int32_t* mask, int32_t* idx_out,
                    float* val_out, void* stream) {
    if (!c) return SAEV_INVALID_ARG;
    REQUIRE(c, h && idx_out && val_out && n > 0 && k > 0, SAEV_INVALID_ARG, "saev_topk_dense: bad arguments");
    REQUIRE(c, k <= c->cfg.d_sae, SAEV_INVALID_ARG, "saev_topk_dense: k > d_sae");
    SelectDenseArgs a{};
    a.h = h; a.n_rows = n; a.S = c->cfg.d_sae; a.k = k; a.mask = mask;
    a.idx_out = idx_out; a.val_out = val_out; a.out_stride = k;
    HIPCHK(c, launch_select_dense(a, (hipStream_t)stream));
    return SAEV_OK;
}

// encode + top-k into (idx_out, val_out); fused path with exact dense fallback on overflow
static int encode_topk_impl(saev_ctx* c, const float* x, int n, int32_t* idx_out, float* val_out,
                            const int32_t* pre_flag, hipStream_t s, const float* xmax_dev = nullptr, bool x_borrowed = false) {
    const int K = c->cfg.top_k;
    int32_t* need_dense = c->flags + 1;
    const bool f16r_mode = c->cfg.encoder_mode == SAEV_ENCODER_F16R;
    const bool predict_mode = fused_supported(c->cfg) && c->cfg.bound_mode == 1 && c->cfg.encoder_mode != SAEV_ENCODER_F32 &&
                              f16_ngroups(c) == 32;
    const bool one_launch_pre = fused_supported(c->cfg) && !predict_mode;  // margins + encoder state + list flags in one launch
    if (c->follow_stream) {
        // nothing to prepare: the x side is the lender's, the W side this context's own Adam has left (its W scale with it)
        HIPCHK(c, launch_follower_scales(c->leader->xside_keep, c->wmax_prev, scl(c), const_cast<int32_t*>(pre_flag), 1, s));
    } else if (!c->stream_step) {
        int rc0 = prepare_encoder(c, x, n, const_cast<int32_t*>(pre_flag), s, xmax_dev, x_borrowed, one_launch_pre);
        if (rc0 != SAEV_OK) return rc0;
        rc0 = wait_wenc(c, s);  // (the f32 encoder has no preparation: it reads W_enc from here on)
        if (rc0 != SAEV_OK) return rc0;
    }
    if (fused_supported(c->cfg)) {
        const int ng = c->cfg.encoder_mode == SAEV_ENCODER_F32 ? (c->cfg.top_k <= 32 ? 32 : 64) : f16_ngroups(c);
        const bool f16r = c->cfg.encoder_mode == SAEV_ENCODER_F16R;
        // select -> (f16r: exact refinement -> select) on the candidate lists, predicated on `flag == when`
        auto select_stage = [&](const int32_t* flag, int when, int32_t* bad, const int32_t* tau_max, int32_t* ovf = nullptr,
                                const int32_t* first_flag = nullptr) -> int {
            // ovf / first_flag: the first select of the stage also does what overflow_check_kernel did (it is predicated on
            // first_flag, the flag known before the encoder ran; the kernels after it on `flag`, which it may raise)
            SelectCandArgs sc{};
            sc.cand_cnt = c->cand_cnt; sc.cand_val = c->cand_val; sc.cand_idx = c->cand_idx;
            sc.cand_cap = CAND_CAP; sc.cand_stride = CAND_STRIDE; sc.n_rows = n; sc.k = K;
            sc.idx_out = idx_out; sc.val_out = val_out; sc.out_stride = K;
            sc.enable_flag = first_flag ? first_flag : flag; sc.enable_when = when;
            sc.tau_max = tau_max; sc.invalid = bad; sc.ovf = ovf;
            if (f16r) {
                // approximate values: (1) survivors of the cut lowered by the row margin, (2) their exact fp32 values,
                // (3) the final cut on exact values.  A row with more than REFINE_CAP survivors raises `bad`.
                sc.row_margin = c->row_margin; sc.x = x; sc.W_encT = c->dW_encT; sc.b_enc = c->params + c->off_b_enc;
                sc.D = c->cfg.d_model; sc.refine_overflow = bad;
                sc.surv_idx = c->surv_idx; sc.surv_val = c->surv_val; sc.surv_cnt = c->surv_cnt;
                if (c->fwd_step) { sc.surv_rng = c->surv_rng; sc.lat_range = c->rs_lat_range; sc.n_ranges = c->rs_n_ranges; }
                // (The three as ONE launch measured 335 us against 351 when all of them ran at seven waves per SIMD, and slower
                // than them (+0.03 ms per step) once lists of 1 025-2 048 entries stay in registers, which the survivor select
                // needs (tools/experiments/README.md).)  A survivor overflow raises `bad` (= need_dense) like a list overflow
                // does, and the dense route that follows redoes the step exactly
                HIPCHK(c, launch_select_cand(sc, s));
                sc.enable_flag = flag; sc.ovf = nullptr;
                if (c->fwd_step) {  // exact values from 32-column slices of W_enc^T that the XCD L2s hold (select.hip)
                    RefineSlicesArgs rs{};
                    rs.surv_idx = c->surv_idx; rs.surv_cnt = c->surv_cnt; rs.surv_val = c->surv_val; rs.surv_rng = c->surv_rng;
                    rs.xS = c->xS_c; rs.WeS = c->stream_ok ? c->WeS : c->dW_encT; rs.b_enc = sc.b_enc; rs.part = c->rs_part;
                    rs.n_rows = n; rs.S = c->cfg.d_sae; rs.D = c->cfg.d_model;
                    rs.lat_range = c->rs_lat_range; rs.n_ranges = c->rs_n_ranges;
                    rs.enable_flag = flag; rs.enable_when = when;
                    // (the D / 32 shares of a survivor are added by the final select itself: no pass of their own, no round
                    // trip through surv_val)
                    HIPCHK(c, launch_refine_slices(rs, s));
                    sc.sum_part = c->rs_part; sc.sum_bias = sc.b_enc; sc.sum_n = c->cfg.d_model / RS_SLICE; sc.sum_plane = (size_t)n * REFINE_CAP;
                } else {
                    HIPCHK(c, launch_refine_exact(sc, s));
                }
                sc.row_margin = nullptr; sc.tau_max = nullptr;
                if (c->rho_step != 0) sc.kth_out = c->kth_val;  // (the exact k-th largest values: the next step's bounds scale from them)
                sc.cand_cnt = c->surv_cnt; sc.cand_val = c->surv_val; sc.cand_idx = c->surv_idx; sc.cand_cap = REFINE_CAP; sc.cand_stride = REFINE_CAP;
            }
            HIPCHK(c, launch_select_cand(sc, s));
            return SAEV_OK;
        };
        // Predicted bounds (gemm_encode_f16x3.hip, heur_z) for the fp16-image encoders with k <= 32: first a launch whose row
        // bounds are a prediction, verified by the select stage; only if that fails anywhere -- flag `bad1` -- the launch
        // with guaranteed bounds, which is otherwise skipped on the device (every kernel of it exits at once).
        const bool predict = c->cfg.bound_mode == 1 && ng == 32 && c->cfg.encoder_mode != SAEV_ENCODER_F32;
        int32_t *bad1 = c->flags + 9, *run2 = c->flags + 10, *gate = c->flags + 11;
        if (predict) {
            HIPCHK(c, launch_heur_gate(c->heur_state, pre_flag, gate, s));  // gate: no prediction this time
            HIPCHK(c, launch_encoder_init(c->cand_cnt, n, c->gmax, 0, s, c->tau_max));
            timing_begin(c, s);  // the events bracket the encoder kernel alone
            int rc = run_encoder(c, x, n, EPI_TOPK, nullptr, gate, 0, s, true);
            if (rc != SAEV_OK) return rc;
            timing_end(c, s);
            HIPCHK(c, launch_overflow_check(c->cand_cnt, n, CAND_CAP, gate, bad1, c->flags + 2, c->flags + 3, s, need_dense,
                                            nullptr, c->heur_state + 3, nullptr, pre_flag));
            rc = select_stage(bad1, 0, bad1, c->tau_max);
            if (rc != SAEV_OK) return rc;
            HIPCHK(c, launch_heur_update(c->heur_state, bad1, c->heur_state + 3, K, gate, s));
            // the retry with guaranteed bounds
            HIPCHK(c, launch_encoder_init(c->cand_cnt, n, c->gmax, ng * c->gmax_stride, s, nullptr, bad1, 1));
            rc = run_encoder(c, x, n, EPI_TOPK, nullptr, bad1, 1, s);
            if (rc != SAEV_OK) return rc;
            HIPCHK(c, launch_overflow_check(c->cand_cnt, n, CAND_CAP, pre_flag, need_dense, c->flags + 2, c->flags + 3, s, need_dense,
                                            run2, nullptr, bad1));
            rc = select_stage(run2, 1, need_dense, nullptr);
            if (rc != SAEV_OK) return rc;
        } else {
            const int S_ = c->cfg.d_sae;
            if (c->stream_step) {
                // the streamed preparation: one pass over x (gathered from the pool on the way in, if the caller handed a pool),
                // then one small launch; W_enc is not read at all (its images were left by the previous step's Adam)
                const int D_ = c->cfg.d_model;
                XprepArgs xp{};
                xp.x = c->gather_pool != nullptr ? c->gather_pool : x; xp.rows = c->gather_rows; xp.x_out = c->gather_pool != nullptr ? const_cast<float*>(x) : nullptr;
                xp.n = n; xp.D = D_; xp.nks = D_ / 32; xp.n_pad = c->MB_pad; xp.scales = scl(c); xp.mu = c->mu; xp.xs = c->xs; xp.xS = c->xS;
                xp.xn_part = c->xn_part; xp.col_part = c->colsum_partials; xp.amax_part = c->amax_part; xp.cmax_part = c->cmax_part;
                xp.W_enc = c->params + c->off_W_enc; xp.WeS = c->WeS; xp.b_enc = c->params + c->off_b_enc; xp.b_seen = c->b_seen;
                xp.S = S_; xp.salt = ++c->stale_salt; xp.stale = c->flags + 12;
                if (!c->followers.empty()) { xp.mu_keep = c->mu_keep; xp.xside_keep = c->xside_keep; }
                HIPCHK(c, launch_xprep(xp, s));
                PreEncode2Args pe{};
                pe.cand_cnt = c->cand_cnt; pe.n_rows = n; pe.gmax = c->gmax; pe.n_gmax = ng * c->gmax_stride;
                pe.xn_part = c->xn_part; pe.nks = D_ / 32; pe.n_pad = c->MB_pad; pe.D = D_;
                pe.wg_part = c->wnorm_scratch; pe.n_part = (S_ + 255) / 256; pe.scales = scl(c); pe.scales_next = scl_next(c);
                pe.pre_flag = const_cast<int32_t*>(pre_flag); pe.wmax_prev = c->wmax_prev; pe.margin = c->row_margin; pe.xnorm = c->xnorm;
                pe.flags1 = c->flags + 1; pe.col_part = c->colsum_partials; pe.n_rowblk = (n + 255) / 256; pe.mu = c->mu;
                pe.inv_n = 1.0f / (float)n; pe.update_mu = c->train_fused ? 1 : 0;
                pe.amax_part = c->amax_part; pe.cmax_part = c->cmax_part; pe.n_img = ((n + 255) / 256) * (D_ / 32);
                pe.upper = c->upper; pe.stats = c->stats; pe.stale = c->flags + 12; pe.stale_host = c->stale_dev;
                pe.xside_keep = c->followers.empty() ? nullptr : c->xside_keep;
                pe.rho_mode = c->rho_step; pe.rho_state = c->rho_state; pe.row_bound = c->row_bound; pe.tau_max = c->tau_max;
                pe.rho_bad = bad1; pe.rho_gate = gate;
                HIPCHK(c, launch_pre_encode2(pe, s));
                if (c->train_fused) c->mu_serial++;
            } else
            HIPCHK(c, launch_pre_encode(c->cand_cnt, n, c->gmax, ng * c->gmax_stride, f16r_mode ? c->xnorm_c : nullptr, c->cfg.d_model,
                                        c->wnorm_scratch, (S_ + 255) / 256, f16r_mode ? scl(c) : nullptr, const_cast<int32_t*>(pre_flag),
                                        c->wmax_prev, c->row_margin, c->flags + 1, s));
            timing_begin(c, s);  // the events bracket the encoder kernel alone
            if (c->stream_step && c->rho_step == 2) {
                // Norm-predicted bounds: pre_encode2_kernel has formed the rows' bounds from the previous step's ratios
                // and set `gate` (0: use them).  The select stage verifies them; if a row's k-th largest candidate misses its bound, a
                // list overflows or the gate is closed -- flag `bad1` -- the launch with guaranteed bounds follows, which is otherwise
                // left on the device (every kernel of it exits at once).  Its encoder runs on `run_enc` = bad1 and not the step's
                // force-dense flag: a step whose images are unusable goes straight to the dense route, as it always did.
                // (A pause the controller decides on reaches the host through a pinned word -- saev_step_forward -- and the
                // paused steps take the plain branch below: this one then costs the device-gated steps in between only.)
                int32_t* const run_enc = c->flags + 14;
                int rc = run_encoder(c, x, n, EPI_TOPK, nullptr, gate, 0, s, false, nullptr, true);
                if (rc != SAEV_OK) return rc;
                timing_end(c, s);
                rc = select_stage(bad1, 0, bad1, c->tau_max, bad1, gate);
                if (rc != SAEV_OK) return rc;
                HIPCHK(c, launch_repeat_init(c->cand_cnt, n, c->gmax, ng * c->gmax_stride, bad1, pre_flag, run_enc, s));
                rc = run_encoder(c, x, n, EPI_TOPK, nullptr, run_enc, 1, s);
                if (rc != SAEV_OK) return rc;
                HIPCHK(c, launch_overflow_check(c->cand_cnt, n, CAND_CAP, pre_flag, need_dense, c->flags + 2, c->flags + 3, s, need_dense,
                                                run2, nullptr, bad1));
                rc = select_stage(run2, 1, need_dense, nullptr, c->flags + 1, run2);
                if (rc != SAEV_OK) return rc;
            } else {
                int rc = run_encoder(c, x, n, EPI_TOPK, nullptr, pre_flag, 0, s);
                if (rc != SAEV_OK) return rc;
                timing_end(c, s);
                rc = select_stage(need_dense, 0, need_dense, nullptr, c->flags + 1, pre_flag);
                if (rc != SAEV_OK) return rc;
            }
        }
    } else {
        HIPCHK(c, launch_init_i32(need_dense, 1, 1, s));
        HIPCHK(c, hipMemsetAsync(c->flags + 2, 0, 2 * sizeof(int32_t), s));
        timing_begin(c, s);
        timing_end(c, s);
    }
    // exact dense route, predicated on the device flag (list overflow, refinement overflow, or k > 64)
    int rc = run_encoder(c, x, n, EPI_DENSE, c->h_dense, need_dense, 1, s);
    if (rc != SAEV_OK) return rc;
    SelectDenseArgs sd{};
    sd.h = c->h_dense; sd.n_rows = n; sd.S = c->cfg.d_sae; sd.k = K;
    sd.idx_out = idx_out; sd.val_out = val_out; sd.out_stride = K;
    sd.enable_flag = need_dense; sd.enable_when = 1;
    // (behind the fused encoder this launch is a fallback that a healthy step leaves at its first instruction: four workgroups per
    // CU that walk the rows retire in one round instead of n rounds' worth of empty workgroups; armed, the rows are the same)
    if (fused_supported(c->cfg)) sd.walk_grid = 4 * 256;
    HIPCHK(c, launch_select_dense(sd, s));
    return SAEV_OK;
}

int saev_encode_topk(saev_ctx* c, const float* x, int32_t n, int32_t* idx_out, float* val_out, void* stream) {
    if (!c) return SAEV_INVALID_ARG;
    REQUIRE(c, c->cfg.activation == SAEV_ACT_TOPK, SAEV_UNSUPPORTED,
            "saev_encode_topk: a TopK context only (ReLU: saev_encode_relu, BatchTopK: saev_encode_batch_topk)");
    REQUIRE(c, c->params, SAEV_NOT_BOUND, "parameters not bound");
    REQUIRE(c, x && idx_out && val_out && n > 0 && n <= c->cfg.max_batch, SAEV_INVALID_ARG,
            "saev_encode_topk: bad arguments (n_rows must be in 1..max_batch)");
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(c, hipMemsetAsync(c->flags, 0, sizeof(int32_t), s));
    bind_x_sources(c, x, n, false);
    c->xprep_x = nullptr;
    // An API encode always takes the full preparation: `stream_step` is what the LAST step's forward decided, and the images it
    // streamed from may be stale by now (a parameter write announced through saev_params_touched, an unfused tail); the streamed
    // launches would also clear the step's statistics and max |x|, which are not this call's to touch.
    c->stream_step = false;
    c->follow_stream = false;
    c->rho_step = 0; c->rho_valid = false;  // (norm-predicted bounds belong to consecutive training steps)
    return encode_topk_impl(c, x, n, idx_out, val_out, c->flags, s);
}

int saev_scatter_dense(saev_ctx* c, const int32_t* idx, const float* val, int32_t n, int32_t k, float* f_out,
                       void* stream) {
    if (!c) return SAEV_INVALID_ARG;
    REQUIRE(c, idx && val && f_out && n > 0 && k > 0, SAEV_INVALID_ARG, "saev_scatter_dense: bad arguments");
    HIPCHK(c, launch_scatter_dense(idx, val, n, k, k, c->cfg.d_sae, f_out, (hipStream_t)stream));
    return SAEV_OK;
}

int saev_decode_sparse(saev_ctx* c, const int32_t* idx, const float* val, int32_t n, int32_t k,
                       const int64_t* prefixes_host, int32_t n_prefixes, float* x_hats_out, void* stream) {
    if (!c) return SAEV_INVALID_ARG;
    REQUIRE(c, c->params, SAEV_NOT_BOUND, "parameters not bound");
    REQUIRE(c, idx && val && x_hats_out && n > 0 && k > 0, SAEV_INVALID_ARG, "saev_decode_sparse: bad arguments");
    const int S = c->cfg.d_sae, D = c->cfg.d_model;
    int64_t single = S;
    if (!prefixes_host) { prefixes_host = &single; n_prefixes = 1; }
    REQUIRE(c, n_prefixes >= 1 && prefixes_host[n_prefixes - 1] == S && prefixes_host[0] >= 1, SAEV_INVALID_ARG,
            "prefixes must end at d_sae and start at >= 1");
    for (int p = 1; p < n_prefixes; ++p)
        REQUIRE(c, prefixes_host[p] > prefixes_host[p - 1], SAEV_INVALID_ARG, "prefixes must be strictly increasing");
    // x_hats is (n, P, D).  One decode launch per prefix (cut = prefixes[p]); with P > 1 each prefix is
    // decoded into (n, D) scratch and copied into its strided slot.
    REQUIRE(c, n <= c->cfg.max_batch || n_prefixes == 1, SAEV_INVALID_ARG, "n_rows > max_batch");
    hipStream_t s = (hipStream_t)stream;
    for (int p = 0; p < n_prefixes; ++p) {
        DecodeArgs a{};
        a.x = nullptr;  // reconstruction only
        a.idx = idx; a.val = val; a.code_stride = k; a.k = k;
        a.W_dec = c->params + c->off_W_dec; a.b_dec = c->params + c->off_b_dec;
        a.n_rows = n; a.D = D; a.S = S; a.idx_limit = (int)prefixes_host[p];
        a.x_hat = (n_prefixes == 1) ? x_hats_out : c->g;
        HIPCHK(c, launch_decode(a, s));
        if (n_prefixes > 1)
            HIPCHK(c, hipMemcpy2DAsync(x_hats_out + (size_t)p * D, (size_t)n_prefixes * D * sizeof(float), c->g,
                                       (size_t)D * sizeof(float), (size_t)D * sizeof(float), n,
                                       hipMemcpyDeviceToDevice, s));
    }
    return SAEV_OK;
}

// ---- BatchTopK activation (batchtopk.hip) --------------------------------------------------------

namespace {
// select + compaction (training) or threshold compaction over a dense h into padded rows of the context's row capacity
int btk_codes(saev_ctx* c, const float* h, int n, int training, int32_t* row_nnz_out, int32_t* idx_out, float* val_out,
              int32_t* overflow_out, hipStream_t s) {
    BtkArgs a{};
    a.h = h; a.n_rows = n; a.S = c->cfg.d_sae; a.top_k = c->btk_k; a.row_cap = c->cfg.top_k; a.training = training ? 1 : 0;
    a.update_threshold = a.training; a.momentum = c->btk_momentum; a.threshold = c->threshold;
    a.idx_out = idx_out; a.val_out = val_out; a.row_nnz_out = row_nnz_out; a.overflow = overflow_out;
    a.ws = c->btk_ws; a.max_rows = c->cfg.max_batch; a.list_cap = c->btk_list_cap;
    HIPCHK(c, launch_batch_topk(a, s));
    return SAEV_OK;
}
}  // namespace

}  // extern "C"

// h = x W_enc + b_enc into the context's dense buffer: the exact fp32 kernel in the f32 and f16r modes, the split-fp16 one in f16x3
int encode_dense_h(saev_ctx* c, const float* x, int n, hipStream_t s) {
    if (c->relu_train && c->cfg.encoder_mode == SAEV_ENCODER_F16X3) {
        // (relu_train_forward has left max |x| in `upper`; the pair is the one its backward forms again for x's k-major images)
        int rc = prepare_dense_scaled(c, x, n, c->upper, c->rt_scales + 6, s);
        if (rc != SAEV_OK) return rc;
        return run_encoder(c, x, n, EPI_DENSE, c->h_dense, nullptr, 0, s, false, c->rt_scales + 6);
    }
    if (c->cfg.encoder_mode != SAEV_ENCODER_F16R) {
        int rc = prepare_encoder(c, x, n, nullptr, s);
        if (rc != SAEV_OK) return rc;
    } else {
        int rc = wait_wenc(c, s);
        if (rc != SAEV_OK) return rc;
    }
    return run_encoder(c, x, n, EPI_DENSE, c->h_dense, nullptr, 0, s);
}

extern "C" {

int saev_batch_topk_dense(saev_ctx* c, const float* h, int32_t n, int32_t training, int32_t* row_nnz_out, int32_t* idx_out,
                          float* val_out, int32_t* overflow_out, void* stream) {
    if (!c) return SAEV_INVALID_ARG;
    REQUIRE(c, c->btk, SAEV_UNSUPPORTED, "saev_batch_topk_dense: the context is not a BatchTopK context");
    REQUIRE(c, h && row_nnz_out && idx_out && val_out && overflow_out && n > 0 && n <= c->cfg.max_batch, SAEV_INVALID_ARG,
            "saev_batch_topk_dense: bad arguments (n_rows must be in 1..max_batch)");
    REQUIRE(c, ((uintptr_t)h % 16) == 0, SAEV_INVALID_ARG, "h must be 16-byte aligned");
    return btk_codes(c, h, n, training, row_nnz_out, idx_out, val_out, overflow_out, (hipStream_t)stream);
}

int saev_encode_batch_topk(saev_ctx* c, const float* x, int32_t n, int32_t training, int32_t* row_nnz_out, int32_t* idx_out,
                           float* val_out, int32_t* overflow_out, void* stream) {
    if (!c) return SAEV_INVALID_ARG;
    REQUIRE(c, c->btk, SAEV_UNSUPPORTED, "saev_encode_batch_topk: the context is not a BatchTopK context");
    REQUIRE(c, c->params, SAEV_NOT_BOUND, "parameters not bound");
    REQUIRE(c, x && row_nnz_out && idx_out && val_out && overflow_out && n > 0 && n <= c->cfg.max_batch, SAEV_INVALID_ARG,
            "saev_encode_batch_topk: bad arguments (n_rows must be in 1..max_batch)");
    REQUIRE(c, ((uintptr_t)x % 16) == 0, SAEV_INVALID_ARG, "x must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    bind_x_sources(c, x, n, false);
    c->xprep_x = nullptr;
    int rc = encode_dense_h(c, x, n, s);
    if (rc != SAEV_OK) return rc;
    return btk_codes(c, c->h_dense, n, training, row_nnz_out, idx_out, val_out, overflow_out, s);
}

// ---- ReLU SAE forward (relu.hip) --------------------------------------------------------------

int saev_encode_relu(saev_ctx* c, const float* x, int32_t n, int32_t row_cap, int32_t* row_nnz_out, int32_t* idx_out,
                     float* val_out, int32_t* overflow_out, void* stream) {
    if (!c) return SAEV_INVALID_ARG;
    REQUIRE(c, c->params, SAEV_NOT_BOUND, "parameters not bound");
    REQUIRE(c, c->cfg.activation == SAEV_ACT_RELU, SAEV_UNSUPPORTED, "saev_encode_relu: the context is not a ReLU context");
    REQUIRE(c, c->cfg.encoder_mode != SAEV_ENCODER_BF16, SAEV_UNSUPPORTED,
            "saev_encode_relu: the bf16 encoder is not available for ReLU (use f32, f16x3 or f16r)");
    REQUIRE(c, x && row_nnz_out && idx_out && val_out && overflow_out && n > 0 && row_cap > 0, SAEV_INVALID_ARG,
            "saev_encode_relu: bad arguments");
    REQUIRE(c, ((uintptr_t)x % 16) == 0, SAEV_INVALID_ARG, "x must be 16-byte aligned");
    REQUIRE(c, c->off_W_enc % 4 == 0, SAEV_UNSUPPORTED, "saev_encode_relu: W_enc is not 16-byte aligned in this layout");
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(c, hipMemsetAsync(overflow_out, 0, sizeof(int32_t), s));
    ReluEncodeArgs a{};
    a.x = x; a.W_enc = c->params + c->off_W_enc; a.b_enc = c->params + c->off_b_enc;
    a.n_rows = n; a.D = c->cfg.d_model; a.S = c->cfg.d_sae; a.row_cap = row_cap;
    a.idx_out = idx_out; a.val_out = val_out; a.row_nnz_out = row_nnz_out; a.max_nnz_out = overflow_out;
    HIPCHK(c, launch_relu_encode(a, s));
    return SAEV_OK;
}

int saev_decode_rows(saev_ctx* c, const int32_t* idx, const float* val, const int32_t* row_nnz, int32_t row_cap, int32_t n,
                     const int64_t* prefixes_host, int32_t n_prefixes, float* x_hats_out, void* stream) {
    if (!c) return SAEV_INVALID_ARG;
    REQUIRE(c, c->params, SAEV_NOT_BOUND, "parameters not bound");
    REQUIRE(c, idx && val && row_nnz && x_hats_out && n > 0 && row_cap > 0, SAEV_INVALID_ARG, "saev_decode_rows: bad arguments");
    const int S = c->cfg.d_sae;
    int64_t single = S;
    if (!prefixes_host) { prefixes_host = &single; n_prefixes = 1; }
    REQUIRE(c, n_prefixes >= 1 && n_prefixes <= 16, SAEV_INVALID_ARG, "saev_decode_rows: 1 to 16 prefixes");
    REQUIRE(c, prefixes_host[n_prefixes - 1] == S && prefixes_host[0] >= 1, SAEV_INVALID_ARG,
            "prefixes must end at d_sae and start at >= 1");
    for (int p = 1; p < n_prefixes; ++p)
        REQUIRE(c, prefixes_host[p] > prefixes_host[p - 1], SAEV_INVALID_ARG, "prefixes must be strictly increasing");
    ReluDecodeArgs a{};
    a.idx = idx; a.val = val; a.row_nnz = row_nnz; a.row_cap = row_cap; a.n_rows = n; a.D = c->cfg.d_model;
    a.W_dec = c->params + c->off_W_dec; a.b_dec = c->params + c->off_b_dec;
    a.n_prefixes = n_prefixes;
    for (int p = 0; p < n_prefixes; ++p) a.prefixes[p] = prefixes_host[p];
    a.x_hats = x_hats_out;
    HIPCHK(c, launch_relu_decode(a, (hipStream_t)stream));
    return SAEV_OK;
}

int saev_scatter_rows(saev_ctx* c, const int32_t* idx, const float* val, const int32_t* row_nnz, int32_t row_cap, int32_t n,
                      float* f_out, void* stream) {
    if (!c) return SAEV_INVALID_ARG;
    REQUIRE(c, idx && val && row_nnz && f_out && n > 0 && row_cap > 0, SAEV_INVALID_ARG, "saev_scatter_rows: bad arguments");
    HIPCHK(c, launch_relu_scatter(idx, val, row_nnz, row_cap, n, c->cfg.d_sae, f_out, (hipStream_t)stream));
    return SAEV_OK;
}

int saev_remove_parallel_grads(saev_ctx* c, void* stream) {
    if (!c) return SAEV_INVALID_ARG;
    REQUIRE(c, c->params && c->grads, SAEV_NOT_BOUND, "parameters/grads not bound");
    if (!c->cfg.remove_parallel_grads) return SAEV_OK;
    HIPCHK(c, launch_rpg(c->grads + c->off_W_dec, c->params + c->off_W_dec, c->cfg.d_sae, c->cfg.d_model,
                         (hipStream_t)stream));
    return SAEV_OK;
}

int saev_gather_rows(saev_ctx* c, const float* pool, const int64_t* rows, int32_t n, float* out, void* stream) {
    if (!c) return SAEV_INVALID_ARG;
    REQUIRE(c, pool && rows && out && n > 0, SAEV_INVALID_ARG, "saev_gather_rows: bad arguments");
    HIPCHK(c, launch_gather_rows(pool, rows, n, c->cfg.d_model, out, (hipStream_t)stream));
    return SAEV_OK;
}

// ------------------------------------------------------------------------------------------
// the step
// ------------------------------------------------------------------------------------------

int saev_step_forward(saev_ctx* c, const float* x, int32_t n, int64_t n_rows_global, int32_t training,
                      void* stream) {
    if (!c) return SAEV_INVALID_ARG;
    if (c->relu_train) return relu_train_forward(c, x, n, n_rows_global, training, (hipStream_t)stream);
    REQUIRE(c, c->cfg.activation != SAEV_ACT_RELU, SAEV_UNSUPPORTED, "saev_step_forward: a ReLU context runs the forward entries only");
    REQUIRE(c, c->params, SAEV_NOT_BOUND, "parameters not bound");
    REQUIRE(c, x && n > 0 && n <= c->cfg.max_batch, SAEV_INVALID_ARG,
            "saev_step_forward: n_rows must be in 1..max_batch");
    REQUIRE(c, ((uintptr_t)x % 16) == 0, SAEV_INVALID_ARG, "x must be 16-byte aligned");
    REQUIRE(c, n_rows_global >= n, SAEV_INVALID_ARG, "n_rows_global < n_rows");
    hipStream_t s = (hipStream_t)stream;
    const int S = c->cfg.d_sae, D = c->cfg.d_model, K = c->cfg.top_k;
    c->x_last = x;
    c->n_last = n;
    c->training_last = training;
    c->ov_x = nullptr; c->ov_n = 0;  // an override serves one backward
    c->unused_valid = false;
    // The reference renormalises the rows of W_dec at the top of a training step (train.py:334-335).  Nothing before the
    // decode reads W_dec, so it is done right in front of the decode instead: the rows it has just written are what the
    // decode gathers next (3.053 -> 3.034 ms per step against doing it first), and a caller whose decoder half of the
    // parameters is still arriving on another stream (saev_wdec_ready_event: the sharded tail's all-gather) is waited for
    // only there -- the encoder hides the transfer.
    hipEvent_t wdec_ev = c->wdec_ready;
    c->wdec_ready = nullptr;
    // everything that depends on x alone comes from the context this one shares its batches with, if that one has just
    // built it for this very batch (saev_share_x); otherwise it is built here
    const bool btk = c->btk;  // (BatchTopK: nothing is shared, streamed or fused -- dense h, select, compaction, then the generic decode)
    const bool borrowed = bind_x_sources(c, x, n, !btk);
    // The streamed preparation: this context neither lends nor borrows, a previous batch has left a centre, a scale
    // and a normaliser, and the operand images of W_enc describe the parameters as they are, centred on that very centre.
    if (c->stale_host != nullptr && reinterpret_cast<volatile int32_t*>(c->stale_host)[1] != 0) {
        // the fused Adam of an earlier step read W_enc tiles that were not the ones it had written: that step's forward ran on
        // operand images of other values.  Nothing can be redone: say so, loudly; the next forward prepares from scratch.
        const int n_tiles = reinterpret_cast<volatile int32_t*>(c->stale_host)[1];
        reinterpret_cast<volatile int32_t*>(c->stale_host)[1] = 0;
        c->wimg_fresh = false; c->wimg_bf16_fresh = false; c->wn2_fresh = false;  // (answers AdamImageArgs::chk, stale word [1]; these three, not params_moved)
        c->err = "W_enc was written outside the library without saev_params_touched (" + std::to_string(n_tiles) +
                 " 32 x 256 tiles changed between two optimizer steps): a recent step encoded with operand images of the OLD values. "
                 "Announce such writes (saev_params_touched / SaeEngine.params_touched) or make them through torch in-place "
                 "operations on the parameter tensors; the context prepares from scratch from here on";
        return SAEV_STALE_PARAMS;
    }
    if (c->stale_host != nullptr && *reinterpret_cast<volatile int32_t*>(c->stale_host) != 0) {
        // a streamed step found W_enc / b_enc changed behind its back (it took the exact route itself): prepare from scratch
        *reinterpret_cast<volatile int32_t*>(c->stale_host) = 0;
        c->wimg_fresh = false;  // (answers xprep_kernel's samples, stale word [0]; these two, not params_moved)
        c->wn2_fresh = false;
    }
    // (a lender streams like a context on its own; what its followers need beyond its second launch it keeps: XprepArgs::mu_keep)
    c->stream_step = c->stream_ok && c->prep_valid && c->wimg_fresh && c->wimg_mu_serial == c->mu_serial && c->leader == nullptr &&
                     c->wenc_ready == nullptr && c->fwd_step && (c->followers.empty() || c->dbg.group_route == 0);
    if (!borrowed) {
        c->fwd_streamed = c->stream_step;
        c->fwd_moves_mu = c->stream_step && c->train_fused;
        c->fwd_mu_serial = c->mu_serial;
    }
    // A follower of a streamed step whose own Adam has left W images centred on that very mu prepares nothing at all.
    c->follow_stream = borrowed && c->borrow_streamed && c->stream_ok && c->wimg_fresh && c->wimg_mu_serial == c->leader->fwd_mu_serial &&
                       c->wenc_ready == nullptr && c->fwd_step && c->cfg.encoder_mode == SAEV_ENCODER_F16R;
    c->fwd_reused_wimg = c->stream_step || c->follow_stream;  // (the bf16 encoder decides in prepare_encoder)
    {
        // Norm-predicted bounds (bound_mode 2): for the streamed training step of a plain TopK context on its own.  Such a step
        // leaves the smallest ratio of its rows for the next one; the next one predicts if nothing else came in between (another kind
        // of forward, a full preparation -- parameters announced as touched, a new centre --, another batch size).
        const bool rho_mode = c->cfg.bound_mode == 2 && c->rho_state != nullptr && c->stream_step && !borrowed && !btk && training &&
                              c->train_fused && c->P == 1 && c->followers.empty() && c->cfg.encoder_mode == SAEV_ENCODER_F16R &&
                              fused_supported(c->cfg) && f16_ngroups(c) == 32;
        // (a pause the device-side controller has decided on -- tail.hip: rho_controller -- arrives in two pinned words, serial and
        // length, without a synchronisation; until the host has seen it the device's own gate holds the prediction back.  A paused
        // step is a plain guaranteed step that leaves its ratios: none of the repeat's predicated launches)
        if (rho_mode && c->stale_host != nullptr) {
            const volatile int32_t* hw = c->stale_host + 4;
            const int32_t serial = hw[0];
            if (serial != c->rho_serial_seen) { c->rho_serial_seen = serial; c->rho_pause_left = hw[1]; }
        }
        const bool paused = rho_mode && c->rho_pause_left > 0;
        if (paused) c->rho_pause_left--;
        c->rho_step = rho_mode ? ((c->rho_valid && c->rho_n == n && !paused) ? 2 : 1) : 0;
        c->rho_valid = rho_mode;
        c->rho_n = n;
    }
    if (c->gather_pool != nullptr && !c->stream_step)  // (the batch as a contiguous matrix first: every other route reads x itself)
        HIPCHK(c, launch_gather_rows(c->gather_pool, c->gather_rows, n, D, const_cast<float*>(x), s));
    if (c->stream_step) {
        c->xprep_x = nullptr;  // (xprep_kernel / pre_encode2_kernel, enqueued by encode_topk_impl, do all of the below)
    } else if (!borrowed && !btk && c->cfg.encoder_mode == SAEV_ENCODER_F16R) {
        // one pass: max|x| for the MSE and the column sums the encoder centres on; the launch that finishes them also clears
        // the step's statistics and the force-dense flag (flags[0])
        c->xprep_x = nullptr;
        HIPCHK(c, launch_colsum_absmax(x, n, D, c->colsum_partials, c->mu, c->xabs_part, c->upper, s, 1.0f / (float)n, c->stats, c->flags));
        c->mu_ready = true;
        c->mu_serial++;
    } else {
        HIPCHK(c, launch_step_zero(c->stats, c->upper, c->flags, s));
        if (!borrowed) {
            c->xprep_x = nullptr;
            HIPCHK(c, launch_absmax(x, (long)n * D, c->upper, s));
        }
    }
    (void)n_rows_global;
    int rc;
    if (btk) {
        rc = encode_dense_h(c, x, n, s);
        if (rc == SAEV_OK) rc = btk_codes(c, c->h_dense, n, training, c->row_nnz, c->idx, c->val, c->btk_over, s);
        if (rc == SAEV_OK) {
            // the step's one read-back: no row may be truncated, and nothing downstream can be sized on the device
            int32_t need = 0;
            HIPCHK(c, hipMemcpyAsync(&need, c->btk_over, sizeof(int32_t), hipMemcpyDeviceToHost, s));
            HIPCHK(c, hipStreamSynchronize(s));
            if (need > 0) {
                c->btk_need = need;
                c->x_last = nullptr; c->n_last = 0; c->training_last = 0;  // no step is in flight: a backward or tail must not follow
                c->err = "BatchTopK: a row holds " + std::to_string(need) + " codes, the context's row_cap is " + std::to_string(K) +
                         " (create a context with a larger saev_batch_topk_cfg.row_cap and repeat the forward; the threshold has not moved)";
                return SAEV_ROW_OVERFLOW;
            }
        }
    } else {
        rc = encode_topk_impl(c, x, n, c->idx, c->val, c->flags, s, c->upper_c, borrowed);
    }
    if (rc != SAEV_OK) return rc;
    if (!borrowed) { c->xprep_x = x; c->xprep_n = n; c->xprep_serial++; }
    if (!borrowed && c->stream_ok && !c->stream_step && c->fwd_step) {
        // a full preparation seeds the streamed one: this batch's x scale is in scl(c)[0] already, its max |x| becomes the normaliser
        HIPCHK(c, hipMemcpyAsync(scl(c) + 4, c->upper, sizeof(float), hipMemcpyDeviceToDevice, s));
        c->prep_valid = true;
    }
    if (wdec_ev != nullptr) HIPCHK(c, hipStreamWaitEvent(s, wdec_ev, 0));
    if (training) {
        c->wn2_fresh = false;
        if (c->cfg.normalize_w_dec) {
            HIPCHK(c, launch_normalize_rows(c->params + c->off_W_dec, S, D, s, c->wn2));
            c->wn2_fresh = c->wn2 != nullptr;
        }
    }

    DecodeArgs a{};
    a.x = x; a.idx = c->idx; a.val = c->val; a.code_stride = K; a.k = K;
    a.W_dec = c->params + c->off_W_dec; a.b_dec = c->params + c->off_b_dec;
    a.n_rows = n; a.D = D; a.S = S; a.idx_limit = S;
    a.upper = c->upper_c;
    a.gscale = 2.0f / ((float)n * (float)D * (float)c->P);
    a.training = training ? 1 : 0;
    a.g = c->g; a.x_hat = c->x_hat; a.fired = c->fired; a.rowstats = c->rowstats;
    c->dws_rows = 0;
    c->dval_fwd = false;
    // (slice-major copies for the weight gradients: dL/dx_hat always from the decode, x only when split_f16r has not left one)
    if (training && c->dws_ok && (c->P == 1 || c->GS != nullptr)) { a.gS = c->P == 1 ? c->gS : c->GS; a.xS = c->fwd_step ? nullptr : c->xS; c->dws_rows = n; }
    // (... and the products dval, from the decoder rows while the decode holds them in registers)
    if (c->dws_rows == n && c->dval_rows != nullptr && (c->P == 1 || decode_matry_forms_dval(D, K))) { a.dval_out = c->dval_rows; c->dval_fwd = true; }
    // (saev_train_step's own backward takes the column slices over all latents and the column sums of db_dec from gS as well: the
    // plain decode writes no row-major g then -- n x d_model floats nobody reads.  The phases keep it: saev_copy_step_state, dw_rows)
    c->g_rows_valid = !(c->train_fused && training && c->P == 1 && c->dws_rows == n);
    if (!c->g_rows_valid) a.g = nullptr;
    // The decode reads every code anyway: it sets the (latent, row) bits of the backward's pair-list build (0.5 M scattered atomics
    // that csc_fill paid 35 us for on their own), provided the bit map is clean at this row pitch -- the previous full backward
    // cleared it behind itself -- and this context's backwards run over its own rows.
    c->bitmap_prefill_words = 0;
    if (training && c->dbg.csc_route == 0 && c->bitmap != nullptr && c->bitmap_clean && !c->last_backward_gathered) {
        const int words = ((n + 31) / 32 + 7) / 8 * 8;
        if (words <= c->bitmap_clean_words) {
            a.csc_bitmap = c->bitmap; a.csc_words = words;
            c->bitmap_prefill_words = words; c->bitmap_prefill_rows = n;
            c->bitmap_clean = false;
        }
    }
    if (c->P > 1) {
        MatryArgs m{};
        m.P = c->P;
        for (int p = 0; p < c->P; ++p) m.cuts[p] = c->cuts[p];
        m.G = c->G;
        m.g_rows_all = c->fused_forward ? 0 : 1;  // (saev_train_step's own backward reads the slice-major copy and block 0 alone)
        HIPCHK(c, launch_decode_matry(a, m, s));
    } else {
        HIPCHK(c, launch_decode(a, s));
    }
    c->P_last = c->P;
    for (int p = 0; p < c->P; ++p) c->cuts_last[p] = c->cuts[p];  // a later saev_set_prefixes must not reach this step's backward
    // (list statistics from the candidate counters themselves unless the fused encoder is out of play or predicts bounds,
    // where overflow_check_kernel leaves them in flags[2..3])
    const bool lists = !btk && fused_supported(c->cfg) && !(c->cfg.bound_mode == 1 && c->cfg.encoder_mode != SAEV_ENCODER_F32 && f16_ngroups(c) == 32);
    c->stats_pending = false;
    if (c->train_fused && training) {  // (saev_train_step: the tracker update that follows takes this reduction into its launch)
        c->stats_pending = true;
        c->stats_lists = lists;
        return SAEV_OK;
    }
    HIPCHK(c, launch_stats_reduce(c->rowstats, n, D, c->P, c->cfg.alpha, 0, c->upper_c, c->flags + 2, c->stats, s, nullptr, c->stats_scratch,
                                  lists ? c->cand_cnt : nullptr, CAND_CAP));
    return SAEV_OK;
}

}  // extern "C"
