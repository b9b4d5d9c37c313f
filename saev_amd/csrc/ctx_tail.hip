// The optimizer tails behind the C ABI (clip norm, Adam, Muon) and the fused train step that strings the phases together.
#include "ctx.h"

extern "C" {

// The element ranges a tail call works on: everything (shard_rank < 0), or rank `shard_rank`'s chunk of each half.
namespace {
struct TailRanges { long a_lo, a_hi, b_lo, b_hi; };
int tail_ranges(saev_ctx* c, int shard_rank, TailRanges* r) {
    if (shard_rank < 0) {
        *r = {0, c->off_W_enc, c->off_W_enc, c->n_params};
        return SAEV_OK;
    }
    REQUIRE(c, shard_rank < c->shard_world, SAEV_INVALID_ARG, "shard_rank >= saev_cfg.shard_world");
    r->a_lo = (long)shard_rank * c->chunk_a; r->a_hi = r->a_lo + c->chunk_a;
    r->b_lo = c->off_W_enc + (long)shard_rank * c->chunk_b; r->b_hi = r->b_lo + c->chunk_b;
    return SAEV_OK;
}
// Adam's constants for this step, the clip and the loss scale: what the Adam launches of both tails share (p / g / m / v / n per launch)
AdamArgs adam_args(saev_ctx* c, float lr, float max_norm, float grad_scale, int64_t adam_step) {
    AdamArgs a{};
    a.lr = lr; a.beta1 = 0.9f; a.beta2 = 0.999f; a.eps = 1e-8f;
    a.omb1 = (float)(1.0 - 0.9); a.omb2 = (float)(1.0 - 0.999);
    a.bc1 = (float)(1.0 - std::pow(0.9, (double)adam_step));
    a.bc2_sqrt = (float)std::sqrt(1.0 - std::pow(0.999, (double)adam_step));
    a.grad_scale = grad_scale; a.max_norm = max_norm; a.sumsq = saev_sumsq_device(c); a.stats = c->stats;
    return a;
}
}  // namespace

double* saev_sumsq_device(saev_ctx* c) { return c ? (c->sumsq_bound ? c->sumsq_bound : c->sumsq_total) : nullptr; }

int saev_bind_sumsq(saev_ctx* c, double* sumsq) {
    if (!c) return SAEV_INVALID_ARG;
    c->sumsq_bound = sumsq;
    return SAEV_OK;
}

int saev_wenc_ready_event(saev_ctx* c, void* event) {
    if (!c) return SAEV_INVALID_ARG;
    c->wenc_ready = (hipEvent_t)event;
    return SAEV_OK;
}

int saev_wdec_ready_event(saev_ctx* c, void* event) {
    if (!c) return SAEV_INVALID_ARG;
    c->wdec_ready = (hipEvent_t)event;
    return SAEV_OK;
}

int saev_tail_prepare(saev_ctx* c, int32_t shard_rank, void* stream) {
    if (!c) return SAEV_INVALID_ARG;
    REQUIRE(c, c->cfg.activation != SAEV_ACT_RELU || c->relu_train, SAEV_UNSUPPORTED, "saev_tail_prepare: a ReLU context runs the forward entries only");
    REQUIRE(c, c->params && c->grads, SAEV_NOT_BOUND, "saev_tail_prepare: params/grads not bound");
    TailRanges r;
    int rc = tail_ranges(c, shard_rank, &r);
    if (rc != SAEV_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    const long S = c->cfg.d_sae, D = c->cfg.d_model;
    c->tail_proj_in_adam = false;
    if (c->wenc_t_pending) {
        // saev_train_step left the W_enc gradient in the transposed scratch: its squares come from the rows' statistics too
        // (enc_sq), and the one Adam launch reads it from there (adam_fused_kernel) -- no transpose pass at all
        REQUIRE(c, c->row_proj_valid && shard_rank < 0, SAEV_INVALID_ARG, "saev_tail_prepare: pending transposed gradient without a full backward");
        c->row_proj_valid = false;
        HIPCHK(c, launch_sumsq_final_ex(nullptr, 0, c->row_proj, (int)S, c->grads + S * D, r.a_hi - S * D,
                                        c->grads + c->off_b_enc, r.b_hi - c->off_b_enc, saev_sumsq_device(c), c->sumsq_partials,
                                        c->tickets + 1, s, c->enc_sq, c->sq_wave_n > 0 ? c->sq_wave : nullptr, 2l * c->sq_wave_n));
        c->sq_wave_n = 0;
        c->tail_proj_in_adam = true;
        return SAEV_OK;
    }
    if (c->trust_grads && c->wenc_sq_valid && c->row_proj_valid && shard_rank < 0) {
        // The caller vouches that nothing has touched the gradient since the backward: the kernels that wrote the decoder
        // rows left each row's projection coefficient and projected squares (row_proj), the transpose the squares of dW_enc
        // tile by tile.  One small reduction gives the clip norm, and Adam applies the projection to the rows as it reads
        // them: the gradient is streamed once by the whole tail instead of three times (rpg read + write, Adam read).
        c->wenc_sq_valid = false; c->row_proj_valid = false;
        const double* tsq = c->sumsq_partials + 2 * sumsq_blocks() + (S + 3) / 4;
        HIPCHK(c, launch_sumsq_final_ex(tsq, transpose_blocks((int)S, (int)D), c->row_proj, (int)S, c->grads + S * D, r.a_hi - S * D,
                                        c->grads + c->off_b_enc, r.b_hi - c->off_b_enc, saev_sumsq_device(c), c->sumsq_partials,
                                        c->tickets + 1, s));
        c->tail_proj_in_adam = true;
        return SAEV_OK;
    }
    c->row_proj_valid = false;
    // decoder rows of the range: projection (modeling.py:419-445) and their squares in one pass over the gradient
    const long row_lo = std::min(r.a_lo / D, S), row_hi = std::min(r.a_hi / D, S);
    const int n_rows = (int)(row_hi - row_lo);
    const int nb = sumsq_blocks();
    double* part = c->sumsq_partials;  // [0, nb): rest of the first half; [nb, 2 nb): second half; then one per 4 rows
    HIPCHK(c, launch_rpg(c->grads + row_lo * D, c->params + row_lo * D, n_rows, (int)D, s, part + 2 * nb,
                         c->cfg.remove_parallel_grads ? 1 : 0));
    const long rest_lo = std::max(r.a_lo, S * D);
    HIPCHK(c, launch_sumsq_partials(c->grads + rest_lo, std::max(0L, r.a_hi - rest_lo), part, s));
    c->wenc_sq_valid = false;
    HIPCHK(c, launch_sumsq_partials(c->grads + r.b_lo, r.b_hi - r.b_lo, part + nb, s));
    HIPCHK(c, launch_sumsq_final(part, 2 * nb + (n_rows + 3) / 4, saev_sumsq_device(c), s));
    return SAEV_OK;
}

int saev_tail_apply(saev_ctx* c, float lr, float max_norm, float grad_scale, int64_t adam_step, int32_t shard_rank,
                    void* stream) {
    if (!c) return SAEV_INVALID_ARG;
    REQUIRE(c, c->cfg.activation != SAEV_ACT_RELU || c->relu_train, SAEV_UNSUPPORTED, "saev_tail_apply: a ReLU context runs the forward entries only");
    REQUIRE(c, c->params && c->grads && c->adam_m && c->adam_v, SAEV_NOT_BOUND,
            "saev_tail_apply: params/grads/adam state not bound");
    REQUIRE(c, adam_step >= 1, SAEV_INVALID_ARG, "adam_step is 1-based");
    TailRanges r;
    int rc = tail_ranges(c, shard_rank, &r);
    if (rc != SAEV_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    // (a follower's images are centred on its lender's NEXT mu -- there once the lender's step, which ran first, was a streamed
    // saev_train_step: fwd_moves_mu -- and carry the lender's serial of it)
    const bool emit_follow = c->leader != nullptr && c->borrow_streamed && c->leader->fwd_moves_mu && c->dbg.group_route == 0 &&
                             c->cfg.encoder_mode == SAEV_ENCODER_F16R && c->fwd_step;
    const bool emit = c->train_fused && c->stream_ok && (c->leader == nullptr ? c->prep_valid && (c->followers.empty() || c->dbg.group_route == 0) : emit_follow) &&
                      shard_rank < 0 && c->tail_proj_in_adam && c->wenc_t_pending;
    const bool chk_was_valid = c->wchk_valid;
    const bool emit_bf16 = c->train_fused && c->cfg.encoder_mode == SAEV_ENCODER_BF16 && c->wimg_bf16_fresh && shard_rank < 0 &&
                           c->tail_proj_in_adam && c->wenc_t_pending;
    params_moved(c);  // (W_dec and W_enc move: only the fused Adam below leaves images of what it writes)
    AdamArgs a = adam_args(c, lr, max_norm, grad_scale, adam_step);
    const long lo[2] = {r.a_lo, r.b_lo}, hi[2] = {r.a_hi, r.b_hi};
    if (shard_rank < 0 && c->tail_proj_in_adam && c->wenc_t_pending) {  // everything in one launch (adam_fused_kernel)
        c->tail_proj_in_adam = false; c->wenc_t_pending = false;
        const long S = c->cfg.d_sae, D = c->cfg.d_model;
        a.p = c->params; a.g = c->grads; a.m = c->adam_m; a.v = c->adam_v; a.n = c->n_params;
        AdamImageArgs im{};
        if (emit) {
            // this step's images were built (or found) with scl(c); a step that took the full preparation hands its x scale and
            // normaliser on to the next one (a streamed step's second launch has written them already)
            if (!c->stream_step) HIPCHK(c, hipMemcpyAsync(scl_next(c), scl(c), 8 * sizeof(float), hipMemcpyDeviceToDevice, s));
            im.ws = c->ws; im.WeS = c->WeS; im.dot_part = reinterpret_cast<double*>(c->dot_part); im.sq_part = c->sq_part;
            im.mu = c->leader != nullptr ? c->leader->mu : c->mu; im.wmax_prev = c->wmax_prev; im.scales_next = scl_next(c); im.nks = c->Dp / 32; im.S_pad = c->S_pad;
        }
        if (emit_bf16) { im.ws = c->ws; im.nks = c->Dp / 32; im.S_pad = c->S_pad; im.mode = 1; }
        if ((emit || emit_bf16) && c->wchk != nullptr) {
            // the tiles' checksums: left for the next step, and -- when this step's forward ran on images an earlier Adam left --
            // compared with what that Adam left (an evaluation forward in between changes nothing: W_enc did not move)
            im.chk = c->wchk; im.late = c->stale_dev != nullptr ? c->stale_dev + 1 : nullptr;
            im.verify = (chk_was_valid && c->fwd_reused_wimg && im.late != nullptr) ? 1 : 0;
            im.early = (emit && c->leader == nullptr) ? c->flags + 13 : nullptr;  // (a follower's first kernels do not look at W_enc)
        }
        HIPCHK(c, launch_adam_fused(a, c->row_proj, c->dW_encT, (int)S, (int)D, S * D, c->off_W_enc - S * D, c->off_W_enc,
                                    c->off_b_enc, c->n_params - c->off_b_enc, s, c->unused_valid ? c->lat_unused : nullptr,
                                    (emit || emit_bf16) ? &im : nullptr));
        c->unused_valid = false;
        c->wchk_valid = (emit || emit_bf16) && c->wchk != nullptr;
        c->wimg_bf16_fresh = emit_bf16;
        if (emit) {
            // the bias of the next centred first pass and the column-norm maxima its margins need: W-only, so they are finished here
            HIPCHK(c, launch_bias_finish(reinterpret_cast<const double*>(c->dot_part), c->sq_part, c->Dp, (int)S, c->S_pad, scl_next(c) + 1,
                                         c->params + c->off_b_enc, c->b_shift, c->wnorm_scratch, s, c->b_seen));
            c->scale_par ^= 1;
            c->wimg_fresh = true;
            c->wimg_mu_serial = c->leader != nullptr ? c->leader->mu_serial : c->mu_serial;
        }
        return SAEV_OK;
    }
    if (shard_rank < 0 && c->tail_proj_in_adam) {  // decoder rows with the projection applied on the way in, then the rest
        c->tail_proj_in_adam = false;
        const long S = c->cfg.d_sae, D = c->cfg.d_model;
        a.p = c->params; a.g = c->grads; a.m = c->adam_m; a.v = c->adam_v; a.n = S * D;
        HIPCHK(c, launch_adam_rows(a, c->row_proj, (int)S, (int)D, s));
        a.p += S * D; a.g += S * D; a.m += S * D; a.v += S * D; a.n = c->n_params - S * D;
        HIPCHK(c, launch_adam(a, s));
        return SAEV_OK;
    }
    c->tail_proj_in_adam = false;
    if (shard_rank < 0) {  // one contiguous stream over everything
        a.p = c->params; a.g = c->grads; a.m = c->adam_m; a.v = c->adam_v; a.n = c->n_params;
        HIPCHK(c, launch_adam(a, s));
        return SAEV_OK;
    }
    for (int h = 0; h < 2; ++h) {
        a.p = c->params + lo[h]; a.g = c->grads + lo[h]; a.m = c->adam_m + lo[h]; a.v = c->adam_v + lo[h]; a.n = hi[h] - lo[h];
        HIPCHK(c, launch_adam(a, s));
    }
    return SAEV_OK;
}

int saev_step_tail(saev_ctx* c, float lr, float max_norm, float grad_scale, int64_t adam_step, void* stream) {
    int rc = saev_tail_prepare(c, -1, stream);
    if (rc != SAEV_OK) return rc;
    return saev_tail_apply(c, lr, max_norm, grad_scale, adam_step, -1, stream);
}

int saev_train_step_gather(saev_ctx* c, const float* pool, const int64_t* rows, float* x_out, int32_t n, float lr, float max_norm,
                           int64_t adam_step, void* stream) {
    if (!c) return SAEV_INVALID_ARG;
    REQUIRE(c, pool && rows && x_out, SAEV_INVALID_ARG, "saev_train_step_gather: NULL buffer");
    REQUIRE(c, !c->btk, SAEV_UNSUPPORTED, "saev_train_step_gather: not for a BatchTopK context (draw the batch first: saev_gather_rows)");
    REQUIRE(c, !c->relu_train, SAEV_UNSUPPORTED, "saev_train_step_gather: not for a ReLU training context (draw the batch first: saev_gather_rows)");
    c->gather_pool = pool; c->gather_rows = rows;
    const int rc = saev_train_step(c, x_out, n, lr, max_norm, adam_step, stream);
    c->gather_pool = nullptr; c->gather_rows = nullptr;
    return rc;
}

// ---- Muon tail (include/saev_amd.h: MUON; kernels in muon.hip) ------------------------------------------------------------
namespace {
// the shortest decimal that rounds to f, as a double: the value a caller wrote (0.95, 0.1) when it came from a float field, so
// that 1 - momentum and 1 - lr * weight_decay round as torch's Python-float arithmetic does
double muon_dec(float f) {
    char buf[32];
    for (int p = 1; p <= 9; ++p) {
        std::snprintf(buf, sizeof buf, "%.*g", p, (double)f);
        const double d = std::strtod(buf, nullptr);
        if ((float)d == f) return d;
    }
    return (double)f;
}
}  // namespace

int saev_muon_tail(saev_ctx* c, float lr, float max_norm, float grad_scale, int64_t adam_step, const saev_muon_cfg* cfg, void* stream) {
    if (!c) return SAEV_INVALID_ARG;
    REQUIRE(c, c->cfg.activation != SAEV_ACT_RELU || c->relu_train, SAEV_UNSUPPORTED, "saev_muon_tail: a ReLU context runs the forward entries only");
    REQUIRE(c, c->params && c->grads && c->adam_m && c->adam_v, SAEV_NOT_BOUND, "saev_muon_tail: params/grads/adam state not bound");
    REQUIRE(c, adam_step >= 1, SAEV_INVALID_ARG, "adam_step is 1-based");
    REQUIRE(c, !c->wenc_t_pending, SAEV_INVALID_ARG, "saev_muon_tail: runs after the phases, not inside saev_train_step");
    saev_muon_cfg m;
    saev_muon_default_cfg(&m);
    if (cfg) m = *cfg;
    {
        std::string why;
        const int rc = muon_cfg_check(m, &why);
        REQUIRE(c, rc == SAEV_OK, rc, "saev_muon_tail: " + why);
    }
    hipStream_t s = (hipStream_t)stream;
    const int S = c->cfg.d_sae, D = c->cfg.d_model;
    REQUIRE(c, D <= S, SAEV_UNSUPPORTED, "saev_muon_tail: d_model > d_sae");
    const MuonLayout L = muon_layout(D, S);
    if (c->muon_ws == nullptr) {
        void* q = nullptr;
        HIPCHK(c, hipMalloc(&q, L.bytes));
        c->allocs.push_back(q);
        c->muon_ws = static_cast<uint8_t*>(q);
        c->muon_bytes = L.bytes;
        // the padding of both X buffers stays zero from here on: the passes write [0, D) x [0, S) only, the products keep zeros
        HIPCHK(c, hipMemsetAsync(c->muon_ws, 0, L.off_G, s));
    }
    // remove_parallel_grads in place and the clip norm's sum of squares (the generic route: Muon reads the projected gradient)
    c->row_proj_valid = false;
    int rc = saev_tail_prepare(c, -1, stream);
    if (rc != SAEV_OK) return rc;
    params_moved(c);  // (W_enc / W_dec move)
    AdamArgs a = adam_args(c, lr, max_norm, grad_scale, adam_step);
    const long off_b[2] = {c->off_b_dec, c->off_b_enc}, n_b[2] = {D, S};
    for (int h = 0; h < 2; ++h) {
        a.p = c->params + off_b[h]; a.g = c->grads + off_b[h]; a.m = c->adam_m + off_b[h]; a.v = c->adam_v + off_b[h]; a.n = n_b[h];
        HIPCHK(c, launch_adam(a, s));
    }
    const double lr_d = muon_dec(lr);
    const float decay = (float)(1.0 - lr_d * muon_dec(m.weight_decay));
    for (int h = 0; h < 2; ++h) {  // W_dec (S, D), then W_enc (D, S)
        const long off = h == 0 ? c->off_W_dec : c->off_W_enc;
        const int trans = h == 0 ? 1 : 0;
        const double rows = h == 0 ? S : D, cols = h == 0 ? D : S;
        const double ratio = m.adjust_lr == 0 ? std::sqrt(std::max(1.0, rows / cols)) : m.adjust_lr == 1 ? 0.2 * std::sqrt(std::max(rows, cols)) : 1.0;
        MuonMomArgs mo{};
        mo.g = c->grads + off; mo.m = c->adam_m + off; mo.sumsq = saev_sumsq_device(c); mo.grad_scale = grad_scale; mo.max_norm = max_norm;
        mo.w_buf = (float)(1.0 - muon_dec(m.momentum)); mo.mu = m.momentum; mo.nesterov = m.nesterov ? 1 : 0; mo.trans = trans;
        mo.D = D; mo.S = S; mo.ldx = L.Sp; mo.X = reinterpret_cast<uint16_t*>(c->muon_ws + L.off_X[0]);
        mo.sq_part = reinterpret_cast<double*>(c->muon_ws + L.off_sq);
        HIPCHK(c, launch_muon_momentum(mo, s));
        hipError_t e = hipSuccess;
        const int cur = muon_newton_schulz(c->muon_ws, L, D, S, 1, m.ns_steps, m.a, m.b, m.c, m.eps, s, &e);
        if (cur < 0) HIPCHK(c, e);
        HIPCHK(c, launch_muon_apply(c->params + off, reinterpret_cast<const uint16_t*>(c->muon_ws + L.off_X[cur]), L.Sp, D, S, trans,
                                    decay, (float)(lr_d * ratio), s));
    }
    return SAEV_OK;
}

int saev_train_step(saev_ctx* c, const float* x, int32_t n, float lr, float max_norm, int64_t adam_step,
                    void* stream) {
    if (!c) return SAEV_INVALID_ARG;
    if (c->btk || c->relu_train) {  // the four phases back to back: nothing of the fused tail applies
        int rcb = saev_step_forward(c, x, n, n, 1, stream);
        if (rcb == SAEV_OK) rcb = saev_step_dead(c, n, stream);
        if (rcb == SAEV_OK) rcb = saev_step_backward(c, stream);
        if (rcb == SAEV_OK) rcb = saev_step_tail(c, lr, max_norm, 1.0f, adam_step, stream);
        return rcb;
    }
    c->fused_forward = c->dws_ok && c->GS != nullptr;  // (the backward below takes the column slices: nothing reads G's blocks 1..P-1)
    c->train_fused = true;
    int rc = saev_step_forward(c, x, n, n, 1, stream);
    c->fused_forward = false;
    if (rc != SAEV_OK) { c->train_fused = false; return rc; }
    rc = saev_step_dead(c, n, stream);
    if (rc != SAEV_OK) { c->train_fused = false; return rc; }
    // (no saev_backward_end: the W_enc gradient stays in the transposed scratch the backward writes; the tail's single Adam
    // launch reads it there through LDS tiles.  The W_enc segment of the gradient buffer is NOT updated by this entry point
    // -- callers that want to look at gradients use the phases)
    c->fused_step = true;
    rc = saev_backward_begin(c, stream);
    if (rc == SAEV_OK) rc = saev_backward_rows(c, 0, c->cfg.d_sae, stream);
    c->fused_step = false;
    if (rc != SAEV_OK) { c->train_fused = false; return rc; }
    c->wenc_t_pending = true;
    rc = saev_step_tail(c, lr, max_norm, 1.0f, adam_step, stream);
    c->wenc_t_pending = false;
    c->train_fused = false;
    return rc;
}

}  // extern "C"
