// The dense ReLU train step behind the C ABI (include/saev_amd.h: RELU TRAINING): its scratch, the forward and backward launch
// sequences, saev_copy_last_rows.  Kernels in relu_train.hip; the contractions run on the split-fp16 encoder kernel as the dense
// AuxK route's do (ctx_auxk.hip), here with "the dead set" = all latents, "the selection" = f > 0 and the target = x.
#include "ctx.h"

int relu_train_alloc(saev_ctx* c) {
    const size_t S = c->cfg.d_sae, D = c->cfg.d_model, MB = c->cfg.max_batch;
    const size_t S256 = (S + 255) / 256 * 256, D256 = (D + 255) / 256 * 256;
    c->rt_Sp = (int)((S + 31) / 32 * 32);
    int ns, Kp;
    ksplit_shape((int)S, (int)D, (int)MB, &ns, &Kp);  // (the slices depend on S and D alone; Kp grows with the rows)
    c->rt_kpad = Kp;
    int rc = SAEV_OK;
#define A(p, n) if (rc == SAEV_OK) rc = alloc(c, &c->p, (size_t)(n))
    A(rt_dA, MB * S);
    A(rt_parts, std::max(relu_act_parts((int)MB), relu_dact_parts((int)MB, (int)S)));
    A(rt_colpart, (size_t)relu_dact_row_blocks((int)MB) * S);
    A(rt_scales, 12);
    A(rt_xsF, (size_t)c->MB_pad * 2 * c->rt_Sp); A(rt_xsG, (size_t)c->MB_pad * 2 * c->Dp);
    A(rt_wsR, S256 * 2 * c->Dp); A(rt_wsK, D256 * 2 * c->rt_Sp);
    A(rt_kF, S256 * 2 * Kp); A(rt_kG, D256 * 2 * Kp); A(rt_kX, D256 * 2 * Kp);
    A(rt_wparts, ns > 1 ? (size_t)ns * S * D : 1);
#undef A
    if (rc != SAEV_OK) return rc;
    // (image rows past a matrix's last 64-column tile are never written: zeros, so that no padding row ever holds a NaN pattern)
    HIPCHK(c, hipMemset(c->rt_xsF, 0, (size_t)c->MB_pad * 2 * c->rt_Sp * sizeof(_Float16)));
    HIPCHK(c, hipMemset(c->rt_xsG, 0, (size_t)c->MB_pad * 2 * c->Dp * sizeof(_Float16)));
    HIPCHK(c, hipMemset(c->rt_wsR, 0, S256 * 2 * c->Dp * sizeof(_Float16)));
    HIPCHK(c, hipMemset(c->rt_wsK, 0, D256 * 2 * c->rt_Sp * sizeof(_Float16)));
    HIPCHK(c, hipMemset(c->rt_kF, 0, S256 * 2 * Kp * sizeof(_Float16)));
    HIPCHK(c, hipMemset(c->rt_kG, 0, D256 * 2 * Kp * sizeof(_Float16)));
    HIPCHK(c, hipMemset(c->rt_kX, 0, D256 * 2 * Kp * sizeof(_Float16)));
    return SAEV_OK;
}

namespace {

// out (n_rows x S_out) = rows-operand x cols-operand + bias: images xs (k = Kc) and ws (scaled by 256), xs's scale in scale_dev[0]
int rt_dense(saev_ctx* c, const _Float16* xs, const _Float16* ws, const float* bias, int n_rows, int Kc, int S_out, float* out,
             const float* scale_dev, hipStream_t s) {
    EncodeF16Args a{};
    a.scale_dev = scale_dev;
    a.xs = xs; a.ws = ws; a.b_enc = bias;
    a.n_rows = n_rows; a.Dp = Kc; a.S = S_out; a.w_scale = 256.0f; a.arith = 0;
    a.s_splits = encoder_splits(n_rows, S_out, encode_f16x3_tile_rows(), encode_f16x3_tile_latents(), 256);
    a.h_out = out;
    a.ngroups = 32;
    HIPCHK(c, launch_encode_f16x3(a, EPI_DENSE, s));
    return SAEV_OK;
}

// out (R x C) = the contraction over the batch of two k-major images (k padded to Kp, cut into n_split slices that run as one
// batched launch and are added in slice order): a weight gradient in its natural layout
int rt_ksplit(saev_ctx* c, const _Float16* imgP, const float* sP, int R, const _Float16* imgQ, const float* sQ, int C, int n_split,
              int Kp, float* out, hipStream_t s) {
    EncodeF16Args a{};
    a.scale_dev = sP; a.scale_dev_b = sQ;
    a.xs = imgP; a.ws = imgQ; a.b_enc = c->zero_bias;
    a.n_rows = R; a.Dp = Kp / n_split; a.S = C; a.w_scale = 1.0f; a.arith = 0;
    a.s_splits = encoder_splits(R, C, encode_f16x3_tile_rows(), encode_f16x3_tile_latents(), 256);
    a.ngroups = 32;
    a.n_batches = n_split; a.blk_imgs = Kp / 16; a.out_bstride = (long)R * C;
    a.h_out = n_split > 1 ? c->rt_wparts : out;
    HIPCHK(c, launch_encode_f16x3(a, EPI_DENSE, s));
    if (n_split > 1) HIPCHK(c, launch_sum_parts(c->rt_wparts, n_split, (long)R * C, out, s));
    return SAEV_OK;
}

}  // namespace

int relu_train_forward(saev_ctx* c, const float* x, int n, int64_t n_rows_global, int training, hipStream_t s) {
    REQUIRE(c, c->params, SAEV_NOT_BOUND, "parameters not bound");
    REQUIRE(c, x && n > 0 && n <= c->cfg.max_batch, SAEV_INVALID_ARG, "saev_step_forward: n_rows must be in 1..max_batch");
    REQUIRE(c, ((uintptr_t)x % 16) == 0, SAEV_INVALID_ARG, "x must be 16-byte aligned");
    REQUIRE(c, n_rows_global == n, SAEV_UNSUPPORTED, "saev_step_forward: a ReLU training context runs on one GPU (n_rows_global must equal n_rows)");
    const int S = c->cfg.d_sae, D = c->cfg.d_model;
    c->x_last = x;
    c->n_last = n;
    c->training_last = training;
    c->P_last = 1;
    c->aux_route = AUX_NONE;
    c->stats_pending = false;
    c->rt_fwd_live = false;
    // (nothing is shared with another context: what the encoder derives from x is this context's own)
    c->upper_c = c->upper; c->mu_c = c->mu; c->xnorm_c = c->xnorm; c->xabs_c = c->xabs_part; c->xs_c = c->xs;
    c->xprep_x = nullptr;
    hipEvent_t wdec_ev = c->wdec_ready;
    c->wdec_ready = nullptr;
    HIPCHK(c, launch_step_zero(c->stats, c->upper, c->flags, s));
    HIPCHK(c, launch_absmax(x, (long)n * D, c->upper, s));
    int rc = encode_dense_h(c, x, n, s);
    if (rc != SAEV_OK) return rc;
    float* f = c->h_dense;
    HIPCHK(c, launch_relu_act(f, n, S, training ? 1 : 0, c->fired, c->rowstats, c->rt_parts, c->rt_scales, s));
    if (wdec_ev != nullptr) HIPCHK(c, hipStreamWaitEvent(s, wdec_ev, 0));
    if (training && c->cfg.normalize_w_dec) HIPCHK(c, launch_normalize_rows(c->params + c->off_W_dec, S, D, s));
    int ns, Kp;
    ksplit_shape(S, D, n, &ns, &Kp);
    // W_dec in both operand forms from one pass (rows = latents: dA; rows = its d_model columns: x_hat), f likewise (row operand:
    // x_hat; k-major: dW_dec)
    HIPCHK(c, launch_split_both(c->params + c->off_W_dec, S, D, 256.0f, nullptr, c->rt_wsR, c->Dp, c->rt_wsK, c->rt_Sp, s));
    HIPCHK(c, launch_split_both(f, n, S, 1.0f, c->rt_scales, c->rt_xsF, c->rt_Sp, training ? c->rt_kF : nullptr, Kp, s));
    rc = rt_dense(c, c->rt_xsF, c->rt_wsK, c->params + c->off_b_dec, n, c->rt_Sp, D, c->x_hat, c->rt_scales, s);
    if (rc != SAEV_OK) return rc;
    HIPCHK(c, launch_relu_mse(x, c->x_hat, n, D, c->upper, 2.0f / ((float)n * (float)D), c->g, c->rowstats, c->rt_parts, c->rt_scales + 2, s));
    HIPCHK(c, launch_stats_reduce(c->rowstats, n, D, 1, c->cfg.alpha, 0, c->upper, nullptr, c->stats, s, nullptr, c->stats_scratch));
    c->rt_fwd_live = training != 0;
    return SAEV_OK;
}

int relu_train_backward(saev_ctx* c, hipStream_t s) {
    REQUIRE(c, c->x_last && c->training_last, SAEV_INVALID_ARG, "saev_step_backward: no training forward in flight");
    REQUIRE(c, c->grads, SAEV_NOT_BOUND, "gradient buffer not bound");
    // (the backward writes dH over dA and dH's k-major images over f's: it runs once per training forward)
    REQUIRE(c, c->rt_fwd_live, SAEV_INVALID_ARG, "saev_step_backward: this forward's backward has run already (a ReLU training context keeps "
            "f's operand images only until then: repeat saev_step_forward)");
    c->rt_fwd_live = false;
    const int S = c->cfg.d_sae, D = c->cfg.d_model, n = c->n_last;
    const float* f = c->h_dense;
    int ns, Kp;
    ksplit_shape(S, D, n, &ns, &Kp);
    c->row_proj_valid = false;
    c->wenc_sq_valid = false;
    HIPCHK(c, launch_colsum(c->g, n, D, c->colsum_partials, c->grads + c->off_b_dec, 0, nullptr, s));
    // dA = g W_dec^T (g as a row operand; k-major for dW_dec from the same pass)
    HIPCHK(c, launch_split_both(c->g, n, D, 1.0f, c->rt_scales + 2, c->rt_xsG, c->Dp, c->rt_kG, Kp, s));
    int rc = rt_dense(c, c->rt_xsG, c->rt_wsR, c->zero_bias, n, c->Dp, S, c->rt_dA, c->rt_scales + 2, s);
    if (rc != SAEV_OK) return rc;
    // dH in place, db_enc, the scale of dH's images
    HIPCHK(c, launch_relu_dact(c->rt_dA, f, n, S, (float)(c->rt_l1 / (double)n), c->rt_colpart, c->grads + c->off_b_enc, c->rt_parts,
                               c->rt_scales + 4, s));
    // dW_dec = f^T g, straight into the gradient buffer
    rc = rt_ksplit(c, c->rt_kF, c->rt_scales, S, c->rt_kG, c->rt_scales + 2, D, ns, Kp, c->grads + c->off_W_dec, s);
    if (rc != SAEV_OK) return rc;
    // dW_enc = x^T dH (f's k-major images are done: dH's take their place)
    HIPCHK(c, launch_pow2_scale(c->upper, c->rt_scales + 6, s));
    HIPCHK(c, launch_split_both(c->x_last, n, D, 1.0f, c->rt_scales + 6, nullptr, 0, c->rt_kX, Kp, s));
    HIPCHK(c, launch_split_both(c->rt_dA, n, S, 1.0f, c->rt_scales + 4, nullptr, 0, c->rt_kF, Kp, s));
    return rt_ksplit(c, c->rt_kX, c->rt_scales + 6, D, c->rt_kF, c->rt_scales + 4, S, ns, Kp, c->grads + c->off_W_enc, s);
}

extern "C" {

int saev_copy_last_rows(saev_ctx* c, int32_t n_rows, int32_t row_cap, int32_t* row_nnz_out, int32_t* idx_out, float* val_out,
                        int32_t* overflow_out, void* stream) {
    if (!c) return SAEV_INVALID_ARG;
    REQUIRE(c, c->relu_train, SAEV_UNSUPPORTED, "saev_copy_last_rows: the context is not a ReLU training context");
    REQUIRE(c, c->n_last > 0 && n_rows == c->n_last, SAEV_INVALID_ARG,
            "saev_copy_last_rows: n_rows differs from the batch of the last forward (or none has run)");
    REQUIRE(c, row_nnz_out && idx_out && val_out && overflow_out && row_cap > 0, SAEV_INVALID_ARG, "saev_copy_last_rows: bad arguments");
    BtkCompactArgs a{};
    a.h = c->h_dense; a.n_rows = n_rows; a.S = c->cfg.d_sae; a.row_cap = row_cap; a.training = 0;
    a.threshold = c->zero_bias;  // (a zero word: the compaction keeps f > 0)
    a.idx_out = idx_out; a.val_out = val_out; a.row_nnz_out = row_nnz_out; a.overflow = overflow_out;
    HIPCHK(c, launch_threshold_compact(a, (hipStream_t)stream));
    return SAEV_OK;
}

}  // extern "C"
