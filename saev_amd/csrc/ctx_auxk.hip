// The auxiliary (AuxK) loss behind the C ABI: its dead-set buffers, its forward and backward launch sequences, saev_step_dead.
#include "ctx.h"

int alloc_aux_buffers(saev_ctx* c, int cap) {
    const size_t MB = c->cfg.max_batch, D = c->cfg.d_model;
    const size_t capA = std::max(cap, AUX_SMALL_MAX);  // the few-dead-latents kernels use AUX_SMALL_MAX columns / rows
    auto grab = [&](size_t bytes) -> void* {
        void* q = nullptr;
        if (hipMalloc(&q, bytes) != hipSuccess) return nullptr;
        c->aux_allocs.push_back(q);
        c->aux_bytes += bytes;
        return q;
    };
    c->Wenc_dead = (float*)grab(D * capA * 4);
    c->Wdec_dead = (float*)grab(capA * D * 4);
    c->H_dead = (float*)grab(MB * capA * 4);
    c->A_dead = (float*)grab(MB * capA * 4);
    c->A_mask = (uint8_t*)grab(MB * capA);
    c->dWd = (float*)grab(capA * D * 4);
    c->dWe = (float*)grab(capA * D * 4);
    c->dbe = (float*)grab(capA * 4);
    c->aux_partials = (float*)grab(((MB + 63) / 64) * capA * 4);
    // (the matrix-core kernels take dead sets up to AUX_MFMA_MAX where the compact buffers hold that many rows and the step's
    // backward runs over this context's own rows: gathered backwards -- max_backward_rows -- keep the round-5 limit)
    const size_t mcap = (aux_mfma_supported((int)D) && capA >= (size_t)AUX_MFMA_MAX && c->cfg.max_backward_rows == 0 && c->dbg.aux_wide_route == 0)
                            ? (size_t)AUX_MFMA_MAX : (size_t)AUX_SMALL_MAX;
    c->aux_mfma_cap = (int)mcap;
    c->WencT_dead = (float*)grab(mcap * D * 4);
    c->aux_small_part = (float*)grab(((MB + 63) / 64) * (size_t)2 * mcap * D * 4);
    c->aux_small_part2 = (float*)grab((size_t)(((MB + 63) / 64 + 63) / 64) * mcap * D * 4);
    c->aux_small_partbe = (float*)grab((size_t)((MB + 63) / 64) * mcap * 4);  // (aux_mfma_wgrad_kernel: the blocks' column sums of dA)
    bool fast_ok = true;
    {  // operand images of the five contractions (every encoder mode runs them on the split-fp16 MFMA kernel)
        const size_t cap256 = ((size_t)cap + 255) / 256 * 256, D256 = (D + 255) / 256 * 256;
        c->aux_Dp2 = (int)(((size_t)cap + 31) / 32 * 32);
        c->aux_ws1 = (_Float16*)grab(cap256 * 2 * c->Dp * sizeof(_Float16));          // W_enc[:, dl]^T, later W_dec[dl]
        c->aux_ws2 = (_Float16*)grab(D256 * 2 * c->aux_Dp2 * sizeof(_Float16));        // W_dec[dl] as a (n_dead x D) "encoder"
        c->aux_xsA = (_Float16*)grab((size_t)c->MB_pad * 2 * c->aux_Dp2 * sizeof(_Float16));
        c->aux_xsg = (_Float16*)grab((size_t)c->MB_pad * 2 * c->Dp * sizeof(_Float16));
        c->bias_dead = (float*)grab(cap256 * sizeof(float));
        // weight gradients: contraction over the batch axis, split into AUX_KSPLIT_MAX slices at most
        c->aux_kpad = (int)((MB + 16 * AUX_KSPLIT_MAX - 1) / (16 * AUX_KSPLIT_MAX) * (16 * AUX_KSPLIT_MAX));
        c->aux_kA = (_Float16*)grab(cap256 * 2 * (size_t)c->aux_kpad * sizeof(_Float16));   // A^T, later dA^T
        c->aux_kD = (_Float16*)grab(D256 * 2 * (size_t)c->aux_kpad * sizeof(_Float16));     // g_aux^T, later x^T
        c->aux_kX = (_Float16*)grab(D256 * 2 * (size_t)c->aux_kpad * sizeof(_Float16));     // x^T when the forward writes both forms of x at once (split_both_kernel)
        c->aux_parts = (float*)grab((size_t)AUX_KSPLIT_MAX * cap * D * sizeof(float));
        fast_ok = c->aux_ws1 && c->aux_ws2 && c->aux_xsA && c->aux_xsg && c->bias_dead && c->aux_kA && c->aux_kD && c->aux_kX && c->aux_parts;
    }
    if (!fast_ok || !c->Wenc_dead || !c->Wdec_dead || !c->H_dead || !c->A_dead || !c->A_mask || !c->dWd || !c->dWe || !c->dbe ||
        !c->aux_partials || !c->WencT_dead || !c->aux_small_part || !c->aux_small_part2) {
        c->err = "AuxK: out of device memory for the dead-set buffers (lower saev_cfg.aux_dead_cap)";
        return SAEV_HIP_ERROR;
    }
    c->nd_cap = cap;
    return SAEV_OK;
}

namespace {

// out (n_rows x S_out, row-major) = rows-operand x cols-operand + bias on the f16x3 encoder kernel (dense epilogue):
// the three AuxK contractions whose long axis is the batch are exactly the encoder's shape.  `scale` is the product
// of the power-of-two scales applied to the two operands when they were split.
int dense_f16x3(saev_ctx* c, const _Float16* xs, const _Float16* ws, const float* bias, int n_rows, int Dp, int S_out,
                float scale, float* out, hipStream_t s, const float* scale_dev = nullptr) {
    EncodeF16Args a{};
    a.scale_dev = scale_dev;
    a.xs = xs; a.ws = ws; a.b_enc = bias;
    a.n_rows = n_rows; a.Dp = Dp; a.S = S_out; a.w_scale = scale; a.arith = 0;
    a.s_splits = encoder_splits(n_rows, S_out, encode_f16x3_tile_rows(), encode_f16x3_tile_latents(), 256);
    a.h_out = out;
    a.ngroups = 32;
    a.enable_flag = nullptr; a.enable_when = 0;
    HIPCHK(c, launch_encode_f16x3(a, EPI_DENSE, s));
    return SAEV_OK;
}

// out (R x C) = sum over the long axis k (length K <= aux_kpad) of P[k][r] * Q[k][c] for two k-major fp32 matrices
// P (K x R), Q (K x C): the AuxK weight gradients.  Both are split into hi/lo fp16 images of their transposes
// (split_wT), the contraction is cut into n_split slices that run as one batched launch of the encoder kernel (a single
// slice would leave most CUs idle: R x C is only a few tiles), and the slices are added in a fixed order.
// (ksplit_shape -- ctx.h -- gives the slices and the padded length, <= aux_kpad)
// imgP / imgQ: the operand's k-major images if somebody has written them already (split_both_kernel, with THIS Kp), else NULL
int ksplit_f16x3(saev_ctx* c, const float* P, const float* sP, int R, const float* Q, const float* sQ, int C, int K,
                 float* out, hipStream_t s, const _Float16* imgP = nullptr, const _Float16* imgQ = nullptr) {
    const int R256 = (R + 255) / 256 * 256, C256 = (C + 255) / 256 * 256;
    int n_split, Kp;
    ksplit_shape(R, C, K, &n_split, &Kp);
    if (imgP == nullptr) { HIPCHK(c, launch_split_wT(P, K, R, R256, Kp, 1.0f, c->aux_kA, 0, s, sP)); imgP = c->aux_kA; }
    if (imgQ == nullptr) { HIPCHK(c, launch_split_wT(Q, K, C, C256, Kp, 1.0f, c->aux_kD, 0, s, sQ)); imgQ = c->aux_kD; }
    EncodeF16Args a{};
    a.scale_dev = sP; a.scale_dev_b = sQ;  // (the two operands' scales where their producers left them)
    a.xs = imgP; a.ws = imgQ; a.b_enc = c->zero_bias;
    a.n_rows = R; a.Dp = Kp / n_split; a.S = C; a.w_scale = 1.0f; a.arith = 0;
    a.s_splits = encoder_splits(R, C, encode_f16x3_tile_rows(), encode_f16x3_tile_latents(), 256);
    a.ngroups = 32;
    a.n_batches = n_split; a.blk_imgs = Kp / 16; a.out_bstride = (long)R * C;
    a.h_out = n_split > 1 ? c->aux_parts : out;
    HIPCHK(c, launch_encode_f16x3(a, EPI_DENSE, s));
    if (n_split > 1) HIPCHK(c, launch_sum_parts(c->aux_parts, n_split, (long)R * C, out, s));
    return SAEV_OK;
}

// A handful of dead latents, all of them selected (n_dead <= min(AUX_SMALL_MAX, k_aux)): one row-wise pass instead of the
// dense algebra.  Every kernel takes the count from the device (flags[4]) and exits when it is zero, so this sequence is
// what a step enqueues when the host only knows a bound of the count.
int auxk_small_forward(saev_ctx* c, hipStream_t s, int bound) {
    const int S = c->cfg.d_sae, D = c->cfg.d_model, n = c->n_last;
    const int32_t* nd_dev = c->flags + 4;
    c->aux_small = true;
    c->aux_all = false;
    c->aux_fused = false;
    c->aux_mfma = false;
    if (!c->dead_list_ready) HIPCHK(c, launch_dead_compact(c->dead, S, c->dead_list, s, nd_dev));
    c->aux_ndp = bound > AUX_SMALL_MAX ? AUX_MFMA_MAX : AUX_SMALL_MAX;
    HIPCHK(c, launch_gather_dead_small(c->params + c->off_W_enc, c->params + c->off_W_dec, c->dead_list, nd_dev, D, S,
                                       c->WencT_dead, c->Wdec_dead, s, c->aux_ndp));
    if (bound <= AUX_FUSED_MAX && aux_fused_supported(D) && c->dbg.aux_small_max != AUX_SMALL_MAX) {
        // a handful of dead latents: one pass over x and x_hat leaves the block partials of every gradient of the auxiliary term
        // (partials in the buffers the two-kernel form uses for its own: aux_small_part; g_aux and A_dead are free in this form)
        c->aux_fused = true;
        HIPCHK(c, launch_aux_small_fused(c->x_last, c->x_hat, c->WencT_dead, c->Wdec_dead, c->params + c->off_b_enc,
                                         c->params + c->off_b_dec, c->dead_list, n, D, nd_dev,
                                         c->cfg.alpha * 2.0f / ((float)n * (float)D), c->aux_small_part, c->g_aux, c->A_dead, c->rowstats, s, bound));
        // (inside saev_train_step the backward's ordered-sum launch also forms the step's auxiliary loss: aux_stats_pending)
        c->aux_stats_pending = c->train_fused;
        if (!c->aux_stats_pending)
            HIPCHK(c, launch_stats_reduce(c->rowstats, n, D, c->P_last, c->cfg.alpha, 2, c->upper_c, nullptr, c->stats, s, nd_dev, c->stats_scratch));
        return SAEV_OK;
    }
    if (bound <= c->aux_mfma_cap && aux_mfma_supported(D) && c->dbg.aux_small_route == 0) {
        c->aux_mfma = true;
        HIPCHK(c, launch_aux_mfma_forward(c->x_last, c->x_hat, c->WencT_dead, c->Wdec_dead, c->params + c->off_b_enc,
                                          c->params + c->off_b_dec, c->dead_list, n, D, nd_dev,
                                          c->cfg.alpha * 2.0f / ((float)n * (float)D), c->A_dead, c->H_dead, c->g_aux, c->rowstats, s, bound, c->aux_ndp));
        c->aux_mfma_bound = bound;
        // (inside saev_train_step the backward's ordered-sum launch also forms the step's auxiliary loss, as for the one-pass kernel)
        c->aux_stats_pending = c->train_fused;
        if (c->aux_stats_pending) return SAEV_OK;
    } else
    HIPCHK(c, launch_aux_small_fwd(c->x_last, c->x_hat, c->WencT_dead, c->Wdec_dead, c->params + c->off_b_enc,
                                   c->params + c->off_b_dec, c->dead_list, n, D, nd_dev,
                                   c->cfg.alpha * 2.0f / ((float)n * (float)D), c->A_dead, c->H_dead, c->g_aux, c->rowstats, s));
    HIPCHK(c, launch_stats_reduce(c->rowstats, n, D, c->P_last, c->cfg.alpha, 2, c->upper_c, nullptr, c->stats, s, nd_dev, c->stats_scratch));
    return SAEV_OK;
}

// forward of the auxiliary loss as dense algebra over n_dead_host dead latents (see auxk.hip)
int auxk_forward(saev_ctx* c, hipStream_t s) {
    const int S = c->cfg.d_sae, D = c->cfg.d_model, n = c->n_last;
    const int nd = c->n_dead_host, ku = c->k_use_host;
    const int ndp = (nd + 3) / 4 * 4;
    REQUIRE(c, ndp <= c->nd_cap, SAEV_UNSUPPORTED, "AuxK: more dead latents than the dense buffers hold (raise saev_cfg.aux_dead_cap)");
    int rc = SAEV_OK;
    // Every encoder mode runs the five contractions on the split-fp16 MFMA kernel (three products per fp32 product:
    // fp32-accurate, gemm_encode_f16x3.hip), whatever arithmetic its own encoder uses: the auxiliary loss is defined on
    // the exact pre-activations (the bf16 mode's oracle does the same).  Only the f16x3 mode already has hi/lo x images.
    const bool own_images = c->cfg.encoder_mode != SAEV_ENCODER_F16X3;
    const int ndp256 = (ndp + 255) / 256 * 256, Dp2 = (ndp + 31) / 32 * 32;
    // Operand images in both forms from one pass over their source (split.hip: split_both_kernel): six image launches instead of
    // ten, bit-identical images (saev_debug_cfg.aux_split_route = 1 keeps the ten)
    c->aux_both = own_images && c->dbg.aux_split_route == 0 && D % 4 == 0;
    // aux_dev_count: nd / ku are upper bounds (the tracker record of a few steps ago, saev_step_dead); the true count and
    // min(k_aux, count) are flags[4] / flags[5].  Columns of the dead set past the true count are padding -- zero weights,
    // bias -inf (never selected) or 0 (all-selected mode) -- exactly like the columns that pad nd to a multiple of four,
    // so every product below has its usual shape and nothing is read back.
    const int32_t* nd_dev = c->aux_dev_count ? c->flags + 4 : nullptr;
    const int32_t* ku_dev = c->aux_dev_count ? c->flags + 5 : nullptr;
    if (!c->dead_list_ready) HIPCHK(c, launch_dead_compact(c->dead, S, c->dead_list, s));
    HIPCHK(c, launch_gather_dead(c->params + c->off_W_enc, c->params + c->off_W_dec, c->dead_list, nd, ndp, D, S,
                                 c->Wenc_dead, c->Wdec_dead, s, nd_dev));
    c->aux_small = false;
    c->aux_all = false;
    // n_dead <= k_aux: every dead latent is selected, the codes are H itself (padding columns zero) and there is no mask
    c->aux_all = ku == nd;
    {
        // H = x W_enc[:, dl] + b_enc[dl]: in f16x3 mode the x images of this step are already there (prepare_encoder)
        HIPCHK(c, launch_split_wT(c->Wenc_dead, D, ndp, ndp256, c->Dp, 256.0f, c->aux_ws1, 0, s));
        HIPCHK(c, launch_dead_bias_vec(c->params + c->off_b_enc, c->dead_list, nd, ndp, c->bias_dead, s, c->aux_all, nd_dev));
        const _Float16* xs_hl = c->xs_c;
        if (own_images) {  // the step's x images are single fp16 / bf16 or absent: make the hi/lo ones (the buffer is free until the backward)
            // (with the step's power-of-two x scale, so that no activation magnitude can overflow fp16)
            HIPCHK(c, launch_pow2_scale(c->upper_c, c->aux_scales + 6, s));  // from max|x| of the step (uncentred here)
            if (c->aux_both) {  // ... and its k-major images for the backward's dWe, from the same pass over x
                int ns, Kp;
                ksplit_shape(ndp, D, n, &ns, &Kp);
                HIPCHK(c, launch_split_both(c->x_last, n, D, 1.0f, c->aux_scales + 6, c->aux_xsg, c->Dp, c->aux_kX, Kp, s));
            } else
            HIPCHK(c, launch_split_rows(c->x_last, n, D, c->Dp, c->aux_xsg, 0, s, 1.0f, c->aux_scales + 6));
            xs_hl = c->aux_xsg;
        }
        rc = dense_f16x3(c, xs_hl, c->aux_ws1, c->bias_dead, n, c->Dp, ndp, 256.0f, c->aux_all ? c->A_dead : c->H_dead, s,
                         own_images ? c->aux_scales + 6 : nullptr);
        if (rc != SAEV_OK) return rc;
    }
    const bool fused_select = aux_select_supported(ndp) && c->dbg.aux_dense_route == 0;  // (1: the round-4 select / fill / scatter sequence)
    if (!c->aux_all) {
        SelectDenseArgs sd{};
        sd.h = c->H_dead; sd.n_rows = n; sd.S = ndp; sd.k = ku; sd.k_dev = ku_dev;
        sd.idx_out = c->aux_idx; sd.val_out = c->aux_val; sd.out_stride = c->cfg.k_aux;
        if (fused_select) {
            // codes, mask, max |code| and the codes' operand scale in one launch (auxk.hip: aux_select_kernel)
            HIPCHK(c, launch_aux_select(c->H_dead, n, ndp, ku, ku_dev, c->A_dead, c->A_mask, c->aux_sync, c->aux_scales + 2, s));
        } else {
            HIPCHK(c, launch_select_dense(sd, s));
            HIPCHK(c, hipMemsetAsync(c->A_dead, 0, (size_t)n * ndp * sizeof(float), s));
            HIPCHK(c, hipMemsetAsync(c->A_mask, 0, (size_t)n * ndp, s));
            HIPCHK(c, launch_aux_scatter(c->aux_idx, c->aux_val, n, ku, c->cfg.k_aux, ndp, c->A_dead, c->A_mask, s, ku_dev));
        }
    }
    {
        // E = A W_dec[dl]: rows = batch, contraction over the dead set, "latents" = the d_model outputs
        // (the codes are pre-activations of unknown magnitude: power-of-two scale from their device-side max)
        if (c->aux_all || !fused_select) HIPCHK(c, launch_absmax_pow2(c->A_dead, (long)n * ndp, c->aux_sync, c->aux_scales + 2, s));
        if (c->aux_both) {
            int ns, Kp;
            ksplit_shape(ndp, D, n, &ns, &Kp);
            // the codes as a row operand (E) and k-major (dWd); the dead latents' decoder rows k-major (E) and as a row operand (dA:
            // aux_ws1 is free again, H is done)
            HIPCHK(c, launch_split_both(c->A_dead, n, ndp, 1.0f, c->aux_scales + 2, c->aux_xsA, Dp2, c->aux_kA, Kp, s));
            HIPCHK(c, launch_split_both(c->Wdec_dead, ndp, D, 256.0f, nullptr, c->aux_ws1, c->Dp, c->aux_ws2, Dp2, s));
        } else {
        HIPCHK(c, launch_split_rows(c->A_dead, n, ndp, Dp2, c->aux_xsA, 0, s, 1.0f, c->aux_scales + 2));
        HIPCHK(c, launch_split_wT(c->Wdec_dead, ndp, D, (D + 255) / 256 * 256, Dp2, 256.0f, c->aux_ws2, 0, s));
        }
        rc = dense_f16x3(c, c->aux_xsA, c->aux_ws2, c->zero_bias, n, Dp2, D, 256.0f, c->g_aux, s, c->aux_scales + 2);
    }
    if (rc != SAEV_OK) return rc;
    // (g_aux leaves with its max and the operand scale the backward splits it with: aux_scales + 4)
    HIPCHK(c, launch_aux_resid(c->g_aux, c->x_last, c->x_hat, c->params + c->off_b_dec, n, D,
                               c->cfg.alpha * 2.0f / ((float)n * (float)D), c->rowstats, s, nd_dev, c->aux_sync, c->aux_scales + 4));
    HIPCHK(c, launch_stats_reduce(c->rowstats, n, D, c->P_last, c->cfg.alpha, 1, c->upper_c, nullptr, c->stats, s, nullptr,
                                  c->stats_scratch));
    return SAEV_OK;
}

}  // namespace

// gradients of the auxiliary loss, accumulated into the gradient buffer / the transposed W_enc scratch
int auxk_backward(saev_ctx* c, hipStream_t s) {
    const int D = c->cfg.d_model, n = c->n_last;
    const int nd = c->n_dead_host;
    const int ndp = (nd + 3) / 4 * 4;
    float* dA = c->H_dead;  // H is dead after the select
    int rc;
    if (c->aux_small) {  // dA is there already (auxk_small_forward); weight gradients block-wise, then two column sums;
                         // all predicated on the device-side count like the forward (rows past it are never scattered)
        const int nb = (n + 63) / 64, L = AUX_SMALL_MAX;
        const int32_t* nd_dev = c->flags + 4;
        if (c->aux_fused) {  // the forward has left block partials of all four gradients: one launch of ordered sums finishes them
            const int blocks = aux_fused_blocks(n);
            // (the dead count may be zero on the device: db_aux must then read as zeros, and b_dec's gradient stay untouched -- the
            // kernel leaves at once in that case, hence the memset)
            if (c->ov_x != nullptr) HIPCHK(c, hipMemsetAsync(c->db_aux, 0, (size_t)D * sizeof(float), s));
            HIPCHK(c, launch_aux_fused_wsum(c->aux_small_part, blocks, D, nd_dev, c->dWd, c->dWe, s, c->g_aux,
                                            c->ov_x != nullptr ? c->db_aux : c->grads + c->off_b_dec, c->ov_x != nullptr ? 0 : 1, c->A_dead, c->dbe,
                                            c->aux_stats_pending ? c->rowstats : nullptr, n, c->cfg.alpha, c->stats));
            c->aux_stats_pending = false;
            return SAEV_OK;
        }
        if (c->aux_mfma) {
            // weight-gradient partials per block of 64 rows with the blocks' column sums of g_aux and dA riding along; ONE launch of
            // ordered sums finishes all four gradients (and the auxiliary loss inside saev_train_step)
            HIPCHK(c, launch_aux_mfma_wgrad(c->A_dead, dA, c->g_aux, c->x_last, n, D, nd_dev, c->aux_small_part, c->aux_small_part2,
                                            c->aux_small_partbe, s, c->aux_mfma_bound, c->aux_ndp));
            if (c->ov_x != nullptr) HIPCHK(c, hipMemsetAsync(c->db_aux, 0, (size_t)D * sizeof(float), s));  // (the count may be zero on the device)
            HIPCHK(c, launch_aux_fused_wsum(c->aux_small_part, nb, D, nd_dev, c->dWd, c->dWe, s, c->aux_small_part2,
                                            c->ov_x != nullptr ? c->db_aux : c->grads + c->off_b_dec, c->ov_x != nullptr ? 0 : 1, c->aux_small_partbe, c->dbe,
                                            c->aux_stats_pending ? c->rowstats : nullptr, n, c->cfg.alpha, c->stats, c->aux_ndp));
            c->aux_stats_pending = false;
            return SAEV_OK;
        }
        HIPCHK(c, launch_aux_small_wgrad(c->A_dead, dA, c->g_aux, c->x_last, n, D, nd_dev, c->aux_small_part, s));
        HIPCHK(c, launch_aux_small_wsum(c->aux_small_part, nb, D, nd_dev, c->dWd, c->dWe, s));
        HIPCHK(c, launch_colsum(dA, n, L, c->aux_partials, c->dbe, 0, nd_dev, s, 0, 1.0f, 1));
        if (c->ov_x != nullptr) {  // gathered backward: the local share travels with the compact rows (saev_aux_compact_export)
            HIPCHK(c, hipMemsetAsync(c->db_aux, 0, (size_t)D * sizeof(float), s));  // (the count may be zero on the device)
            HIPCHK(c, launch_colsum(c->g_aux, n, D, c->colsum_partials, c->db_aux, 0, nd_dev, s));
        } else {
            HIPCHK(c, launch_colsum(c->g_aux, n, D, c->colsum_partials, c->grads + c->off_b_dec, 1, nd_dev, s));
        }
        return SAEV_OK;
    }
    {
        // dA = g_aux W_dec[dl]^T.  g_aux carries the factor alpha * 2 / (n D) (~1e-10) times a residual of unknown
        // magnitude: bring it to [2^13, 2^14) with an exact power of two from its device-side max before the fp16 split;
        // W_dec[dl] rows are already "latent-major", so they split like x.
        // (the scale from g_aux's device-side max: aux_resid_kernel left it at aux_scales + 4)
        if (c->aux_both) {  // g_aux in both forms (dA here, dWd below); the decoder rows' row-form images are the forward's
            int ns, Kp;
            ksplit_shape(ndp, D, n, &ns, &Kp);
            HIPCHK(c, launch_split_both(c->g_aux, n, D, 1.0f, c->aux_scales + 4, c->aux_xsg, c->Dp, c->aux_kD, Kp, s));
        } else {
        HIPCHK(c, launch_split_rows(c->g_aux, n, D, c->Dp, c->aux_xsg, 0, s, 1.0f, c->aux_scales + 4));
        HIPCHK(c, launch_split_rows(c->Wdec_dead, ndp, D, c->Dp, c->aux_ws1, 0, s, 256.0f));
        }
        rc = dense_f16x3(c, c->aux_xsg, c->aux_ws1, c->zero_bias, n, c->Dp, ndp, 256.0f, dA, s, c->aux_scales + 4);
    }
    if (rc != SAEV_OK) return rc;
    // the selection's mask applied, max |dA| and dA's operand scale (aux_scales + 10) in one pass
    if (!c->aux_all) HIPCHK(c, launch_mask_apply_absmax(dA, c->A_mask, (long)n * ndp, c->aux_sync, c->aux_scales + 10, s));
    else HIPCHK(c, launch_absmax_pow2(dA, (long)n * ndp, c->aux_sync, c->aux_scales + 10, s));
    {
        // operand scales: A from the forward (aux_scales + 2), g_aux from above (+ 4), x from max|x| (+ 6), dA fresh
        rc = ksplit_f16x3(c, c->A_dead, c->aux_scales + 2, ndp, c->g_aux, c->aux_scales + 4, D, n, c->dWd, s,
                          c->aux_both ? c->aux_kA : nullptr, c->aux_both ? c->aux_kD : nullptr);
        if (rc != SAEV_OK) return rc;
        // (x's scale: the forward formed it when it made its own hi/lo images of x)
        if (c->cfg.encoder_mode == SAEV_ENCODER_F16X3) HIPCHK(c, launch_pow2_scale(c->upper_c, c->aux_scales + 6, s));
        rc = ksplit_f16x3(c, dA, c->aux_scales + 10, ndp, c->x_last, c->aux_scales + 6, D, n, c->dWe, s, nullptr,
                          c->aux_both ? c->aux_kX : nullptr);
        if (rc != SAEV_OK) return rc;
    }
    HIPCHK(c, launch_colsum(dA, n, ndp, c->aux_partials, c->dbe, 0, nullptr, s));
    HIPCHK(c, launch_colsum(c->g_aux, n, D, c->colsum_partials, c->ov_x != nullptr ? c->db_aux : c->grads + c->off_b_dec,
                            c->ov_x != nullptr ? 0 : 1, nullptr, s));
    // the compact rows dWd / dWe / dbe are added into the gradient rows of the dead latents by saev_backward_rows
    return SAEV_OK;
}

extern "C" {

int saev_step_dead(saev_ctx* c, int64_t n_rows_global, void* stream) {
    if (!c) return SAEV_INVALID_ARG;
    REQUIRE(c, c->x_last && c->training_last, SAEV_INVALID_ARG, "saev_step_dead: no training forward in flight");
    hipStream_t s = (hipStream_t)stream;
    const int S = c->cfg.d_sae;
    const int64_t step = ++c->dead_steps;
    c->tokens_seen += n_rows_global;
    DeadArgs d{};
    d.toks = c->toks; d.fired = c->fired; d.dead = c->dead; d.S = S;
    d.add_tokens = n_rows_global; d.threshold = c->cfg.dead_threshold_tokens; d.k_aux = c->cfg.k_aux;
    d.n_dead = c->flags + 4; d.k_use = c->flags + 5; d.stats = c->stats; d.scratch = c->flags + 6;
    // (how many steps old the record is that sizes this step's auxiliary work: a shorter lag gives a tighter bound of the dead
    // count, a longer one lets the host run further ahead of the device)
    d.horizon_tokens = (int64_t)DEAD_LAG * n_rows_global;
    d.step = step; d.cum_tokens = c->tokens_seen;
    d.rec = c->rec_dev ? c->rec_dev + step % DEAD_RING : nullptr;
    c->dead_list_ready = false;
    if (c->stats_pending) {
        c->stats_pending = false;
        d.dead_list = c->cfg.k_aux > 0 ? c->dead_list : nullptr;
        RhoArgs rho{};  // (a step of the norm-predicted bounds: this launch reduces its ratios and steers the safety factor)
        if (c->rho_step != 0) {
            rho.kth = c->kth_val; rho.xnorm = c->xnorm; rho.state = c->rho_state; rho.flags = c->flags; rho.scratch = c->rho_scratch;
            rho.k = c->cfg.top_k; rho.host = c->stale_dev != nullptr ? c->stale_dev + 4 : nullptr;
        }
        HIPCHK(c, launch_stats_dead(c->rowstats, c->n_last, c->cfg.d_model, c->P_last, c->cfg.alpha, c->upper_c, c->flags + 2, c->stats,
                                    c->stats_scratch, c->stats_lists ? c->cand_cnt : nullptr, CAND_CAP, d, s, c->rho_step != 0 ? &rho : nullptr));
        c->dead_list_ready = d.dead_list != nullptr;
    } else {
        HIPCHK(c, launch_dead_update(d, s));
    }
    c->n_dead_host = 0;
    c->k_use_host = 0;
    c->aux_route = AUX_NONE;
    c->aux_small = false;
    c->aux_dev_count = false;
    if (c->cfg.k_aux <= 0) return SAEV_OK;
    HIPCHK(c, hipEventRecord(c->dead_ev[step % DEAD_RING], s));
    // A latent can only be dead once `threshold` tokens went by since the tracker was last known to be all-zero.
    if (!c->tracker_dirty && c->tokens_seen < c->cfg.dead_threshold_tokens) return SAEV_OK;
    // The reference reads n_dead back every step (modeling.py:92).  Here the record the device wrote DEAD_LAG steps ago
    // bounds it: a latent dead now had at most DEAD_LAG steps' worth of tokens to go then (n_near counts those).  While
    // the bound fits the few-dead-latents kernels -- which covers zero, the usual state of a healthy run -- they are
    // enqueued with the count left on the device and nothing is read back.  The wait below is for an event DEAD_LAG
    // steps in the past; it only ever blocks a host that has run further ahead than that, and never drains the queue.
    // (saev_debug_cfg.aux_small_max: -1 sends every dead set down the dense route, for tests and A/B runs)
    // Default AUX_SMALL_DEFAULT: where the two routes cost the same at configs[1] (tools/experiments/r4_aux_sweep.sh: the
    // few-dead-latents kernels grow with the count, the dense algebra is flat up to 256 dead latents).
    // (with the fp32-MFMA kernels -- d_model % 128 == 0 -- the few-dead-latents route costs +0.24 ms up to 32 and +0.32 ... +0.35 up to 64 dead
    // latents against the dense route's +0.56: it takes everything it can hold, profiles/r05b_aux_mfma_sweep.txt)
    // (round 6: up to AUX_MFMA_MAX = 128 where the context's buffers allow -- aux_mfma_cap -- with one launch per count window
    // [1, 32], [33, 64], [65, 128] up to the bound: the device-side count picks the one that runs)
    const bool mfma_route = aux_mfma_supported(c->cfg.d_model) && c->dbg.aux_small_route == 0;
    const int small_default = mfma_route ? std::max((int)AUX_SMALL_MAX, c->aux_mfma_cap) : (int)AUX_SMALL_DEFAULT;
    const int small_cap = c->dbg.aux_small_max < 0 ? 0 : (c->dbg.aux_small_max == 0 ? small_default : std::min(c->dbg.aux_small_max, (int)AUX_SMALL_MAX));
    const int small_max = std::min(small_cap, c->cfg.k_aux);
    const int64_t s0 = step - DEAD_LAG;
    if (s0 >= c->rec_valid_from) {
        HIPCHK(c, hipEventSynchronize(c->dead_ev[s0 % DEAD_RING]));
        const volatile DeadRecord* r = c->rec_host + s0 % DEAD_RING;
        if (r->step == s0 && c->tokens_seen - r->cum_tokens <= r->horizon_tokens) {
            const int bound = r->n_near;  // >= the dead count of this step
            // nobody was within reach of the threshold then: nothing can be dead now, the auxiliary term is exactly zero
            // and its dozen count-predicated launches (each ~5 us of an empty grid) are not enqueued at all
            if (bound == 0) return SAEV_OK;
            if (bound <= small_max && c->cfg.d_model <= 2048) {
                c->aux_route = AUX_SMALL_DEVICE;
                return auxk_small_forward(c, s, bound);
            }
            // A larger dead set: the dense algebra, sized by the bound, with the count left on the device (round 2 read it
            // back here: one blocking read per step whenever more than a few dozen latents were dead -- configs[2]'s regime)
            if ((bound + 3) / 4 * 4 <= c->nd_cap) {
                c->aux_route = AUX_DENSE;
                c->aux_dev_count = true;
                c->n_dead_host = bound;
                c->k_use_host = std::min(c->cfg.k_aux, bound);
                return auxk_forward(c, s);
            }
        }
    }
    int32_t host[2] = {0, 0};
    HIPCHK(c, hipMemcpyAsync(host, c->flags + 4, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    c->n_readbacks++;
    c->n_dead_host = host[0];
    c->k_use_host = host[1];
    if (c->n_dead_host <= 0) return SAEV_OK;
    if ((c->n_dead_host + 3) / 4 * 4 > c->nd_cap && !(c->n_dead_host <= small_max && c->cfg.d_model <= 2048)) {
        // More dead latents than the dense buffers were sized for (saev_cfg.aux_dead_cap): grow them here -- the stream is
        // idle after the read-back, the buffers carry nothing from step to step -- to twice the need, capped at d_sae.  An
        // exceptional event (a run whose dictionary collapses); it costs a device-wide allocation, never a wrong result.
        const int s4 = (S + 3) / 4 * 4;
        const int cap = std::min(s4, std::max(2 * c->nd_cap, (2 * c->n_dead_host + 1023) / 1024 * 1024));
        for (void* q : c->aux_allocs) hipFree(q);
        c->aux_allocs.clear();
        c->aux_bytes = 0;
        c->nd_cap = 0;
        int rcg = alloc_aux_buffers(c, cap);
        if (rcg != SAEV_OK) {
            c->err = "AuxK: " + std::to_string(c->n_dead_host) + " dead latents exceed saev_cfg.aux_dead_cap and the buffers could not be grown to " +
                     std::to_string(cap) + " (out of device memory)";
            return rcg;
        }
        std::fprintf(stderr, "[saev_amd] AuxK: %d dead latents exceeded the dead-set buffers; grown to %d inside the step "
                             "(device-synchronising; saev_cfg.aux_dead_cap sizes them up front)\n", c->n_dead_host, cap);
    }
    if (c->n_dead_host <= small_max && c->cfg.d_model <= 2048) {
        c->aux_route = AUX_SMALL_HOST;
        return auxk_small_forward(c, s, c->n_dead_host);
    }
    c->aux_route = AUX_DENSE;
    return auxk_forward(c, s);
}

}  // extern "C"
