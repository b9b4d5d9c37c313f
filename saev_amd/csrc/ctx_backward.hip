// The backward launch sequences behind the C ABI: pair-list build, weight gradients, the gathered-backward override, the compact AuxK rows.
#include "ctx.h"

extern "C" {

// ---- backward in three pieces (saev_step_backward = all of them over the full latent range) -------------------------

int saev_backward_begin(saev_ctx* c, void* stream) {
    if (!c) return SAEV_INVALID_ARG;
    REQUIRE(c, !c->relu_train, SAEV_UNSUPPORTED, "saev_backward_begin: a ReLU training context runs its dense backward in one piece (saev_step_backward)");
    REQUIRE(c, c->x_last && c->training_last, SAEV_INVALID_ARG, "saev_backward_begin: no training forward in flight");
    REQUIRE(c, c->grads, SAEV_NOT_BOUND, "gradient buffer not bound");
    hipStream_t s = (hipStream_t)stream;
    const int S = c->cfg.d_sae, D = c->cfg.d_model, K = c->cfg.top_k;
    const bool ov = c->ov_x != nullptr;
    const int n = ov ? c->ov_n : c->n_last;  // rows whose (row, latent) pairs this backward covers
    const int words = ((n + 31) / 32 + 7) / 8 * 8;
    c->row_proj_valid = false;
    CscArgs a{};
    a.idx = ov ? c->ov_idx : c->idx; a.code_stride = K; a.k = K; a.k_dev = nullptr; a.n_rows = n; a.S = S;
    a.bitmap = c->bitmap; a.words = words; a.grp_prefix = c->grp_prefix; a.scan_totals = c->scan_totals;
    a.counts = c->counts; a.starts = c->starts; a.pairs = c->pairs;
    a.chunk_starts = c->chunk_starts; a.part_starts = c->part_starts; a.work_latent = c->work_latent;
    // (a gathered backward -- the rows of all ranks, row-major -- gets its slice-major copies here; Matryoshka ones keep dw_rows)
    const bool ov_slices = ov && c->dws_ok && c->P_last == 1 && n <= c->back_rows;
    c->dws_pairs = ov ? ov_slices : c->dws_rows == n;
    if (ov_slices) {
        c->xS_bwd = c->xS;
        if (!c->followers.empty()) {
            if (c->xS_ov == nullptr) {  // (once per context: a device-wide allocation outside any steady-state step)
                int rca = alloc(c, &c->xS_ov, (size_t)c->back_rows * D);
                if (rca != SAEV_OK) return rca;
            }
            c->xS_bwd = c->xS_ov;
        }
        HIPCHK(c, launch_slice_major_copy(c->ov_g, c->ov_x, n, D, c->gS, c->xS_bwd, s));
        c->dws_rows = 0;  // (the copies no longer describe the forward's own rows)
    }
    c->csc_epoch = c->csc_epoch == 0x7fffffff ? 1 : c->csc_epoch + 1;
    a.epoch = c->dbg.csc_route == 2 ? 0 : c->csc_epoch;  // (csc_route 2: the two-launch scan)
    if (c->dws_pairs) {
        a.zero_word = c->cut_list;
        a.pv = c->pv; a.plat = c->plat; a.val = ov ? c->ov_val : c->val;
        a.P = c->P_last;
        for (int p = 0; p < c->P_last; ++p) a.cuts[p] = c->cuts_last[p];
        if (!ov && c->dval_fwd) { a.pv2 = c->pv2; a.dval = c->dval_rows; }
    }
    c->dval_pairs_ready = c->dws_pairs && a.pv2 != nullptr;
    // (inside saev_train_step the column slices take the whole backward: the row kernels' pair list and work items are not built)
    if (c->fused_step && c->dws_pairs) { a.pairs = nullptr; a.chunk_starts = nullptr; a.part_starts = nullptr; a.work_latent = nullptr; }
    // (the bit map row pitch depends on the batch: a map cleaned for a pitch covers every shorter one, S * words <= before)
    // db_dec = column sums of dL/dx_hat (Matryoshka: of the suffix sums C_0), formed in the grids of the CSC build's first two
    // launches; the AuxK contractions add theirs
    const float* gmat = ov ? c->ov_g : (c->P_last > 1 ? c->G : c->g);
    // (saev_train_step's plain forward leaves dL/dx_hat slice-major alone: the same values, the same rows per partial, the same order)
    const bool g_slices = !ov && c->P_last == 1 && !c->g_rows_valid;
    if (g_slices) {
        REQUIRE(c, c->dws_rows == n, SAEV_INVALID_ARG, "saev_backward_begin: the forward in flight left no gradient rows");
        gmat = c->gS;
    }
    // (prefilled: this forward's decode has set the bits of exactly these codes: no clear, no fill pass)
    const bool prefilled = !ov && c->bitmap_prefill_words == words && c->bitmap_prefill_rows == n;
    HIPCHK(c, launch_csc_build(a, s, c->bitmap_clean && words <= c->bitmap_clean_words, gmat, D, (long)c->P_last * D,
                               c->colsum_partials, c->grads + c->off_b_dec, prefilled, g_slices));
    c->bitmap_prefill_words = 0;
    c->last_backward_gathered = ov;
    c->bitmap_clean = false;
    c->bitmap_words_last = words;
    if (c->aux_route != AUX_NONE) {
        int rc = auxk_backward(c, s);
        if (rc != SAEV_OK) return rc;
    }
    return SAEV_OK;
}

int saev_backward_rows(saev_ctx* c, int32_t lat_lo, int32_t lat_hi, void* stream) {
    return saev_backward_rows_part(c, lat_lo, lat_hi, 0, stream);
}

int saev_backward_rows_part(saev_ctx* c, int32_t lat_lo, int32_t lat_hi, int32_t part, void* stream) {
    if (!c) return SAEV_INVALID_ARG;
    REQUIRE(c, !c->relu_train, SAEV_UNSUPPORTED, "saev_backward_rows: a ReLU training context runs its dense backward in one piece, over all latents (saev_step_backward)");
    REQUIRE(c, part >= 0 && part <= 2, SAEV_INVALID_ARG, "saev_backward_rows_part: part must be 0 (both), 1 (decoder) or 2 (encoder)");
    REQUIRE(c, c->x_last && c->training_last && c->grads, SAEV_INVALID_ARG, "saev_backward_rows: call saev_backward_begin first");
    const int S = c->cfg.d_sae, D = c->cfg.d_model, K = c->cfg.top_k;
    const bool ov = c->ov_x != nullptr;
    const int n = ov ? c->ov_n : c->n_last;
    REQUIRE(c, 0 <= lat_lo && lat_lo < lat_hi && lat_hi <= S, SAEV_INVALID_ARG, "saev_backward_rows: bad latent range");
    REQUIRE(c, !c->btk || (part == 0 && lat_lo == 0 && lat_hi == S), SAEV_UNSUPPORTED,
            "saev_backward_rows: a BatchTopK context runs the backward over all latents in one part");
    hipStream_t s = (hipStream_t)stream;
    DwRowsArgs a{};
    a.starts = c->starts; a.chunk_starts = c->chunk_starts; a.work_latent = c->work_latent;
    a.part_starts = c->part_starts; a.pairs = c->pairs; a.val = ov ? c->ov_val : c->val; a.W_dec = c->params + c->off_W_dec;
    a.g = ov ? c->ov_g : (c->P_last > 1 ? c->G : c->g);  // Matryoshka: rows receive the suffix-summed gradients C_p
    const bool slices_all = lat_lo == 0 && lat_hi == S && c->dws_pairs && (ov || c->dws_rows == n);
    REQUIRE(c, ov || c->P_last > 1 || c->g_rows_valid || slices_all, SAEV_INVALID_ARG,
            "saev_backward_rows: the fused step's forward keeps no row-major gradient (a latent range needs the phase forward)");
    a.x = ov ? c->ov_x : c->x_last;
    a.D = D; a.S = S; a.k_dev = nullptr; a.accumulate = 0;
    a.P = c->P_last;
    for (int p = 0; p < c->P_last; ++p) a.cuts[p] = c->cuts_last[p];
    a.dW_dec = c->grads + c->off_W_dec; a.dW_encT = c->dW_encT; a.db_enc = c->grads + c->off_b_enc;
    a.partials = c->partials; a.db_partials = c->db_partials;
    a.lat_lo = lat_lo; a.lat_hi = lat_hi;
    a.part = part; a.dval = c->dval_pairs;
    const bool all_rows = part == 0 && lat_lo == 0 && lat_hi == S;
    // a pass over all latents also clears the CSC bit map behind itself (nothing reads it after the build)
    const bool clears = part != 2 && lat_lo == 0 && lat_hi == S && c->bitmap_words_last > 0;
    if (clears) { a.clear_bitmap = c->bitmap; a.clear_words = c->bitmap_words_last; }
    a.row_proj = all_rows ? c->row_proj : nullptr; a.project = c->cfg.remove_parallel_grads ? 1 : 0;
    a.enc_sq = all_rows ? c->enc_sq : nullptr;
    // upper bound of the work items of the range (one per latent + one per 64 pairs): the kernel knows the exact count
    const int max_work = (lat_hi - lat_lo) + (int)(((long)n * K + DW_CHUNK - 1) / DW_CHUNK);
    if (slices_all) {
        // all latents of this context's own batch (in one pass or as the decoder / encoder halves of a two-pass backward): column slices out of the XCD L2s (kernels.h: DwSlicesArgs)
        DwSlicesArgs w{};
        w.starts = c->starts; w.pv = c->pv; w.pv2 = c->pv2; w.plat = c->plat; w.gS = c->P_last > 1 ? c->GS : c->gS; w.W_dec = a.W_dec; w.P = c->P_last;
        // (the forward's own slice-major x: split_f16r's -- possibly the leader's -- or the decode's; gathered rows: the copy saev_backward_begin made)
        w.xS = ov ? c->xS_bwd : (c->fwd_step ? c->xS_c : c->xS);
        w.n_rows = n; w.D = D; w.S = S; w.pair_cap = (int)((long)c->back_rows * K);
        w.dvp = c->dvp; w.dW_dec = a.dW_dec; w.dW_encT = a.dW_encT; w.db_enc = a.db_enc;
        const size_t runs_cap = ((size_t)w.pair_cap + DWS_RUN - 1) / DWS_RUN;
        w.part_dec = c->partials; w.part_enc = c->partials + 2 * runs_cap * D;  // (max_part * 2 rows hold 4 * runs_cap)
        w.cut_lat = c->cut_lat; w.cut_list = c->cut_list;
        w.lat_unused = (all_rows && c->fused_step) ? c->lat_unused : nullptr;
        c->unused_valid = w.lat_unused != nullptr;
        w.row_proj = a.row_proj; w.project = a.project; w.enc_sq = a.enc_sq;
        w.clear_bitmap = a.clear_bitmap; w.clear_words = a.clear_words;
        w.have_dval = c->dval_pairs_ready ? 1 : 0;
        c->sq_wave_n = 0;
        if (c->dval_pairs_ready && c->wn2_fresh && part == 0) {
            w.wn2 = c->wn2;
            if (c->fused_step && all_rows && c->sq_wave != nullptr && c->dbg.fin_route != 2) {  // (fin_route 2: the finalize reads the rows for their squares)
                c->sq_wave_n = dw_slices_waves(D, (int)((long)n * K));
                w.sq_wave_dec = c->sq_wave; w.sq_wave_enc = c->sq_wave + c->sq_wave_n;
            }
        }
        HIPCHK(c, launch_dw_slices(w, (int)((long)n * K), part, s));
    } else {
        c->unused_valid = false;
        HIPCHK(c, launch_dw_rows(a, max_work, s));
    }
    if (c->aux_route == AUX_DENSE)  // (the count on the device when the host only had a bound of it: aux_dev_count)
        HIPCHK(c, launch_scatter_add_dead(c->dead_list, c->n_dead_host, D, c->dWd, c->dWe, c->dbe, c->grads + c->off_W_dec,
                                          c->dW_encT, c->grads + c->off_b_enc, lat_lo, lat_hi, s,
                                          c->aux_dev_count ? c->flags + 4 : nullptr, part, a.row_proj, a.W_dec, a.project, a.enc_sq,
                                          c->unused_valid ? c->lat_unused : nullptr, c->sq_wave_n > 0 ? c->starts : nullptr));
    else if (c->aux_route != AUX_NONE)  // few dead latents: the device knows how many
        HIPCHK(c, launch_scatter_add_dead(c->dead_list, c->aux_mfma ? c->aux_ndp : AUX_SMALL_MAX, D, c->dWd, c->dWe, c->dbe, c->grads + c->off_W_dec,
                                          c->dW_encT, c->grads + c->off_b_enc, lat_lo, lat_hi, s, c->flags + 4, part,
                                          a.row_proj, a.W_dec, a.project, a.enc_sq, c->unused_valid ? c->lat_unused : nullptr,
                                          c->sq_wave_n > 0 ? c->starts : nullptr));
    // gathered backward: the auxiliary term's share of db_dec (summed over the ranks by the caller, like the compact rows)
    if (ov && c->aux_route != AUX_NONE && part != 2 && lat_lo == 0)
        HIPCHK(c, launch_colsum(c->db_aux, 1, D, c->colsum_partials, c->grads + c->off_b_dec, 1, nullptr, s));
    c->row_proj_valid = all_rows;
    if (clears) { c->bitmap_clean = true; c->bitmap_clean_words = c->bitmap_words_last; }
    return SAEV_OK;
}

float* saev_grad_w_enc_t(saev_ctx* c) { return c ? c->dW_encT : nullptr; }

int saev_bind_w_enc_t(saev_ctx* c, float* scratch) {
    if (!c || !scratch) return SAEV_INVALID_ARG;
    c->dW_encT = scratch;
    return SAEV_OK;
}

int saev_copy_step_state(saev_ctx* c, int32_t n_rows, float* g_out, int32_t* idx_out, float* val_out, void* stream) {
    if (!c) return SAEV_INVALID_ARG;
    REQUIRE(c, !c->btk, SAEV_UNSUPPORTED, "saev_copy_step_state: not for a BatchTopK context (no sparse-state exchange)");
    REQUIRE(c, !c->relu_train, SAEV_UNSUPPORTED, "saev_copy_step_state: not for a ReLU training context (its step state is dense: no sparse-state exchange)");
    REQUIRE(c, c->n_last > 0 && c->training_last && n_rows == c->n_last, SAEV_INVALID_ARG,
            "saev_copy_step_state: n_rows must be the row count of the training forward in flight");
    hipStream_t s = (hipStream_t)stream;
    // (Matryoshka: P suffix-summed gradients per row, (n_rows, P, d_model) -- what the backward consumes in that case)
    const size_t nk = (size_t)n_rows * c->cfg.top_k, nd = (size_t)n_rows * c->cfg.d_model * (size_t)c->P_last;
    REQUIRE(c, !g_out || c->P_last > 1 || c->g_rows_valid, SAEV_INVALID_ARG,
            "saev_copy_step_state: the fused step's forward keeps no row-major gradient (use saev_step_forward)");
    if (g_out) HIPCHK(c, hipMemcpyAsync(g_out, c->P_last > 1 ? c->G : c->g, nd * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (idx_out) HIPCHK(c, hipMemcpyAsync(idx_out, c->idx, nk * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    if (val_out) HIPCHK(c, hipMemcpyAsync(val_out, c->val, nk * sizeof(float), hipMemcpyDeviceToDevice, s));
    return SAEV_OK;
}

int saev_backward_override(saev_ctx* c, const float* x_all, const float* g_all, const int32_t* idx_all, const float* val_all,
                           int32_t n_all) {
    if (!c) return SAEV_INVALID_ARG;
    if (x_all == nullptr) { c->ov_x = nullptr; c->ov_n = 0; return SAEV_OK; }
    REQUIRE(c, !c->btk, SAEV_UNSUPPORTED, "saev_backward_override: not for a BatchTopK context (a batch-wide top-k over ranks needs a distributed select)");
    REQUIRE(c, !c->relu_train, SAEV_UNSUPPORTED, "saev_backward_override: not for a ReLU training context (one GPU: the dense backward runs over its own rows)");
    REQUIRE(c, g_all && idx_all && val_all && n_all > 0, SAEV_INVALID_ARG, "saev_backward_override: NULL buffer");
    REQUIRE(c, n_all <= c->back_rows, SAEV_INVALID_ARG,
            "saev_backward_override: the gathered row count exceeds saev_cfg.max_backward_rows (set it to the GLOBAL batch)");
    REQUIRE(c, c->x_last && c->training_last, SAEV_INVALID_ARG, "saev_backward_override: no training forward in flight");
    REQUIRE(c, ((uintptr_t)x_all % 16) == 0 && ((uintptr_t)g_all % 16) == 0, SAEV_INVALID_ARG, "x_all / g_all must be 16-byte aligned");
    c->ov_x = x_all; c->ov_g = g_all; c->ov_idx = idx_all; c->ov_val = val_all; c->ov_n = n_all;
    return SAEV_OK;
}

int32_t saev_aux_compact_rows(const saev_ctx* c) {
    if (!c || c->aux_route == AUX_NONE) return 0;
    return c->aux_route == AUX_DENSE ? (c->n_dead_host + 3) / 4 * 4 : (c->aux_mfma ? c->aux_ndp : AUX_SMALL_MAX);
}

// [dWd rows x D | dWe rows x D | dbe rows | db_aux D]
static int aux_compact_copy(saev_ctx* c, float* buf, bool out, hipStream_t s) {
    const size_t rows = (size_t)saev_aux_compact_rows(c), D = c->cfg.d_model;
    if (rows == 0) return SAEV_OK;
    REQUIRE(c, buf != nullptr, SAEV_INVALID_ARG, "saev_aux_compact_*: NULL buffer");
    float* seg[4] = {c->dWd, c->dWe, c->dbe, c->db_aux};
    const size_t len[4] = {rows * D, rows * D, rows, D};
    size_t off = 0;
    for (int i = 0; i < 4; ++i) {
        if (out) HIPCHK(c, hipMemcpyAsync(buf + off, seg[i], len[i] * sizeof(float), hipMemcpyDeviceToDevice, s));
        else HIPCHK(c, hipMemcpyAsync(seg[i], buf + off, len[i] * sizeof(float), hipMemcpyDeviceToDevice, s));
        off += len[i];
    }
    return SAEV_OK;
}
int saev_aux_compact_export(saev_ctx* c, float* buf, void* stream) {
    if (!c) return SAEV_INVALID_ARG;
    return aux_compact_copy(c, buf, true, (hipStream_t)stream);
}
int saev_aux_compact_import(saev_ctx* c, const float* buf, void* stream) {
    if (!c) return SAEV_INVALID_ARG;
    return aux_compact_copy(c, const_cast<float*>(buf), false, (hipStream_t)stream);
}

int saev_trust_gradients(saev_ctx* c, int32_t on) {
    if (!c) return SAEV_INVALID_ARG;
    c->trust_grads = on != 0;
    return SAEV_OK;
}

int saev_backward_end(saev_ctx* c, void* stream) {
    if (!c) return SAEV_INVALID_ARG;
    REQUIRE(c, !c->relu_train, SAEV_UNSUPPORTED, "saev_backward_end: a ReLU training context runs its dense backward in one piece (saev_step_backward)");
    REQUIRE(c, c->grads, SAEV_NOT_BOUND, "gradient buffer not bound");
    // (the per-tile squares land behind the tail's other partial sums: [2 nb + ceil(S / 4), ...))
    double* sq = c->sumsq_partials + 2 * sumsq_blocks() + (c->cfg.d_sae + 3) / 4;
    HIPCHK(c, launch_transpose(c->dW_encT, c->grads + c->off_W_enc, c->cfg.d_sae, c->cfg.d_model, (hipStream_t)stream, sq));
    c->wenc_sq_valid = true;
    return SAEV_OK;
}

int saev_step_backward(saev_ctx* c, void* stream) {
    if (c && c->relu_train) return relu_train_backward(c, (hipStream_t)stream);
    int rc = saev_backward_begin(c, stream);
    if (rc != SAEV_OK) return rc;
    rc = saev_backward_rows(c, 0, c->cfg.d_sae, stream);
    if (rc != SAEV_OK) return rc;
    return saev_backward_end(c, stream);
}

}  // extern "C"
