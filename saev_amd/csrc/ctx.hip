// C ABI of libsaev_amd.so (see include/saev_amd.h): context, scratch, and the launch sequences of
// the train step.  No torch types; plain device pointers and a hipStream_t per call.
// This unit: create / destroy / bind, links between contexts, accessors, read-outs and the entries that take no context; the
// launch sequences are in ctx_forward.hip, ctx_auxk.hip, ctx_backward.hip, ctx_tail.hip and ctx_dp.hip, the context in ctx.h.
#include "ctx.h"

int muon_cfg_check(const saev_muon_cfg& m, std::string* why) {
    if (m.ns_steps < 0 || m.ns_steps >= 100) { *why = "ns_steps must be in [0, 100)"; return SAEV_INVALID_ARG; }
    if (m.adjust_lr < 0 || m.adjust_lr > 2) { *why = "adjust_lr must be 0 (original), 1 (match_rms_adamw) or 2 (none)"; return SAEV_INVALID_ARG; }
    if (!(m.momentum >= 0.f) || !(m.weight_decay >= 0.f)) { *why = "momentum and weight_decay must be >= 0"; return SAEV_INVALID_ARG; }
    return SAEV_OK;
}

extern "C" {

int saev_abi_version(void) { return SAEV_AMD_ABI_VERSION; }

int saev_layout(const saev_cfg* cfg, saev_layout_t* out) {
    if (!cfg || !out || cfg->d_model <= 0 || cfg->d_sae <= 0) return SAEV_INVALID_ARG;
    const int64_t S = cfg->d_sae, D = cfg->d_model, N = std::max(1, cfg->shard_world);
    out->chunk_a = (S + 1 + N - 1) / N * D;
    out->chunk_b = ((D * S + S + N - 1) / N + 3) / 4 * 4;
    out->off_W_dec = 0;
    out->off_b_dec = S * D;
    out->off_W_enc = N * out->chunk_a;
    out->off_b_enc = out->off_W_enc + D * S;
    out->n_total = N * out->chunk_a + N * out->chunk_b;
    return SAEV_OK;
}

// (the context-free entries of batchstats.hip leave their message per thread; a NULL context reads it)
const char* saev_last_error(const saev_ctx* ctx) { return ctx ? ctx->err.c_str() : free_error(); }

int saev_create(const saev_cfg* cfg, int device, saev_ctx** out) { return saev_create_ex(cfg, nullptr, device, out); }

int saev_create_ex(const saev_cfg* cfg, const saev_debug_cfg* dbg, int device, saev_ctx** out) {
    return saev_create_batch_topk(cfg, dbg, nullptr, device, out);
}

int saev_create_batch_topk(const saev_cfg* cfg, const saev_debug_cfg* dbg, const saev_batch_topk_cfg* bt_in, int device, saev_ctx** out) {
    return create_context(cfg, dbg, bt_in, nullptr, device, out);
}

int saev_create_relu_train(const saev_cfg* cfg, const saev_debug_cfg* dbg, const saev_relu_train_cfg* rt, int device, saev_ctx** out) {
    if (!cfg || !out) return SAEV_INVALID_ARG;
    *out = nullptr;
    if (cfg->activation != SAEV_ACT_RELU || cfg->k_aux != 0) return SAEV_INVALID_ARG;
    saev_relu_train_cfg r{};
    if (rt != nullptr && rt->struct_size > 0) std::memcpy(&r, rt, std::min((size_t)rt->struct_size, sizeof(r)));
    if (!(r.l1_coeff >= 0.0) || !std::isfinite(r.l1_coeff)) return SAEV_INVALID_ARG;
    if (cfg->encoder_mode == SAEV_ENCODER_BF16 || cfg->shard_world > 1 || cfg->max_backward_rows > cfg->max_batch) return SAEV_UNSUPPORTED;
    r.struct_size = (int32_t)sizeof(r);
    return create_context(cfg, dbg, nullptr, &r, device, out);
}

}  // extern "C"

int create_context(const saev_cfg* cfg, const saev_debug_cfg* dbg, const saev_batch_topk_cfg* bt_in, const saev_relu_train_cfg* rt, int device,
                   saev_ctx** out) {
    if (!cfg || !out) return SAEV_INVALID_ARG;
    *out = nullptr;
    if (cfg->activation != SAEV_ACT_TOPK && cfg->activation != SAEV_ACT_RELU && cfg->activation != SAEV_ACT_BATCHTOPK) return SAEV_INVALID_ARG;
    const bool btk = cfg->activation == SAEV_ACT_BATCHTOPK;
    if (bt_in != nullptr && !btk) return SAEV_INVALID_ARG;
    saev_batch_topk_cfg bt{};
    if (bt_in != nullptr && bt_in->struct_size > 0) std::memcpy(&bt, bt_in, std::min((size_t)bt_in->struct_size, sizeof(bt)));
    else bt.batch_momentum = 0.1;
    // a BatchTopK context: everything TopK sizes by top_k is sized by the row capacity instead
    saev_cfg btk_cfg;
    int btk_k = 0;
    if (btk) {
        if (cfg->top_k <= 0 || cfg->d_sae <= 0 || bt.row_cap < 0 || bt.list_cap < 0 || !(bt.batch_momentum >= 0.0 && bt.batch_momentum <= 1.0))
            return SAEV_INVALID_ARG;
        if (cfg->encoder_mode == SAEV_ENCODER_BF16 || cfg->shard_world > 1 || cfg->max_backward_rows > cfg->max_batch) return SAEV_UNSUPPORTED;
        if ((uint64_t)cfg->max_batch * (uint64_t)cfg->d_sae >= (1ull << 31)) return SAEV_UNSUPPORTED;  // (32-bit counts of the select)
        btk_k = std::min(cfg->top_k, cfg->d_sae);
        const long want = bt.row_cap > 0 ? bt.row_cap : std::max(64L, 4L * btk_k);
        btk_cfg = *cfg;
        btk_cfg.top_k = (int32_t)std::min<long>(cfg->d_sae, (want + 63) / 64 * 64);
        cfg = &btk_cfg;
    }
    // a ReLU context (forward entries only) has no k: its TopK-sized scratch is sized for k = 1
    saev_cfg relu_cfg;
    if (cfg->activation == SAEV_ACT_RELU) {
        if (cfg->k_aux != 0) return SAEV_UNSUPPORTED;
        relu_cfg = *cfg;
        relu_cfg.top_k = 1;
        cfg = &relu_cfg;
    }
    if (cfg->d_model <= 0 || cfg->d_sae <= 0 || cfg->top_k <= 0 || cfg->max_batch <= 0) return SAEV_INVALID_ARG;
    // candidate lists are addressed with 32-bit byte offsets (max_batch <= 246 723 rows per call)
    if ((uint64_t)cfg->max_batch * CAND_STRIDE * 4ull >= (1ull << 32)) return SAEV_INVALID_ARG;
    if (cfg->d_model % 4 != 0 || cfg->d_sae % 4 != 0 || cfg->d_model > 4096) return SAEV_UNSUPPORTED;
    if (cfg->k_aux < 0 || cfg->k_aux > 1024) return SAEV_UNSUPPORTED;
    if (cfg->encoder_mode != SAEV_ENCODER_F32 && cfg->encoder_mode != SAEV_ENCODER_F16X3 && cfg->encoder_mode != SAEV_ENCODER_BF16 &&
        cfg->encoder_mode != SAEV_ENCODER_F16R)
        return SAEV_INVALID_ARG;
    saev_ctx* c = new saev_ctx();
    c->cfg = *cfg;
    c->cfg.top_k = std::min(cfg->top_k, cfg->d_sae);
    if (dbg != nullptr && dbg->struct_size > 0)
        std::memcpy(&c->dbg, dbg, std::min((size_t)dbg->struct_size, sizeof(saev_debug_cfg)));
    c->device = device;
    c->btk = btk; c->btk_k = btk_k; c->btk_momentum = bt.batch_momentum; c->btk_list_cap = bt.list_cap;
    c->relu_train = rt != nullptr;
    c->rt_l1 = rt != nullptr ? rt->l1_coeff : 0.0;
    if (hipSetDevice(device) != hipSuccess) {
        delete c;
        return SAEV_HIP_ERROR;
    }
    const long S = cfg->d_sae, D = cfg->d_model, MB = cfg->max_batch, K = c->cfg.top_k, KA = cfg->k_aux;
    // rows a BACKWARD may cover: the context's own batch, or -- gathered backward of a data-parallel run that exchanges the
    // sparse step state -- every rank's rows.  Only the latent-major pair order, the slice-major copies and the partial rows
    // are sized by it; everything the forward writes stays at max_batch.
    const long MBB = std::max<long>(MB, cfg->max_backward_rows);
    c->back_rows = (int)MBB;
    if ((uint64_t)MBB * K >= (1ull << 31)) { delete c; return SAEV_INVALID_ARG; }
    // Flat layout [W_dec | b_dec | pad | W_enc | b_enc | pad].  With shard_world = N > 1 each half is padded to N equal
    // chunks -- chunks of the first half are whole decoder rows -- so that a data-parallel run can reduce-scatter the
    // gradient halves, let every rank run the tail on its chunk of each, and all-gather the parameter halves separately
    // (the encoder half first: the next forward needs it first).  N = 1: no padding, the state_dict order as it is.
    {
        saev_layout_t lay;
        saev_layout(cfg, &lay);
        c->shard_world = std::max(1, cfg->shard_world);
        c->chunk_a = lay.chunk_a; c->chunk_b = lay.chunk_b;
        c->off_W_dec = lay.off_W_dec; c->off_b_dec = lay.off_b_dec; c->off_W_enc = lay.off_W_enc; c->off_b_enc = lay.off_b_enc;
        c->n_params = lay.n_total;
    }
    int rc = SAEV_OK;
#define A(p, n) if (rc == SAEV_OK) rc = alloc(c, &c->p, (size_t)(n))
    c->gmax_stride = (int)((MB + 255) / 256 * 256);  // (padding the group pitch changes nothing: measured)
    A(cand_cnt, MB); A(gmax, (size_t)64 * c->gmax_stride); A(cand_idx, MB * CAND_STRIDE); A(cand_val, MB * CAND_STRIDE);
    A(h_dense, MB * S);
    A(idx, MB * K); A(val, MB * K);
    if (KA > 0) { A(aux_idx, MB * KA); A(aux_val, MB * KA); A(g_aux, MB * D); A(dead_list, S); }
    A(x_hat, MB * D); A(g, MB * D);
    A(rowstats, MB);
    c->bitmap_words = (int)(((MBB + 31) / 32 + 7) / 8 * 8);
    A(bitmap, S * c->bitmap_words);
    A(grp_prefix, S * (c->bitmap_words / 8));
    A(scan_totals, ((S + 1023) / 1024) * 4);
    A(counts, S); A(starts, S + 1); A(pairs, MBB * K); A(dval_pairs, MBB * (size_t)cfg->top_k);
    {
        const long max_pairs = MBB * K;
        c->max_work = (int)(S + (max_pairs + DW_CHUNK - 1) / DW_CHUNK);
        c->max_part = (int)(2 * ((max_pairs + DW_CHUNK - 1) / DW_CHUNK) + 2);
    }
    A(chunk_starts, S + 1); A(part_starts, S); A(work_latent, c->max_work);
    A(dW_encT, S * D); A(partials, (size_t)c->max_part * 2 * D); A(db_partials, c->max_part); A(row_proj, S); A(enc_sq, S);
    {
        const bool rows_only = c->dbg.dw_route == 1;
        c->dws_ok = !rows_only && !btk && D % DWS_SLICE == 0 && (uint64_t)S * D * 4ull < (1ull << 32) && MBB < (1l << 24) &&
                    (uint64_t)MBB * K < (1ull << 31);
    }
    c->fwd_slices = !btk && c->cfg.encoder_mode == SAEV_ENCODER_F16R && c->dbg.fwd_route == 0 && D % RS_SLICE == 0 &&
                    (uint64_t)S * 128ull < (1ull << 32) - 256ull && fused_supported(c->cfg);
    if (c->fwd_slices) {
        A(rs_part, (size_t)(D / RS_SLICE) * MB * REFINE_CAP); A(surv_rng, MB * RS_MAX_RANGES);
        // passes over a slice cover RS_LAT_RANGE latents each (x 128 bytes = 4 MB = an XCD's L2: tools/ubench/row_gather.hip gathers
        // out of a whole 4 MB slice at 20-22 TB/s; 16 384-latent ranges made refine_slices 4 % slower), at most RS_MAX_RANGES
        c->rs_lat_range = (int)std::max<long>(RS_LAT_RANGE, ((S + RS_MAX_RANGES - 1) / RS_MAX_RANGES + 255) / 256 * 256);
        c->rs_n_ranges = (int)((S + c->rs_lat_range - 1) / c->rs_lat_range);
    }
    if (c->fwd_slices && !c->dws_ok) A(xS, MBB * D);
    if (c->dws_ok) {
        A(gS, MBB * D); A(xS, MBB * D); A(dvp, (size_t)(D / DWS_SLICE) * MBB * K);
        if (c->dbg.dw_route != 2 && decode_forms_dval((int)D, (int)K)) A(dval_rows, MB * K);  // (route 0: dval from the decode)
        A(pv, MBB * K); A(pv2, MBB * K); A(plat, MBB * K); A(cut_lat, (MBB * K + DWS_RUN - 1) / DWS_RUN); A(cut_list, 4 * (1 + (MBB * K + DWS_RUN - 1) / DWS_RUN)); A(lat_unused, S);
        if (c->dval_rows != nullptr && c->dbg.fin_route == 0) { A(wn2, S); A(sq_wave, (size_t)2 * dw_slices_waves((int)D, (int)(MBB * K))); }
    }
    A(colsum_partials, ((MBB + 63) / 64) * D);
    A(sumsq_partials, 2 * 1024 + (S + 3) / 4 + 8 + transpose_blocks((int)S, (int)D)); A(sumsq_total, 1);
    if (c->cfg.encoder_mode != SAEV_ENCODER_F32 || KA > 0 || c->relu_train) {  // (the f32 encoder needs the image geometry for AuxK and the dense ReLU step only)
        c->Dp = (int)((D + 31) / 32 * 32);
        c->S_pad = (int)((S + 255) / 256 * 256);
        c->MB_pad = (int)((MB + 255) / 256 * 256);
        A(zero_bias, std::max(S, D)); A(aux_scales, 16); A(aux_sync, absmax_parts_max((int)MB));
    }
    if (c->cfg.encoder_mode != SAEV_ENCODER_F32) {
        A(xs, (size_t)c->MB_pad * 2 * c->Dp);
        A(ws, (size_t)c->S_pad * 2 * c->Dp);
        A(row_margin, MB); A(wnorm_scratch, std::max((S + 3) / 4, 3 * ((S + 255) / 256))); A(f16r_scales, 16); A(mu, D); A(xnorm, 2 * MB); A(b_shift, S);
        A(xabs_part, (MB + 3) / 4);
        if (c->cfg.encoder_mode == SAEV_ENCODER_F16R) { A(dot_part, (size_t)2 * (c->Dp / 32) * c->S_pad); A(sq_part, (size_t)2 * (c->Dp / 32) * c->S_pad); A(wmax_prev, 1); }
        if (c->cfg.encoder_mode == SAEV_ENCODER_F16R) { A(surv_idx, MB * REFINE_CAP); A(surv_val, MB * REFINE_CAP); A(surv_cnt, MB); }
    }
    c->stream_ok = c->fwd_slices && c->cfg.bound_mode != 1 && c->dbg.prep_route == 0 && D % 32 == 0 && c->Dp == (int)D;
    if (c->stream_ok) {
        A(WeS, S * D); A(xn_part, (size_t)(D / 32) * c->MB_pad * 2);
        A(amax_part, (size_t)(c->MB_pad / 256) * (D / 32)); A(cmax_part, (size_t)(c->MB_pad / 256) * (D / 32)); A(b_seen, S);
        A(mu_keep, D); A(xside_keep, 4);
        if (c->cfg.bound_mode == 2) { A(rho_state, 16); A(rho_scratch, 32); A(row_bound, MB); A(kth_val, MB); }
    }
    if (c->stream_ok || c->cfg.encoder_mode == SAEV_ENCODER_BF16) A(wchk, (size_t)2 * ((S + 255) / 256) * ((D + 31) / 32));
    A(toks, S); A(fired, S); A(dead, S); A(flags, 16); A(upper, 1); A(stats, 1);
    A(tau_max, MB); A(heur_state, 8); A(stats_scratch, STATS_SCRATCH_DOUBLES); A(tickets, 8); A(db_aux, D);
    if (btk) { A(btk_ws, btk_workspace_words((int)MB)); A(row_nnz, MB); A(btk_over, 1); A(threshold_own, 1); }
#undef A
    if (rc == SAEV_OK && c->relu_train) rc = relu_train_alloc(c);
    if (rc != SAEV_OK) {
        // keep the context so the caller can read the message, but report failure
        for (void* p : c->allocs) hipFree(p);
        delete c;
        return rc;
    }
    hipMemset(c->toks, 0, S * sizeof(int64_t));
    hipMemset(c->fired, 0, S * sizeof(int32_t));
    hipMemset(c->dead, 0, S * sizeof(int32_t));
    hipMemset(c->flags, 0, 16 * sizeof(int32_t));
    if (btk) {
        hipMemset(c->threshold_own, 0, sizeof(float));
        hipMemset(c->btk_ws, 0, BTK_ST_WORDS * sizeof(uint32_t));
        hipMemset(c->btk_over, 0, sizeof(int32_t));
        c->threshold = c->threshold_own;
    }
    if (c->stream_ok || c->cfg.encoder_mode == SAEV_ENCODER_BF16) {
        void* hp = nullptr;
        if (hipHostMalloc(&hp, 64, hipHostMallocMapped) == hipSuccess &&
            hipHostGetDevicePointer(reinterpret_cast<void**>(&c->stale_dev), hp, 0) == hipSuccess) {
            c->stale_host = static_cast<int32_t*>(hp);
            for (int i = 0; i < 16; ++i) c->stale_host[i] = 0;  // ([4], [5]: the pauses of the norm-predicted bounds, RhoArgs::host)
        } else {
            if (hp) hipHostFree(hp);
            c->stale_host = nullptr; c->stale_dev = nullptr;  // (the device-side part of the check still works)
        }
    }
    hipMemset(c->scan_totals, 0, ((S + 1023) / 1024) * 4 * sizeof(int32_t));  // (no workgroup's "ready" word equals a build's epoch)
    hipMemset(c->stats, 0, sizeof(saev_step_stats));
    hipMemset(c->stats_scratch, 0, STATS_SCRATCH_DOUBLES * sizeof(double));
    hipMemset(c->tickets, 0, 8 * sizeof(int));
    {
        const float init[8] = {2.6f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};  // z starts where a Gaussian row of 32 k latents has ~8 k values above its bound
        hipMemcpy(c->heur_state, init, sizeof(init), hipMemcpyHostToDevice);
    }
    if (c->rho_state) {
        // c starts at 0.9; [6] = NaN: no ratio yet (kernels.h: RhoArgs)
        const float init[16] = {0.9f, 0.f, 0.f, 0.f, 0.f, 0.f, __builtin_nanf(""), 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        hipMemcpy(c->rho_state, init, sizeof(init), hipMemcpyHostToDevice);
        hipMemset(c->rho_scratch, 0, 32 * sizeof(float));
    }
    hipMemset(c->rowstats, 0, MB * sizeof(RowStats));
    if (c->xs) hipMemset(c->xs, 0, (size_t)c->MB_pad * 2 * c->Dp * sizeof(_Float16));
    if (c->zero_bias) hipMemset(c->zero_bias, 0, std::max(S, D) * sizeof(float));
    if (c->f16r_scales) hipMemset(c->f16r_scales, 0, 16 * sizeof(float));
    if (KA > 0) {
        // Every AuxK buffer is sized here for the dead set a healthy run meets: no allocation happens inside such a run's
        // steps.  Default min(d_sae, max(4096, 8 k_aux)) dead latents (2.3 GB at configs[1]; d_sae would be 11.5 GB
        // there and 37 GB at configs[3]); a step that meets more grows them (saev_step_dead, reported on stderr).
        const int s4 = (int)((S + 3) / 4 * 4);
        const int want = cfg->aux_dead_cap > 0 ? cfg->aux_dead_cap : std::max(4096, 8 * (int)KA);
        const int cap = std::min((want + 3) / 4 * 4, s4);
        rc = alloc_aux_buffers(c, cap);
        if (rc == SAEV_OK) {
            void* h = nullptr;
            if (hipHostMalloc(&h, DEAD_RING * sizeof(DeadRecord), hipHostMallocMapped) != hipSuccess ||
                hipHostGetDevicePointer(reinterpret_cast<void**>(&c->rec_dev), h, 0) != hipSuccess) {
                rc = SAEV_HIP_ERROR;
            } else {
                c->rec_host = static_cast<DeadRecord*>(h);
                std::memset(h, 0, DEAD_RING * sizeof(DeadRecord));
                for (int i = 0; i < DEAD_RING && rc == SAEV_OK; ++i)
                    if (hipEventCreateWithFlags(&c->dead_ev[i], hipEventDisableTiming) != hipSuccess) rc = SAEV_HIP_ERROR;
                c->dead_ev_created = rc == SAEV_OK;
            }
        }
        if (rc != SAEV_OK) {
            for (void* q : c->allocs) hipFree(q);
            for (void* q : c->aux_allocs) hipFree(q);
            if (c->rec_host) hipHostFree(c->rec_host);
            delete c;
            return rc;
        }
    }
    hipDeviceSynchronize();
    *out = c;
    return SAEV_OK;
}

extern "C" {

// c stops following its leader (which forgets it, or is going away: the caller takes c off its list)
static void detach_follower(saev_ctx* c) {
    c->leader = nullptr;
    centre_owner_changed(c);
    c->borrow_streamed = false;
    c->follow_stream = false;
}

static void unlink_from_leader(saev_ctx* c) {
    if (c->leader != nullptr) {
        auto& f = c->leader->followers;
        f.erase(std::remove(f.begin(), f.end(), c), f.end());
        detach_follower(c);
    }
}

void saev_destroy(saev_ctx* c) {
    if (!c) return;
    // no dangling links either way: followers fall back to their own x-derived buffers, the leader forgets this context
    for (saev_ctx* f : c->followers) detach_follower(f);
    c->followers.clear();
    unlink_from_leader(c);
    hipSetDevice(c->device);
    hipDeviceSynchronize();
    saev_comm_destroy(c);
    for (void* p : c->allocs) hipFree(p);
    for (void* p : c->aux_allocs) hipFree(p);
    if (c->G) hipFree(c->G);
    if (c->GS) hipFree(c->GS);
    if (c->rec_host) hipHostFree(c->rec_host);
    if (c->stale_host) hipHostFree(c->stale_host);
    if (c->dead_ev_created)
        for (int i = 0; i < DEAD_RING; ++i) hipEventDestroy(c->dead_ev[i]);
    if (c->ev_created)
        for (int i = 0; i < TIMING_RING; ++i) {
            hipEventDestroy(c->ev_start[i]);
            hipEventDestroy(c->ev_stop[i]);
        }
    delete c;
}

int saev_bind(saev_ctx* c, float* params, float* grads, float* adam_m, float* adam_v) {
    if (!c) return SAEV_INVALID_ARG;
    REQUIRE(c, params != nullptr, SAEV_INVALID_ARG, "saev_bind: params is NULL");
    REQUIRE(c, ((uintptr_t)params % 16) == 0, SAEV_INVALID_ARG, "saev_bind: params must be 16-byte aligned");
    c->params = params;
    params_moved(c);
    c->grads = grads;
    c->adam_m = adam_m;
    c->adam_v = adam_v;
    return SAEV_OK;
}

int saev_bind_tracker(saev_ctx* c, int64_t* toks, int32_t* fired) {
    if (!c) return SAEV_INVALID_ARG;
    REQUIRE(c, toks && fired, SAEV_INVALID_ARG, "saev_bind_tracker: NULL buffer");
    c->toks = toks;
    c->fired = fired;
    c->tracker_dirty = true;
    c->rec_valid_from = c->dead_steps + 1;
    return SAEV_OK;
}

int saev_set_prefixes(saev_ctx* c, const int64_t* prefixes_host, int32_t n) {
    if (!c) return SAEV_INVALID_ARG;
    const int S = c->cfg.d_sae;
    if (prefixes_host == nullptr || n <= 1) {
        REQUIRE(c, prefixes_host == nullptr || (n == 1 && prefixes_host[0] == S), SAEV_INVALID_ARG,
                "a single prefix must equal d_sae");
        c->P = 1;
        return SAEV_OK;
    }
    REQUIRE(c, !c->relu_train, SAEV_UNSUPPORTED, "saev_set_prefixes: the dense ReLU step implements the plain objective only (n_prefixes = 1)");
    REQUIRE(c, n <= MAX_PREFIXES, SAEV_UNSUPPORTED, "at most 16 Matryoshka prefixes are supported");
    REQUIRE(c, prefixes_host[0] >= 1 && prefixes_host[n - 1] == S, SAEV_INVALID_ARG,
            "prefixes must start at >= 1 and end at d_sae");
    for (int p = 1; p < n; ++p)
        REQUIRE(c, prefixes_host[p] > prefixes_host[p - 1], SAEV_INVALID_ARG, "prefixes must be strictly increasing");
    if (n > c->P_cap) {
        hipDeviceSynchronize();
        if (c->G) hipFree(c->G);
        if (c->GS) hipFree(c->GS);
        c->G = nullptr;
        c->GS = nullptr;
        c->P_cap = 0;
        void* q = nullptr;
        if (hipMalloc(&q, (size_t)c->cfg.max_batch * n * c->cfg.d_model * sizeof(float)) != hipSuccess) {
            c->err = "out of device memory for the Matryoshka gradient buffer";
            return SAEV_HIP_ERROR;
        }
        c->G = (float*)q;
        // (virtual row p * rows + b of a pair word must fit 24 bits: otherwise the row kernels serve the Matryoshka backward)
        if (c->dws_ok && (long)c->cfg.max_batch * n < (1l << 24)) {
            if (hipMalloc(&q, (size_t)c->cfg.max_batch * n * c->cfg.d_model * sizeof(float)) != hipSuccess) {
                c->err = "out of device memory for the Matryoshka gradient buffer (slice-major copy)";
                return SAEV_HIP_ERROR;
            }
            c->GS = (float*)q;
        }
        c->P_cap = n;
    }
    c->P = n;
    for (int p = 0; p < n; ++p) c->cuts[p] = (int32_t)prefixes_host[p];
    return SAEV_OK;
}

int saev_tracker_touched(saev_ctx* c) {
    if (!c) return SAEV_INVALID_ARG;
    c->tracker_dirty = true;
    c->rec_valid_from = c->dead_steps + 1;  // older records describe a tracker that no longer exists
    return SAEV_OK;
}

int saev_share_x(saev_ctx* c, saev_ctx* leader) {
    if (!c) return SAEV_INVALID_ARG;
    if (leader == nullptr || leader == c) { unlink_from_leader(c); return SAEV_OK; }
    REQUIRE(c, !c->btk && !leader->btk, SAEV_UNSUPPORTED, "saev_share_x: a BatchTopK context neither lends nor borrows");
    REQUIRE(c, !c->relu_train && !leader->relu_train, SAEV_UNSUPPORTED, "saev_share_x: a ReLU training context neither lends nor borrows (its step derives nothing but max |x| from x alone)");
    REQUIRE(c, leader->device == c->device && leader->cfg.d_model == c->cfg.d_model && leader->cfg.encoder_mode == c->cfg.encoder_mode,
            SAEV_INVALID_ARG, "saev_share_x: both contexts must live on one device with the same d_model and encoder mode");
    REQUIRE(c, leader->leader == nullptr, SAEV_INVALID_ARG, "saev_share_x: the leader must build its own x-derived buffers");
    REQUIRE(c, c->followers.empty(), SAEV_INVALID_ARG, "saev_share_x: a context that lends its buffers cannot borrow");
    unlink_from_leader(c);
    c->leader = leader;
    centre_owner_changed(c);
    leader->followers.push_back(c);
    c->leader_serial_seen = leader->xprep_serial;  // nothing built before this call is borrowed
    return SAEV_OK;
}

int saev_last_aux_route(const saev_ctx* c) { return c ? c->aux_route : -1; }
int64_t saev_scratch_bytes(const saev_ctx* c, int32_t which) {
    if (!c) return -1;
    const size_t matry = (c->G ? (size_t)c->cfg.max_batch * c->P_cap * c->cfg.d_model * sizeof(float) : 0) * (c->GS ? 2 : 1);
    return (int64_t)(which == 1 ? c->aux_bytes : which == 2 ? matry : which == 3 ? c->muon_bytes
                                                                      : c->scratch_bytes + c->aux_bytes + matry + c->muon_bytes);
}
int64_t saev_dead_readbacks(const saev_ctx* c) { return c ? c->n_readbacks : -1; }

int saev_copy_last(saev_ctx* c, int32_t n_rows, int32_t* idx_out, float* val_out, float* x_hat_out, void* stream) {
    if (!c) return SAEV_INVALID_ARG;
    REQUIRE(c, c->n_last > 0, SAEV_INVALID_ARG, "saev_copy_last: no forward has run");
    REQUIRE(c, n_rows == c->n_last, SAEV_INVALID_ARG,
            "saev_copy_last: n_rows differs from the batch of the last forward (the caller's buffers are sized by it)");
    hipStream_t s = (hipStream_t)stream;
    const size_t nk = (size_t)c->n_last * c->cfg.top_k, nd = (size_t)c->n_last * c->cfg.d_model;
    if (idx_out) HIPCHK(c, hipMemcpyAsync(idx_out, c->idx, nk * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    if (val_out) HIPCHK(c, hipMemcpyAsync(val_out, c->val, nk * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (x_hat_out) HIPCHK(c, hipMemcpyAsync(x_hat_out, c->x_hat, nd * sizeof(float), hipMemcpyDeviceToDevice, s));
    return SAEV_OK;
}

int saev_copy_last_row_nnz(saev_ctx* c, int32_t n_rows, int32_t* row_nnz_out, void* stream) {
    if (!c) return SAEV_INVALID_ARG;
    REQUIRE(c, c->btk, SAEV_UNSUPPORTED, "saev_copy_last_row_nnz: the context is not a BatchTopK context");
    REQUIRE(c, c->n_last > 0 && n_rows == c->n_last && row_nnz_out, SAEV_INVALID_ARG,
            "saev_copy_last_row_nnz: n_rows differs from the batch of the last forward (or none has run)");
    HIPCHK(c, hipMemcpyAsync(row_nnz_out, c->row_nnz, (size_t)n_rows * sizeof(int32_t), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return SAEV_OK;
}

int saev_bind_threshold(saev_ctx* c, float* threshold) {
    if (!c) return SAEV_INVALID_ARG;
    REQUIRE(c, c->btk, SAEV_UNSUPPORTED, "saev_bind_threshold: the context is not a BatchTopK context");
    c->threshold = threshold != nullptr ? threshold : c->threshold_own;
    return SAEV_OK;
}
float* saev_threshold_device(saev_ctx* c) { return c ? c->threshold : nullptr; }
int32_t saev_row_cap(const saev_ctx* c) { return c && c->btk ? c->cfg.top_k : 0; }
int32_t saev_row_overflow_need(const saev_ctx* c) { return c ? c->btk_need : 0; }

int saev_batch_topk_state(saev_ctx* c, float* cut, int64_t* n_above, int64_t* tie_quota, int64_t* n_ties, void* stream) {
    if (!c) return SAEV_INVALID_ARG;
    REQUIRE(c, c->btk, SAEV_UNSUPPORTED, "saev_batch_topk_state: the context is not a BatchTopK context");
    uint32_t h[BTK_ST_WORDS];
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(c, hipMemcpyAsync(h, c->btk_ws, sizeof(h), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    if (cut) std::memcpy(cut, &h[BTK_ST_CUT], sizeof(float));
    if (n_above) *n_above = h[BTK_ST_ABOVE];
    if (tie_quota) *tie_quota = h[BTK_ST_RANK];
    if (n_ties) *n_ties = h[BTK_ST_TIES];
    return SAEV_OK;
}

int64_t* saev_toks_since_active(saev_ctx* c) { return c ? c->toks : nullptr; }
int32_t* saev_fired_flags(saev_ctx* c) { return c ? c->fired : nullptr; }
const saev_step_stats* saev_stats_device(saev_ctx* c) { return c ? c->stats : nullptr; }
const int32_t* saev_last_idx(saev_ctx* c) { return c ? c->idx : nullptr; }
const float* saev_last_val(saev_ctx* c) { return c ? c->val : nullptr; }
const float* saev_last_x_hat(saev_ctx* c) { return c ? c->x_hat : nullptr; }

int saev_read_stats(saev_ctx* c, saev_step_stats* out_host, void* stream) {
    if (!c || !out_host) return SAEV_INVALID_ARG;
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(c, hipMemcpyAsync(out_host, c->stats, sizeof(saev_step_stats), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    return SAEV_OK;
}

int saev_bound_state(saev_ctx* c, float* z, int64_t* launches, int64_t* repeats, float* mean_candidates, void* stream) {
    if (!c) return SAEV_INVALID_ARG;
    float h[4] = {0.f, 0.f, 0.f, 0.f};
    hipStream_t s = (hipStream_t)stream;
    // (the norm-predicted bounds keep the same four figures in their own state: [0] is their safety factor c)
    HIPCHK(c, hipMemcpyAsync(h, c->rho_state != nullptr ? c->rho_state : c->heur_state, sizeof(h), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    if (z) *z = h[0];
    if (repeats) *repeats = (int64_t)h[1];
    if (launches) *launches = (int64_t)h[2];
    if (mean_candidates) *mean_candidates = h[3];
    return SAEV_OK;
}

int saev_bound_ratio(saev_ctx* c, float* rho_lo, int64_t* pause_left, void* stream) {
    if (!c) return SAEV_INVALID_ARG;
    float h[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, __builtin_nanf(""), 0.f};
    hipStream_t s = (hipStream_t)stream;
    if (c->rho_state != nullptr) {
        HIPCHK(c, hipMemcpyAsync(h, c->rho_state, sizeof(h), hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
    }
    if (rho_lo) *rho_lo = h[6];
    if (pause_left) *pause_left = (int64_t)h[5];
    return SAEV_OK;
}

int saev_enable_kernel_timing(saev_ctx* c, int32_t enable) {
    if (!c) return SAEV_INVALID_ARG;
    if (enable && !c->ev_created) {
        for (int i = 0; i < TIMING_RING; ++i) {
            HIPCHK(c, hipEventCreate(&c->ev_start[i]));
            HIPCHK(c, hipEventCreate(&c->ev_stop[i]));
        }
        c->ev_created = true;
    }
    c->timing = enable != 0;
    c->ev_count = 0;
    return SAEV_OK;
}

// mean duration (ms) of the encoder kernel over the steps recorded since timing was enabled
// (at most the last TIMING_RING); caller must have synchronised the stream.
float saev_last_encoder_ms(saev_ctx* c) {
    if (!c || !c->ev_created || c->ev_count == 0) return -1.f;
    const long n = std::min<long>(c->ev_count, TIMING_RING);
    double tot = 0;
    for (long i = 0; i < n; ++i) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, c->ev_start[i], c->ev_stop[i]) != hipSuccess) return -1.f;
        tot += ms;
    }
    return (float)(tot / n);
}

int saev_params_touched(saev_ctx* c) {
    if (!c) return SAEV_INVALID_ARG;
    params_moved(c);
    return SAEV_OK;
}

// ---- Muon (include/saev_amd.h: MUON; kernels in muon.hip) -----------------------------------------------------------------
void saev_muon_default_cfg(saev_muon_cfg* out) {
    if (!out) return;
    *out = saev_muon_cfg{0.95f, 0.1f, 3.4445f, -4.7750f, 2.0315f, 1e-7f, 1, 5, 0};
}

int64_t saev_muon_workspace_bytes(int64_t rows, int64_t cols) {
    if (rows <= 0 || cols <= 0 || rows > cols || cols > (int64_t)1 << 30) return -1;
    return (int64_t)muon_layout((int)rows, (int)cols).bytes;
}

int saev_muon_newton_schulz(const void* x_in, int64_t rows, int64_t cols, void* x_out, const saev_muon_cfg* cfg, int32_t normalize,
                            void* workspace, int64_t workspace_bytes, void* stream) {
    if (!x_in || !x_out || !workspace) return SAEV_INVALID_ARG;
    const int64_t need = saev_muon_workspace_bytes(rows, cols);
    if (need < 0 || workspace_bytes < need || ((uintptr_t)workspace & 255) != 0) return SAEV_INVALID_ARG;
    saev_muon_cfg m;
    saev_muon_default_cfg(&m);
    if (cfg) m = *cfg;
    std::string why;
    if (muon_cfg_check(m, &why) != SAEV_OK) return SAEV_INVALID_ARG;
    hipStream_t s = (hipStream_t)stream;
    const int D = (int)rows, S = (int)cols;
    const MuonLayout L = muon_layout(D, S);
    uint8_t* ws = static_cast<uint8_t*>(workspace);
    // (the padding must be zero: the whole X buffer is cleared, then the caller's matrix is copied in)
    if (hipMemsetAsync(ws + L.off_X[0], 0, (size_t)L.Dp * L.Sp * 2, s) != hipSuccess) return SAEV_HIP_ERROR;
    if (launch_muon_load(static_cast<const uint16_t*>(x_in), D, S, reinterpret_cast<uint16_t*>(ws + L.off_X[0]), L.Sp,
                         reinterpret_cast<double*>(ws + L.off_sq), s) != hipSuccess) return SAEV_HIP_ERROR;
    hipError_t e = hipSuccess;
    const int cur = muon_newton_schulz(ws, L, D, S, normalize, m.ns_steps, m.a, m.b, m.c, m.eps, s, &e);
    if (cur < 0) return SAEV_HIP_ERROR;
    if (hipMemcpy2DAsync(x_out, (size_t)S * 2, ws + L.off_X[cur], (size_t)L.Sp * 2, (size_t)S * 2, (size_t)D, hipMemcpyDeviceToDevice, s) != hipSuccess)
        return SAEV_HIP_ERROR;
    return SAEV_OK;
}

// ---- dictionary coherence (include/saev_amd.h: COHERENCE; kernels in coherence.hip) ---------------------------------------
int64_t saev_coherence_workspace_bytes(int64_t S, int64_t D) {
    if (S < 1 || S > ((int64_t)1 << 20) || D < 4 || D > 4096 || D % 4 != 0) return -1;
    return (int64_t)coherence_layout((int)S, (int)D).bytes;
}

int saev_dictionary_coherence(const float* W, int64_t S, int64_t D, int32_t route, void* workspace, int64_t workspace_bytes,
                              float* out_value, int32_t* out_pair, int32_t* out_info, void* stream) {
    const int64_t need = saev_coherence_workspace_bytes(S, D);
    if (need < 0 || (route != SAEV_COH_AUTO && route != SAEV_COH_EXACT)) return SAEV_INVALID_ARG;
    if (!W || !workspace || !out_value || !out_pair || !out_info) return SAEV_INVALID_ARG;
    if (workspace_bytes < need || ((uintptr_t)workspace & 255) != 0 || ((uintptr_t)W & 15) != 0) return SAEV_INVALID_ARG;
    const CohLayout L = coherence_layout((int)S, (int)D);
    if (launch_coherence(W, (int)S, (int)D, route, static_cast<uint8_t*>(workspace), L, out_value, out_pair, out_info,
                         (hipStream_t)stream) != hipSuccess)
        return SAEV_HIP_ERROR;
    return SAEV_OK;
}

// ---- dictionary match (include/saev_amd.h: DICTIONARY MATCH; kernels in dictmatch.hip) --------------------------------------
int64_t saev_dictionary_match_workspace_bytes(int64_t Sa, int64_t Sb, int64_t D) {
    const int64_t smax = (int64_t)1 << 20;
    if (Sa < 1 || Sa > smax || Sb < 1 || Sb > smax || D < 4 || D > 4096 || D % 4 != 0) return -1;
    return (int64_t)dictmatch_layout(Sa, Sb, (int)D).bytes;
}

int saev_dictionary_match(const float* A, int64_t Sa, const float* B, int64_t Sb, int64_t D, int32_t absolute, int32_t route,
                          void* workspace, int64_t workspace_bytes, float* out_value, int32_t* out_index, int32_t* out_info,
                          void* stream) {
    const int64_t need = saev_dictionary_match_workspace_bytes(Sa, Sb, D);
    if (need < 0 || (route != SAEV_MATCH_AUTO && route != SAEV_MATCH_EXACT)) return SAEV_INVALID_ARG;
    if (!B && Sb != Sa) return SAEV_INVALID_ARG;  // self mode: Sb repeats Sa
    if (!A || !workspace || !out_value || !out_index || !out_info) return SAEV_INVALID_ARG;
    if (workspace_bytes < need || ((uintptr_t)workspace & 255) != 0 || ((uintptr_t)A & 15) != 0 || ((uintptr_t)B & 15) != 0)
        return SAEV_INVALID_ARG;
    const DmLayout L = dictmatch_layout(Sa, Sb, (int)D);
    if (launch_dictmatch(A, (int)Sa, B, (int)Sb, (int)D, absolute, route, static_cast<uint8_t*>(workspace), L, out_value, out_index,
                         out_info, (hipStream_t)stream) != hipSuccess)
        return SAEV_HIP_ERROR;
    return SAEV_OK;
}

}  // extern "C"
