/*
 * saev_amd.h — C ABI of libsaev_amd.so: the MI355X (gfx950) TopK / BatchTopK / ReLU SAE train-step path and the ReLU forward.
 *
 * This is the drop-in boundary for the hot path of OSU-NLP-Group/saev.  The reference has no FFI of
 * its own (it is pure PyTorch); each entry point below names the reference code it replaces
 * (paths relative to the reference root, src/saev/...).  The Python host in saev_amd/ binds these
 * with ctypes (see INTEGRATION.md for the stub a saev maintainer would add).
 *
 * Conventions
 *   - plain pointers + sizes; all pointers are DEVICE pointers unless the name ends in _host;
 *   - every call returns 0 or a negative saev_status; saev_last_error() gives the message;
 *   - all work is enqueued on the hipStream_t passed as `stream` (void*; NULL = default stream);
 *     nothing synchronises unless documented;
 *   - the library never frees caller memory; scratch is owned by the context;
 *   - a context is bound to one device and is not thread-safe.
 *
 * Layout of the flat parameter-sized buffers (params, grads, Adam m, Adam v), fp32, in
 * state_dict order (nn/modeling.py:312-327):
 *   [ W_dec (d_sae x d_model, row-major) | b_dec (d_model) | W_enc (d_model x d_sae) | b_enc (d_sae) ]
 */
#ifndef SAEV_AMD_H
#define SAEV_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SAEV_AMD_ABI_VERSION 12

typedef enum {
    SAEV_OK = 0,
    SAEV_INVALID_ARG = -1,
    SAEV_HIP_ERROR = -2,
    SAEV_UNSUPPORTED = -3,
    SAEV_NOT_BOUND = -4,
    SAEV_RCCL_ERROR = -5,
    SAEV_STALE_PARAMS = -6, /* W_enc was written outside the library without saev_params_touched and a step has already run on
                              stale operand images (PARAMETER OWNERSHIP below); the context itself recovers */
    SAEV_ROW_OVERFLOW = -7  /* BatchTopK: a row of the forward has more codes than the context's row_cap.  Nothing was decoded, the
                               threshold was not updated, no step is in flight; saev_row_overflow_need gives the capacity that
                               holds every row -- create a context with at least that row_cap and repeat the forward */
} saev_status;

/* Static configuration of one SAE (nn/modeling.py:259-284 SparseAutoencoderConfig, :119-130 TopK,
 * :66-73 AuxK; nn/objectives.py:13-25 Matryoshka). */
typedef struct {
    int32_t d_model;
    int32_t d_sae;
    int32_t top_k;
    int32_t k_aux;                 /* 0 = no auxiliary loss (NoAux)                         */
    float alpha;                   /* AuxK scale                                            */
    int64_t dead_threshold_tokens; /* objectives.py:24                                      */
    int32_t normalize_w_dec;       /* modeling.py:283                                       */
    int32_t remove_parallel_grads; /* modeling.py:281                                       */
    int32_t max_batch;             /* scratch is sized for this many activation rows        */
    int32_t encoder_mode;          /* SAEV_ENCODER_F32, _F16X3, _BF16 or _F16R              */
    int32_t aux_dead_cap;          /* largest dead set the dense AuxK buffers are sized for at saev_create (no allocation
                                      happens inside a healthy step); 0 = min(d_sae, max(4096, 8 k_aux)) -- 4 096 dead latents are
                                      2.3 GB of buffers at configs[1], d_sae would be 11.5 GB (37 GB at configs[3]).  A step
                                      that meets more dead latents than this grows the buffers (twice the need, at most d_sae) after its
                                      read-back of the count -- a device-wide allocation, once; pass d_sae to rule it out.       */
    int32_t shard_world;           /* 0 / 1: the flat buffers are exactly the layout above.  N > 1: each half of it,
                                      [W_dec | b_dec] and [W_enc | b_enc], is padded with zeros to N equal chunks (chunks
                                      of the first half are whole decoder rows) so that N data-parallel ranks can
                                      reduce-scatter the gradient, run the tail on 1/N each and all-gather the parameters
                                      (saev_tail_prepare / saev_tail_apply); see saev_layout.                        */
    int32_t bound_mode;            /* TopK candidate bounds of the fused fp16-image encoders (top_k <= 32):
                                      0 guaranteed bounds only (running minimum over group maxima);
                                      1 predicted bounds first -- each row's bound is mean + z * sigma of its
                                        pre-activations over a sample of the latents -- verified by the select stage
                                        (the k-th largest candidate found must reach every bound used for the row),
                                        with an automatic second launch on guaranteed bounds whenever a prediction
                                        fails; codes and values are the same either way (saev_bound_state reports z
                                        and how often the second launch was needed);
                                      2 guaranteed bounds, except in the streamed f16r training step of a plain TopK context
                                        (saev_train_step on consecutive batches of one size): there a row's bound is
                                        c * rho_lo * ||x_b - mu||, rho_lo the smallest ratio (exact k-th largest
                                        pre-activation) / ||x_b - mu|| over the rows of the previous step and c a safety
                                        factor steered on the device, verified and repeated like mode 1.  A first step, a step
                                        after saev_params_touched, another batch size or any other forward in between takes
                                        the guaranteed bounds.                                                       */
    int32_t max_backward_rows;     /* 0 = max_batch.  Larger: the backward may cover that many rows (saev_backward_override:
                                      the rows of ALL data-parallel ranks); sizes only the backward's pair order, slice-major
                                      copies and partial rows -- the forward's buffers (candidate lists, dense fallback,
                                      AuxK, ...) stay at max_batch, which is then the LOCAL batch.                      */
    int32_t activation;            /* SAEV_ACT_TOPK (0), SAEV_ACT_RELU or SAEV_ACT_BATCHTOPK (BATCHTOPK below).  A ReLU context (nn/modeling.py:111-113 Relu, :150-156
                                      ReluActivation) ignores top_k and needs k_aux = 0.  Made by saev_create / saev_create_ex it
                                      runs the forward entries only: saev_encode_relu, saev_decode_rows, saev_scatter_rows and the
                                      single ops, while the step entries and saev_encode_topk return SAEV_UNSUPPORTED -- it
                                      allocates none of a step's scratch.  TRAINING a ReLU SAE takes a context kind of its own,
                                      made by saev_create_relu_train (RELU TRAINING below).                              */
} saev_cfg;

#define SAEV_ACT_TOPK 0
#define SAEV_ACT_RELU 1
#define SAEV_ACT_BATCHTOPK 2

/* Element offsets of the four tensors inside each flat buffer, its total length, and the per-rank chunk lengths of the
 * two halves (all in floats) for this configuration.  Without shard_world: off_W_dec 0, off_b_dec S*D, off_W_enc
 * S*D + D, off_b_enc 2*S*D + D, n_total 2*S*D + S + D. */
typedef struct {
    int64_t off_W_dec, off_b_dec, off_W_enc, off_b_enc, n_total, chunk_a, chunk_b;
} saev_layout_t;
int saev_layout(const saev_cfg* cfg, saev_layout_t* out);

/* Encoder arithmetic.  F32, F16X3 and F16R are fp32-accurate (error vs fp64 at the level of a native fp32 GEMM):
 *   F32   : v_mfma_f32_32x32x2_f32, exact fp32 products;
 *   F16X3 : operands split into fp16 hi+lo (22 significand bits), three v_mfma_f32_32x32x16_f16 per
 *           product pair, fp32 accumulate -- 16/3 of the F32 matrix rate;
 *   BF16  : x and W_enc rounded to bf16 (nearest even) for the encoder contraction only, one
 *           v_mfma_f32_32x32x16_bf16 per product, fp32 accumulate; bias, TopK, decode, losses, all
 *           gradients and Adam stay fp32 on the fp32 master weights (BASELINE.json configs[3]). */
#define SAEV_ENCODER_F32 0
#define SAEV_ENCODER_F16X3 1
#define SAEV_ENCODER_BF16 2
/*   F16R  : one v_mfma_f32_16x16x32_f16 per product on fp16-rounded operands as a FIRST PASS, run on activations
 *           centred on the batch mean (the bias absorbs mean * W_enc) and pre-scaled by device-side powers of two.  Its
 *           error is bounded per row b from the rounding errors the images ACTUALLY carry (their norms are measured by
 *           the passes that write the images), by Cauchy-Schwarz:
 *             E_b = 1.02 (||dx_b|| wmax + ||x_b - mean|| dwmax + ||dx_b|| dwmax)
 *                   + (1.05 d_model 2^-22 + 2^-17) ||x_b - mean|| wmax + sqrt(d_model) 2^-14 wmax / scale_x + 2^-23 max |bias|,
 *           wmax / dwmax = the largest column norm of W_enc / of its rounding error (select.hip: f16r_margin).
 *           Candidates are kept down to the running bound minus 2 E_b, and the select stage recomputes every
 *           survivor exactly in fp32 (dot product of the uncentred row with the fp32 encoder column + b_enc) before the
 *           final cut.  Codes and values are those of exact fp32 arithmetic; a dense h (saev_encode_dense, overflow
 *           route) always comes from the exact fp32 kernel.  Default of the Python host. */
#define SAEV_ENCODER_F16R 3

/* Scalars of one step (nn/objectives.py:57-89 MatryoshkaLoss + train.py:356-362 grad norm). */
typedef struct {
    float mse;
    float aux;
    float l0;
    float l1;
    float grad_norm; /* pre-clip global L2 norm                                             */
    float upper;     /* max |x| of the batch (objectives.py:227)                            */
    int32_t n_dead;
    int32_t n_overflow_rows; /* rows whose candidate list overflowed (step re-ran on the exact dense route) */
    int32_t cand_max;        /* longest per-row candidate list the fused encoder produced              */
    int32_t dense_route;     /* 1 when the step's codes came from the exact dense route (candidate-list or refinement
                                overflow, or k > 64), 0 when the fused route held                       */
    double sse;      /* sum (x - x_hat)^2 accumulated in fp64 (train.py:398-401, :561-562)  */
    double sum_sq;   /* sum x^2 in fp64 (train.py:383, :554)                                */
} saev_step_stats;

typedef struct saev_ctx saev_ctx;

/* Route switches for A/B measurements and for tests that must reach a particular kernel.  Every field 0 = the shipped
 * default; results are the same on every route (tests/test_gpu_parity.py, tests/test_gpu_dw_slices.py compare them).
 * The library itself reads no environment variable: the Python host maps its documented SAEV_AMD_* variables onto this
 * struct (saev_amd/engine.py: EngineConfig). */
typedef struct {
    int32_t struct_size;   /* sizeof(saev_debug_cfg) of the caller (fields past it read as 0)                            */
    int32_t dw_route;      /* weight gradients: 0 column slices out of the XCD L2s where the geometry allows, with the products
                              dval = <dL/dx_hat row, decoder row> left by the decode where the shape allows (top_k <= 32,
                              d_model 256 / 512 / 768 / 1024); 1 whole-row gathers (dw_rows) always; 2 column slices with dval
                              formed by their first pass (the only form for other shapes and for gathered backwards)              */
    int32_t aux_small_max; /* largest dead set the few-dead-latents AuxK kernels take: 0 = 128 where d_model % 128 == 0 (fp32-MFMA kernels; 64 with aux_wide_route = 1), else 40; -1 = never (dense algebra
                              whatever the count); values above 64 are clamped                                           */
    int32_t fwd_route;     /* exact refinement of the f16r encoder: 0 = from 32-column slices of W_enc^T that the XCD L2s hold
                              where the geometry allows (their D / 32 shares per survivor added by the final select), 1 = whole-row
                              gathers always                                                                              */
    int32_t csc_route;     /* latent-major pair list of the backward: 0 = the training decode sets the (latent, row) bits of the
                              build's bit map while it holds the codes, 1 = the build's own fill pass always, 2 = as 0 with the
                              round-4 scan (two launches) instead of the single look-back scan                               */
    int32_t fin_route;     /* end of the column-slice backward: 0 = one launch; the projection coefficient comes from the pair lists
                              (<dW_dec[i], w_i> = sum val * dval) and ||w||^2 from normalize_rows, the decoder rows are not read,
                              1 = the round-4 kernels (dw_finalize, dw_finalize_cut, dw_clear_bitmap: three launches, every
                              gradient and decoder row read back)                                                           */
    int32_t prep_route;    /* f16r forward preparation: 0 = streamed where possible (one pass over x centred / scaled with what the
                              previous batch left, W_enc images left by the previous step's Adam), 1 = the full preparation on
                              every step (statistics, centring and both image passes from x and W_enc: the round-4 sequence)    */
    int32_t aux_dense_route; /* selection of the dense AuxK algebra: 0 = one launch leaves the code matrix, its mask, its maximum and its
                              operand scale (dead sets up to 4 096 columns), 1 = the round-4 sequence (radix select, two fills, scatter,
                              absmax, scale: six launches)                                                                    */
    int32_t aux_small_route; /* 9 ... 64 dead latents (and 1 ... 8 where the one-pass kernel does not take the shape), d_model % 128 == 0:
                              0 = the contractions as fp32 MFMA tiles (v_mfma_f32_32x32x2_f32), 1 = the vector-ALU kernels of rounds 3-4 */
    int32_t group_route;   /* several SAEs on the same batches (saev_share_x): 0 = the lender streams its preparation like a context on
                              its own and every member's fused Adam leaves its own W_enc images (from the third step of a group nobody
                              prepares anything from scratch), 1 = round 5: every member prepares from scratch on every step        */
    int32_t aux_split_route; /* dense AuxK route, operand images of the split-fp16 contractions: 0 = the codes, g_aux, x and the dead latents'
                              decoder rows written in BOTH operand forms by one pass each (six image launches), 1 = round 5: one launch
                              per form (ten)                                                                                  */
    int32_t aux_wide_route; /* few-dead-latents AuxK on the fp32 matrix cores: 0 = dead sets bounded by up to 128 (one launch per count window
                              [1, 32], [33, 64], [65, 128], the device-side count picks), 1 = round 5: up to 64, the dense algebra beyond */
} saev_debug_cfg;

int saev_abi_version(void);
const char* saev_last_error(const saev_ctx* ctx);

/* Lifetime.  `device` is the HIP device ordinal. */
int saev_create(const saev_cfg* cfg, int device, saev_ctx** out);
/* The same with route switches (dbg may be NULL = all defaults). */
int saev_create_ex(const saev_cfg* cfg, const saev_debug_cfg* dbg, int device, saev_ctx** out);
void saev_destroy(saev_ctx* ctx);

/* BATCHTOPK (nn/modeling.py:132-140 BatchTopK, :183-244 BatchTopKActivation; nn/objectives.py:101-156).  saev_cfg.activation =
 * SAEV_ACT_BATCHTOPK; saev_cfg.top_k keeps its meaning, codes per row ON AVERAGE.  For h = x W_enc + b_enc of shape (n, S):
 *   training   the T = min(top_k n, S n) largest entries of the flattened h by signed value are kept (negative and zero values too
 *              when they are among the largest), f = h there and 0 elsewhere.  Ties at the cut are deterministic: among entries
 *              EQUAL to the cut value, lower flat index (row-major) first (the reference's are unspecified).  Then
 *              threshold <- (1 - momentum) threshold + momentum min{f : f > 0}, on every training-mode encode as in the reference;
 *              a batch without a positive kept value leaves the threshold as it is (the reference raises there)
 *   eval       f = h where h > threshold (h > 0 when threshold <= 0), elementwise; the threshold does not move
 *   gradient   df/dh is the mask; the threshold carries none.  l0 counts f != 0, the dead-latent tracker |f| > 0; AuxK, Matryoshka
 *              prefixes, the MSE rescale, remove_parallel_grads, the clip, Adam / Muon and renormalisation as for TopK.
 * Codes are PADDED ROWS as for ReLU: idx / val (n x row_cap), row b's entries in its first row_nnz[b] slots in ascending latent
 * order, the other slots idx = -1, val = 0.  row_cap is fixed per context (saev_batch_topk_cfg.row_cap; 0 = min(d_sae, max(64,
 * 4 top_k)) rounded up to 64) and sizes everything a TopK context sizes by top_k.  OVERFLOW IS NEVER SILENT: a forward one of whose rows
 * needs more slots returns SAEV_ROW_OVERFLOW before anything is decoded (and before the threshold moves, so a repeated training
 * forward applies the update once); the forward reads one device word back per call to know (4 bytes, one synchronisation of the
 * stream -- an open lever).  The count reported is taken BEFORE the tie rule drops cut-valued entries, so a batch with many ties at
 * the cut may ask for more than its final rows hold.
 * The select is exact (integer keys and counts, no floating-point atomics) and works on the dense h that the exact fp32 encoder
 * writes (as saev_encode_dense); encoder_mode BF16 is SAEV_UNSUPPORTED.  On such a context saev_step_forward / _dead / _backward /
 * _tail, saev_muon_tail and saev_train_step (= the four phases back to back) run; saev_encode_topk, saev_encode_relu,
 * saev_share_x (either side), saev_train_step_gather, saev_train_step_dp, saev_backward_override, saev_copy_step_state and a
 * backward over part of the latents return SAEV_UNSUPPORTED (a batch-wide top-k over several ranks needs a distributed select). */
typedef struct {
    int32_t struct_size;   /* sizeof(saev_batch_topk_cfg) of the caller (fields past it read as 0)                          */
    int32_t row_cap;       /* slots per padded code row; 0 = the default above                                              */
    double batch_momentum; /* EMA weight m of the threshold update (modeling.py:139), a double as the reference's Python float is:
                              the kernel multiplies by float(1 - m) and float(m) as torch's mul_ / add_ do.  The default
                              without this struct is 0.1                                                                    */
    int32_t list_cap;      /* 0 = default.  Route switch for tests: capacity of the select's key list (a cut bin with more
                              entries sends the select's later levels over h again; same result)                          */
    int32_t reserved;
} saev_batch_topk_cfg;
/* saev_create_ex for a BatchTopK context with its own settings (bt NULL: the defaults, as saev_create_ex gives them). */
int saev_create_batch_topk(const saev_cfg* cfg, const saev_debug_cfg* dbg, const saev_batch_topk_cfg* bt, int device, saev_ctx** out);
/* The threshold word (one device float, 0 at creation) is owned by the context unless the caller binds its own -- a torch buffer
 * that aliases it, like the tracker (the value is NOT copied: seed the caller's word first). */
int saev_bind_threshold(saev_ctx* ctx, float* threshold);
float* saev_threshold_device(saev_ctx* ctx);
int32_t saev_row_cap(const saev_ctx* ctx);             /* 0 unless BatchTopK */
int32_t saev_row_overflow_need(const saev_ctx* ctx);   /* after SAEV_ROW_OVERFLOW: the largest row count met */
/* The activation alone on a dense h (n x d_sae, 16-byte aligned, n <= max_batch) the caller holds: select + compaction (training != 0,
 * threshold update included) or the threshold compaction, into idx_out / val_out (n x row_cap of the context) and row_nnz_out (n,
 * exact also past row_cap).  *overflow_out (device int32) = 0, or the largest row count when that exceeds row_cap: the caller reads
 * it back, as after saev_encode_relu; the threshold moves only when it is 0. */
int saev_batch_topk_dense(saev_ctx* ctx, const float* h, int32_t n_rows, int32_t training, int32_t* row_nnz_out, int32_t* idx_out,
                          float* val_out, int32_t* overflow_out, void* stream);
/* modeling.py:343-347 encode + the activation, for encode / encode_sparse: the same on h = x W_enc + b_enc (exact fp32). */
int saev_encode_batch_topk(saev_ctx* ctx, const float* x, int32_t n_rows, int32_t training, int32_t* row_nnz_out, int32_t* idx_out,
                           float* val_out, int32_t* overflow_out, void* stream);
/* What the last training-mode select left on the device, read back (synchronises `stream`): the cut value, the number of entries
 * strictly above it, how many entries equal to it are kept (>= 1) and how many entries equal it. */
int saev_batch_topk_state(saev_ctx* ctx, float* cut, int64_t* n_above, int64_t* tie_quota, int64_t* n_ties, void* stream);
/* row_nnz (n_rows int32) of the last saev_step_forward of a BatchTopK context, copied like saev_copy_last copies the padded rows
 * (idx / val there are n_rows x row_cap). */
int saev_copy_last_row_nnz(saev_ctx* ctx, int32_t n_rows, int32_t* row_nnz_out, void* stream);

/* RELU TRAINING (nn/modeling.py:109-117 Relu, :150-156 ReluActivation; nn/objectives.py:101-156 with L1Sparsity / NoSparsity):
 * a dense step on the matrix cores.  For h = x W_enc + b_enc (n x S), f = max(h, 0), x_hat = f W_dec + b_dec:
 *     loss = mse(x_hat, x) + l1_coeff * mean_b sum_s f[b, s]          (the rescaled mse of objectives.py:224-237, mean over n D)
 * With b_enc = 0 about half of the latents fire in every row, so the codes are not sparse and the step is four dense contractions
 * whose cost does not depend on the density: x_hat = f W_dec, dA = g W_dec^T, dW_dec = f^T g, dW_enc = x^T dH with
 * g = dL/dx_hat and dH = (dA + l1_coeff / n) where f > 0, else 0 -- all on the split-fp16 MFMA kernel (fp32-accurate), h from the
 * context's exact dense encoder (as saev_encode_dense).  Every sum has a fixed order: the same inputs give the same bits.
 * saev_create_relu_train makes the context: cfg->activation must be SAEV_ACT_RELU and cfg->k_aux 0 (anything else is
 * SAEV_INVALID_ARG, before the device is touched); encoder_mode BF16 and shard_world > 1 are SAEV_UNSUPPORTED.  It serves what a
 * forward-only ReLU context serves (saev_encode_relu, saev_decode_rows, saev_scatter_rows, the single ops) and saev_step_forward /
 * _dead / _backward / _tail, saev_muon_tail and saev_train_step (= the four phases back to back).  saev_step_stats: mse, l0 (mean
 * count of f > 0 per row), l1 (mean sum of f per row), sse, sum_sq, upper, n_dead, grad_norm; aux = 0, saev_last_aux_route = 0.
 * TWO LIMITS.  (1) The plain objective only: saev_set_prefixes with more than one prefix is SAEV_UNSUPPORTED (nested prefixes over
 * dense contractions are one contraction per prefix block -- a piece of work of its own).  (2) One GPU, one piece: n_rows_global
 * must equal n_rows; saev_train_step_dp, saev_train_step_gather, saev_share_x (either side), saev_backward_begin / _rows / _end
 * (the backward runs whole: saev_step_backward), saev_backward_override and saev_copy_step_state are SAEV_UNSUPPORTED.
 * saev_last_idx / _val mean nothing on such a context (its codes are the dense f): saev_copy_last_rows compacts them. */
typedef struct {
    int32_t struct_size;   /* sizeof(saev_relu_train_cfg) of the caller (fields past it read as 0)                           */
    int32_t reserved;
    double l1_coeff;       /* L1Sparsity.coeff as the reference's Python float (0: NoSparsity); the kernels use float(l1_coeff / n) */
} saev_relu_train_cfg;
/* rt NULL: l1_coeff = 0 */
int saev_create_relu_train(const saev_cfg* cfg, const saev_debug_cfg* dbg, const saev_relu_train_cfg* rt, int device, saev_ctx** out);
/* The codes of the last saev_step_forward of a ReLU training context as PADDED ROWS, compacted from its dense f into the caller's
 * buffers: idx_out / val_out (n_rows x row_cap), row b's entries (f > 0) in its first row_nnz_out[b] slots in ascending latent
 * order, the other slots idx = -1, val = 0.  row_nnz_out[b] is exact also past row_cap; *overflow_out (a device int32) = 0 when
 * every row fit, else the largest count -- the caller reads it back and repeats the call with row_cap >= that count, as after
 * saev_encode_relu (a row is never silently truncated).  n_rows must equal the batch of that forward. */
int saev_copy_last_rows(saev_ctx* ctx, int32_t n_rows, int32_t row_cap, int32_t* row_nnz_out, int32_t* idx_out, float* val_out,
                        int32_t* overflow_out, void* stream);

/* Borrow the caller's flat buffers (see layout above).  grads/adam_m/adam_v may be NULL for a
 * forward-only context.  Pointers must stay valid until re-bound or destroy. */
int saev_bind(saev_ctx* ctx, float* params, float* grads, float* adam_m, float* adam_v);

/* Dead-latent tracker state, (d_sae) int64, owned by the context (objectives.py:99,107-120).
 * Exposed so the host can read/seed it (it is not part of the checkpoint in the reference). */
int64_t* saev_toks_since_active(saev_ctx* ctx);
/* Per-latent "fired this step" flags, (d_sae) int32 0/1; in data-parallel runs the host
 * max-all-reduces this buffer between saev_step_forward and saev_step_dead. */
int32_t* saev_fired_flags(saev_ctx* ctx);
/* Let the host own the tracker state instead (both buffers d_sae long, zero-initialised by the
 * caller): lets a torch tensor alias them for all-reduce / inspection. */
int saev_bind_tracker(saev_ctx* ctx, int64_t* toks_since_active, int32_t* fired_flags);
/* Tell the context that the host wrote the tracker buffer (so dead latents may exist before
 * dead_threshold_tokens tokens have been processed). */
int saev_tracker_touched(saev_ctx* ctx);
/* Device copy of the current step's saev_step_stats (valid after the producing call completes). */
const saev_step_stats* saev_stats_device(saev_ctx* ctx);
/* Blocking read-back of the stats (synchronises `stream`). */
int saev_read_stats(saev_ctx* ctx, saev_step_stats* out_host, void* stream);

/* ---- single ops (API-compat surface of SparseAutoencoder) ---------------------------------- */

/* modeling.py:411-417  W_dec[i,:] /= ||W_dec[i,:]||  (no-op when cfg.normalize_w_dec == 0). */
int saev_normalize_w_dec(saev_ctx* ctx, void* stream);
/* modeling.py:343-347  h = x @ W_enc + b_enc, dense (n_rows x d_sae) output. */
int saev_encode_dense(saev_ctx* ctx, const float* x, int32_t n_rows, float* h_out, void* stream);
/* modeling.py:169-179  per-row top-k of a dense (n_rows x d_sae) matrix -> idx/val (n_rows x k), each row in ascending latent
 * order.  `mask` (d_sae int32, may be NULL) restricts candidates to latents with mask != 0 (any non-zero word).  A mask that
 * leaves e < k eligible latents gives those e codes followed by k - e slots of idx = -1, val = 0.
 * The order is a total order on the bit patterns: key = bits ^ 0xFFFFFFFF if the sign bit is set, else bits | 0x80000000; the
 * larger key wins and equal keys go to the lower latent index.  So +NaN is above +inf, a NaN with the sign bit set is below
 * -inf, and -0.0 < +0.0.  Values are emitted with their bits unchanged.  1 <= k <= d_sae. */
int saev_topk_dense(saev_ctx* ctx, const float* h, int32_t n_rows, int32_t k, const int32_t* mask,
                    int32_t* idx_out, float* val_out, void* stream);
/* encode + TopK without materialising h (the fast path): idx/val (n_rows x top_k). */
int saev_encode_topk(saev_ctx* ctx, const float* x, int32_t n_rows, int32_t* idx_out, float* val_out,
                     void* stream);
/* scatter codes into a dense zero-initialised (n_rows x d_sae) matrix (f_x for API compat). */
int saev_scatter_dense(saev_ctx* ctx, const int32_t* idx, const float* val, int32_t n_rows, int32_t k,
                       float* f_out, void* stream);
/* modeling.py:351-409 with sparse input: x_hat[b, p, :] = b_dec + sum_{j: idx < prefixes[p]} val*W_dec[idx].
 * `prefixes_host` has n_prefixes ascending cut points ending at d_sae (NULL => one prefix). */
int saev_decode_sparse(saev_ctx* ctx, const int32_t* idx, const float* val, int32_t n_rows, int32_t k,
                       const int64_t* prefixes_host, int32_t n_prefixes, float* x_hats_out, void* stream);
/* ---- ReLU SAE forward (variable-length rows) ------------------------------------------------
 * A ReLU code row has no fixed length.  Rows are PADDED: idx (n_rows x row_cap) int32 and val (n_rows x row_cap) fp32 hold
 * row b's entries in their first row_nnz[b] slots, in ascending latent order (the CSR-block order framework/inference.py
 * relies on); slots past row_nnz[b] are unspecified. */
/* modeling.py:343-347 encode + :150-156 ReluActivation: f = relu(x @ W_enc + b_enc) without a dense h.  row_nnz_out[b] is the
 * EXACT number of positives of row b, also when it exceeds row_cap; only the first row_cap entries of such a row are stored and
 * *overflow_out (a device int32) receives the largest count: 0 when every row fit, else > row_cap -- the caller reads it back
 * and repeats the call with row_cap >= that count (a row is never silently truncated).  Arithmetic: exact fp32 products and
 * sums in every fp32-accurate encoder mode (F32, F16X3, F16R); BF16 returns SAEV_UNSUPPORTED.  The entries past row_nnz of
 * a padded row are not touched.  Needs a context with activation = SAEV_ACT_RELU. */
int saev_encode_relu(saev_ctx* ctx, const float* x, int32_t n_rows, int32_t row_cap, int32_t* row_nnz_out, int32_t* idx_out,
                     float* val_out, int32_t* overflow_out, void* stream);
/* modeling.py:351-409 on padded rows: x_hat[b, p, :] = b_dec + sum_{j < row_nnz[b], idx < prefixes[p]} val * W_dec[idx]; the
 * cost grows with row_nnz, not with row_cap (a row_nnz above row_cap reads as row_cap).  With n_prefixes > 1 (at most 16,
 * ascending, ending at d_sae) the entries of each row must be in ascending latent order, as saev_encode_relu writes them.
 * x_hats_out is (n_rows, n_prefixes, d_model).  Any activation. */
int saev_decode_rows(saev_ctx* ctx, const int32_t* idx, const float* val, const int32_t* row_nnz, int32_t row_cap,
                     int32_t n_rows, const int64_t* prefixes_host, int32_t n_prefixes, float* x_hats_out, void* stream);
/* saev_scatter_dense for padded rows: f_out[b, idx] = val for the first min(row_nnz[b], row_cap) entries of each row, into a
 * zero-initialised (n_rows x d_sae) matrix (dense f_x for API compatibility). */
int saev_scatter_rows(saev_ctx* ctx, const int32_t* idx, const float* val, const int32_t* row_nnz, int32_t row_cap,
                      int32_t n_rows, float* f_out, void* stream);
/* modeling.py:419-445 on the bound grad buffer. */
int saev_remove_parallel_grads(saev_ctx* ctx, void* stream);
/* Row gather out of a device-resident activation pool (replaces ReservoirBuffer.get,
 * data/buffers.py:179-216): out[r,:] = pool[rows[r],:]. */
int saev_gather_rows(saev_ctx* ctx, const float* pool, const int64_t* rows, int32_t n_rows, float* out,
                     void* stream);

/* ---- the train step, in phases (framework/train.py:332-460) --------------------------------- */

/* Matryoshka prefix cut points for the following steps (objectives.py:125-138): n ascending latent counts ending at
 * d_sae, n <= 16; the loss is the mean over all n nested reconstructions.  NULL / n = 1 restores the plain
 * objective.  (The host samples them per step: objectives.py:159-201.) */
int saev_set_prefixes(saev_ctx* ctx, const int64_t* prefixes_host, int32_t n);

/* Several SAEs trained on the same batches (the reference's answer to an I/O-bound loop: one batch feeds every SAE of
 * a parallel group, train.py:3, :334-348): everything a step derives from x alone -- max|x| of the MSE rescale, the
 * column means the f16r encoder centres on, the centred row norms behind its error margins, the power-of-two x scale
 * and the fp16 / bf16 operand images -- is built once, by `leader`, and read by every context that shares with it.
 * A saev_step_forward of `ctx` borrows them when `leader`'s last saev_step_forward was given the same x pointer and
 * row count and nothing has borrowed-or-rebuilt in between; otherwise it builds its own, so results never depend on
 * the sharing.  Same device, d_model and encoder mode; both contexts on one stream (or ordered by the caller); the
 * leader must outlive the link.  leader = NULL detaches. */
int saev_share_x(saev_ctx* ctx, saev_ctx* leader);

/* Phase 1: renormalise W_dec (train.py:334-335), encode + TopK, fired flags, sparse decode, MSE,
 * main-path gradient pieces.  `training` = 0 gives the eval-mode forward (no tracker, no aux).
 * `n_rows_global` = rows of this step summed over all data-parallel ranks (= n_rows on one GPU);
 * it must equal the value later passed to saev_step_dead. */
int saev_step_forward(saev_ctx* ctx, const float* x, int32_t n_rows, int64_t n_rows_global, int32_t training,
                      void* stream);
/* Phase 2: tracker update with `n_rows_global` tokens (objectives.py:118-120), dead mask, AuxK
 * forward (modeling.py:75-103).  Training mode only.  The reference reads n_dead back on every step
 * (`.item()`, modeling.py:92).  Here the update kernel leaves a record in pinned host memory each step; the
 * call looks at the record of four steps earlier, which bounds the current count from above, and while that
 * bound is <= min(128, k_aux) (fp32 matrix-core kernels, d_model % 128 == 0: one launch per count window, saev_debug_cfg.aux_wide_route; 40 for other widths;
 * saev_debug_cfg.aux_small_max) -- zero dead latents included -- it enqueues kernels that take the count from
 * the device: no read-back, no stream synchronisation.  Only when the bound is larger (or no valid record
 * exists yet: the first four steps after creation / saev_bind_tracker / saev_tracker_touched) does it read
 * n_dead back and size the dense AuxK algebra on the host.  saev_last_aux_route tells which happened:
 * 0 no auxiliary work, 1 few-dead-latents kernels without a read-back, 2 the same after a read-back,
 * 3 dense algebra after a read-back; saev_dead_readbacks counts the read-backs so far. */
int saev_step_dead(saev_ctx* ctx, int64_t n_rows_global, void* stream);
int saev_last_aux_route(const saev_ctx* ctx);
/* Device memory the context itself owns, in bytes (the four flat buffers belong to the caller): which = 0 everything,
 * 1 the AuxK dead-set buffers (sized by saev_cfg.aux_dead_cap), 2 the Matryoshka gradient blocks (saev_set_prefixes),
 * 3 the Muon workspace (allocated by the first saev_muon_tail, saev_muon_workspace_bytes(d_model, d_sae)). */
int64_t saev_scratch_bytes(const saev_ctx* ctx, int32_t which);
int64_t saev_dead_readbacks(const saev_ctx* ctx);
/* Phase 3: all four parameter gradients into the bound grad buffer (replaces autograd,
 * train.py:347-348), un-projected and un-clipped. */
int saev_step_backward(saev_ctx* ctx, void* stream);
/* Phase 3 in pieces, for data-parallel runs that overlap the gradient exchange with the backward:
 *   saev_backward_begin   latent-major ordering of the codes, db_dec, the AuxK contractions;
 *   saev_backward_rows    rows [lat_lo, lat_hi) of dW_dec (in the bound gradient buffer), of the TRANSPOSED W_enc
 *                         gradient (saev_grad_w_enc_t: (d_sae, d_model) row-major) and entries [lat_lo, lat_hi) of db_enc
 *                         are final when it returns (in stream order) -- the host may start reducing them;
 *   saev_backward_end     transposes saev_grad_w_enc_t (after the host has reduced it) into the W_enc segment.
 * saev_step_backward == begin + rows(0, d_sae) + end.  saev_bind_w_enc_t lets the host own the transposed-gradient
 * scratch ((d_sae * d_model) floats) so that a torch tensor can alias it for the collectives; the f16r encoder also
 * uses it as W_enc^T scratch during the forward. */
int saev_backward_begin(saev_ctx* ctx, void* stream);
int saev_backward_rows(saev_ctx* ctx, int32_t lat_lo, int32_t lat_hi, void* stream);
/* The same in two passes over the latents' (row, latent) pairs: part 1 forms the decoder gradient (rows of dL/dx_hat) and
 * keeps the per-pair dot products, part 2 the encoder gradient and db_enc (rows of x).  part 0 = saev_backward_rows.  A
 * data-parallel caller runs part 1, starts the exchange of the decoder half [W_dec | b_dec] -- final at that point -- and
 * lets it travel while part 2 and saev_backward_end run.  Both parts must cover the same latent ranges before
 * saev_backward_end. */
int saev_backward_rows_part(saev_ctx* ctx, int32_t lat_lo, int32_t lat_hi, int32_t part, void* stream);
int saev_backward_end(saev_ctx* ctx, void* stream);
/* Gathered backward -- the low-traffic exchange for strong scaling ("all-gather the sparse step state"; the
 * reference has no distributed training, framework/train.py:760-769).  Instead of summing the 4 N_p-byte gradient over
 * the ranks, every rank all-gathers what the backward consumes -- x, dL/dx_hat, the codes: (8 D + 8 k) bytes per row --
 * and forms the FULL gradient of the global batch itself, redundantly and bit-identically on every rank:
 *   saev_copy_step_state     this rank's rows of dL/dx_hat and of the codes into caller buffers (the rank's slice of the
 *                            all-gather outputs); n_rows = the rows of the training forward in flight.  With P Matryoshka
 *                            prefixes dL/dx_hat is the (n_rows, P, d_model) block of suffix-summed gradients;
 *   saev_backward_override   the gathered buffers (n_all <= max_batch rows of all ranks, rank-major) for the NEXT
 *                            saev_backward_begin / _rows: pairs, db_dec and both weight gradients then cover all n_all
 *                            rows.  One-shot (the next forward cancels it); NULL cancels.  Matryoshka: g_all is
 *                            (n_all, P, d_model) and every rank must have set the same cut points.
 * The auxiliary loss stays local to a rank's rows; its gradient is a few rows: saev_aux_compact_rows rows of
 * [dW_dec | dW_enc^T] for the dead latents, their db_enc and the term's share of db_dec.  Between saev_backward_begin and
 * saev_backward_rows the caller exports them (rows * (2 d_model + 1) + d_model floats), sums over ranks, imports:
 *   saev_aux_compact_rows / _export / _import.
 * Gradients carry the local 1/(n_local d_model) factor as in every data-parallel mode: tail with grad_scale = 1/world.
 * saev_trust_gradients(1) lets saev_step_tail use what the backward left behind (row statistics, tile squares) as
 * saev_train_step does -- the caller vouches that nothing writes the gradient between saev_backward_end and the tail.
 * All of this follows saev_step_forward: the forward inside saev_train_step keeps dL/dx_hat in the column-slice layout its own
 * backward reads and writes no row-major copy, so g_out and a ranged backward behind it are SAEV_INVALID_ARG. */
int saev_copy_step_state(saev_ctx* ctx, int32_t n_rows, float* g_out, int32_t* idx_out, float* val_out, void* stream);
int saev_backward_override(saev_ctx* ctx, const float* x_all, const float* g_all, const int32_t* idx_all,
                           const float* val_all, int32_t n_all);
int32_t saev_aux_compact_rows(const saev_ctx* ctx);
int saev_aux_compact_export(saev_ctx* ctx, float* buf, void* stream);
int saev_aux_compact_import(saev_ctx* ctx, const float* buf, void* stream);
int saev_trust_gradients(saev_ctx* ctx, int32_t on);
float* saev_grad_w_enc_t(saev_ctx* ctx);
int saev_bind_w_enc_t(saev_ctx* ctx, float* scratch);
/* Phase 4: grads *= grad_scale (1/world_size after a sum all-reduce), remove_parallel_grads
 * (train.py:351-352), global-norm clip (train.py:356-362; torch's formula for max_norm >= 0, so 0 zeroes the
 * gradient as in the reference; max_norm < 0 disables clipping), Adam with torch
 * defaults (train.py:294,444-446). `adam_step` is the 1-based step count. */
int saev_step_tail(saev_ctx* ctx, float lr, float max_norm, float grad_scale, int64_t adam_step, void* stream);
/* Phase 4 in two parts, over everything (shard_rank < 0: saev_step_tail == prepare + apply) or over rank
 * `shard_rank`'s chunk of each half of the flat buffers (saev_cfg.shard_world ranks; the gradient chunks must hold the
 * cross-rank SUM, e.g. after a reduce-scatter):
 *   saev_tail_prepare  remove_parallel_grads on the decoder rows of the range and the sum of squares of the range's
 *                      (projected, unscaled) gradient into saev_sumsq_device -- the caller all-reduces that one double
 *                      (SUM) when the ranges are per-rank, so that every rank clips with the same global norm;
 *   saev_tail_apply    clip coefficient from that sum, Adam on the range.
 * saev_bind_sumsq hands the context a caller-owned device double (a torch tensor a collective can run on). */
int saev_tail_prepare(saev_ctx* ctx, int32_t shard_rank, void* stream);
int saev_tail_apply(saev_ctx* ctx, float lr, float max_norm, float grad_scale, int64_t adam_step, int32_t shard_rank,
                    void* stream);
double* saev_sumsq_device(saev_ctx* ctx);
int saev_bind_sumsq(saev_ctx* ctx, double* sumsq);
/* One-shot: the next saev_step_forward waits for this hipEvent_t (on its stream) before it first touches W_dec, and
 * renormalises W_dec there instead of at its top -- for a caller whose decoder half of the parameter all-gather is
 * still running on another stream.  NULL cancels. */
int saev_wdec_ready_event(saev_ctx* ctx, void* event);
/* One-shot, the encoder half's counterpart: the next forward (saev_step_forward / saev_encode_topk) enqueues what depends
 * on the batch alone -- statistics, centring, fp16 images of x -- and waits for this hipEvent_t only before it first reads
 * W_enc or b_enc.  NULL cancels. */
int saev_wenc_ready_event(saev_ctx* ctx, void* event);

/* Phases 1-4 back to back for the single-GPU case -- with one difference to calling the four phases: the gradient
 * buffer is NOT a valid gradient afterwards.  The W_enc gradient stays in the transposed scratch (saev_grad_w_enc_t) and
 * is consumed there by the step's single Adam launch, and the rows of dW_dec are stored un-projected (the projection of
 * remove_parallel_grads is applied inside Adam as the rows are read).  Callers that want to look at gradients -- the log
 * steps of train() do -- run the phases: saev_step_backward ends with saev_backward_end, saev_step_tail projects in place. */
int saev_train_step(saev_ctx* ctx, const float* x, int32_t n_rows, float lr, float max_norm,
                    int64_t adam_step, void* stream);
/* The same with the batch drawn from an activation pool inside the step: row r of the batch is pool row rows[r] (the reference's
 * reservoir draw, data/buffers.py:201-211 + the loader's batch assembly, data/shuffled.py:506-552).  x_out (n_rows, d_model)
 * receives the batch as a contiguous matrix -- the first kernel of the step writes it while it reads the rows, so the draw costs
 * no pass of its own; it stays valid until the next call and is what saev_copy_last / the log block read as "x". */
int saev_train_step_gather(saev_ctx* ctx, const float* pool, const int64_t* rows, float* x_out, int32_t n_rows, float lr,
                           float max_norm, int64_t adam_step, void* stream);
/* DATA PARALLEL behind the ABI (SURVEY 8b "DDP": absent in the reference, whose train.py:760-769 has no distributed code at all).
 * One process per GPU, one context per process.  saev_comm_unique_id fills 128 bytes on one rank (ncclGetUniqueId); the caller
 * hands them to every rank by whatever means it has (torchrun's store, MPI, a file) and each rank calls saev_comm_init with its
 * rank and the world size (ncclCommInitRank over xGMI).  RCCL is taken from the process at run time (the librccl the process
 * has already loaded -- torch's, in the Python host -- else the system's): libsaev_amd.so does not link against it, and without
 * it these entry points return SAEV_UNSUPPORTED.
 * saev_train_step_dp is saev_train_step for a batch that is split evenly over the ranks: x_local holds this rank's n_local
 * rows, the global batch is n_local * world rows.  Enqueued on `stream`, nothing read back:
 *     forward on the local rows (the loss terms divide by the global row count)
 *     all-reduce MAX of the "fired this step" flags      (d_sae int32: the dead-latent tracker counts the global batch)
 *     dead-latent update and the auxiliary term, backward on the local rows
 *     all-reduce SUM of the flat gradient buffer        (n_params fp32, one collective)
 *     projection, clip on the global norm, Adam, with the gradient scaled by 1 / world (the mean over ranks of per-rank means)
 * -- the sequence framework/ddp.py runs from Python with tail="replicated", exchange="dense" (the sharded tail and the sparse
 * exchange exist there only).  Parameters must be identical on all ranks when the first step starts (broadcast them, or create
 * every rank from the same seed); they stay identical because every rank applies the same update. */
int saev_comm_unique_id(void* id128);
int saev_comm_init(saev_ctx* ctx, const void* id128, int32_t rank, int32_t world);
int saev_comm_world(const saev_ctx* ctx);   /* 0: no communicator */
int saev_comm_destroy(saev_ctx* ctx);
int saev_train_step_dp(saev_ctx* ctx, const float* x_local, int32_t n_local, float lr, float max_norm, int64_t adam_step,
                       void* stream);
/* MUON (torch.optim.Muon, torch >= 2.9, with the reference's split: Muon on the two weight matrices, fused Adam on the biases).
 * saev_muon_tail replaces saev_step_tail after the phases (saev_step_forward / _dead / _backward): remove_parallel_grads, the
 * global-norm clip, Adam on b_dec / b_enc (adam_step counts the Adam steps, 1-based) and, for W_dec and W_enc:
 *     m  <- lerp(m, g, 1 - momentum)                      fp32, bit-identical to torch's lerp_
 *     u  =  lerp(g, m, momentum) (nesterov) or m
 *     X  =  bf16(u) in the (d_model, d_sae) orientation (W_dec's is transposed), X /= clamp(bf16(||X||), eps) in bf16
 *     ns_steps x:  G = X X^T;  U = b G + c G G;  X = a X + U X
 *     p  <- p (1 - lr weight_decay) - adj_lr X (transposed back for W_dec)
 * with adj_lr = lr sqrt(max(1, rows / cols)) (adjust_lr 0, torch's "original"), lr 0.2 sqrt(max(rows, cols)) (1,
 * "match_rms_adamw") or lr (2).  The momentum lives in the W_dec / W_enc segments of the bound adam_m (their adam_v segments
 * are not used).  Rounding of the Newton-Schulz products: fp32 accumulation, fp32 epilogue alpha acc + beta C, one rounding to
 * bf16 per output element, as the vendor BLAS does for torch's bf16 addmm -- not bit-equal to torch, equal to an emulation
 * that rounds at the same points within one bf16 ulp per product.  Split-K sums run in a fixed order: two runs, two ranks
 * holding the same gradient, give identical bits.  Scratch (two bf16 (d_model, d_sae) matrices, two bf16 d_model^2, the
 * split-K partials) is allocated by the first call.  The operand images of W_enc are invalidated internally, as
 * saev_params_touched does: a Muon step never ends in SAEV_STALE_PARAMS.  saev_train_step / _gather / _dp run Adam only;
 * data-parallel Muon goes through the phases with the gradient summed on every rank (grad_scale = 1 / world). */
typedef struct {
    float momentum, weight_decay, a, b, c, eps;
    int32_t nesterov, ns_steps, adjust_lr;
} saev_muon_cfg;
/* torch's defaults: momentum 0.95, weight_decay 0.1, (a, b, c) = (3.4445, -4.7750, 2.0315), eps 1e-7, nesterov 1, 5 steps, "original" */
void saev_muon_default_cfg(saev_muon_cfg* out);
/* cfg NULL: the defaults */
int saev_muon_tail(saev_ctx* ctx, float lr, float max_norm, float grad_scale, int64_t adam_step, const saev_muon_cfg* cfg,
                   void* stream);
/* Newton-Schulz alone, context-free: x_in / x_out are (rows, cols) bf16 row-major with rows <= cols (transpose a taller matrix
 * first); normalize != 0 divides by the clamped bf16 norm first, as the tail does.  workspace: saev_muon_workspace_bytes(rows,
 * cols) bytes of device memory, 256-byte aligned. */
int64_t saev_muon_workspace_bytes(int64_t rows, int64_t cols);
int saev_muon_newton_schulz(const void* x_in, int64_t rows, int64_t cols, void* x_out, const saev_muon_cfg* cfg, int32_t normalize,
                            void* workspace, int64_t workspace_bytes, void* stream);
/* COHERENCE (the log block's metrics/dictionary_coherence, train.py:409-414), context-free.  W is (S, D) fp32 row-major, 16-byte
 * aligned, 1 <= S <= 2^20, 4 <= D <= 4096, D % 4 == 0.  The value is the reference expression
 *     (W_n @ W_n.T).abs().triu(1).max(),   W_n = W / W.norm(dim=1, keepdim=True)
 * with each row divided in fp32 by its fp32 norm: the max of |c_ij| over i < j and the pair (i, j) that attains it, ties to the
 * lexicographically smallest pair.  S = 1: 0.0 and the pair (-1, -1).  A row whose normalised form is not finite (a zero row,
 * an inf or NaN entry): NaN, as torch's max propagates it, with the smallest pair that holds the first such row.
 * route SAEV_COH_AUTO: an fp16 MFMA pass over the upper-triangle tiles of the fp16 images h_i = fp16(2^13 w_i / n_i) bounds every
 * pair: |c~_ij - c_ij| <= E_ij = 1.02 (||d_i|| ||w^_j|| + ||w^_i|| ||d_j|| + ||d_i|| ||d_j|| + 2.1 Dp 2^-22 (||w^_i|| + ||d_i||)
 * (||w^_j|| + ||d_j||)), with w^_i = w_i / n_i, d_i = w^_i - 2^-13 h_i measured on the values the MFMA consumes (fp16 subnormals
 * are flushed in the image) and Dp = D rounded up to 64 -- Cauchy-Schwarz on the rounding errors plus the fp32 accumulation of
 * the filter and of the exact value.  With L = max over pairs of |c~| - E, every pair with |c~| + E >= L is a candidate: the
 * maximiser p has |c~_p| + E_p >= c_p = max >= L, so it is always one.  A second pass over the tiles that can hold such a pair
 * writes the list; each candidate is then recomputed exactly: the fp32 dot product of the fp32 rows w^, in a fixed k order.
 * Value and pair are bit-reproducible from call to call.  List capacity: min(2^20, S (S - 1) / 2) pairs.  OVERFLOW is never
 * silent: if more pairs qualify, the call answers on the exact route instead.  route SAEV_COH_EXACT forces that route: fp32 MFMA
 * (v_mfma_f32_32x32x2_f32) of the rows w^ over the whole upper triangle, the max taken with the same tie rule.
 * Results are written on the device, nothing is read back: *out_value, out_pair[2] = (i, j), out_info[4] = {route taken
 * (SAEV_COH_FILTERED / _EXACT / _OVERFLOW), candidates found (may exceed the capacity), tiles the second pass recomputed,
 * capacity}.  workspace: saev_coherence_workspace_bytes(S, D) bytes of device memory, 256-byte aligned (-1: unsupported shape). */
#define SAEV_COH_AUTO 0
#define SAEV_COH_EXACT 1
#define SAEV_COH_FILTERED 0   /* route taken: fp16 filter and exact refinement */
#define SAEV_COH_OVERFLOW 2   /* route taken: the list overflowed, the exact route answered */
int64_t saev_coherence_workspace_bytes(int64_t S, int64_t D);
int saev_dictionary_coherence(const float* W, int64_t S, int64_t D, int32_t route, void* workspace, int64_t workspace_bytes,
                              float* out_value, int32_t* out_pair, int32_t* out_info, void* stream);
/* DICTIONARY MATCH (the per-row form of COHERENCE: "mean max cosine similarity" between two dictionaries), context-free.  A is
 * (Sa, D) and B is (Sb, D), fp32 row-major, 16-byte aligned, 1 <= Sa, Sb <= 2^20, 4 <= D <= 4096, D % 4 == 0.  With a^_i = a_i / ||a_i||
 * and b^_j likewise (each row divided in fp32 by its fp32 norm, exactly as COHERENCE does it), c_ij = <a^_i, b^_j> and the score
 * s_ij = c_ij (absolute == 0) or |c_ij| (absolute != 0):
 *     out_value[i] = max_j s_ij,   out_index[i] = the smallest j that attains it among the exactly recomputed values
 * over the admissible j.  SELF MODE (B == NULL, Sb == Sa): B = A and the pair j == i is not admissible; Sa == 1 then gives 0.0 and
 * index -1.  If a^_i is not finite (a zero row, an inf or NaN entry) row i is NaN with the smallest admissible j; otherwise, if some
 * b^_j is not finite, row i is NaN with the smallest such j -- as torch's max propagates NaN.
 * route SAEV_MATCH_AUTO: COHERENCE's scheme with the bound made per row.  An fp16 MFMA pass over all tiles of the Sa x Sb rectangle
 * gives per pair c~_ij and the same E_ij >= |c~_ij - c_ij|, hence s~_ij with |s~_ij - s_ij| <= E_ij in both score modes.  With
 * L_i = max_j (s~_ij - E_ij), every pair with s~_ij + E_ij >= L_i is a candidate of row i: a maximiser p of row i has
 * s~_p + E_p >= s_p >= s_q >= s~_q - E_q for every q of the row, so it (and every pair tied with it) is always one.  A second pass
 * over the tiles that can hold a candidate writes the list; each candidate is recomputed exactly (the fp32 dot product of the fp32
 * rows a^_i and b^_j in a fixed k order) and raised into its row's result by an integer max on (value, ~j).  Value and index are
 * bit-reproducible from call to call.  List capacity: min(Sa Sb, max(4096, 8 Sa)) pairs.  OVERFLOW is never silent: if more pairs
 * qualify, every row is answered on the exact route instead.  route SAEV_MATCH_EXACT forces that route: fp32 MFMA
 * (v_mfma_f32_32x32x2_f32) of the rows a^ and b^ over every tile, the same tie rule.
 * max_i out_value[i] of the self mode with absolute != 0 is the coherence of A to within the fp32 tolerance of either (not bit for
 * bit: the two calls refine different candidates).
 * Results are written on the device, nothing is read back: out_value[Sa], out_index[Sa], out_info[4] = {route taken
 * (SAEV_MATCH_FILTERED / _EXACT / _OVERFLOW), candidates found (may exceed the capacity), tiles the second pass recomputed,
 * capacity}.  workspace: saev_dictionary_match_workspace_bytes(Sa, Sb, D) bytes of device memory, 256-byte aligned (-1: unsupported
 * shape); it holds both fp16 images and Sa x ceil(Sb / 128) floats, never Sa x Sb. */
#define SAEV_MATCH_AUTO 0
#define SAEV_MATCH_EXACT 1
#define SAEV_MATCH_FILTERED 0   /* route taken: fp16 filter and exact refinement */
#define SAEV_MATCH_OVERFLOW 2   /* route taken: the list overflowed, the exact route answered */
int64_t saev_dictionary_match_workspace_bytes(int64_t Sa, int64_t Sb, int64_t D);
int saev_dictionary_match(const float* A, int64_t Sa, const float* B, int64_t Sb, int64_t D, int32_t absolute, int32_t route,
                          void* workspace, int64_t workspace_bytes, float* out_value, int32_t* out_index, int32_t* out_info,
                          void* stream);
/* K-MEANS (the reference's default baseline, contrib/trait_discovery tdiscovery/baselines.py MiniBatchKMeans.partial_fit),
 * context-free: the four device stages of one mini-batch step, with no n x k or k x k distance matrix in memory.  Matrices are fp32
 * row-major, 16-byte aligned: X (n, D) the batch, C (k, D) the centres, 1 <= n, k <= 2^20, 4 <= D <= 4096, D % 4 == 0.  Results are
 * written on the device, nothing is read back, there are no floating-point atomics, and every output is bit-reproducible from
 * call to call.
 * THE REFINED VALUE.  r_ij = the fp32 sum over k = 0 .. D-1, in that order, of (x_ik - c_jk)^2: a subtraction, a product and an
 * addition per k, each rounded once (no contraction), so r_ij depends on (i, j), X and C only.  One device function forms it
 * wherever it is needed; the distance is sqrtf(r_ij).  |r_ij - ||x_i - c_j||^2| <= (D + 3) 2^-24 ||x_i - c_j||^2.
 * ASSIGN.  farthest == 0: out_dist2[i] = min_j r_ij and out_index[i] = the smallest j attaining it among the exactly recomputed
 * values; farthest != 0: the same with max (the re-seeding of collapsed centres).  route SAEV_KMEANS_AUTO is DICTIONARY MATCH's
 * scheme with a bound for squared distances.  X and C are first centred on mu = the fp32 mean of the centres (distances do not
 * depend on it, the bound does: it is proportional to ||x - mu|| ||c - mu||); COHERENCE's prepare pass gives the unit-row fp16 images
 * of the centred rows x' = fl(x - mu), c' = fl(c - mu); an fp16 MFMA pass over all 128 x 128 tiles gives per pair the cosine c~ with
 * COHERENCE's E_cos, hence s~_ij = ||x'||^2 + ||c'||^2 - 2 nx nc c~ (nx, nc the fp32 norms the images were divided by, the squares
 * summed in fp64) and, evaluated in fp64,
 *     E1 = 2 nx nc (E_cos + 1.25e-7 ||x^|| ||c^||) + 1e-12 (||x'||^2 + ||c'||^2),   up = sqrt(max(s~ + E1, 0)),
 *     rho = 5.97e-8 (||x'|| + ||c'||),   dl = rho (2 up + rho),   E_ij = E1 + dl + 1.001 (D + 3) 2^-24 (up^2 + dl)  >= |s~_ij - r_ij|
 * (DESIGN.md 3.18 derives each term: the images, the division by the fp32 norm, the centring's rounding, the fp32 difference form).
 * With g = -s (nearest) or s (farthest) and L_i = max_j (g~_ij - E_ij), every pair with g~_ij + E_ij >= L_i is a candidate of row
 * i: the row's optimum and every pair tied with it always are.  A second pass over the tiles that can hold a candidate writes the
 * list; each candidate's r_ij is recomputed and raised into the row's result by an integer max on (key(value), ~j).  List
 * capacity: min(n k, max(4096, 8 n)) pairs (collapsed: min(k (k - 1) / 2, max(4096, 8 k))).  OVERFLOW is never silent: if more pairs
 * qualify -- or some centred row has no finite unit image: a row equal to mu, a norm outside fp32 -- every row is answered on the
 * exact route and out_info says so.  route SAEV_KMEANS_EXACT forces that route: r_ij of every pair by the same device function,
 * the same tie rule.  BOTH ROUTES RETURN THE SAME BITS.  k == 1 (the one centre is mu: nothing to filter) is answered on the exact
 * route and reported as SAEV_KMEANS_EXACT, in ASSIGN and in COLLAPSED: OVERFLOW always means that the filter was tried and failed.
 * out_info[4] = {route taken (SAEV_KMEANS_FILTERED / _EXACT / _OVERFLOW, or SAEV_KMEANS_NONFINITE: X or C holds an inf or a NaN --
 * every out_index is then -1, which GROUP ignores, the other outputs are unspecified, every write stays in bounds), candidates found (may exceed the capacity), tiles the
 * second pass recomputed, capacity}.  workspace: saev_kmeans_workspace_bytes(n, k, D) bytes of device memory, 256-byte aligned
 * (-1: unsupported shape); it holds the centred fp32 copies, both fp16 images and n x ceil(k / 128) doubles, never n x k.
 * GROUP.  From index[n] (entries outside [0, k) are ignored): counts[k] the rows per centre, starts[k + 1] their exclusive prefix
 * sums, rows[n] the row ids grouped by centre and ASCENDING within each centre -- a stable counting sort's result: the placement
 * uses integer atomics, then every centre's segment is put in order, so scheduling cannot show: a segment of up to 4096 rows is
 * sorted in LDS, a longer one is written afresh as the stable compaction {i : index[i] == j} in one pass over index (at most
 * n / 4096 centres are that long), so one centre may take the whole of the largest batch.
 * UPDATE.  The reference's running-mean update, in place: sums_j = the fp32 sum of centre j's rows in ascending row order (a
 * one-thread index_add_ into zeros); a centre with a batch count above zero becomes (c * prev + sums) / (prev + count) -- a
 * multiply, an add and a correctly rounded divide, uncontracted -- and cluster_counts[j] (the reference's float32 vector) becomes
 * prev + count.  repl_rows (may be NULL): 0 <= repl_rows[j] < n on a centre with no row of the batch is the reference's empty-cluster
 * replacement, "this centre's batch is exactly that one row, with count 1".  out_inertia (one double, may be NULL): the fp64 mean of
 * dist2[n] in a fixed order.
 * COLLAPSED.  For every pair i < j of centres with sqrtf(r_ij) < tol the loser is i if cluster_counts[i] <= cluster_counts[j], else
 * j; out_loser[k] (bytes) is the 0/1 mask of losers -- idempotent stores, no pair list leaves the call.  The same filter in self
 * mode over the tiles I <= J: a pair is a candidate unless s~ - E >= tol^2 (then sqrt(r) > tol, and sqrtf is monotone).  The same
 * overflow rule, exact route and out_info; workspace: saev_kmeans_workspace_bytes(k, k, D).  k == 1 or tol <= 0: no losers. */
#define SAEV_KMEANS_AUTO 0
#define SAEV_KMEANS_EXACT 1
#define SAEV_KMEANS_FILTERED 0    /* route taken: fp16 filter and exact refinement */
#define SAEV_KMEANS_OVERFLOW 2    /* route taken: the filter could not answer (list overflow, a row without an image): exact route */
#define SAEV_KMEANS_NONFINITE (-1) /* X or C holds an inf or a NaN */
int64_t saev_kmeans_workspace_bytes(int64_t n, int64_t k, int64_t D);
int saev_kmeans_assign(const float* X, int64_t n, const float* C, int64_t k, int64_t D, int32_t farthest, int32_t route,
                       void* workspace, int64_t workspace_bytes, float* out_dist2, int32_t* out_index, int32_t* out_info, void* stream);
int saev_kmeans_group(const int32_t* index, int64_t n, int64_t k, int32_t* counts, int32_t* starts, int32_t* rows, void* stream);
int saev_kmeans_update(const float* X, int64_t n, int64_t D, int64_t k, const int32_t* starts, const int32_t* rows,
                       const int32_t* repl_rows, float* centers, float* cluster_counts, double* out_inertia, const float* dist2,
                       void* stream);
int saev_kmeans_collapsed(const float* C, int64_t k, int64_t D, float tol, const float* cluster_counts, int32_t route, void* workspace,
                          int64_t workspace_bytes, uint8_t* out_loser, int32_t* out_info, void* stream);
/* BATCH STATISTICS (the log block, train.py:365-442; evaluate, train.py:510-618; the inference pass, inference.py), context-free:
 * one call per batch leaves every sum those three form, with no n x D or n x k temporary.  Inputs: x (n x D fp32) and its
 * reconstruction x_hat (n x D fp32, may be NULL), both 16-byte aligned; the codes as padded rows, idx (n x cap int32), val
 * (n x cap fp32) and row_nnz (n int32; NULL: every row has cap entries, as TopK rows do; a count above cap reads as cap, as in
 * saev_decode_rows); keep (n bytes, may be NULL): rows with keep[b] == 0 contribute nothing.  4 <= D <= 4096, D % 4 == 0
 * (anything else is SAEV_UNSUPPORTED), any n >= 0, S >= 0, cap >= 0 below 2^31; n = 0 returns SAEV_OK and writes nothing.
 * Outputs are the caller's device buffers in saev_batch_acc; each may be NULL, which skips its work.  The call ADDS to them,
 * so a pass over many batches needs no host arithmetic; flags = SAEV_BATCH_OVERWRITE stores instead (live excepted):
 *   col_sum   (D doubles)  sum over kept rows of x[:, c]
 *   scalars   (8 doubles)  [kept rows, sum x, sum x^2, sum r, sum r^2, 0, 0, 0], r = x - x_hat formed in fp64 from the fp32
 *                          operands (exact to one rounding), squares as fp64 fmas; without x_hat the r sums add 0
 *   n_pos     (S int64)    kept codes with val > 0
 *   value_sum (S doubles)  sum of val over kept codes with val != 0
 *   live      (S int32)    set to 1 where a kept code has |val| > live_eps (plain stores; the call never clears it)
 * Codes whose index lies outside [0, S) are ignored.  NaN and Inf propagate as IEEE arithmetic gives them.
 * col_sum and scalars are BIT-REPRODUCIBLE from run to run: per-workgroup partial sums in the workspace, added in workgroup order
 * by a finishing pass, no floating-point atomics.  n_pos is integer, hence exact.  value_sum uses fp64 vector atomics and is
 * reproducible only to fp64 rounding (the order of the adds is not fixed).
 * workspace: saev_batch_stats_workspace_bytes(n, D) bytes of device memory, 256-byte aligned (-1: unsupported shape); needed only
 * when col_sum or scalars is asked for.  Arguments are checked before the device is touched; a refused call leaves its message
 * with saev_last_error(NULL) (per thread).  Nothing synchronises. */
#define SAEV_BATCH_OVERWRITE 1
typedef struct {
    int32_t struct_size;   /* sizeof(saev_batch_acc) of the caller (fields past it read as 0) */
    int32_t flags;         /* 0 or SAEV_BATCH_OVERWRITE                                       */
    float live_eps;        /* the log block passes 1e-12 (train.py:404)                       */
    int32_t reserved;
    double* col_sum;
    double* scalars;
    int64_t* n_pos;
    double* value_sum;
    int32_t* live;
} saev_batch_acc;
int64_t saev_batch_stats_workspace_bytes(int64_t n, int64_t D);
int saev_batch_stats(const float* x, const float* x_hat, const int32_t* idx, const float* val, const int32_t* row_nnz,
                     const uint8_t* keep, int64_t n, int64_t D, int64_t S, int64_t cap, const saev_batch_acc* acc, void* workspace,
                     int64_t workspace_bytes, void* stream);
/* metrics/avg_decoder_row_norm (train.py:406): *out = the mean over the S rows of W (S x D fp32 row-major, 16-byte aligned, same
 * limits on D, S >= 1) of each row's fp32 L2 norm -- the squares exact in fp64, summed in a fixed order, the root rounded once to
 * fp32 -- added in a fixed order as doubles: one device double, bit-reproducible.  workspace: SAEV_ROW_NORM_WORKSPACE_BYTES bytes,
 * 256-byte aligned. */
#define SAEV_ROW_NORM_WORKSPACE_BYTES 8192
int saev_row_norm_mean(const float* W, int64_t S, int64_t D, double* out, void* workspace, int64_t workspace_bytes, void* stream);
/* LATENT TOP-K (the reference's saev.helpers.csr_topk(arr, k=..., axis=0) over token_acts.npz, as a streaming update that rides
 * along the inference pass), context-free: for every latent j the k largest codes seen so far and the rows they sit in.
 * State is the caller's device memory, latent-major, ZERO-INITIALISED by the caller before the first update:
 *   top_val (S x k fp32), top_row (S x k int64), top_cnt (S int32; entries held, at most k)
 * After every update latent j's first top_cnt[j] slots hold its best entries in the order (value descending, row ascending) --
 * the TIE RULE: among equal values the lower row wins, whatever order the batches arrive in; the later slots are never written
 * (they keep the caller's zeros, which is how the reference pads).  1 <= k <= 64 (anything else is SAEV_UNSUPPORTED).
 * One update consumes one batch of n rows in ONE of two forms (both or neither is SAEV_INVALID_ARG):
 *   padded rows  idx (n x cap int32), val (n x cap fp32), row_nnz (n int32, may be NULL: every slot is an entry; a count above cap
 *                reads as cap)
 *   CSR          row_ptr (n + 1 int64, absolute positions into indices / data, non-decreasing), indices (int32), data (fp32), and
 *                nnz = row_ptr[n] - row_ptr[0] given by the host (nothing is read back)
 * keep (n bytes, may be NULL): rows with keep[b] == 0 contribute nothing.  The row id of local row b is row_base + b.
 * An ENTRY is a slot with val != 0 (zeros of both signs are none) whose latent lies in [0, S); negatives and +-Inf are entries;
 * NaN is outside the contract, and so is more than one entry per (row, latent).
 * Exact and BIT-REPRODUCIBLE: integer atomics only (candidate counts and placement), the lists ordered by a total order on
 * (value, row).  No n x S temporary, nothing read back, nothing synchronises.  n = 0 returns SAEV_OK and writes nothing.
 * workspace: saev_latent_topk_workspace_bytes(n_entries, S) bytes of device memory, 256-byte aligned, n_entries = n cap or nnz
 * (at most 2^31 - 1 per update; -1: unsupported).  Arguments are checked before the device is touched; a refused call leaves its
 * message with saev_last_error(NULL). */
typedef struct {
    int32_t struct_size;   /* sizeof(saev_latent_topk_state) of the caller (fields past it read as 0) */
    int32_t k;
    float* top_val;
    int64_t* top_row;
    int32_t* top_cnt;
} saev_latent_topk_state;
int64_t saev_latent_topk_workspace_bytes(int64_t n_entries, int64_t S);
int saev_latent_topk_update(const int32_t* idx, const float* val, const int32_t* row_nnz, int64_t cap, const int64_t* row_ptr,
                            const int32_t* indices, const float* data, int64_t nnz, const uint8_t* keep, int64_t n, int64_t S,
                            int64_t row_base, const saev_latent_topk_state* state, void* workspace, int64_t workspace_bytes,
                            void* stream);
/* LATENT HISTOGRAM (per-latent activation histograms and exact quantiles over a stream of batches), context-free.
 * THE KEY of a float32 v with bit pattern u is ~u when the sign bit is set, else u | 0x80000000: strictly increasing in v,
 * invertible.  LEVEL 0 is key >> 20 (sign, exponent and three mantissa bits: 4096 bins, eight to the octave, float32 edges
 * 2^e (1 + i/8)), level 1 (key >> 10) & 1023, level 2 key & 1023.
 * An ENTRY is a slot with val != 0 whose latent lies in [0, S) -- the rules of LATENT TOP-K: negatives, denormals and +-Inf are
 * entries, zeros of both signs are none, NaN and more than one entry per (row, latent) are outside the contract.
 * saev_latent_hist_update consumes one batch of n rows in one of saev_latent_topk_update's two forms (padded rows or CSR; both or
 * neither is SAEV_INVALID_ARG) with the optional keep bytes, and ADDS to the caller's ZERO-INITIALISED device state:
 *   level 0      counts (S x 4096 uint32): counts[j, b] += entries of latent j with level-0 bin b
 *   level 1, 2   counts (S x T x 1024 uint32): counts[j, t, d] += entries of latent j whose key carries prefix[j, t] (its level-0
 *                bin at level 1, its top 22 bits at level 2) and whose digit of this level is d; prefix is S x 16 uint32, the first
 *                T <= 16 of a row live, 0xffffffff = a target already resolved.  Two targets with one prefix count twice.
 *   every level  *n_rows (int64) += the kept rows of the batch
 * counts and prefix are 16-byte aligned; a table holds fewer than 2^32 - 1 counters (SAEV_UNSUPPORTED otherwise).  Counts are
 * uint32: the caller offers fewer than 2^32 rows.  Integer atomics only: the counts are exact and the same for every order and
 * every split of the batches.  workspace: saev_latent_hist_workspace_bytes(n_entries, S) bytes, 256-byte aligned (the batch's
 * kept-row count; -1: unsupported).
 * saev_latent_hist_locate is one launch that reads nothing back.  For latent j let M_j be its entries (over_rows = 0) or the kept
 * rows *n_rows (over_rows = 1: the M_j - entries silent rows enter as one block of zeros between level-0 bins 2047 and 2048, in
 * closed form).  For quantile q_i: h = (M_j - 1) q_i as one fp64 product; target 2 i is rank floor(h), target 2 i + 1 rank ceil(h)
 * of the sorted multiset.  At level 0 it writes count[j] = M_j and, per target, the level-0 bin holding the rank (prefix), the
 * rank left inside that bin (rank) and resolved: 0 open, 1 inside the zero block (the value is 0.0), 2 empty multiset.  At levels
 * 1 and 2 it extends prefix by the digit found in the target's own 1024 counters and replaces rank.  After level 2 it also writes
 * lower, higher (S x Q fp32: the floats of the 32 located bits, exact) and linear (S x Q fp64) =
 * lower + (h - floor(h)) (higher - lower), each operation rounded once, = lower when lower == higher; NaN in all three when
 * M_j = 0.  1 <= Q <= 8 (SAEV_UNSUPPORTED), every q in [0, 1], and at levels 1, 2 the state's T = 2 Q.
 * Arguments are checked before the device is touched; a refused call leaves its message with saev_last_error(NULL); n = 0 (S = 0
 * for locate) returns SAEV_OK and writes nothing; nothing synchronises. */
typedef struct {
    int32_t struct_size;   /* sizeof(saev_latent_hist_state) of the caller (fields past it read as 0) */
    int32_t level;         /* 0, 1 or 2 */
    int32_t T;             /* levels 1, 2: live targets per latent */
    int32_t reserved;
    uint32_t* counts;
    int64_t* n_rows;
    uint32_t* prefix;      /* levels 1, 2 */
} saev_latent_hist_state;
typedef struct {
    int32_t struct_size;   /* sizeof(saev_latent_hist_targets) of the caller */
    int32_t Q;
    int32_t over_rows;
    int32_t reserved;
    double q[8];
    uint32_t* prefix;      /* S x 16 */
    uint32_t* rank;        /* S x 16 */
    int32_t* resolved;     /* S x 16 */
    int64_t* count;        /* S */
    float* lower;          /* S x Q, after level 2 */
    float* higher;
    double* linear;
} saev_latent_hist_targets;
int64_t saev_latent_hist_workspace_bytes(int64_t n_entries, int64_t S);
int saev_latent_hist_update(const int32_t* idx, const float* val, const int32_t* row_nnz, int64_t cap, const int64_t* row_ptr,
                            const int32_t* indices, const float* data, int64_t nnz, const uint8_t* keep, int64_t n, int64_t S,
                            const saev_latent_hist_state* state, void* workspace, int64_t workspace_bytes, void* stream);
int saev_latent_hist_locate(const saev_latent_hist_state* state, const saev_latent_hist_targets* targets, int64_t S, void* stream);
/* LATENT EDITS (the intervention of the reference's contrib/interactive_interp/semseg: set a latent, decode, add the SAE's error
 * back), context-free.  For an SAE x_hat = b_dec + sum_j f_j W_dec[j, :] and edits e = (latent l_e, target t_e(f)),
 *   x' = (x - x_hat) + x_hat_mod = x + sum_e c_e W_dec[l_e, :],   c_e = t_e(f_l) - f_l
 * b_dec and every unedited latent cancel: one pass over x, a few W_dec rows, no n x S matrix and no decode.
 * AN EDIT is 16 bytes.  op is SAEV_EDIT_SET (t = value), SAEV_EDIT_SCALE (t = value f) or SAEV_EDIT_ADD (t = f + value), optionally
 * | SAEV_EDIT_IF_ACTIVE (the edit applies only where f != 0).  group is -1 (the GLOBAL list: every row) or g in [0, n_groups) (the
 * list of group g: rows with row_group[b] == g).  Edits do not compose: each reads the ORIGINAL f.
 * saev_edit_plan_build validates on the host, in this order, before the device is touched: (1) sizes -- negative sizes and S outside
 * [1, 2^31) are SAEV_INVALID_ARG, n_edits or n_groups above 65 536 SAEV_UNSUPPORTED, edits NULL with n_edits > 0 SAEV_INVALID_ARG;
 * (2) every latent in [0, S); (3) every op known; (4) every group in [-1, n_groups) (SAEV_INVALID_ARG each); (5) at most 256 edits
 * in the global list and in each group's list (SAEV_UNSUPPORTED); (6) no latent twice in one list, none in both the global list and
 * a group's list (SAEV_INVALID_ARG); then (7) plan NULL with plan_bytes == 0 VALIDATES ONLY (SAEV_OK, no device needed), any other plan NULL, smaller than saev_edit_plan_bytes(n_edits, n_groups) (-1: unsupported
 * sizes) or not 256-byte aligned (SAEV_INVALID_ARG).  It writes the edits grouped into the device plan -- the global list, then each
 * group's list, a CSR over the lists; inside a list the caller's order is kept -- and WAITS for `stream` (the host images are its
 * own).  A plan serves any number of saev_intervene_rows calls with the same n_edits and n_groups and an S no smaller.
 * saev_intervene_rows takes x (n_rows x D fp32), W_dec (S x D fp32 row-major) and the codes as padded rows (as saev_decode_rows):
 * row b's entries in its first min(row_nnz[b], row_cap) slots of idx / val (n_rows x row_cap); row_nnz NULL = every row has
 * row_cap entries (the TopK form); a negative count reads as 0.  For each row b:
 *   1. f_l is the value of the FIRST slot whose idx equals l, or 0 when there is none.
 *   2. the applicable edits are the global list, then the list of group row_group[b] (row_group NULL, or a value outside
 *      [0, n_groups): no group list).  A row with row_keep[b] == 0 (row_keep may be NULL) has none at all.
 *   3. c_e in fp32 from the original f: value - f (SET), fmaf(value, f, -f) (SCALE), value (ADD).  An edit with c_e == 0, or
 *      IF_ACTIVE with f == 0, is SKIPPED: it loads no W_dec row (an Inf or NaN there does not reach the output).
 *   4. out[b, d] = x[b, d], then one fmaf(c_e, W_dec[l_e, d], .) per remaining edit in list order.  Columns are independent.
 *   5. a row without a remaining edit gets out[b, :] = x[b, :] BIT FOR BIT.
 * out == x (in place) is allowed; out overlapping x in any other way, or W_dec, idx or val, is SAEV_INVALID_ARG.  rows_changed (int64
 * per edit in the CALLER's index, may be NULL) is ADDED the number of rows where the edit's c_e was applied: integer atomics,
 * summed per workgroup first.  No floating-point atomic: two calls give the same bits, and in place gives the bits of out of place.
 * Any D >= 1: 16-byte vector accesses when D % 4 == 0 and x, out and W_dec are 16-byte aligned, scalar ones otherwise (the same
 * values).  n_rows, D, S, row_cap < 2^31 (SAEV_UNSUPPORTED); n_rows = 0 returns SAEV_OK; n_edits = 0 copies x (plan may be NULL).
 * Nothing is allocated, nothing read back, nothing synchronises. */
#define SAEV_EDIT_SET 0
#define SAEV_EDIT_SCALE 1
#define SAEV_EDIT_ADD 2
#define SAEV_EDIT_IF_ACTIVE 4
typedef struct {
    int32_t latent;
    int32_t op;
    float value;
    int32_t group;
} saev_edit;
int64_t saev_edit_plan_bytes(int64_t n_edits, int64_t n_groups);
int saev_edit_plan_build(const saev_edit* edits_host, int64_t n_edits, int64_t n_groups, int64_t S, void* plan_dev, int64_t plan_bytes,
                         void* stream);
int saev_intervene_rows(const float* x, int64_t n_rows, int64_t D, const float* W_dec, int64_t S, const int32_t* idx, const float* val,
                        const int32_t* row_nnz, int64_t row_cap, const void* plan_dev, int64_t n_edits, int64_t n_groups,
                        const int32_t* row_group, const uint8_t* row_keep, float* out, int64_t* rows_changed, void* stream);
/* CLASS FIRING COUNTS (the reference's semseg quantitative.get_latent_lookup: for every class the latent whose firing best
 * predicts it, by F1 over a few thresholds), context-free, from the sparse codes alone.  State is the caller's device memory,
 * ZERO-INITIALISED before the first call: hist (C x T x S uint32), pos (T x S uint32), n_rows_c (C int64); calls accumulate.
 * thr (T floats on the HOST): >= 0, strictly ascending, 1 <= T <= 8.  A row (padded codes as above) is KEPT when 0 <= label[b] < C
 * and row_keep (may be NULL) allows it; a kept row adds 1 to n_rows_c[label[b]].  Each stored entry (s, v) of a kept row with s in
 * [0, S) has m = #{t : v > thr_t} (strict; a NaN gives 0); m >= 1 adds 1 to hist[label][m - 1][s] and to pos[m - 1][s] -- one pair
 * of integer atomics per code, not one per threshold.  Exact, order-independent.
 * saev_class_fire_f1: TP[c, t, s] = sum over u >= t of hist[c][u][s], POS likewise from pos, FP = POS - TP, FN = n_rows_c[c] - TP,
 *   f1[c, t, s] = float32(2 TP) / (float32(2 TP + FP + FN) + 1e-10f)   (integers exact, each converted once; fp32 division)
 * f1[c, s] = max over t, a tie going to the LOWEST t, which best_t[c, s] records; latent_mask (S bytes, may be NULL): a latent with
 * mask 0 gets f1 = -1, best_t = 0.  A zero denominator gives 0.
 * ONE DIFFERENCE from the reference: a batch without a row of class c still adds its firing rows to c's false positives (POS is
 * global); the reference's loop over the batch's unique classes skips such batches, so its FP depends on the batching.
 * Refusals, in this order: negative sizes (SAEV_INVALID_ARG); S >= 2^31 (SAEV_UNSUPPORTED); S < 1 (SAEV_INVALID_ARG); C outside
 * [1, 4096], T outside [1, 8] (SAEV_UNSUPPORTED); counts only: n_rows, row_cap or n_rows * row_cap >= 2^31 (SAEV_UNSUPPORTED), thr
 * NULL, negative, NaN or not ascending (SAEV_INVALID_ARG); C * T * S >= 2^31 (SAEV_UNSUPPORTED); a NULL state or output pointer
 * (SAEV_INVALID_ARG).  n_rows = 0 returns SAEV_OK. */
int saev_class_fire_counts(const int32_t* idx, const float* val, const int32_t* row_nnz, int64_t row_cap, int64_t n_rows,
                           const int32_t* label, const uint8_t* row_keep, int64_t S, int64_t C, const float* thr_host, int32_t T,
                           uint32_t* hist, uint32_t* pos, int64_t* n_rows_c, void* stream);
int saev_class_fire_f1(const uint32_t* hist, const uint32_t* pos, const int64_t* n_rows_c, int64_t S, int64_t C, int32_t T,
                       const uint8_t* latent_mask, float* f1, uint8_t* best_t, void* stream);
/* PROBE1D (the reference's contrib/trait_discovery tdiscovery.probe1d.Sparse1DProbe: what writes probe1d_metrics.npz next to
 * token_acts.npz), context-free: for each of the S x C (latent j, class c) pairs the two-parameter logistic regression
 * y_c ~ sigma(b + w x_j) over N rows, fitted by damped Newton (Levenberg-Marquardt) steps, and its loss and confusion counts.
 * x is CSR: row_ptr (N + 1 int64, absolute positions into indices / data, non-decreasing), indices (int32 in [0, S)), data (fp32),
 * nnz = row_ptr[N] - row_ptr[0] given by the host.  1 <= N, S < 2^31, 0 <= nnz < 2^31, 1 <= C <= 4096 (else SAEV_UNSUPPORTED).
 * EVENT RULE: an event of latent j is a STORED entry of column j -- an explicitly stored 0.0 counts (unlike LATENT TOP-K), values may
 * be negative; more than one entry per (row, latent) is outside the contract.  n_j = events of j; qx_j = max(sqrt(sum v^2 / n_j),
 * 1e-6), 1 when n_j = 0; the N - n_j other rows of latent j enter every formula in closed form.
 * LABELS, one of three forms (none or several is SAEV_INVALID_ARG): class ids class_u8 (N uint8, C <= 256) or class_i32 (N int32), the
 * one-hot matrix implied; or y_matrix (N x C bytes, each 0 or 1).  They are packed to ybits (N x ceil(C / 32) uint32, bit c % 32 of
 * word c / 32) and counted per class (pos, C int64; pi_c = pos_c / N); both forms of the same labels give the same bits.
 * prepare writes into the caller's workspace (byte offsets: saev_probe1d_layout_of): the events latent-major -- starts (S + 1 int64),
 * row (nnz int32) and val (nnz fp32), inside a latent in ASCENDING ROW ORDER --, qx (S fp64), chunk_starts (S + 1 int32: latent j is
 * cut into ceil(n_j / chunk) chunks of chunk = 512 events), ybits, pos, and err (int32[0]: 0, or the largest SAEV_PROBE1D_ERR_* met
 * -- a class id outside [0, C), a latent outside [0, S), a label byte above 1 -- found on the device; the caller reads it when it
 * next synchronises, and every later result of that workspace is void if it is not 0).
 * ARITHMETIC: everything is fp64.  For an event with value v (fp32, widened) and label y of pair (b, w): z = b + w v (product and sum
 * rounded separately), e = exp(-|z|), sigma(|z|) = 1 / (1 + e), sigma(-|z|) = e sigma(|z|); mu = sigma(z), 1 - mu = sigma(-z) and
 * s = mu (1 - mu) = sigma(|z|) sigma(-|z|) are taken from these two (no cancellation); the seven EVENT SUMS of a pair, in this order
 * (sums: S x 7 x C fp64), are  mu,  (mu - y) v,  s,  s v,  s v^2,  the BCE-with-logits loss max(z, 0) - y z + log1p(e)  and  y.
 * ORDER: a latent's events in ascending row order; each sub-chunk of 64 events is summed from zero, the sub-chunks of a chunk are
 * added in order, the chunk sums of a latent are added in chunk order.  The order does not depend on C, on the launch or on timing:
 * the sums are BIT-REPRODUCIBLE, and those of a class computed alone equal those computed among others.  Integer atomics only
 * (counts, placement cursors, the slab maximum as the bit pattern of a non-negative double); none touches a sum.
 * SOLVER, per pair, as the reference's fit: start b = base_c = logit(clamp(pi_c, 1e-8, 1 - 1e-8)), w = 0, lam = lam_init, prev_pred =
 * prev_loss = NaN.  Per iteration, with mu0 = clamp(sigma(b), 1e-8, 1 - 1e-8), s0 = mu0 (1 - mu0), zf = (N - n_j) / N:
 *   g0 = sum_mu / N + zf mu0 - pi + ridge (b - base),  g1 = sum_g1 / N + ridge w,  h0 = sum_s / N + zf s0 + ridge,
 *   h1 = sum_sv / N,  h2 = sum_svv / N + ridge;  pos_zero = min(max(pi - sum_y / N, 0), zf), neg_zero = zf - pos_zero,
 *   loss = sum_loss / N - (pos_zero log mu0 + neg_zero log1p(-min(mu0, 1 - 1e-8))) + ridge / 2 (w^2 + (b - base)^2).
 * If prev_pred and prev_loss are finite: rho = (prev_loss - loss) / max(prev_pred, 1e-18); lam *= lam_shrink when rho >= 0.75 and the
 * previous step was not clipped; lam *= lam_grow when rho <= 0.25 or it was; lam clamped to [1e-12, 1e12].  A pair with
 * max(|g0|, |g1|) <= tol takes no step.  Otherwise up to five tries: det = (h0 + lam)(h2 + lam qx^2) - h1^2, valid if |det| > 1e-18
 * (else the try's step is 0); (db, dw) = ((h2 + lam qx^2) g0 - h1 g1, (h0 + lam) g1 - h1 g0) / det, scaled by delta_logit / (norm +
 * 1e-18) when norm = |(db, qx dw)| > delta_logit (CLIPPED); pred = g0 db + g1 dw - (h0 db^2 + 2 h1 db dw + h2 dw^2) / 2; accepted if
 * pred is finite and > 0, else lam = clamp(lam lam_grow).  After five failures: (db, dw) = -alpha (g0, g1), alpha = 1e-3 delta_logit /
 * (|(g0, max(qx, 1e-12) g1)| + 1e-18), pred = NaN, clipped.  Then b -= db, w -= dw, prev_loss = loss, prev_pred = pred.  A latent without
 * events keeps b = base, w = 0, lam = lam_init, prev_pred = NaN, not clipped (its prev_loss is set like any other).
 * TERMINATION per SLAB of class_slab_size consecutive classes: a slab stops after the first iteration at which the largest
 * max(|g0|, |g1 / max(qx, 1e-12)|) over its pairs is <= tol (that iteration's step is applied); its pairs are never touched again.
 * n_iter of a class is its slab's count.  fit = init, then max_iter x (events, update) with stopped slabs skipped on the device; with
 * poll_every > 0 the host reads the number of running slabs every poll_every iterations (the call's only synchronisation) and stops
 * launching at 0 -- the results do not depend on it.  coef / intercept (S x C) are rounded once to out_dtype on the way out.
 * evaluate(b, w: S x C fp64, threshold in (0, 1)): per pair the mean BCE loss, the events' share summed in the order above and the
 * zero rows as pos_zero softplus(-b) + neg_zero softplus(b) with the COUNTS pos_zero = min(max(pos_c - pos_nz, 0), N - n_j); and
 * tp / fp / tn / fn with prediction mu > threshold (sigma(b) > threshold on the zero rows): exact integers, stored in out_dtype.
 * evaluate and stats use the workspace's sums and partials as scratch.  update (exposed for tests, as stats is) runs one solver
 * iteration on the workspace's state from `sums` (NULL: the workspace's); step_out (S x C x 4 fp64: db, dw, pred, lam; may be NULL) and
 * flags_out (S x C int32: SAEV_PROBE1D_STEP_* | tries << 8; may be NULL) tell which branch a pair took.
 * Arguments are checked before the device is touched; a refused call leaves its message with saev_last_error(NULL).  Nothing is
 * allocated and, the poll of fit aside, nothing synchronises.  workspace: saev_probe1d_workspace_bytes(N, S, C, nnz) bytes of device
 * memory, 256-byte aligned (-1: unsupported shape); it holds prepare's outputs, the solver state and 56 bytes per pair and per
 * (chunk, class) of sums -- never an (nnz, C) array. */
#define SAEV_PROBE1D_ERR_CLASS 1
#define SAEV_PROBE1D_ERR_LATENT 2
#define SAEV_PROBE1D_ERR_LABEL 3
#define SAEV_PROBE1D_F32 0
#define SAEV_PROBE1D_F64 1
#define SAEV_PROBE1D_STEP_INACTIVE 1
#define SAEV_PROBE1D_STEP_CLIPPED 2
#define SAEV_PROBE1D_STEP_SINGULAR 4   /* some try met |det| <= 1e-18 */
#define SAEV_PROBE1D_STEP_FALLBACK 8
#define SAEV_PROBE1D_STEP_EMPTY 16
#define SAEV_PROBE1D_STEP_GROWN 32     /* the rho rule grew lam before the step */
#define SAEV_PROBE1D_STEP_SHRUNK 64
typedef struct {
    int32_t struct_size;       /* sizeof(saev_probe1d_cfg) of the caller (fields past it read as 0) */
    int32_t max_iter;
    int32_t class_slab_size;
    int32_t poll_every;        /* 0: the host never looks */
    int32_t out_dtype;         /* SAEV_PROBE1D_F32 or SAEV_PROBE1D_F64 */
    int32_t reserved;
    double ridge, tol, lam_init, lam_shrink, lam_grow, delta_logit;
} saev_probe1d_cfg;
typedef struct {               /* byte offsets into the workspace (all multiples of 256) */
    int32_t struct_size;
    int32_t chunk;             /* events per chunk */
    int64_t words;             /* ceil(C / 32) */
    int64_t max_chunks;        /* bound of chunk_starts[S] */
    int64_t parts;
    int64_t total_bytes;
    int64_t off_err, off_starts, off_chunk_starts, off_row, off_val, off_qx, off_ybits, off_pos, off_cnt, off_tot;
    int64_t off_b, off_w, off_lam, off_prev_pred, off_prev_loss, off_clipped;   /* state: S x C fp64 each, clipped int32 */
    int64_t off_sums, off_part, off_gmax, off_done, off_n_iter, off_active;     /* done, n_iter: per slab int32 */
} saev_probe1d_layout;
int64_t saev_probe1d_workspace_bytes(int64_t N, int64_t S, int64_t C, int64_t nnz);
int saev_probe1d_layout_of(int64_t N, int64_t S, int64_t C, int64_t nnz, saev_probe1d_layout* out);
int saev_probe1d_prepare(const int64_t* row_ptr, const int32_t* indices, const float* data, int64_t nnz, int64_t N, int64_t S, int64_t C,
                         const uint8_t* class_u8, const int32_t* class_i32, const uint8_t* y_matrix, void* workspace, int64_t workspace_bytes,
                         void* stream);
int saev_probe1d_stats(int64_t N, int64_t S, int64_t C, int64_t nnz, const double* b, const double* w, double* sums_out, void* workspace,
                       int64_t workspace_bytes, void* stream);
int saev_probe1d_init(int64_t N, int64_t S, int64_t C, int64_t nnz, const saev_probe1d_cfg* cfg, void* workspace, int64_t workspace_bytes,
                      void* stream);
int saev_probe1d_update(int64_t N, int64_t S, int64_t C, int64_t nnz, const saev_probe1d_cfg* cfg, const double* sums, double* step_out,
                        int32_t* flags_out, void* workspace, int64_t workspace_bytes, void* stream);
int saev_probe1d_fit(int64_t N, int64_t S, int64_t C, int64_t nnz, const saev_probe1d_cfg* cfg, void* coef_out, void* intercept_out,
                     int32_t* n_iter_out, void* workspace, int64_t workspace_bytes, void* stream);
int saev_probe1d_evaluate(int64_t N, int64_t S, int64_t C, int64_t nnz, const double* b, const double* w, double threshold, int32_t out_dtype,
                          void* loss, void* tp, void* fp, void* tn, void* fn, void* workspace, int64_t workspace_bytes, void* stream);
/* LATENT AP (the concept audit of the reference's contrib/trait_discovery tdiscovery.classification: compute_ap_for_latent over every
 * latent and class, what eval_worker_fn turns into audit_ap_s.npy and Yield@B), context-free: AP[j, c], the average precision of
 * latent j's activation as a detector of class c over N rows, EXACT AND TIE-AWARE (McSherry and Najork 2008: the expectation over
 * all orders of tied scores), for all S x C pairs in one call.
 * x is CSR: row_ptr (N + 1 int64, absolute positions into indices / data, non-decreasing), indices (int32 in [0, S)), data (fp32),
 * nnz = row_ptr[N] - row_ptr[0] given by the host.  1 <= N, S < 2^31, 0 <= nnz < 2^31, 1 <= C <= 4096 (else SAEV_UNSUPPORTED, and
 * -1 from the workspace-size function).
 * CLASSES, one class per row in one of two forms (none or both is SAEV_INVALID_ARG): class_i32 (N int32, -1 = the row belongs to no
 * class; it is still ranked), or class_u8 (N bytes) with an optional remap (256 int32: byte -> column or -1; NULL = the identity).
 * EVENT RULE: an event of latent j is a stored entry of column j with value != 0 -- +0.0 and -0.0 are NOT events (as in LATENT
 * TOP-K, unlike PROBE1D); negative values and +-Inf are.  NaN, and more than one entry per (row, latent), are outside the contract.
 * m_j = events of j.
 * RANKING: latent j ranks all N rows by activation, descending; a row without an event has activation 0.  A TIE GROUP is a maximal
 * set of rows of equal activation (fp32 ==).  The groups of a latent in order: its distinct positive values, descending; the ZERO
 * GROUP of the Z_j = N - m_j rows without an event (if Z_j > 0); its distinct negative values, descending.  For group g: t = rows
 * ranked before it, n = its size, r = its rows of class c, R = the sum of r over earlier groups.
 *   term(g, c) = 0                                                                  if r = 0
 *              = r (R + 1) / (t + 1)                                                if n = 1
 *              = sum_{q = 0 .. n-1} ((r / n) (R + 1 + q a)) / (t + 1 + q)           if 2 <= n <= direct_max,  a = (r - 1) / (n - 1)
 *              = (r / n) ((R + 1 - a (t + 1)) dH + a n)                             otherwise,  dH = H_{t+n} - H_t
 * pos_c = rows of class c;  AP[j, c] = (sum over g of term(g, c)) / pos_c, 0 when pos_c = 0.
 * dH (harmonic numbers) is never a difference of two table entries.  For t >= 32: dH = log1p(n / t) + corr with m = t + n and
 *   corr = (((((-(m^-10 - t^-10) / 132 + (m^-8 - t^-8) / 240) - (m^-6 - t^-6) / 252) + (m^-4 - t^-4) / 120)
 *            + n (t + m) (t^-2 m^-2) / 12) - n / (2 t m)),
 * the powers built from 1 / t and 1 / m by squaring.  For t < 32: the terms 1 / p for p = min(t + n, 32) down to t + 1, added in
 * that order, plus (when t + n > 32) the formula above at t = 32, n = t + n - 32.
 * ARITHMETIC AND ORDER: everything is fp64, every operation rounded on its own (no contraction); counts are integers.  The sum of a
 * pair starts at 0 and receives its non-zero terms one at a time in the group order above -- no blocking, no partial sums; the q
 * loop of a small group runs from 0 upwards into a sum of its own that is then added as one term.  The order depends on the pair's
 * own events only -- not on other latents or classes, C, the launch or timing: two calls give the same bits, a latent scored alone
 * gives the bits it has among others, and so does a class.  Integer atomics only (digit counts, class counts, the error word).
 * OUTPUTS (device): ap (S x C fp64), pos (C int64), best_ap (S fp64: the row maximum of ap) and best_class (S int32: the LOWEST
 * column that attains it); best_* may be NULL.  err is int32[0] at off_err of the workspace: 0, or the largest SAEV_LATENT_AP_ERR_*
 * met on the device (a class id outside [-1, C), a latent outside [0, S)); the caller reads it when it next synchronises, and the
 * outputs are void if it is not 0.
 * The call also leaves in the workspace (byte offsets, all multiples of 256: saev_latent_ap_layout_of) the stored entries sorted by
 * (latent, value descending, row ascending), non-events last: key (nnz uint32: ~k(v), k the order-preserving image of the fp32
 * value), latent (nnz uint32; S for a non-event), row (nnz int32), and starts (S + 1 int64: latent j's events are
 * [starts[j], starts[j + 1]), starts[S] = the number of events).  The sort is a stable LSD radix sort of `passes` 8-bit passes over
 * `parts` contiguous parts of part_len entries; key2 / latent2 / row2 and hist (the 256 x parts digit table and 256 totals) are its scratch.
 * Arguments are checked before the device is touched; a refused call leaves its message with saev_last_error(NULL).  Nothing is
 * allocated, nothing is read back and nothing synchronises.  workspace: saev_latent_ap_workspace_bytes(N, S, C, nnz) bytes of device
 * memory, 256-byte aligned; its size depends on nnz and S only (24 bytes per stored entry, 8 per latent) -- never an N x S, N x C
 * or nnz x C array. */
#define SAEV_LATENT_AP_ERR_CLASS 1
#define SAEV_LATENT_AP_ERR_LATENT 2
typedef struct {               /* byte offsets into the workspace (all multiples of 256) */
    int32_t struct_size;
    int32_t direct_max;        /* tie groups of at most this many rows are summed term by term */
    int64_t parts, part_len;   /* the sort's parts */
    int64_t passes;            /* 4 over the value + as many as the bytes of S */
    int64_t total_bytes;
    int64_t off_err, off_starts, off_hist, off_key, off_latent, off_row, off_key2, off_latent2, off_row2;
} saev_latent_ap_layout;
int64_t saev_latent_ap_workspace_bytes(int64_t N, int64_t S, int64_t C, int64_t nnz);
int saev_latent_ap_layout_of(int64_t N, int64_t S, int64_t C, int64_t nnz, saev_latent_ap_layout* out);
int saev_latent_ap(const int64_t* row_ptr, const int32_t* indices, const float* data, int64_t nnz, int64_t N, int64_t S, int64_t C,
                   const uint8_t* class_u8, const int32_t* remap, const int32_t* class_i32, double* ap, int64_t* pos, double* best_ap,
                   int32_t* best_class, void* workspace, int64_t workspace_bytes, void* stream);
/* PROBE AP (the reference's contrib/trait_discovery tdiscovery.metrics: the fitted probes of PROBE1D scored on another split),
 * context-free; DESIGN.md 3.21.  For every pair (j, c) with w = w[j, c] and b = b[j, c]: the exact tie-aware AP of the score
 * w * a + b of latent j as a detector of class c over N rows, the counts behind precision and recall at the threshold s > 0, and
 * the top rows of every latent.
 * CARRIED OVER FROM LATENT AP UNCHANGED: x, the shapes and their limits, the two label forms, the event rule (a stored +-0.0 is no
 * event), term(g, c), dH, direct_max, pos_c, the arithmetic and the order of addition, the workspace
 * (saev_latent_ap_workspace_bytes(N, S, C, nnz), the same layout, the same sorted arrays left behind), the argument checks before
 * the device is touched, saev_last_error(NULL); nothing is allocated, nothing is read back, nothing synchronises; integer atomics
 * only.
 * SCORE: s(a) = fl(fl(w * a) + b) in the arithmetic of score_dtype (0 = fp32, 1 = fp64; w and b are S x C arrays of that type), each
 * operation rounded on its own, no contraction; in fp64 a is converted exactly -- what numpy computes for
 * acts.astype(float32) * w + b.  A row without an event has a = 0, so s = b.  With finite a, w and b no NaN arises; w * a may
 * overflow to +-Inf, an ordinary ordered value.
 * VOID PAIR: if w or b is not finite, ap = NaN and tp = pred_pos = 0 (also when pos_c = 0); the error word is not set and no other
 * pair is touched.
 * RANKING: all N rows by s, descending.  A TIE GROUP is a maximal set of rows of equal s (== in the score's type, so +0 == -0).
 * TIES ARE DEFINED ON THE ROUNDED SCORE, not on the activation: the score is what a user of the probe ranks by, and two rows whose
 * scores round to the same number cannot be told apart by it.  s is monotone in a (non-decreasing for w > 0, non-increasing for
 * w < 0), so the groups are runs of the value-sorted events: walked by descending value for w > 0, by ascending value for w < 0;
 * w == +-0 gives one group of N rows.  The Z_j rows without an event enter as ONE BLOCK at a = 0 with score b -- behind the positive
 * events and before the negative ones for w > 0, the mirror image for w < 0 (so FIRST when every event is positive) -- and the
 * block MERGES with the neighbouring events whose score equals b (|w a| < ulp(b) / 2 makes such neighbours).
 * t, n, r, R of a group and AP[j, c] = (sum over g of term(g, c)) / pos_c (0 when pos_c = 0) are LATENT AP's, in the group order
 * of this ranking.
 * COUNTS: pred_pos = the rows with s > 0 (the zero block counts when b > 0), tp = those of them that belong to class c; exact
 * integers.
 * DETERMINISM: a pair's bits depend on its own events, w and b only -- not on other pairs, C, the launch or timing; two calls give
 * the same bits.  With w = 1, b = 0 the ranking is LATENT AP's and so are the bits of ap.
 * TOP ROWS (top_k > 0): top_row[j, i] for i < min(top_k, m_j) = the row of latent j's i-th event in (value descending, row
 * ascending) order, and 0 for the remaining i (the padding of csr_topk(axis=0)); any top_k up to N.
 * OUTPUTS (device): ap (S x C fp64), pos (C int64), tp and pred_pos (S x C int64), top_row (S x top_k int64, or top_k = 0 and NULL).
 * top_k < 0 or top_k > N, a score_dtype other than 0 or 1, and a NULL w, b, ap, pos, tp or pred_pos are SAEV_INVALID_ARG.  err is
 * int32[0] at off_err of the workspace: 0, or the largest of SAEV_LATENT_AP_ERR_CLASS, SAEV_LATENT_AP_ERR_LATENT and
 * SAEV_PROBE_AP_ERR_VALUE (a stored value that is not finite: unlike LATENT AP, +-Inf is refused, for Inf * w + b need not be
 * ordered) met on the device; the outputs are void if it is not 0. */
#define SAEV_PROBE_AP_ERR_VALUE 3
int saev_probe_ap(const int64_t* row_ptr, const int32_t* indices, const float* data, int64_t nnz, int64_t N, int64_t S, int64_t C,
                  const uint8_t* class_u8, const int32_t* remap, const int32_t* class_i32,
                  const void* w, const void* b, int32_t score_dtype,          /* S x C each; 0 = fp32, 1 = fp64 */
                  double* ap, int64_t* pos, int64_t* tp, int64_t* pred_pos,   /* S x C, C, S x C, S x C */
                  int32_t top_k, int64_t* top_row,                            /* S x top_k, or top_k = 0 and NULL */
                  void* workspace, int64_t workspace_bytes, void* stream);
/* LATENT AUROC (the reference's contrib/mimics mimics.scoring: every latent ranked by AUROC on every binary task; and the
 * one-vs-rest companion of LATENT AP at token level), context-free; DESIGN.md 3.23.  AUROC[j, t] of latent j's activation as a
 * detector of task t's positives against its negatives over the N rows, EXACT AND TIE-AWARE (the Mann-Whitney statistic with a tied
 * pair counted half), for all S x T pairs in one call, with the per-role supports and sums of the activation.
 * CARRIED OVER FROM LATENT AP UNCHANGED: x, the shapes and their limits, the two label forms, the event rule (a stored +-0.0 is no
 * event; negative values and +-Inf are ordered events), pos, the sorted arrays left behind in the workspace, the argument checks
 * before the device is touched, saev_last_error(NULL); nothing is allocated, nothing is read back, nothing synchronises; integer
 * atomics only.
 * TASKS: role is T x C uint8, row-major, on the device: role[t, c] = 0 leaves the rows of class c out of task t, 1 makes them its
 * negatives, 2 its positives.  1 <= T <= 4096 (else SAEV_UNSUPPORTED, and -1 from the workspace-size function).  A row of class -1
 * is left out of every task.  Tasks may overlap freely.  A role byte above 2 sets SAEV_LATENT_AUROC_ERR_ROLE in the error word.
 * COUNTS: n_pos[t] / n_neg[t] = the rows whose class has role 2 / 1 in task t.
 * STATISTIC: a TIE GROUP is a maximal set of rows of equal activation (fp32 ==; a row without an event has activation 0).  For task
 * t, over its included rows only and the groups taken in descending order, with p_g / q_g the group's positives / negatives and P_g
 * the positives in strictly higher groups:
 *   U2[j, t] = sum_g (2 q_g P_g + p_g q_g)        = 2 x (pairs with the positive strictly above the negative) + (tied pairs).
 * The rows without an event are ONE group between the positive and the negative values; one forward walk of the events in (value
 * descending) order computes the sum as if that group were absent and keeps Ppos (positives among the events of value > 0), Qneg
 * (negatives among the events of value < 0) and the event totals Pev, Qev; with p0 = n_pos - Pev and q0 = n_neg - Qev the walk ends
 * with U2 += 2 q0 Ppos + p0 q0 + 2 p0 Qneg.  All of it is int64: U2 <= 2 n_pos n_neg < 2^62.
 *   auroc[j, t] = (double)U2 / ((2.0 * (double)n_pos) * (double)n_neg), one fp64 division, no contraction; NaN (0x7ff8000000000000)
 * when n_pos n_neg = 0 (U2 is 0 then).  A latent without events gets exactly 0.5.
 * PER-ROLE STATISTICS: fire_pos / fire_neg[j, t] = the included rows of that role with value > 0; sum_pos / sum_neg[j, t] = the event
 * values of that role, each converted exactly to fp64 and added one at a time in walk order (value descending, row ascending) to a
 * sum that starts at +0; a non-finite sum is what IEEE gives.
 * DETERMINISM: a pair's outputs depend on its own latent's events, the row classes and its own row of role only -- not on other
 * latents or tasks, T, the launch or timing; two calls give the same bits, a task scored alone gives the bits it has among others,
 * and so does a latent.
 * OUTPUTS (device): auroc (S x T fp64), u2 (S x T int64), n_pos and n_neg (T int64), fire_pos and fire_neg (S x T int64), sum_pos and
 * sum_neg (S x T fp64), pos (C int64); none may be NULL, nor may role (SAEV_INVALID_ARG).  err is int32[0] at off_err of the
 * workspace: 0, or the largest of SAEV_LATENT_AP_ERR_CLASS, SAEV_LATENT_AP_ERR_LATENT and SAEV_LATENT_AUROC_ERR_ROLE met on the
 * device; the outputs are void if it is not 0.
 * WORKSPACE: saev_latent_auroc_workspace_bytes(N, S, C, T, nnz) bytes, 256-byte aligned.  It BEGINS with LATENT AP's layout for
 * (N, S, C, nnz) -- saev_latent_ap_layout_of locates err, starts and the sorted arrays -- and at that layout's total_bytes follows
 * the class-major role table: (C + 1) rows of Tp = 64 ceil(T / 64) bytes, row c + 1 = the roles of class c in tasks 0 .. Tp - 1
 * (0 behind T, and for a byte above 2), row 0 = zeros for class -1.  Nothing else. */
#define SAEV_LATENT_AUROC_ERR_ROLE 4
int64_t saev_latent_auroc_workspace_bytes(int64_t N, int64_t S, int64_t C, int64_t T, int64_t nnz);
int saev_latent_auroc(const int64_t* row_ptr, const int32_t* indices, const float* data, int64_t nnz, int64_t N, int64_t S, int64_t C,
                      const uint8_t* class_u8, const int32_t* remap, const int32_t* class_i32,
                      const uint8_t* role, int64_t T,                             /* T x C */
                      double* auroc, int64_t* u2, int64_t* n_pos, int64_t* n_neg, /* S x T, S x T, T, T */
                      int64_t* fire_pos, int64_t* fire_neg, double* sum_pos, double* sum_neg, /* S x T each */
                      int64_t* pos,                                               /* C */
                      void* workspace, int64_t workspace_bytes, void* stream);
/* LATENT OPERATING POINTS (the second property of a good latent in the reference's contrib/mimics logbook: "high precision and
 * recall ... for some threshold"), context-free; DESIGN.md 3.29.  For every latent j and every binary task t: the threshold theta at
 * which the rule "a >= theta => positive" has the best F1, the one at which it has the best Youden J, and the confusion counts at
 * both, for all S x T pairs in one call, EXACT: the scores are ratios of integers and the argmax is decided on the integers.
 * CARRIED OVER FROM LATENT AUROC UNCHANGED: x, the shapes and their limits (1 <= T <= 4096), the two label forms, the event rule (a
 * stored +-0.0 is no event; negative values and +-Inf are ordered events; a row without an event has activation 0; NaN is outside the
 * contract), role (0 out, 1 negative, 2 positive), n_pos, n_neg, pos, the error word and its three codes, the workspace and what is
 * left in it, the argument checks before the device is touched; nothing is allocated, nothing is read back, nothing synchronises;
 * integer atomics only, and only in the shared front half (class counts, the sort's digit counts, the error word).
 * CANDIDATES: for latent j and task t, over the task's included rows only: "predict nothing" (reported theta = +Inf, TP = FP = 0), and
 * every distinct activation value v of those rows (the rows without an event contribute the value 0), with
 *   TP(v) / FP(v) = the task's positives / negatives with a >= v (fp32 comparison).
 * OBJECTIVES, both maximised over the candidates on integers:
 *   F1 = 2 TP / (TP + FP + n_pos): candidate a beats candidate b iff TP_a (TP_b + FP_b + n_pos) > TP_b (TP_a + FP_a + n_pos) as
 *        unsigned 64-bit products of factors below 2^32;
 *   J  = TP / n_pos - FP / n_neg: J2 = TP n_neg - FP n_pos compared as int64, |J2| < 2^62.
 * TIES go to the HIGHER threshold, "predict nothing" being the highest.  So a value whose rows change neither count of the task
 * never wins, the winning J2 is >= 0 with 0 meaning "predict nothing", and a winner with TP + FP = 0 is "predict nothing".  An event
 * value of +Inf that wins reports theta = +Inf as well, with TP + FP > 0; theta = -Inf predicts every included row.
 * OUTPUTS (device, S x T each): f1 (fp64) = (2.0 * (double)TP) / (double)(TP + FP + n_pos), one division, no contraction, NaN
 * (0x7ff8000000000000) when n_pos = 0; f1_thr (fp32) the winning threshold; f1_tp, f1_fp (int64) the counts there; j2 (int64) the
 * winning TP n_neg - FP n_pos; youden (fp64) = (double)j2 / ((double)n_pos * (double)n_neg), NaN when n_pos n_neg = 0; j_thr (fp32),
 * j_tp, j_fp (int64).  And n_pos, n_neg (T int64), pos (C int64) as LATENT AUROC leaves them.  Precision TP / (TP + FP) and recall
 * TP / n_pos at either point follow from the counts.  ONE ORIENTATION, "high activation => positive": a caller who wants the other
 * swaps the role bytes 1 and 2 in a second task row.
 * DETERMINISM as LATENT AUROC: a pair's outputs depend on its own latent's events, the row classes and its own row of role only.
 * FLAGS: 0, or SAEV_OPERATING_SORTED: the caller vouches that the workspace was left by saev_latent_auroc or saev_latent_operating
 * called with the same x, N, S, C, nnz, labels, T and role, and passes that call's n_pos, n_neg and pos back: they are INPUTS then.
 * The entry then neither counts the classes, nor sorts, nor builds the role table, nor clears the error word (it stays what that
 * call left); x and role are checked for NULL as always and not read, the labels are read.  Without the flag everything is rebuilt.
 * ERRORS: the shape and label refusals of LATENT AUROC in its order, then: role NULL; one of the nine per-pair outputs NULL; a bit of
 * flags other than SAEV_OPERATING_SORTED; n_pos, n_neg or pos NULL; a workspace that is NULL or smaller than
 * saev_latent_operating_workspace_bytes (all SAEV_INVALID_ARG); a workspace that is not 256-byte aligned.
 * WORKSPACE: saev_latent_operating_workspace_bytes(N, S, C, T, nnz) = saev_latent_auroc_workspace_bytes(N, S, C, T, nnz), the same
 * layout. */
#define SAEV_OPERATING_SORTED 1
int64_t saev_latent_operating_workspace_bytes(int64_t N, int64_t S, int64_t C, int64_t T, int64_t nnz);
int saev_latent_operating(const int64_t* row_ptr, const int32_t* indices, const float* data, int64_t nnz, int64_t N, int64_t S, int64_t C,
                          const uint8_t* class_u8, const int32_t* remap, const int32_t* class_i32,
                          const uint8_t* role, int64_t T, int32_t flags,              /* T x C */
                          double* f1, float* f1_thr, int64_t* f1_tp, int64_t* f1_fp,  /* S x T each */
                          int64_t* j2, double* youden, float* j_thr, int64_t* j_tp, int64_t* j_fp, /* S x T each */
                          int64_t* n_pos, int64_t* n_neg, int64_t* pos,               /* T, T, C: outputs, or inputs with the flag */
                          void* workspace, int64_t workspace_bytes, void* stream);
/* LATENT SPATIAL(the third property of a good latent in the reference's contrib/mimics logbook -- spatial coherence -- and idea 4
 * of its README, "spatial activation heatmaps": where on the patch grid a latent fires, per group of images), context-free;
 * DESIGN.md 3.27.  For every latent j and every group g of images: the exact counts behind adjacency, clustering and position
 * consistency (saev_amd/spatial.py), the per-cell maps, and the activation-weighted moments of the firing positions.
 * INPUT: x is CSR over N = n_images * T rows, T = gh * gw: row_ptr, indices, data and nnz as LATENT AP takes them (absolute
 * positions, nnz = row_ptr[N] - row_ptr[0] given by the host).  Rows must be CANONICAL: at most one entry per (row, latent).  Row
 * i * T + p is position p of image i, at grid row r = p / gw and grid column c = p % gw.  group_i32 (n_images int32, device):
 * group_i32[i] in [-1, G); an image of group -1 contributes to nothing.
 * LIMITS (SAEV_UNSUPPORTED, and -1 from the workspace-size function): 1 <= G <= 64; 1 <= gh, gw and T <= 4096; 1 <= N, S < 2^31 and
 * 0 <= nnz < 2^31; S * G * T < 2^31.  N != n_images * gh * gw is SAEV_INVALID_ARG.
 * EVENT RULE: a stored entry FIRES when value > thr (fp32 compare), thr >= 0 given by the host.  NaN never fires; a stored 0, a
 * negative value and a value equal to thr do not fire; +Inf fires.
 * INTEGER OUTPUTS (S x G int64 each, exact).  With F(j, i) the firing positions of latent j in image i and m = |F(j, i)|, summed
 * over the images i of group g:
 *   n_events       sum of m
 *   n_images_fire  images with m >= 1
 *   pairs_h        pairs {(r, c), (r, c + 1)} with both positions in F -- never across the end of a grid row
 *   pairs_v        pairs {(r, c), (r + 1, c)} with both positions in F -- never into the next image
 *   sum_m2         sum of m^2
 *   overlap        sum over p of count_map[j, g, p]^2
 * count_map (S x G x T int32): count_map[j, g, p] = the images of g in which j fires at p.  n_group_images (G int64) = the images of
 * group g.
 * MOMENTS (S x G x 5 fp64): moments[j, g, :] = sum v, sum v r, sum v c, sum v r^2, sum v c^2 over the firing entries.  v is widened
 * exactly to fp64, r^2 and c^2 are integers, and each product is formed in fp64 and is exact (24 bits by at most 24).  Each sum
 * starts at +0 and takes its terms one at a time in ASCENDING ROW order -- no blocking, no partial sums.  sum_map (S x G x T fp64,
 * may be NULL): sum_map[j, g, p] = the same sum of v per cell, in ascending image order.  A non-finite sum is what IEEE gives
 * (+Inf at r = 0 makes sum v r NaN).
 * DETERMINISM: no floating-point atomic.  The outputs of (j, g) depend on j's events and the group ids only -- not on other latents,
 * on G beyond g, on the launch or on timing: two calls give the same bits, and a latent scored alone gives the bits it has among
 * others.  The entry overwrites every output wholly; the caller need not clear them.
 * ERRORS: arguments are checked before the device is touched, in this order: a negative size (N, S, nnz, n_images, gh, gw, G);
 * N, S or nnz of 2^31 or more; N or S of 0; G outside [1, 64]; the grid (gh or gw of 0, T above 4096); N != n_images * gh * gw;
 * S * G * T of 2^31 or more; thr negative or NaN; row_ptr NULL; indices or data NULL with nnz > 0; group_i32 NULL; an output other
 * than sum_map NULL; the workspace NULL or too small; the workspace not 256-byte aligned.  The message is left with
 * saev_last_error(NULL).  err is int32[0] at BYTE 0 of the workspace: 0, or the largest of SAEV_LATENT_SPATIAL_ERR_GROUP (a group id
 * outside [-1, G)) and SAEV_LATENT_SPATIAL_ERR_LATENT (an index outside [0, S)) met on the device.  Both are found in the first pass
 * over the entries (the group ids of images without entries in a pass over group_i32), before any index is used as an address;
 * the caller reads err when it next synchronises, and the outputs are void if it is not 0.  Nothing is allocated, nothing is read
 * back and nothing synchronises.
 * WORKSPACE: saev_latent_spatial_workspace_bytes(n_images, T, S, G, nnz) bytes of device memory, 256-byte aligned: 12 bytes per
 * stored entry, 12 per latent and the counting sort's table of at most 2^26 counters -- never an N x S or nnz x G array.
 * LIMIT: a latent's events are walked by one wave, 64 at a time; a latent that fires on most rows is a serial walk. */
#define SAEV_LATENT_SPATIAL_ERR_GROUP 1
#define SAEV_LATENT_SPATIAL_ERR_LATENT 2
int64_t saev_latent_spatial_workspace_bytes(int64_t n_images, int64_t T, int64_t S, int64_t G, int64_t nnz);
int saev_latent_spatial(const int64_t* row_ptr, const int32_t* indices, const float* data, int64_t nnz, int64_t N, int64_t n_images,
                        int64_t gh, int64_t gw, int64_t S, const int32_t* group_i32, int64_t G, float thr,
                        int64_t* n_group_images,                                    /* G */
                        int64_t* n_events, int64_t* n_images_fire, int64_t* pairs_h, int64_t* pairs_v, int64_t* sum_m2,
                        int64_t* overlap,                                           /* S x G each */
                        double* moments,                                            /* S x G x 5 */
                        int32_t* count_map, double* sum_map,                        /* S x G x T each; sum_map may be NULL */
                        void* workspace, int64_t workspace_bytes, void* stream);
/* LATENT EXEMPLARS (ideas 1 and 5 of the reference's contrib/mimics README: per-class activation grids with labels, and the
 * counter-example explorer -- the wrong class's images that fire strongly, the right class's images that stay silent),
 * context-free; DESIGN.md 3.28.  For every latent j and every group g of images: the k strongest firing images, the k weakest firing
 * images and the first k silent ones, each firing image with its max-pooled value and the patch where that maximum sits.
 * INPUT: as LATENT SPATIAL takes it.  x is CSR over N = n_images * T rows: row_ptr int64 (absolute positions), indices int32, data
 * fp32, nnz = row_ptr[N] - row_ptr[0] given by the host.  Row i * T + p is patch p of image i; T = 1: the rows are images already.
 * At most one entry per (row, latent); rows need not be sorted by column.  group_i32 (n_images int32, device): group_i32[i] in
 * [-1, G); -1 leaves the image out.  thr >= 0 and k >= 1 given by the host.
 * EVENT: a stored entry is an event when its latent lies in [0, S), its value is > thr (fp32 compare: NaN and a value equal to thr
 * are never events, +Inf is) and its image's group is >= 0.
 * PER IMAGE: image i FIRES for latent j when it holds at least one event of j.  Then M(i, j) is the largest event value -- because
 * thr >= 0 the pool_images("max") value -- and P(i, j) the SMALLEST patch index that attains it.
 * OUTPUTS (saev_latent_exemplars_out; latent-major, every one written whole by the call: the caller need not clear them):
 *   n_group_images  G int64: the images of group g (n_g below)
 *   n_fire          S x G int32: the firing images of the group
 *   top_val fp32, top_img int32, top_patch int32 (S x G x k each): the group's firing images in the order (M descending, image
 *                   ascending), the first min(k, n_fire) of them: M, i and P
 *   bot_val, bot_img, bot_patch: the same in the order (M ascending, image ascending).  An image stands in both lists when
 *                   n_fire < 2 k
 *   silent_img      S x G x k int32: the first min(k, n_g - n_fire) images of the group that do NOT fire, in ascending image order
 * Unused slots hold val 0.0, img -1, patch -1.
 * LIMITS (SAEV_UNSUPPORTED; -1 from the workspace-size function for those on its arguments): 1 <= n_images, S < 2^31 and
 * 0 <= nnz < 2^31; 1 <= G <= 64; 1 <= k <= 32; 1 <= T <= 4096; n_images * T < 2^31; S * G * k < 2^31.  nnz = 0 is valid: every list
 * is empty and the silent lists are the first k members of each group.
 * DETERMINISM: no floating-point atomic and no read-back.  Both orders are total, so the outputs of (j, g) depend on j's events and
 * the group ids only -- not on other latents, on the other groups, on the launch or on timing: two calls give the same bits, a
 * latent scored alone (a CSR of that one column) gives the bits it has among others, and so does a group scored alone.
 * ERRORS: arguments are checked before the device is touched, in this order: the refusals every (N, S, C, nnz) analysis entry makes
 * on (n_images, S, nnz) -- a negative size; n_images, S or nnz of 2^31 or more; n_images or S of 0 --; G outside [1, 64]; k outside
 * [1, 32]; T outside [1, 4096]; n_images * T of 2^31 or more; S * G * k of 2^31 or more; thr negative or NaN; row_ptr NULL;
 * indices or data NULL with nnz > 0; group_i32 NULL; out NULL or its struct_size unset; an output NULL; the workspace NULL or too
 * small; the workspace not 256-byte aligned.  The message is left with saev_last_error(NULL).  err is int32[0] at BYTE 0 of the
 * workspace: 0, or the largest of SAEV_LATENT_EXEMPLARS_ERR_GROUP (a group id outside [-1, G)) and
 * SAEV_LATENT_EXEMPLARS_ERR_LATENT (an index outside [0, S)) met on the device, found before any index is used as an address; the
 * caller reads err when it next synchronises, and the outputs are void if it is not 0.  Nothing is allocated, nothing is read back
 * and nothing synchronises.
 * WORKSPACE: saev_latent_exemplars_workspace_bytes(nnz, S, n_images, G) bytes of device memory, 256-byte aligned: 12 bytes per
 * stored entry, 12 per latent, 8 per image and the counting sort's table of at most 2^26 counters -- never an n_images x S array.
 * LIMIT: a latent's events are walked by one wave, 64 at a time; a latent that fires on most rows is a serial walk.
 *
 * saev_latent_patch_rows gathers the patch vectors behind chosen (latent, image) pairs, for the overlays: for query q,
 * out[q, p] (Q x T fp32) = the STORED value of latent q_latent[q] in row q_image[q] * T + p on the bits -- whatever its sign, event
 * or not -- or 0.0 where the row stores none (the first stored one where a row breaks the contract and stores two).  A query with
 * image -1, the padding of the lists above, gives a row of zeros.  err (one int32 on the device, zeroed by the call): 0, or the
 * largest of SAEV_LATENT_EXEMPLARS_ERR_LATENT (a q_latent outside [0, S)) and SAEV_LATENT_EXEMPLARS_ERR_IMAGE (a q_image outside
 * [-1, n_images)) met; such a query's row is zeros.  Refusals, in order: those of the (N, S, C, nnz) entries on (n_images, S, nnz);
 * T outside [1, 4096]; n_images * T of 2^31 or more; Q negative; Q * T of 2^31 or more; then, unless Q = 0 -- which returns SAEV_OK
 * and writes nothing --, row_ptr NULL; indices or data NULL with nnz > 0; q_latent, q_image, out or err NULL. */
#define SAEV_LATENT_EXEMPLARS_ERR_GROUP 1
#define SAEV_LATENT_EXEMPLARS_ERR_LATENT 2
#define SAEV_LATENT_EXEMPLARS_ERR_IMAGE 3
typedef struct {
    int32_t struct_size;     /* sizeof(saev_latent_exemplars_out) of the caller (fields past it read as NULL) */
    int32_t reserved;
    int64_t* n_group_images; /* G */
    int32_t* n_fire;         /* S x G */
    float* top_val;          /* S x G x k, as the six below */
    int32_t* top_img;
    int32_t* top_patch;
    float* bot_val;
    int32_t* bot_img;
    int32_t* bot_patch;
    int32_t* silent_img;
} saev_latent_exemplars_out;
int64_t saev_latent_exemplars_workspace_bytes(int64_t nnz, int64_t S, int64_t n_images, int64_t G);
int saev_latent_exemplars(const int64_t* row_ptr, const int32_t* indices, const float* data, int64_t nnz, const int32_t* group_i32,
                          int64_t n_images, int64_t T, int64_t S, int64_t G, int64_t k, float thr, const saev_latent_exemplars_out* out,
                          void* workspace, int64_t workspace_bytes, void* stream);
int saev_latent_patch_rows(const int64_t* row_ptr, const int32_t* indices, const float* data, int64_t nnz, int64_t n_images, int64_t T,
                           int64_t S, const int32_t* q_latent, const int32_t* q_image, int64_t Q, float* out, int32_t* err, void* stream);
/* SPARSE LINEAR (the training half of the concept audit, the reference's contrib/trait_discovery tdiscovery.classification:
 * aggregate_to_images and the LogisticRegression(penalty="l1") of train_worker_fn), context-free; DESIGN.md 3.20.
 *
 * POOLING.  saev_pool_images turns a token CSR of n_images * tokens_per_image rows (indptr: that many + 1 int64 absolute positions
 * with indptr[last] <= nnz, indices int32 in [0, n_latents), data fp32) into out (n_images x n_latents fp32, row-major): per image
 * and latent the maximum or the mean over the image's tokens_per_image dense values.
 *   SAEV_POOL_MAX   the largest stored value, and 0 as well when the latent is stored in fewer than tokens_per_image of the image's
 *                   rows (so a latent stored in every row with negative values only has a negative maximum).
 *   SAEV_POOL_MEAN  the fp32 sum of the stored values in ascending row order (what a row-by-row fp32 reduction of the dense block
 *                   gives: the implicit zeros change nothing), then ONE fp32 division by (float)tokens_per_image.
 * Rows must be CANONICAL: no column twice in a row (the value of such a column is unspecified; nothing is read or written out of
 * bounds).  The sign of a zero is not specified.  err (one int32 on the device, zeroed by the call): 0, or the largest
 * SAEV_POOL_ERR_* met -- the outputs are void then; the caller reads it when it next synchronises.  A workgroup owns one image and
 * saev_pool_images_range() consecutive latents (accumulators and patch counts in LDS); out is written once, no memset.  1 <=
 * n_images * tokens_per_image < 2^31, 1 <= n_latents < 2^31 and at most 65535 ranges (else SAEV_UNSUPPORTED).  Nothing is allocated,
 * read back or synchronised.
 *
 * L1 LOGISTIC.  Minimises  F(W, b) = C * sum_i loss_i(W, b) + ||W||_1  (the intercept b is not penalised) over X (n x S fp32,
 * row-major, finite) and y (n int32 class indices in [0, K)): scikit-learn's LogisticRegression(penalty="l1", C=C) problem.
 *   K == 2   loss_i = log(1 + exp(-t_i z_i)), t_i = +1 for class 1 and -1 for class 0, z = X w + b: ONE coefficient row.
 *   K >= 3   loss_i = logsumexp_k(z_ik) - z_{i y_i}, Z = X W^T + b: K rows; the intercepts are reported with mean zero.
 * coef_rows = K == 2 ? 1 : K.  2 <= K <= 64, 1 <= n < 2^31, 1 <= S <= 2^30 (else SAEV_UNSUPPORTED, -1 from the size function; K < 2
 * is SAEV_INVALID_ARG); C > 0 and finite, kkt_tol >= 0.
 * STOPPING RULE.  With g = C dLoss/dW and g_b = C dLoss/db at a point (W, b): the residual of a coefficient is |g + sign(w)| where
 * w != 0 and max(|g| - 1, 0) where w == 0, that of an intercept |g_b|; the KKT residual is the largest of them, and the fit is
 * done when it is <= kkt_tol.
 * METHOD.  FISTA in fp64 with backtracking on L (start 1, doubling, never lowered) and function-value restart.  The logits of the
 * last two iterates are kept, so the logits of the extrapolated point y are a combination of the two: an iteration is one gradient
 * pass over X (at y) and one forward pass (at the candidate).  The KKT residual is evaluated AT y, whose gradient the iteration has:
 * when it is within kkt_tol, y is the answer.  A step that fails  f(w+) <= f(y) + <g, w+ - y> + L/2 |w+ - y|^2 + 1e-12 |f(y)|
 * doubles L and the next iteration retries it with the kept gradient; an accepted step whose objective is above the last
 * iterate's while beta != 0 is dropped and the momentum restarts (t = 1) from that iterate.  Control lives in the state block
 * (SAEV_L1_STATE_* doubles at off_state): the kernels of a finished fit, or of a phase an iteration does not need, leave on it in
 * their first instructions, and the host may read it as seldom as it likes -- saev_l1_logistic_iterate(n_iters) enqueues n_iters
 * iterations and never synchronises.  Sums are in an order fixed by (n, S, K): rows of a gradient chunk ascending, chunks ascending,
 * lanes by a butterfly; no float atomics: two fits give the same bits, however the iterations are split over calls.
 * ENTRIES.  _init zeroes the iterate (W = 0, b = 0) and checks X and y (err: int32[0] at off_err, the largest SAEV_L1_ERR_* met);
 * _iterate continues; _result writes coef (coef_rows x S fp64), intercept (coef_rows fp64) and scalars (8 fp64: iterations run, the
 * KKT residual of the returned point, its objective F, done 0/1, L, rejected steps, restarts, 0).  Of a fit that is done the
 * returned point is y; of one that is not, the last iterate -- _result then evaluates its gradient (one more pass), and drops the
 * momentum, so that the residual and the objective are those of what it returns.  All entries of one fit take the same X, y, n, S,
 * K, C, kkt_tol and workspace (saev_l1_logistic_workspace_bytes(n, S, K) bytes of device memory, 256-byte aligned: three weight
 * and three logit arrays, the gradient, n_chunks partial gradients, r, two loss vectors and the per-block sums).  Arguments are
 * checked before the device is touched; a refused call leaves its message with saev_last_error(NULL). */
#define SAEV_POOL_MAX 0
#define SAEV_POOL_MEAN 1
#define SAEV_POOL_ERR_COLUMN 1
#define SAEV_POOL_ERR_VALUE 2
#define SAEV_POOL_ERR_INDPTR 3
#define SAEV_L1_ERR_VALUE 1
#define SAEV_L1_ERR_CLASS 2
#define SAEV_L1_STATE_WORDS 16
#define SAEV_L1_STATE_ITER 0       /* iterations run (accepted, rejected and restarted ones alike) */
#define SAEV_L1_STATE_L 1
#define SAEV_L1_STATE_T 2
#define SAEV_L1_STATE_BETA 3       /* y = w + beta (w - w_prev) */
#define SAEV_L1_STATE_F 4          /* F of the last iterate */
#define SAEV_L1_STATE_FY 5         /* C * loss at y */
#define SAEV_L1_STATE_KKT 6        /* the KKT residual last evaluated (at y) */
#define SAEV_L1_STATE_OBJ 7        /* F of the returned point, once done or after _result */
#define SAEV_L1_STATE_DONE 8
#define SAEV_L1_STATE_NEED_GRAD 9  /* 0 after a rejected step: the next iteration keeps the gradient */
#define SAEV_L1_STATE_CUR 10       /* which of the three weight / logit arrays holds w, w_prev and the candidate */
#define SAEV_L1_STATE_PREV 11
#define SAEV_L1_STATE_NEXT 12
#define SAEV_L1_STATE_REJECTS 13
#define SAEV_L1_STATE_RESTARTS 14
typedef struct {               /* byte offsets into the workspace (all multiples of 256) */
    int32_t struct_size;
    int32_t coef_rows;         /* K == 2 ? 1 : K */
    int64_t chunk_rows, n_chunks;  /* the gradient's row chunks: a multiple of 64 rows each, at most 32 */
    int64_t col_blocks;        /* workgroups of 256 columns over the S + 1 columns (the intercept is column S) */
    int64_t total_bytes;
    int64_t off_err, off_state, off_w, off_z, off_g, off_part, off_r, off_loss, off_bp;
} saev_l1_logistic_layout;
int64_t saev_pool_images_range(void);
int saev_pool_images(const int64_t* indptr, const int32_t* indices, const float* data, int64_t nnz, int64_t n_images,
                     int64_t tokens_per_image, int64_t n_latents, int32_t agg, float* out, int32_t* err, void* stream);
int64_t saev_l1_logistic_workspace_bytes(int64_t n, int64_t S, int64_t K);
int saev_l1_logistic_layout_of(int64_t n, int64_t S, int64_t K, saev_l1_logistic_layout* out);
int saev_l1_logistic_init(const float* X, const int32_t* y, int64_t n, int64_t S, int64_t K, double C, double kkt_tol, void* workspace,
                          int64_t workspace_bytes, void* stream);
int saev_l1_logistic_iterate(const float* X, const int32_t* y, int64_t n, int64_t S, int64_t K, double C, double kkt_tol, int32_t n_iters,
                             void* workspace, int64_t workspace_bytes, void* stream);
int saev_l1_logistic_result(const float* X, const int32_t* y, int64_t n, int64_t S, int64_t K, double C, double kkt_tol, double* coef,
                            double* intercept, double* scalars, void* workspace, int64_t workspace_bytes, void* stream);
/* POOL CSR (token codes pooled to an image-level CSR, never through an n_images x n_latents matrix: what the image-level forms of
 * LATENT AUROC, LATENT OPERATING, LATENT HIST and COACTIVATION read), context-free; DESIGN.md 3.30.
 *
 * INPUT.  A token CSR as saev_pool_images takes it: indptr (n_images * tokens_per_image + 1 int64 absolute positions with
 * indptr[last] <= nnz), indices int32 in [0, n_latents), data fp32; row i * tokens_per_image + p is patch p of image i.  Columns
 * inside a row need not be sorted and a column may occur twice in a row.  The threshold of latent l is thr_vec[l] when thr_vec (n_latents
 * fp32 on the device) is not NULL, and the scalar thr otherwise.
 * CONTRACT.  Entry (i, l) of the output exists iff some patch of image i stores a value a of latent l with a > thr_l (strict: a NaN
 * threshold passes nothing, +Inf silences the latent).  out_indptr (n_images + 1 int64, out_indptr[0] = 0), out_indices (int32,
 * ascending inside every row), out_data (fp32: the maximum of the qualifying stored values, on the bits), and, unless NULL,
 * out_patch (int32: the LOWEST patch index that attains the maximum, as LATENT EXEMPLARS) and out_count (int32: the stored entries
 * of that image and latent that pass, a repeated column counting every time).  With thr = 0 the output is the non-zero pattern and
 * the values of max(saev_pool_images(SAEV_POOL_MAX), 0).  A scalar thr must be finite and >= 0 (a negative one would admit the
 * implicit zeros: SAEV_INVALID_ARG); a negative entry of thr_vec is SAEV_POOL_CSR_ERR_THRESHOLD.
 * TWO CALLS, for the output's length is data.  saev_pool_csr_count writes ALL of out_indptr (the scan over images runs on the
 * device); the caller reads out_indptr[n_images], provides arrays of that length, and saev_pool_csr_fill -- with the same input,
 * thresholds and workspace, which carries every unit's first position from the one call to the other -- writes every element of
 * them below out_indptr[n_images] exactly once: no memset of the outputs is needed and nothing at or past that length is touched.
 * A fill that does not follow such a count writes nothing where the lengths differ and reports SAEV_POOL_CSR_ERR_INDPTR.  Neither
 * call allocates, reads back or synchronises; no floating-point atomics: two calls give the same bits.
 * err (one int32 on the device, zeroed by either call): 0, or the largest SAEV_POOL_CSR_ERR_* met -- the outputs are void then;
 * out-of-range columns and a bad indptr read and write nothing out of bounds.
 * A workgroup owns one image and saev_pool_csr_range() consecutive latents (a bit set, and in the fill pass the keys and counts of
 * the set's members, in LDS), and walks the image's span of stored entries however long it is.  workspace:
 * saev_pool_csr_workspace_bytes(n_images, tokens_per_image, n_latents, nnz) bytes of device memory, 256-byte aligned -- with units =
 * n_images * ceil(n_latents / range): units + 1 int64 and ceil(units / 4096) int64, each rounded up to 256 bytes (-1 for a shape
 * the entries refuse).  LIMITS: 1 <= n_images * tokens_per_image < 2^31, 1 <= n_latents < 2^31, and n_images * ceil(n_latents /
 * saev_pool_csr_range()) < 2^31 (else SAEV_UNSUPPORTED).  Arguments are checked before the device is touched, in the order: sizes,
 * the scalar threshold, input pointers, output pointers, workspace; a refused call leaves its message with saev_last_error(NULL). */
#define SAEV_POOL_CSR_ERR_COLUMN 1     /* a column index outside [0, n_latents) */
#define SAEV_POOL_CSR_ERR_VALUE 2      /* a stored value that is not finite */
#define SAEV_POOL_CSR_ERR_INDPTR 3     /* indptr is not a non-decreasing sequence of positions into indices */
#define SAEV_POOL_CSR_ERR_THRESHOLD 4  /* a negative entry of thr_vec */
int64_t saev_pool_csr_range(void);
int64_t saev_pool_csr_workspace_bytes(int64_t n_images, int64_t tokens_per_image, int64_t n_latents, int64_t nnz);
int saev_pool_csr_count(const int64_t* indptr, const int32_t* indices, const float* data, int64_t nnz, int64_t n_images,
                        int64_t tokens_per_image, int64_t n_latents, float thr, const float* thr_vec, int64_t* out_indptr, void* workspace,
                        int64_t workspace_bytes, int32_t* err, void* stream);
int saev_pool_csr_fill(const int64_t* indptr, const int32_t* indices, const float* data, int64_t nnz, int64_t n_images,
                       int64_t tokens_per_image, int64_t n_latents, float thr, const float* thr_vec, const int64_t* out_indptr,
                       int32_t* out_indices, float* out_data, int32_t* out_patch, int32_t* out_count, void* workspace,
                       int64_t workspace_bytes, int32_t* err, void* stream);
/* COACTIVATION (latents matched by what they fire on: idea 8, "cross-run feature alignment", of the reference's
 * contrib/mimics/README.md, which the reference never built), context-free; DESIGN.md 3.25.
 *
 * A (N x Sa) and B (N x Sb) are CSR matrices over the SAME N rows, each as every analysis entry takes it (indptr: N + 1 int64
 * absolute positions with indptr[last] <= nnz, indices int32 in [0, S), data fp32); rows must be CANONICAL (no column twice in a
 * row; the result for such a row is unspecified, nothing is read or written out of bounds).  A stored entry FIRES when value > thr
 * (value == thr does not).  The firing set of a latent is the set of rows in which it fires; n_a (Sa int32) and n_b (Sb int32) are
 * the set sizes, I(a, b) the number of rows in which a of A and b of B both fire.  For every latent a the call writes its top_m
 * partners b with I(a, b) >= 1 to out_index (Sa x top_m int32) and their I to out_inter (Sa x top_m int32), best first; a latent
 * with fewer partners is padded with index -1 and intersection 0.  b_indptr == NULL matches A against itself: the pair b == a is no
 * partner, Sb, nnz_b, thr_b, b_indices, b_data and n_b are ignored (n_b may be NULL; the supports are n_a).
 * THE ORDER is defined on integers, so that every correct implementation gives the same answer:
 *   SAEV_COACT_JACCARD      I / (n_a + n_b - I).  With U = n_a + n_b - I, b1 ranks before b2 iff I1 * U2 > I2 * U1 in unsigned 64-bit
 *                           (I < 2^31, U < 2^32); on equality iff b1 < b2.
 *   SAEV_COACT_CONTAINMENT  I / n_a ("which latent covers a's rows").  b1 ranks before b2 iff I1 > I2; then n_b1 < n_b2; then b1 < b2.
 * Floating-point similarities are the caller's to form from the integers; none is formed inside.
 * err (one int32 on the device, zeroed by the call): 0, or the largest SAEV_COACT_ERR_* met in A or B -- the outputs are void then,
 * nothing is read or written out of bounds, and the caller reads the word when it next synchronises.
 * METHOD.  The firing entries of A are counted per latent and their rows placed under their latent (integer global atomics; the
 * order inside a latent is free, everything downstream is a count).  A workgroup owns one latent a and a window of
 * saev_coactivation_window() latents of B (fewer, with more workgroups a CU, where Sb is smaller) as uint32 counters in LDS: for every row of a's list a lane group reads B's row and adds 1
 * to the counter of each firing entry inside the window, then the non-zero counters become keys and the best 8 are kept; Sb past
 * the window takes further windows.  A latent with more than saev_coactivation_chunk_rows() rows is cut into chunks of that many,
 * each walked by its own workgroup and added into a global int32 row of Sb counters, which a second kernel ranks;
 * saev_coactivation_slots() such rows exist and the heavy latents are taken that many at a time.  No float atomics: two calls
 * give the same bits, and so does any order of the rows.
 * 1 <= N, Sa, Sb < 2^31, 0 <= nnz_a, nnz_b < 2^31 (else SAEV_UNSUPPORTED, -1 from the size function), 1 <= top_m <= 8.  workspace:
 * saev_coactivation_workspace_bytes(N, Sa, Sb, nnz_a, nnz_b) bytes of device memory, 256-byte aligned (for B == NULL: Sb = Sa, nnz_b =
 * nnz_a): the offsets and cursors (Sa), the event list (nnz_a), the heavy list, and min(heavy bound, slots) x Sb counters, where
 * the heavy bound is min(Sa, nnz_a / (chunk_rows + 1)).  Arguments are checked before the device is touched; a refused call leaves
 * its message with saev_last_error(NULL).  Nothing is allocated, read back or synchronised. */
#define SAEV_COACT_JACCARD 0
#define SAEV_COACT_CONTAINMENT 1
#define SAEV_COACT_ERR_COLUMN 1
#define SAEV_COACT_ERR_VALUE 2
#define SAEV_COACT_ERR_INDPTR 3
int64_t saev_coactivation_chunk_rows(void);
int64_t saev_coactivation_window(void);
int64_t saev_coactivation_slots(void);
int64_t saev_coactivation_workspace_bytes(int64_t N, int64_t Sa, int64_t Sb, int64_t nnz_a, int64_t nnz_b);
int saev_coactivation(const int64_t* a_indptr, const int32_t* a_indices, const float* a_data, int64_t nnz_a, int64_t Sa,
                      const int64_t* b_indptr, const int32_t* b_indices, const float* b_data, int64_t nnz_b, int64_t Sb, int64_t N,
                      float thr_a, float thr_b, int32_t measure, int32_t top_m, int32_t* n_a, int32_t* n_b, int32_t* out_index,
                      int32_t* out_inter, int32_t* err, void* workspace, int64_t workspace_bytes, void* stream);
/* PARAMETER OWNERSHIP.  With the f16r encoder the context keeps, from one call to the next, what its forward needs of W_enc
 * (fp16 operand images, a slice-major fp32 transpose, bias and norm shares: written by the Adam launch of saev_train_step, or by
 * the last forward that prepared them itself) and uses it for as long as only the library has written the parameter buffer.  A
 * caller that writes W_enc / b_enc / W_dec itself -- loads a checkpoint, broadcasts, pokes a value -- must say so before the
 * next call; saev_bind does it implicitly.  (The Python host calls it whenever torch's version counter of the buffer moved.)
 * Behind the contract, two checks so that a forgotten announcement is never a silent wrong answer:
 *   (1) before the images are used: every streamed step compares ALL of b_enc and a few thousand pseudo-random elements of W_enc
 *       with the copies its images came with; a difference sends that step down the exact dense route (correct codes, a slow
 *       step) and makes the next forward prepare from scratch.  Any write to b_enc and any bulk write to W_enc end here.
 *   (2) after they were used: the fused Adam of saev_train_step leaves two checksum words per 32 x 256 tile of W_enc as it writes
 *       it and compares them with the tile as it reads it one step later -- every element, at no extra traffic.  A write to even
 *       one element that (1) missed is found at the end of the first step that ran on the stale images; that step cannot be
 *       redone, so the next saev_step_forward / saev_train_step returns SAEV_STALE_PARAMS (once; saev_last_error says how many
 *       tiles) and the context prepares from scratch from there on. */
int saev_params_touched(saev_ctx* ctx);

/* Codes / reconstruction of the last saev_step_forward (device pointers into context scratch):
 * idx,val (n_rows x top_k); x_hat (n_rows x d_model). */
const int32_t* saev_last_idx(saev_ctx* ctx);
const float* saev_last_val(saev_ctx* ctx);
const float* saev_last_x_hat(saev_ctx* ctx);

/* Device-to-device copies of the same into caller buffers (any may be NULL), which hold `n_rows` rows:
 * n_rows must equal the batch of the last saev_step_forward (anything else is SAEV_INVALID_ARG). */
int saev_copy_last(saev_ctx* ctx, int32_t n_rows, int32_t* idx_out, float* val_out, float* x_hat_out, void* stream);

/* State of the predicted-bound mechanism (saev_cfg.bound_mode = 1 or 2), read back from the device (synchronises `stream`):
 * the current z (mode 2: the safety factor c, 0.5 .. 0.95), how many fused-encoder launches used predicted bounds and how many
 * of those had to be repeated with guaranteed bounds, and the mean candidate-list length of the last launch (mode 2: of the
 * last step that collected ratios, predicted or not).  Mode 2 counts a launch only when the prediction was really used: steps
 * that take the guaranteed bounds -- see bound_mode -- leave `launches` and `repeats` alone. */
int saev_bound_state(saev_ctx* ctx, float* z, int64_t* launches, int64_t* repeats, float* mean_candidates, void* stream);
/* bound_mode 2, read back likewise: rho_lo, the smallest ratio (exact k-th largest pre-activation) / ||x_b - mu|| over the rows of
 * the last step that left one (NaN: none -- no such step yet, or it ended on the dense route), and how many steps of a pause of
 * the prediction are still to come on the device (0: not paused).  NaN and 0 in the other modes. */
int saev_bound_ratio(saev_ctx* ctx, float* rho_lo, int64_t* pause_left, void* stream);

/* Timing hooks for bench.py: wall duration in ms of the encoder kernel of the last step, measured
 * with HIP events on `stream` (call after the stream has been synchronised).  With bound_mode 2 the events bracket the
 * step's FIRST fused-encoder launch: the predicted one in a predicting step, the guaranteed one in every other step (a pause
 * included).  On a step whose prediction failed the guaranteed repeat is a second encoder launch that is not timed, and on the
 * few steps the device holds back before the host has seen a pause the first launch exits at once: the figure is too small there. */
int saev_enable_kernel_timing(saev_ctx* ctx, int32_t enable);
float saev_last_encoder_ms(saev_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* SAEV_AMD_H */
