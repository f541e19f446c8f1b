/*
 * afr.h -- C ABI of libafr.so, the MI355X (gfx950) training hot path of ai-font-renderer.
 *
 * The reference has no FFI/plugin layer: its hot path is reached only through Python
 * (reference model.py:129-204 forward, :268-270 loss, :292-310 step).  Each entry point below
 * names the reference code it replaces.  Conventions:
 *   - plain pointers and sizes, no torch types; every device buffer is CALLER-allocated and
 *     caller-owned (the library never frees or retains them past afr_plan_destroy);
 *   - all work is enqueued on the caller's hipStream_t (passed as void*), asynchronously: no
 *     hidden device synchronisation, no allocation inside any call except afr_plan_create;
 *   - every call returns 0 on success or a negative AFR_E* code; afr_last_error() gives the text
 *     (thread-local).  Nothing throws across the boundary;
 *   - a plan is not thread-safe: one plan per rank, one process per GPU.
 */
#ifndef AFR_H
#define AFR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AFR_VERSION 1

enum { AFR_OK = 0, AFR_EINVAL = -1, AFR_ESTATE = -2, AFR_EHIP = -3, AFR_EUNSUPPORTED = -4 };

enum { AFR_KIND_SHEET = 0,   /* AttentionFontRenderer, model.py:129-204                         */
       AFR_KIND_GLYPH = 1,   /* per-glyph MLP (BASELINE.json configs C1-C4)                     */
       AFR_KIND_PIXEL = 2 }; /* per-pixel-token transformer (BASELINE.json configs[4]): embed_dim = d_model
                                (<= 512, = 64 * heads), fc_dim = ff width, n_hidden = blocks, out_h * out_w = pixel tokens.
                                Every entry point serves it; one backward stage per block, last block first.                */
enum { AFR_F32 = 0,          /* exact-f32 MFMA everywhere: parity mode (<=1e-4 vs reference)     */
       AFR_BF16 = 1,         /* bf16 MFMA operands, f32 accumulate, f32 master weights           */
       AFR_BF16X3 = 2 };     /* AFR_F32 except that every Linear product (afr_op_gemm and the plan's GEMMs) runs as
                                three bf16 MFMAs on operands split x = hi + lo at staging, f32 accumulate: per product
                                term <= 3*2^-16 relative error, with a 2.5 PF / 3 = 833 TF matrix ceiling against the f32
                                MFMA's 157 TF (DESIGN.md 4 has the measured steps).  f32 activations, memory layout, parameter table
                                and workspace of the AFR_F32 plan; the non-GEMM kernels (sheet front end, fused
                                small glyph net, pixel token kernels) run their exact-f32 path. */
enum { AFR_TARGET_U8 = 0,    /* 8-bit pixels as stored in the BMPs; k/255.0f on device           */
       AFR_TARGET_F32 = 1 }; /* float32 targets as helpers.load_string_dataset returns them      */

enum { AFR_LOSS_MSE = 0,     /* clamp(u,0,1) head + F.mse_loss (model.py:156,268-270): the default            */
       AFR_LOSS_BCE = 1 };   /* sigmoid head + F.binary_cross_entropy_with_logits on u, soft targets k/255:
                                  y = sigmoid(u);  loss = sum(max(u,0) - t u + log1p(exp(-|u|))) / mean_elems;
                                  du = (sigmoid(u) - t) / mean_elems                                          */

#define AFR_MAX_HIDDEN 8

typedef struct afr_config {
    int32_t kind;        /* AFR_KIND_*                                                            */
    int32_t dtype;       /* AFR_F32 | AFR_BF16 | AFR_BF16X3                                       */
    int32_t max_batch;   /* largest B any call will pass                                          */
    int32_t vocab;       /* embedding rows (128, model.py:136)                                    */
    int32_t embed_dim;   /* EMBEDDING_DIM (32, model.py:79)                                       */
    int32_t out_h, out_w;/* SHEET_HEIGHT x SHEET_WIDTH (model.py:64-65) or glyph bitmap size       */
    /* sheet model */
    int32_t max_length;  /* MAX_CHARS_PER_SHEET (model.py:66)                                     */
    int32_t heads;       /* NUM_ATTENTION_HEADS (model.py:81)                                     */
    int32_t fc_dim;      /* fc1 width (64, model.py:148)                                          */
    float p_embed, p_attn, p_fc; /* dropout rates (model.py:137,144,149)                          */
    float ln_eps;        /* LayerNorm eps (1e-5)                                                  */
    /* glyph model */
    int32_t n_hidden;
    int32_t hidden[AFR_MAX_HIDDEN];
    int32_t n_fonts;     /* 0 = no font-id embedding                                              */
    /* dropout stream */
    uint64_t seed;
    int32_t rank;        /* data-parallel rank: gives each replica its own dropout stream         */
    int32_t reserved;    /* bit 0: keep the optimizer un-fused in afr_train_step (gradients of every tensor are
                            then materialised; otherwise the sheet model's fc_output.weight is updated inside its
                            weight-gradient GEMM and its gradient never reaches HBM)
                            bit 1: one launch per product in backward (no grouped dW+dX launches): A/B measurements
                            bit 2: small one-hidden-layer glyph nets through the generic per-layer kernels instead of
                            the fused whole-step kernel of afr_train_step (A/B measurements, parity cross-checks)
                            bit 3: unused
                            bit 4: the glyph nets' folded first layer backward through the weight-gradient GEMM + post-pass
                            instead of the fused kernel (A/B measurements, parity cross-checks)
                            bit 5: weight gradients of grouped 256x256 launches as split-K partial slabs summed by the grouped
                            reduce, instead of the cooperative split-K whose slices meet inside the launch (A/B measurements,
                            parity cross-checks: the two give bitwise equal results)
                            bit 6: the glyph nets' first layer through the gather kernel + dense h1 in training steps too,
                            instead of the (character, font) combination table gathered inside the consuming products
                            bit 7: ReLU masks of the input-gradient products read from the stored activations instead of the
                            bit masks the forward epilogues leave (bits 6, 7: A/B measurements; bitwise equal results)
                            bit 8: the output layer's and the last hidden layer's cooperative gradient pairs as two grouped
                            launches instead of ONE chained launch (A/B measurements; bitwise equal results)
                            bit 9: the folded first layer's fused backward as a launch of its own behind that chained launch,
                            instead of as the launch's fifth role, handed its d1 inside the launch (A/B measurements; bitwise
                            equal results)                                                                                  */
    int32_t loss;        /* AFR_LOSS_*: the output head and loss of every entry point below (0 = clamp + MSE); any other
                            value is AFR_EINVAL.  Appended after `reserved` (the struct grew by 8 bytes with it): a zero-initialised
                            config means what it meant, a caller compiled against the older header must be rebuilt          */
} afr_config;
/* the bits of afr_config.reserved, as described above */
enum { AFR_CFG_UNFUSED_OPTIMIZER = 1, AFR_CFG_NO_GROUPED_GEMM = 2, AFR_CFG_NO_FUSED_GLYPH1 = 4, AFR_CFG_L1_BWD_UNFUSED = 16,
       AFR_CFG_SLAB_SPLITK = 32, AFR_CFG_NO_COMBO_TABLE = 64, AFR_CFG_RELU_MASK_FROM_ACT = 128, AFR_CFG_NO_PAIR_CHAIN = 256,
       AFR_CFG_NO_L1_CHAIN = 512 };

typedef struct afr_plan afr_plan;

int afr_version(void);
const char* afr_last_error(void);

/* Build the launch plan (shapes, workspace carve-up).  Replaces nn.Module construction,
 * model.py:130-156 (no parameters are created: see afr_bind). */
int afr_plan_create(const afr_config* cfg, afr_plan** out);
int afr_plan_destroy(afr_plan* plan);

/* Flat parameter layout: all tensors of state_dict(), in state_dict order, live in
 * ONE float32 buffer of afr_param_elems() elements; tensor i starts at offset[i] (multiple of 64
 * elements).  Gradients and the two AdamW moments use the same layout. */
int64_t afr_param_elems(const afr_plan* plan);
int afr_param_count(const afr_plan* plan);
int afr_param_info(const afr_plan* plan, int index, char* name, int name_cap, int64_t* offset,
                   int64_t* numel, int32_t* ndim, int64_t shape[4]);

size_t afr_workspace_bytes(const afr_plan* plan);

/* Attach caller-owned device buffers.  params/grads/exp_avg/exp_avg_sq: afr_param_elems() floats
 * each (grads, moments may be NULL for inference-only use; exp_avg_sq also on a Lion plan, afr_set_optimizer); workspace:
 * afr_workspace_bytes(). */
int afr_bind(afr_plan* plan, float* params, float* grads, float* exp_avg, float* exp_avg_sq,
             void* workspace, size_t workspace_bytes);

/* Re-derive the bf16 shadow weights from the f32 masters after the caller changed them
 * (load_state_dict, helpers.py:100).  No-op in AFR_F32 mode. */
int afr_sync_params(afr_plan* plan, void* stream);

/* forward(x): model.py:158-204.  x int64 [B, L] (sheet; L>max_length truncated, L<max_length
 * zero-padded features) or int64 [B] glyph codes with optional font ids.  y: float32 [B, out_h*out_w]
 * clamped to [0,1] (AFR_LOSS_BCE plan: sigmoid(u)), or NULL when only the saved pre-activation is wanted (training).
 * training!=0 enables the three dropouts with the counter-hash stream (seed, rank, step). */
int afr_forward(afr_plan* plan, const int64_t* x, const int64_t* font, int B, int L, float* y,
                int training, uint64_t step, void* stream);

/* compute_loss + the first backward step: F.mse_loss(clamp(u,0,1), target) (model.py:268-270) and
 * d(loss)/du with the inclusive clamp mask.  Uses the pre-activation the last afr_forward left in
 * the workspace.  mean_elems = B_global*out_h*out_w (the mean's denominator; lets data-parallel
 * shards weight a short last batch exactly).  *loss_accum (device float) += this shard's share.
 * AFR_LOSS_BCE plan: binary cross-entropy with logits on u and du = (sigmoid(u) - t) / mean_elems instead; this call, afr_forward_loss,
 * afr_train_step and the afr_*_rows calls all follow the plan's loss kind. */
int afr_loss_grad(afr_plan* plan, const void* target, int target_dtype, int B, int64_t mean_elems,
                  float* loss_accum, void* stream);

/* Entry for a caller-owned loss (torch.autograd): dy = d(loss)/d(y) for the clamped output y [B, pixels], float32.
 * Applies the clamp's gradient mask (0 <= u <= 1, inclusive) and leaves du where afr_backward expects it.
 * AFR_LOSS_BCE plan: y is the sigmoid output, du = dy * y * (1 - y) with y recomputed from the saved u. */
int afr_set_output_grad(afr_plan* plan, const float* dy, int B, void* stream);

/* loss.backward(): model.py:309.  Overwrites the flat gradient buffer (zero_grad, model.py:292,
 * is implied). */
int afr_backward(afr_plan* plan, void* stream);

/* The same backward in stages (last layer first), for overlapping the gradient all-reduce with the rest of the
 * backward pass under data parallelism: stage k leaves the flat-gradient range [*grad_offset, +*grad_elems) final.
 * Stages must be called in order 0 .. afr_backward_stages()-1. */
int afr_backward_stages(const afr_plan* plan);
int afr_backward_stage(afr_plan* plan, int stage, int64_t* grad_offset, int64_t* grad_elems, void* stream);

/* Training forward with the loss and d(loss)/du computed in the epilogue of the last layer (u never reaches HBM):
 * afr_forward(training) + afr_loss_grad in one pass; follow with afr_backward / afr_backward_stage.  The loss is the plan's
 * (afr_config.loss); fused and unfused paths leave the same du bit for bit. */
int afr_forward_loss(afr_plan* plan, const int64_t* x, const int64_t* font, const void* target, int target_dtype,
                     int B, int L, int64_t mean_elems, float* loss_accum, uint64_t step, void* stream);

/* optimizer.step(): torch.optim.AdamW as configured at model.py:273.  t = 1,2,...; grad_scale
 * multiplies every gradient first (1/world after a sum all-reduce; 1 otherwise). */
int afr_adamw_step(afr_plan* plan, float lr, float beta1, float beta2, float eps, float weight_decay,
                   int64_t t, float grad_scale, void* stream);

/* The optimizer kind of a plan.  AFR_OPT_ADAMW (the default of a new plan) is the update above.  AFR_OPT_LION is Lion (Chen et al.
 * 2023, "Symbolic Discovery of Optimization Algorithms"), which keeps ONE moment:
 *     c = fma(g - m, 1 - beta1, m)                      b1*m + (1-b1)*g
 *     s = (c > 0) - (c < 0)                             0 for c == 0
 *     p = fma(p, decay, -lr * s)                        decay = 1 - lr * weight_decay
 *     m = fma(g - m, 1 - beta2, m)
 * in plain f32, stated once in the library: every path of a step (fused or not, clipped or not, dense or by rows) applies these
 * operations bit for bit.  g enters multiplied by grad_scale (on a clipping plan by fl32(grad_scale * coef), as for AdamW).  Every
 * optimizer step of the plan follows the kind -- afr_adamw_step (which keeps its name), afr_train_step* with do_step -- the way the
 * loss entry points follow afr_config.loss.  eps and t are accepted and ignored by a Lion step (no bias correction; t < 1 stays an
 * error).  exp_avg_sq is neither read nor written: on a Lion plan afr_bind may be given exp_avg_sq = NULL.  The kind may change
 * between steps; an AdamW step on a plan without exp_avg_sq is AFR_ESTATE.  Host-only; any other kind -> AFR_EINVAL. */
enum { AFR_OPT_ADAMW = 0, AFR_OPT_LION = 1 };
int afr_set_optimizer(afr_plan* plan, int kind);

/* ---- optimizer groups: a learning-rate and a weight-decay multiplier per parameter tensor (torch.optim's param groups) ----
 * For the tensor with index i of afr_param_info and multipliers lr_mult[i], wd_mult[i] every optimizer step of the plan uses
 *     lr_i = fl32(lr * lr_mult[i])      wd_i = fl32(weight_decay * wd_mult[i])      (on the host, f32, not contracted)
 * and updates that tensor by the plan's optimizer kind exactly as every site of a step updates it when handed lr_i and wd_i as its
 * lr and weight_decay: the same folding of the scalars, the same roundings -- a multiplier of exactly 1.0f reproduces the bits of a
 * plan without groups.  The 64-element padding behind a tensor belongs to that tensor's range.  beta1, beta2, eps, t, grad_scale,
 * the clip coefficient and the EMA stay global, and the global gradient norm does not see the multipliers.
 * n must equal afr_param_count().  Either pointer may be NULL (all ones for that multiplier); both NULL switch groups off.  Every
 * value must be finite and >= 0 (AFR_EINVAL, checked before anything is stored).  Adjacent tensors with equal multipliers are merged
 * into ranges {end offset, lr_mult, wd_mult} of the flat buffer, which afr_param_group_ranges returns (its result: the number of
 * ranges, 0 = groups off; at most cap of them are written, out may be NULL).  A flat update crosses at most 128 ranges in one launch
 * (AFR_EUNSUPPORTED beyond, never a silent drop).  Host-only: nothing is launched or allocated.  The setting lives in the plan and
 * survives afr_bind; a new plan has no groups.  AFR_ESTATE while afr_use_ema is on. */
typedef struct afr_opt_range { int64_t end; float lr_mult, wd_mult; } afr_opt_range;
int afr_set_param_groups(afr_plan* plan, const float* lr_mult, const float* wd_mult, int n);
int afr_param_group_ranges(const afr_plan* plan, afr_opt_range* out, int cap);

/* Clipping by the GLOBAL gradient norm inside the optimizer step (torch.nn.utils.clip_grad_norm_; the reference's loop has
 * none).  Off by default; with max_norm > 0 every optimizer step of the plan (afr_adamw_step, afr_train_step* with do_step)
 * computes, on the device,
 *     sumsq      = sum of g[i]^2 over the ELEMENTS of the parameter tensors (afr_param_info offsets / numel; the 64-element
 *                  padding between tensors in the flat buffer is not part of the sum)
 *     total_norm = |grad_scale| * sqrt(sumsq)
 *     coef       = min(1, max_norm / (total_norm + 1e-6))                     (f32)
 *     AdamW(p, m, v, g * fl32(grad_scale * coef))
 * The gradient buffer is NOT rescaled in place -- the coefficient lives only inside the update: the one difference from
 * torch.  A sumsq that is not finite (an inf or NaN gradient) SKIPS the step -- params, both moments and the bf16 shadow stay
 * bit-identical -- and sets bit 3 of the error word.  The sum has a fixed order (per lane, wave, block partial, partials in block
 * order): bitwise reproducible.  On a clipping plan afr_train_step* with do_step materialise every gradient (the path
 * AFR_CFG_UNFUSED_OPTIMIZER takes) and end in afr_adamw_step.
 * max_norm: 0 = off; negative or non-finite -> AFR_EINVAL.  stats: caller-owned device float[2] or NULL; every clipped step
 * leaves stats[0] = total_norm, stats[1] = coef.  Host-only: nothing is launched; the setting lives in the plan (a new plan
 * starts with clipping off). */
int afr_set_grad_clip(afr_plan* plan, float max_norm, float* stats);
/* *out (device float) = the sum of squares of the bound gradient buffer over the tensor elements that lie inside
 * [offset, offset + n) of the flat layout -- the logging entry (a gradient norm without copying the buffer back and masking its
 * padding), and the per-rank share of the norm under a sharded optimizer.  offset and n must be multiples of 4 and the range
 * must lie inside the buffer (AFR_EINVAL otherwise).  Works whether clipping is on or off. */
int afr_grad_sumsq(afr_plan* plan, int64_t offset, int64_t n, float* out, void* stream);

/* ---- exponential moving average (EMA) of the weights ----
 * afr_set_ema hands the plan a caller-owned buffer `ema` of afr_param_elems() floats in the parameter layout (256-byte aligned, on
 * the plan's device; the caller initialises it, usually with the parameters -- it is not read before the first update).  From then
 * on every optimizer step the plan performs -- afr_adamw_step, afr_train_step* with do_step, fused or not, clipped or not -- counts
 * one step after its last parameter write, and every `every`-th of them (count % every == 0) ends in ONE more launch over the whole
 * flat buffer, padding included:
 *     alpha = 1.0f - decay                     (f32, on the host)
 *     e[i]  = fmaf(p[i] - e[i], alpha, e[i])   (p: the parameters after the optimizer step)
 * With every = k the average takes every k-th iterate with the same decay (choose decay^k for the same horizon); the pass costs
 * 12 bytes per parameter when it runs.  On a clipping plan (afr_set_grad_clip) a skipped step leaves the EMA bit-identical, like the
 * parameters and the moments; it still ADVANCES the count -- the host cannot know that the step was skipped.
 * ema == NULL switches the EMA off (decay and every are ignored).  Otherwise decay must be finite and inside (0, 1) and every >= 1
 * (AFR_EINVAL; checked before the pointer is looked at).  The call resets the count to 0.  Host-only: nothing is launched.  The
 * setting lives in the plan and survives afr_bind; a new plan starts without an EMA. */
int afr_set_ema(afr_plan* plan, float* ema, float decay, int every);
/* Count one optimizer step that happened OUTSIDE the plan (the sharded data-parallel schedule steps slices with afr_op_adamw /
 * afr_op_lion): the same hook the plan's own steps end in.  sumsq_dev: NULL, or the device word holding the global sum of squared
 * gradients the clipped slice update read -- a non-finite value leaves the EMA untouched.  AFR_ESTATE when no EMA is set. */
int afr_ema_update(afr_plan* plan, const float* sumsq_dev, void* stream);
/* The update on a slice (unit tests; callers that keep an EMA of their own): n a multiple of 4, decay inside (0, 1). */
int afr_op_ema(float* e, const float* p, int64_t n, float decay, const float* sumsq_dev /* NULL = none */, void* stream);
/* Evaluate from the EMA.  on != 0: the plan's parameter and EMA pointers change places and everything a forward reads besides the
 * f32 parameters is re-derived as afr_sync_params does (the bf16 shadow in one pass; the transposed operand copies of the small
 * glyph nets on their next use) -- no second shadow is kept.  While on, afr_forward (training == 0), afr_forward_rows, the
 * afr_loss_grad* that follow them, afr_debug_copy and afr_debug_sheet_gather see the EMA weights, and every call that trains or
 * steps returns AFR_ESTATE: afr_forward with training != 0, afr_forward_loss*, afr_train_step*, afr_backward*, afr_adamw_step,
 * afr_ema_update, afr_set_optimizer (also afr_set_ema and afr_bind).  on == 0 swaps back and re-derives again; a forward saved
 * before either switch cannot be followed by afr_backward.  Switching to the current state launches nothing; switching on without
 * an EMA is AFR_ESTATE. */
int afr_use_ema(afr_plan* plan, int on, void* stream);

/* One whole iteration of the loop body model.py:292-310 on this rank's shard:
 * forward(training) -> loss+grad -> backward [-> AdamW when do_step!=0].  With do_step!=0 the loss is fused into
 * the last forward GEMM and, for the sheet model, the AdamW update of fc_output.weight into its dW GEMM.
 * The loss is the plan's (afr_config.loss). */
int afr_train_step(afr_plan* plan, const int64_t* x, const int64_t* font, const void* target,
                   int target_dtype, int B, int L, int64_t mean_elems, float* loss_accum,
                   uint64_t step, int do_step, float lr, float beta1, float beta2, float eps,
                   float weight_decay, int64_t t, void* stream);

/* ---- HBM-resident data set, addressed by row index (the whole data set lives on the device) ----
 * afr_bind_dataset attaches caller-owned device buffers: x int64 [n_rows][L] codes (glyph / pixel models: L = 1), font
 * int64 [n_rows] or NULL (required when n_fonts > 0), target [n_rows][out_h*out_w] uint8 or float32.  All three NULL
 * unbinds.  Host-only: nothing is launched or copied, the buffers are not read before an afr_*_rows call.  n_rows < 2^31
 * (AFR_EUNSUPPORTED beyond); the target buffer may be larger than 2 GiB (it is addressed with 64-bit arithmetic).
 * The four afr_*_rows calls are the entry points of the same name with a row vector in place of the dense batch: `rows`
 * is a device vector of B int64 indices into the data set, duplicates allowed; batch row b means data-set row rows[b].
 * Dropout is keyed by the in-batch row b, mean_elems / loss_accum / step / the optimizer arguments mean what they mean
 * there, the loss kind is the plan's, and afr_backward / afr_backward_stage / afr_adamw_step follow as usual.  The targets are read where they lie
 * (the loss kernels take the row as an index); codes and font ids of the batch are staged in the workspace by one small
 * kernel, after which (in stream order) `rows` is not read again.  An index outside [0, n_rows) sets bit 2 of the error
 * word and is clamped before anything is addressed with it.  Errors, in this order: no data set bound -> AFR_ESTATE;
 * rows NULL or B outside 1..max_batch -> AFR_EINVAL. */
int afr_bind_dataset(afr_plan* plan, const int64_t* x, const int64_t* font, const void* target, int target_dtype,
                     int64_t n_rows, int L);
int afr_forward_rows(afr_plan* plan, const int64_t* rows, int B, float* y, int training, uint64_t step, void* stream);
/* after afr_forward_rows on the same rows */
int afr_loss_grad_rows(afr_plan* plan, const int64_t* rows, int B, int64_t mean_elems, float* loss_accum, void* stream);
int afr_forward_loss_rows(afr_plan* plan, const int64_t* rows, int B, int64_t mean_elems, float* loss_accum, uint64_t step,
                          void* stream);
int afr_train_step_rows(afr_plan* plan, const int64_t* rows, int B, int64_t mean_elems, float* loss_accum, uint64_t step,
                        int do_step, float lr, float beta1, float beta2, float eps, float weight_decay, int64_t t, void* stream);

/* ---- evaluation on the device: per-sample loss, 8-bit error counts, u8 bitmaps (DESIGN.md 4 "Evaluation") ----
 * afr_eval follows an afr_forward (training 0 or 1) and reads the pre-activation u [B][pixels] that forward saved; afr_eval_rows
 * follows afr_forward_rows on the same rows of the bound data set.  The contract is afr_loss_grad's / afr_loss_grad_rows': B must
 * equal the last forward's.  u is left bit-identical, so afr_loss_grad*, afr_set_output_grad and afr_backward may follow as if
 * nothing had happened.  The call launches ONE kernel and allocates nothing.  Each output is a caller-owned device buffer or NULL.
 * For batch row b and pixel i, with y = the plan's output head of u (clamp(u, 0, 1); sigmoid(u) on an AFR_LOSS_BCE plan) and
 * t = the target as the loss sees it (k / 255.0f for uint8 pixels k, the float otherwise):
 *   q[b][i]      uint8 [B][pixels]: (uint8)(y * 255.0f), truncating -- the level helpers.binary_array_to_image writes to a BMP.
 *                A NaN u gives level 0.  Needs no target.
 *   loss_rows[b] float [B]: (sum_i term(u, t)) / pixels; term = (y - t)^2 (MSE) or max(u,0) - t u + log1p(exp(-|u|)) (BCE), the
 *                values afr_loss_grad sums.  A row that holds a NaN is NaN; no other row is affected.
 *   stats[b][4]  uint32 [B][4], with t8 = k, or rintf(t * 255.f) limited to 0..255 for float targets, and d = |q - t8| over row b:
 *                [0] = #(d >= 1), [1] = #(d >= 2), [2] = max d, [3] = #((q >= 128) != (t8 >= 128)), the wrong-ink pixels.
 * A row is summed by one wave (pixels <= 2048) or one 256-lane workgroup, in float32 and in a fixed order: each of the L = 64 (256)
 * lanes adds the terms of its groups of 8 pixels g = lane, lane + L, ... in ascending order, pixel by pixel; then six butterfly
 * steps across the wave (offsets 32, 16, 8, 4, 2, 1); then, for a workgroup, ((w0 + w1) + w2) + w3 over its four waves; then one
 * division by pixels.  A row's three results therefore depend on that row's data only -- not on B, the row's position or the
 * grid -- and are bitwise reproducible.  No atomics, no communication between workgroups.
 * Errors: all three outputs NULL, target NULL while loss_rows or stats is given, a bad target dtype, B outside 1..max_batch,
 * stats not 16-byte / q or uint8 targets not 8-byte / float32 targets not 16-byte aligned -> AFR_EINVAL; B != the last
 * forward's, or the u buffer already holds du (after afr_loss_grad*, afr_set_output_grad, afr_forward_loss*, afr_train_step*) ->
 * AFR_ESTATE; afr_eval_rows without a bound data set -> AFR_ESTATE.  Both are allowed while afr_use_ema is on: they see whatever
 * the forward saw. */
int afr_eval(afr_plan* plan, const void* target /* or NULL */, int target_dtype, int B,
             float* loss_rows /* or NULL */, uint32_t* stats /* or NULL */, uint8_t* q /* or NULL */, void* stream);
int afr_eval_rows(afr_plan* plan, const int64_t* rows, int B, float* loss_rows, uint32_t* stats, uint8_t* q, void* stream);

/* ---- per-tensor statistics of a flat buffer in the parameter layout (DESIGN.md 4 "Tensor statistics") ----
 * One 32-byte record per parameter tensor, in afr_param_info order.  x is an element of the chosen buffer or, when a second buffer
 * `minus` is given, x = a[i] - minus[i] in f32 (inf - inf then counts as a NaN).  Classification is by bit pattern -- exponent field
 * all ones: infinity (mantissa 0) or NaN; (bits & 0x7fffffff) == 0: zero -- so the counts do not depend on the denormal mode: a
 * denormal is finite and non-zero.  Only the tensor's elements are read, numel of them from its offset; the 64-element padding
 * behind it (arbitrary values after the fused glyph step and the slab reduces) never is. */
typedef struct afr_tensor_stat {
    float    sumsq;   /* sum of x^2 over the FINITE elements, f32, fixed order                   */
    float    sum;     /* sum of x   over the finite elements, f32, same order                    */
    float    min, max;/* over the finite elements; +inf / -inf when there is none                */
    uint32_t n_nan, n_inf, n_zero;   /* n_zero counts +0 and -0                                  */
    uint32_t numel;   /* the tensor's element count as the launch saw it                         */
} afr_tensor_stat;
/* The order of the two sums, with C = afr_tensor_stats_chunk() elements (a compile-time constant of the library, 32768): a tensor of
 * n elements is cut into max(1, ceil(n / C)) chunks, each summed by one 256-lane workgroup.  Lane l takes the groups of 4 elements
 * l, l + 256, ... of its chunk in ascending order and keeps one accumulator pair per position c in the group:
 * q_c = fmaf(x, x, q_c), s_c = s_c + x (a non-finite x enters as 0).  The <= 3 elements behind the tensor's last whole group are
 * added by lanes 0..2 of the tensor's last chunk to their pair 0.  Then (q_0 + q_1) + (q_2 + q_3), six butterfly steps across the
 * wave (offsets 32, 16, 8, 4, 2, 1), (w0 + w1) + (w2 + w3) over the four waves: the chunk's partial record.  A second launch gives
 * one wave to each tensor: lane l adds the partials of chunks l, l + 64, ... in ascending order, then the same butterfly.
 * LOCALITY: a tensor's record depends on that tensor's elements only -- not on its offset, the other tensors in the table or the
 * launch geometry -- and repeats bit for bit.  No atomics, no communication between workgroups, inputs are only read.
 * afr_tensor_stats reads the plan's bound buffer `which` as it stands, launches exactly those two kernels, allocates and synchronises
 * nothing; its partials live in the plan workspace.  minus: NULL, or a device buffer in the flat layout (afr_param_elems() floats,
 * 16-byte aligned).  out: device, afr_param_count() records, 16-byte aligned.
 * GRADIENTS: which gradients a previous call left in the buffer is the caller's knowledge.  After afr_backward, after a
 * do_step == 0 step, on a clipping plan, with AFR_CFG_UNFUSED_OPTIMIZER, or under data parallelism, every tensor's gradient is
 * there; after a fused do_step != 0 step the tensors whose update was fused -- fc_output.weight and the slab-reduced tensors --
 * hold older values.
 * Errors, all detected before anything is launched: out NULL or misaligned, minus misaligned, an unknown `which` -> AFR_EINVAL; the
 * named buffer not bound (no gradients or moments; AFR_STAT_EXP_AVG_SQ on a plan bound without it; AFR_STAT_EMA without afr_set_ema)
 * -> AFR_ESTATE; more than 256 tensors, or one of 2^32 elements or more -> AFR_EUNSUPPORTED, never a silent drop.  Allowed while
 * afr_use_ema is on: AFR_STAT_PARAMS then names the buffer the forward entry points currently read -- the average -- and AFR_STAT_EMA
 * the other one. */
enum { AFR_STAT_PARAMS = 0, AFR_STAT_GRADS = 1, AFR_STAT_EXP_AVG = 2, AFR_STAT_EXP_AVG_SQ = 3, AFR_STAT_EMA = 4 };
int afr_tensor_stats_chunk(void);             /* host-only */
int afr_tensor_stats(afr_plan* plan, int which, const float* minus /* or NULL */, afr_tensor_stat* out, void* stream);

/* Set / read the device-side error word (bit 0: an embedding index outside [0,vocab), the
 * condition on which the reference raises IndexError; model.py:136,167; bit 1: a cooperative split-K
 * workgroup gave up waiting for its partners -- the step's results are invalid; bit 2: a row index of an afr_*_rows call
 * outside the bound data set, clamped into it; bit 3: a clipping plan (afr_set_grad_clip) met gradients whose sum of squares
 * is not finite and skipped that optimizer step).  Reading synchronises and clears. */
int afr_error_flags(afr_plan* plan, void* stream, uint32_t* flags_out);

/* Name and average duration (ms, hipEvent-timed on the launch stream) of the plan's dominant
 * kernel over the calls since the last reset; bench.py's roofline leg.  mode 0: off; 1: time every
 * launch (to find the dominant kernel); 2: from now on time only the kernel that dominated the
 * mode-1 recording (two events per launch of that kernel); 3: like 2 but only every 4th launch of it -- an event
 * record also holds back the next kernel's start (~3.5 us each on MI355X), a sample keeps a timed region honest. */
int afr_profile_dominant(afr_plan* plan, int mode);
int afr_profile_read(afr_plan* plan, char* name, int name_cap, double* avg_ms, int64_t* launches,
                     double* algo_flops, double* algo_bytes);
/* Text table of everything recorded: one "kernel\tlaunches\ttotal_ms\tavg_ms\tflops\tbytes" line per kernel. */
int afr_profile_dump(afr_plan* plan, char* buf, int cap);

/* Inspection for stage-by-stage validation: copy one internal activation buffer of the last call (in the plan's
 * activation dtype: f32, or bf16 in AFR_BF16 mode) to dst (device or host pointer).  *bytes_out = bytes copied. */
enum { AFR_BUF_U = 0,      /* pre-clamp output u [B, pixels]; after afr_loss_grad it holds du                     */
       AFR_BUF_Z = 1,      /* sheet: flattened fc1 features z [B, max_length*fc_dim]                               */
       AFR_BUF_DZ = 2,     /* sheet: gradient w.r.t. z                                                            */
       AFR_BUF_W1T = 4,    /* small glyph nets, bf16: the transposed operand copy W1^T [E][N1] the fused step reads */
       AFR_BUF_W2T = 5,    /*                         and W2^T [N1][pixels] (always bf16)                          */
       AFR_BUF_ACT = 16 }; /* glyph: AFR_BUF_ACT + i = activation i (0 = embedding sum, i = output of hidden i);
                              pixel: AFR_BUF_ACT + i = block i's MLP ReLU output [B * tokens, fc_dim] (its ReLU gates) */
int afr_debug_copy(afr_plan* plan, int which, void* dst, size_t dst_bytes, size_t* bytes_out, void* stream);
/* Inspection of the sheet model's in-kernel embedding gather (model.py:136,167): runs the front end of an eval forward on
 * x [B, L] and leaves the rows it gathered, Emb[x[b][l]] for l < min(L, max_length), in e0 (device, float32
 * [B][min(L, max_length)][embed_dim]) -- before dropout and the positional encoding.  The north star asks this gather to
 * be bit-exact; the glyph nets expose theirs as AFR_BUF_ACT + 0. */
int afr_debug_sheet_gather(afr_plan* plan, const int64_t* x, int B, int L, float* e0, void* stream);

/* ---- single-kernel entry points (unit tests and re-use by callers either side of the path) ---- */
enum { AFR_GEMM_BIAS = 1, AFR_GEMM_RELU = 2, AFR_GEMM_RELU_MASK = 4, AFR_GEMM_OUT_BF16 = 8,
       AFR_GEMM_A_KSTRIDED = 16, AFR_GEMM_B_KSTRIDED = 32 };
/* C[m][n] = sum_k A(m,k) * B(n,k) (+bias[n]) (relu) (* (aux[m][n] > 0)).
 * A(m,k) = A[m*lda+k], or A[k*lda+m] with AFR_GEMM_A_KSTRIDED; B likewise.  dtype selects f32 or
 * bf16 operands (aux has the operand dtype), or AFR_BF16X3: f32 operands and aux, split-bf16 products, f32 C only
 * (AFR_GEMM_OUT_BF16 is AFR_EINVAL).  C is f32 unless AFR_GEMM_OUT_BF16.  splitk>1 writes
 * splitk partial f32 slabs of M*ldc elements each, to be summed by the caller (afr_op_reduce). */
int afr_op_gemm(int dtype, int flags, const void* A, const void* B, void* C, const float* bias,
                const void* aux, int M, int N, int K, int lda, int ldb, int ldc, int ldaux,
                int splitk, void* stream);

/* The same product (bf16 operands, any AFR_GEMM_* epilogue) as split-K WITH the reduction inside the launch, on
 * 256x256 output tiles: the first head_tiles tiles of the kernel's walk are computed whole by one workgroup each, every
 * remaining tile as `splitk` K-slices that are parked in `workspace` and added, in slice order, by whichever slice
 * workgroup arrives last, which then runs the epilogue.  For products whose tile count leaves the chip's last round
 * mostly empty (the sheet model's fc_output forward: 300 tiles = one full round of 256 + 44 tiles cut 5 ways; its input
 * gradient: 100 tiles cut 2 ways).  Measured on R0's input gradient (1024 x 6400 x 19200): 220 us against the 128x128
 * kernel's 276 us with the weight operand warm in the infinity cache, but 343 us against 281 us inside a training step,
 * where the 246 MB weight shadow streams from HBM and one 160-KiB workgroup per CU hides that latency worse than two
 * 64-KiB ones -- so afr_train_step does not use it.  workspace: afr_op_gemm_fix_workspace_bytes() bytes, 16-byte
 * aligned, whose trailing counter words (one per tail tile) are ZERO before the first call; the kernel leaves them zero. */
size_t afr_op_gemm_fix_workspace_bytes(int M, int N, int head_tiles, int splitk);
int afr_op_gemm_fix(int flags, const void* A, const void* B, void* C, const float* bias, const void* aux,
                    int M, int N, int K, int lda, int ldb, int ldc, int ldaux, int head_tiles, int splitk,
                    void* workspace, size_t workspace_bytes, void* stream);
/* A Linear layer's two gradient products exactly as afr_train_step issues them in bf16 mode when the pair fills the chip
 * with 256x256 tiles -- ONE grouped launch (reference: what autograd derives from nn.Linear, model.py:148,152,309):
 *     dW[N][K]      = dy^T . x          f32; the split-K slices are summed INSIDE the launch (cooperative split-K)
 *     db_part[s][N] = column sums of dy over K-slice s, s < splitk (the caller adds the rows)
 *     dX[B][K]      = (dy . W) * (aux > 0)   bf16 (aux NULL: no mask)
 * dy [B][N], x [B][K], W [N][K], aux [B][K]: bf16, row-major, dense.  afr_op_gemm_pair_plan returns AFR_OK with the split
 * and the workspace size, or AFR_EUNSUPPORTED when the shape does not take this form (the step then uses separate
 * launches).  workspace: 256-byte aligned; its contents need not be preserved between calls. */
int afr_op_gemm_pair_plan(int B, int N, int K, int* splitk, size_t* workspace_bytes);
int afr_op_gemm_pair(const void* dy, const void* x, const void* W, const void* aux, float* dW, float* db_part, void* dX,
                     int B, int N, int K, void* workspace, size_t workspace_bytes, void* stream);
/* One product of the Linear y[B][N] = x[B][K] . W[N][K]^T + b exactly as a training step issues it: the launch description the
 * step builds for that product, with the tails a step hangs on it set from `tail`, through the step's launchers.  No afr_op_gemm*
 * flag reaches these tails; this entry adds no kernel and no dispatch rule.  dtype AFR_F32 / AFR_BF16X3: f32 operands and outputs;
 * AFR_BF16: bf16 x, W, dy, aux, y and dx.  dW, db, p, m, v are always float32.  N and K multiples of 8 (bf16) or 4.
 *   AFR_LIN_FWD   out = y [B][N] = x . W^T + bias.  With tail->target: the fused loss -- out receives du instead, *loss_accum +=
 *                 the loss (afr_config.loss semantics, afr_loss_grad's formulas; fused and unfused leave the same du bit for
 *                 bit); target [rows][N] dense uint8 / float32, target_rows (or NULL) int32 [B]: row b's targets are row
 *                 target_rows[b]; loss_scratch: 1040 + ceil(B/128) * ceil(N/128) floats, zero before the first call (afr_op_mse_grad's
 *                 contract).  mask_out (AFR_BF16): AFR_GEMM_RELU is applied and bit n & 7 of mask_out[b * ldmask + n / 8] =
 *                 [stored y(b, n) > 0].  x_rows (AFR_BF16): int32 [B], row b of x is row x_rows[b] of the table x, rows ldx apart.
 *   AFR_LIN_DX    out = dx [B][K] = dy . W, gated by ReLU's mask: (aux[b][k] > 0) with aux [B][ldaux] (rows aux_rows[b] of a
 *                 table when aux_rows is given), or bit k & 7 of mask_in[b * ldmask + k / 8] (AFR_BF16; read INSTEAD of aux).
 *   AFR_LIN_DW    out = dW [N][K] = dy^T . x;  db [N] = column sums of dy (or NULL).  splitk > 1: out = splitk slabs, N * ld_out
 *                 floats apart, and db = splitk rows ld_db apart: slice s covers batch rows [s * len, min(B, (s + 1) * len)), len =
 *                 ceil(B / splitk) rounded up to the kernel's K-tile (32, bf16: 64); a slice that starts at or beyond B is zeros.
 *                 With tail->p (splitk 1 only): the fused optimizer step -- dW is not stored; opt_kind AFR_OPT_ADAMW / AFR_OPT_LION is
 *                 applied to p, m, v (Lion: v unused) and the bf16 `shadow` (or NULL) at the positions [n * ld_out + k].
 *   AFR_LIN_PAIR  (AFR_BF16) both gradient products in ONE grouped launch as afr_op_linear_pair_plan describes it: out = dW
 *                 (cooperative: the finished gradient, or the fused optimizer step as above) or its splitk slabs, db = splitk
 *                 rows, out2 = dx [B][K] with the AFR_LIN_DX gates.  x_rows: the dW member reads x through the row map
 *                 (cooperative launches only).  workspace: workspace_bytes of the plan, 256-byte aligned, contents free.
 *                 The dx member reads W: a fused step leaves W itself alone (the new bf16 weights go to `shadow`).
 * ld_out, ldx, ldaux, ld_db: leading dimensions in elements, 0 = dense.  kernel_name (or NULL) receives the kernel the launch ran on:
 * "gemm_bf16<0,0,4>", "gemm_f32<1,1>", ..., "gemm_bf16_group", "gemm_bf16_group256", "gemm_bf16_group256_lion".
 * Errors: null pointers, bad extents or strides, a tail that `which` does not have -> AFR_EINVAL; a combination the launchers
 * refuse (a row map off the 256x128 ring, a BCE loss on gathered rows, ...) -> AFR_EUNSUPPORTED with a message: never a fallback. */
enum { AFR_LIN_FWD = 0, AFR_LIN_DX = 1, AFR_LIN_DW = 2, AFR_LIN_PAIR = 3 };
typedef struct afr_linear_tail {
    int32_t ld_out, ldx, ldaux, ld_db;          /* elements; 0 = dense                                       */
    /* forward */
    const void* target; const int32_t* target_rows; int32_t target_dtype, loss_kind; int64_t mean_elems;
    float* loss_accum; float* loss_scratch;
    uint8_t* mask_out;
    const int32_t* x_rows;                      /* forward: rows of x; pair: rows of x for the dW member     */
    /* input gradient */
    const void* aux; const int32_t* aux_rows; const uint8_t* mask_in;
    int32_t ldmask;                             /* bytes per row of mask_out / mask_in                       */
    /* weight gradient */
    int32_t splitk;                             /* 0 or 1: none (AFR_LIN_PAIR: the plan's, not read)         */
    float* db;
    int32_t opt_kind, reserved;                 /* AFR_OPT_*                                                 */
    float *p, *m, *v; void* shadow;             /* p != NULL: fused optimizer step                           */
    float lr, beta1, beta2, eps, weight_decay, grad_scale;   /* grad_scale must be 1 (the fused tails take g unscaled) */
    int64_t t;
} afr_linear_tail;
/* How AFR_LIN_PAIR launches at this shape (host-only): *tile256 = 1: 256x256 tiles (gemm_bf16_group256), 0: 256x128
 * (gemm_bf16_group); *splitk = slices of the weight gradient; *coop = 1: the slices meet inside the launch, 0: splitk slabs.
 * AFR_EUNSUPPORTED when the pair does not leave as one grouped launch at this shape. */
int afr_op_linear_pair_plan(int B, int N, int K, int* tile256, int* splitk, int* coop, size_t* workspace_bytes);
int afr_op_linear(int dtype, int which, const void* x, const void* W, const float* bias, const void* dy, void* out, void* out2,
                  int B, int N, int K, const afr_linear_tail* tail /* or NULL */, void* workspace, size_t workspace_bytes,
                  char* kernel_name /* or NULL */, int name_cap, void* stream);
/* Two stacked Linears' gradient pairs as the ONE chained launch a glyph training step issues for its output layer and the hidden
 * layer below it (AFR_BF16): upper y = x_up[B][K_up] . W_up[N_up][K_up]^T, lower x_up = relu(x_lo[B][K_lo] . W_lo[K_up][K_lo]^T).
 * Every operand, output and tail means what it means in two AFR_LIN_PAIR calls -- the upper one with (dy, x_up, W_up) -> out_up =
 * dW_up, mid = its dx [B][K_up]; the lower one with (mid as dy, x_lo, W_lo) -> out_lo = dW_lo, dx_lo [B][K_lo] -- and every result
 * is bit for bit theirs; `mid` is handed from the upper pair's workgroups to the lower pair's inside the launch.  Dense leading dimensions
 * only (the tails' ld_out / ldx must be 0 or the dense value; ldaux, ld_db and ldmask are free).
 * afr_op_linear_chain_plan (host-only): AFR_OK with the two splits and the workspace size when the shapes chain on a device of
 * `cus` compute units (0: the current device's), AFR_EUNSUPPORTED otherwise -- both pairs cooperative 256x256 launches, the block
 * counts of the swapped roles equal (dx_up = dW_lo, dW_up = dx_lo) and whole octets, a CU per workgroup of the upper pair (a step
 * then issues the two launches).  *blocks: the launch's grid, both pairs.
 * afr_op_linear_chain_block (host-only): the kernel's block map.  Block `block` of the launch runs K-slice *slice of the 256x256
 * tile (*tm, *tn) of product *member: 0 = dW_up, 1 = dx_up (mid), 2 = dW_lo, 3 = dx_lo; *phase = 0 for the upper pair, whose
 * workgroups are handed out first, 1 for the lower pair, whose workgroups take the CUs over as the upper ones leave.
 * AFR_EINVAL for a block outside the grid.  workspace: 256-byte aligned, contents free. */
/* 1 when a backward (or training step) of this plan at batch B issues that chained launch on a device of `cus` compute units (0:
 * the bound device's), 0 when it issues the two grouped launches: another model kind or dtype, fewer than two hidden layers,
 * AFR_CFG_NO_PAIR_CHAIN / _NO_GROUPED_GEMM / _SLAB_SPLITK, a shape afr_op_linear_chain_plan refuses.  (afr_backward_stage always
 * issues a launch per stage: its caller reduces each stage's gradient range while the next stage runs.) */
int afr_plan_pair_chain(const afr_plan* plan, int B, int cus);
int afr_op_linear_chain_plan(int B, int N_up, int K_up, int K_lo, int cus, int* splitk_up, int* splitk_lo, int* blocks, size_t* workspace_bytes);
int afr_op_linear_chain_block(int B, int N_up, int K_up, int K_lo, int block, int* phase, int* member, int* tm, int* tn, int* slice);
int afr_op_linear_chain(const void* dy, const void* x_up, const void* W_up, void* out_up, void* mid, const afr_linear_tail* tail_up,
                        const void* x_lo, const void* W_lo, void* out_lo, void* dx_lo, const afr_linear_tail* tail_lo,
                        int B, int N_up, int K_up, int K_lo, void* workspace, size_t workspace_bytes,
                        char* kernel_name /* or NULL */, int name_cap, void* stream);
/* The same launch with the folded first layer's fused backward (afr_op_glyph_l1_bwd_fused; N1 = K_lo, E = 32) as its FIFTH role,
 * as a glyph step issues it when the lower Linear's input is that first layer: the grid is [dW_up | dx_up | dW_lo | dx_lo | L1],
 * the L1 range being that kernel's workgroups (64 glyphs x a column range each), which are handed the rows of d1 = dx_lo inside
 * the launch (one arrival counter per 256-row block).  Every output is bit for bit that of afr_op_linear_chain followed by
 * afr_op_glyph_l1_bwd_fused on its dx_lo.  The refusals are those of both: every one of afr_op_linear_chain, every one of
 * afr_op_glyph_l1_bwd_fused, and AFR_EUNSUPPORTED when d1 is not dx_lo.  loss_partial (or NULL): deferred loss partials of a
 * producer launch of loss_n blocks of loss_bd (256 or 512) threads; ONE appended workgroup adds sum * loss_inv_n to *loss_accum.
 * afr_op_linear_chain_l1_plan (host-only): *blocks = the grid with the L1 range (and the loss-sum workgroup with has_loss),
 * *workspace_bytes = afr_op_linear_chain_plan's plus the second set of counters.
 * afr_op_linear_chain_l1_block (host-only): *role = 0 for a block of the four products (afr_op_linear_chain_block has its tile),
 * 1 for a first-layer workgroup -- glyphs [64 *row_block, +64), column range *col_range, waiting for 256-row block *wait_block
 * of dx_lo --, 2 for the appended loss-sum workgroup; AFR_EINVAL for a block outside the grid. */
int afr_op_linear_chain_l1_plan(int B, int N_up, int K_up, int K_lo, int vocab, int n_fonts, int has_loss, int cus, int* blocks, size_t* workspace_bytes);
int afr_op_linear_chain_l1_block(int B, int N_up, int K_up, int K_lo, int vocab, int n_fonts, int has_loss, int block, int* role,
                                 int* row_block, int* col_range, int* wait_block);
int afr_op_linear_chain_l1(const void* dy, const void* x_up, const void* W_up, void* out_up, void* mid, const afr_linear_tail* tail_up,
                           const void* x_lo, const void* W_lo, void* out_lo, void* dx_lo, const afr_linear_tail* tail_lo,
                           int B, int N_up, int K_up, int K_lo, void* workspace, size_t workspace_bytes,
                           const void* d1, const void* h0, int ldh, const int32_t* h0_rowmap /* or NULL */, const void* W1T, const int64_t* x,
                           const int64_t* font /* or NULL */, int vocab, int n_fonts, float* slabs,
                           const float* loss_partial /* or NULL */, int loss_n, int loss_bd, float loss_inv_n, float* loss_accum,
                           char* kernel_name /* or NULL */, int name_cap, void* stream);
int afr_op_reduce(float* dst, const float* slabs, int nslabs, int64_t slab_stride, int64_t n,
                  float scale, int accumulate, void* stream);
/* Several slab reductions in ONE launch (what a backward pass uses for all its split-K / per-block partial gradients):
 * dst[i][0..n[i]) = sum_s slabs[i][s*stride[i] + ...], s < nslabs[i], fixed order.  At most 32 segments: more is an
 * error (AFR_EINVAL), never a silent drop.  n[i] must be a multiple of 4. */
int afr_op_reduce_group(int nseg, float* const* dst, const float* const* slabs, const int* nslabs,
                        const int64_t* stride, const int64_t* n, void* stream);
/* The grouped reduce exactly as a single-GPU training step issues it, in ONE launch: the step's table (one entry per segment, in the
 * caller's order), its hypers and its launcher; this entry adds no kernel and no dispatch rule.  step NULL, or step->p NULL: the plain
 * reduce above (afr_op_reduce_group calls this entry).  With step->p: the FUSED optimizer step -- the summed gradient of segment i is
 * not stored; opt_kind AFR_OPT_ADAMW / AFR_OPT_LION is applied to the flat elements [dst[i] - gbase, + n[i]) of p, m and v (Lion: v is
 * neither read nor written and may be NULL) and of the bf16 `shadow` (or NULL); dst[i] is only an address, nothing is read or written there.
 *   lr_mult, wd_mult   HOST arrays [nseg] (or NULL: 1): optimizer groups.  Either one present selects the kernel that carries one hyper
 *                      per segment; segment i is stepped with fl32(lr * lr_mult[i]), fl32(weight_decay * wd_mult[i]) (afr_set_param_groups).
 *   shT, tN, tK        HOST arrays [nseg] (or NULL): where shT[i] is not NULL, segment i is a [n[i] / tK[i]][tK[i]] block of weight rows and
 *                      its new bf16 weights are ALSO written transposed, shT[i][k * tN[i] + r] = bf16(p[r][k]): tN[i] is the pitch of the
 *                      transposed copy (>= the segment's rows: a row range of a wider weight points shT[i] at its first column).
 * A segment with n[i] == 0 is allowed and dropped, as in the plain form; lr_mult, wd_mult, shT, tN, tK stay indexed by the CALLER's
 * segment i: the entry moves them to the table's own numbering.
 * kernel_name (or NULL) receives the instantiation, "reduce_group<OPT,GROUPS>": "reduce_group<0,0>" (plain, and fused AdamW),
 * "reduce_group<1,0>" (Lion), "reduce_group<0,1>", "reduce_group<1,1>" (with groups).
 * Refused with AFR_EINVAL and a message, before anything is launched: null required pointers; nseg outside 1..32; n[i] negative or not
 * a multiple of 4; nslabs[i] < 1; stride[i] not a multiple of 4; with a step: dst[i] - gbase negative or not a multiple of 4, t < 1
 * (AdamW), an unknown kind, a multiplier that is negative or not finite, shT[i] with tK[i] % 4 != 0, with n[i] not a multiple of
 * tK[i], or with tN[i] < n[i] / tK[i]; shT[i] without a fused step. */
typedef struct afr_reduce_step {
    int32_t opt_kind, reserved;                 /* AFR_OPT_*                                                 */
    float lr, beta1, beta2, eps, weight_decay, reserved2;
    int64_t t;
    const float* gbase;                         /* the flat gradient buffer's first element                  */
    float *p, *m, *v; void* shadow;             /* p != NULL: fused optimizer step                           */
    const float* lr_mult; const float* wd_mult; /* host [nseg], or NULL                                      */
    void* const* shT; const int32_t* tN; const int32_t* tK;   /* host [nseg], or NULL                        */
} afr_reduce_step;
int afr_op_reduce_group_step(int nseg, float* const* dst, const float* const* slabs, const int* nslabs, const int64_t* stride,
                             const int64_t* n, const afr_reduce_step* step /* or NULL */, char* kernel_name /* or NULL */, int name_cap,
                             void* stream);
int afr_op_adamw(float* p, const float* g, float* m, float* v, void* shadow_bf16, int64_t n, float lr,
                 float beta1, float beta2, float eps, float weight_decay, int64_t t, float grad_scale,
                 void* stream);
/* afr_op_adamw with clipping by a caller-supplied global norm: sumsq_dev is a device float holding the sum of squared gradients
 * of the WHOLE model (under a sharded optimizer: the all-reduced sum of every rank's afr_grad_sumsq over its range); the slice
 * is updated with coef = min(1, max_norm / (|grad_scale| * sqrt(*sumsq_dev) + 1e-6)) as afr_adamw_step does on a clipping plan.
 * A non-finite *sumsq_dev leaves p, m, v untouched (no plan, hence no error word: the caller holds the sum).  max_norm > 0. */
int afr_op_adamw_clip(float* p, const float* g, float* m, float* v, void* shadow_bf16, int64_t n, float lr,
                      float beta1, float beta2, float eps, float weight_decay, int64_t t, float grad_scale,
                      const float* sumsq_dev, float max_norm, void* stream);
/* The Lion update (afr_set_optimizer) on a slice: the sharded optimizer's and the unit tests' entry.  sumsq_dev NULL: no clipping
 * (max_norm is not read); else the clip semantics of afr_op_adamw_clip, a non-finite *sumsq_dev leaving p, m and the shadow untouched. */
int afr_op_lion(float* p, const float* g, float* m, void* shadow_bf16, int64_t n, float lr, float beta1, float beta2,
                float weight_decay, float grad_scale, const float* sumsq_dev /* NULL = no clip */, float max_norm, void* stream);
/* The grouped update (afr_set_param_groups) on a slice, in ONE launch: the sharded optimizer's and the unit tests' entry.  p, g, m, v
 * and shadow_bf16 point at the slice's first element, which is element `first` of the flat buffer the ranges describe; n and first
 * are multiples of 4.  ranges: a HOST array of n_ranges entries in flat coordinates -- ends multiples of 4 and strictly increasing,
 * the last one >= first + n; range k covers [ranges[k-1].end, ranges[k].end) and is updated with fl32(lr * lr_mult), fl32(weight_decay
 * * wd_mult).  kind AFR_OPT_ADAMW: afr_op_adamw's update (afr_op_adamw_clip's with sumsq_dev); AFR_OPT_LION: afr_op_lion's (v, eps and
 * t are not read).  sumsq_dev NULL: no clipping.  Bit for bit what those entries give when launched range by range. */
int afr_op_opt_groups(int kind, float* p, const float* g, float* m, float* v, void* shadow_bf16, int64_t n, int64_t first,
                      const afr_opt_range* ranges, int n_ranges, float lr, float beta1, float beta2, float eps, float weight_decay,
                      int64_t t, float grad_scale, const float* sumsq_dev /* NULL = no clip */, float max_norm, void* stream);
/* scratch: >= 1040 floats, zero before the first call (holds per-block partials and the arrival counter) */
int afr_op_mse_grad(int act_dtype, const void* u, const void* target, int target_dtype, void* du,
                    int64_t rows, int64_t cols, int64_t mean_elems, float* loss_accum, float* scratch,
                    void* stream);
/* The AFR_LOSS_BCE form of the same launch: loss += sum(max(u,0) - t u + log1p(exp(-|u|))) / mean_elems over the logits u,
 * du = (sigmoid(u) - t) / mean_elems (F.binary_cross_entropy_with_logits and its gradient).  Same scratch, same fixed summation order. */
int afr_op_bce_grad(int act_dtype, const void* u, const void* target, int target_dtype, void* du,
                    int64_t rows, int64_t cols, int64_t mean_elems, float* loss_accum, float* scratch,
                    void* stream);
/* afr_eval's kernel on caller-owned buffers: u [rows][cols] float32 (AFR_F32) or bf16 (AFR_BF16), loss_kind AFR_LOSS_*, cols a
 * multiple of 8 (AFR_EUNSUPPORTED otherwise).  rowmap (or NULL): int32 [rows], the targets of row r are row rowmap[r] of target
 * (64-bit addressing); it is not read without a target.  Outputs, formulas, summation order and argument errors as afr_eval. */
int afr_op_eval(int act_dtype, int loss_kind, const void* u, const void* target /* or NULL */, int target_dtype,
                const int32_t* rowmap /* or NULL */, int64_t rows, int64_t cols,
                float* loss_rows, uint32_t* stats, uint8_t* q, void* stream);
/* afr_tensor_stats' pair of launches on caller-owned buffers: record k describes the numel elements from a + off (of a - minus, minus
 * or NULL in the same layout) of segs[k], a HOST array of nseg entries that is not read after the call returns (the table travels to
 * the kernels as an argument).  Formulas, order and locality as above: a record is bit for bit what afr_tensor_stats gives for a
 * tensor with the same elements.  a, minus, out and scratch are device pointers, 16-byte aligned; scratch holds
 * afr_op_tensor_stats_scratch_bytes(segs, nseg) bytes (32 per chunk; 0 for a table that would be refused), needs no initialisation
 * and keeps no state between calls.  Errors, before anything is launched: a, out, scratch or segs NULL or misaligned, nseg outside
 * 1..256, an off negative or not a multiple of 4, numel < 0, scratch_bytes too small -> AFR_EINVAL; a numel of 2^32 or more, or an
 * off of 2^34 or more -> AFR_EUNSUPPORTED. */
typedef struct afr_tensor_seg { int64_t off, numel; } afr_tensor_seg;
size_t afr_op_tensor_stats_scratch_bytes(const afr_tensor_seg* segs, int nseg);
int afr_op_tensor_stats(const float* a, const float* minus /* or NULL */, const afr_tensor_seg* segs, int nseg,
                        afr_tensor_stat* out, void* scratch, size_t scratch_bytes, void* stream);
int afr_op_f32_to_bf16(const float* src, void* dst, int64_t n, void* stream);

/* ---- the sheet data set composed on the device: the two launches that replace the reference's offline generator
 * (generate_font.ts:64-142,164-206 -- the seeded text source, the word wrap, and fillText line by line into a BMP per sample).  Plain
 * ops: no plan, nothing allocated.  Everything is integer arithmetic, so the outputs are bit-exact functions of their arguments.
 *   dataset_text   one lane per sample j of n: the text of the reference's LCG source for seed first_seed + (seed_rows ? seed_rows[j]
 *                  : j) -- state = state * 1664525 + 1013904223 mod 2^32, int(rnd() * k) = (state * k) >> 32; a length in min_len ..
 *                  max_len, words of 1..10 letters A-Z separated by single spaces -- as int64 codes, zero-padded, in row r = out_rows ?
 *                  out_rows[j] : j of codes [rows][ldx]; len[r] (int32, or NULL) = the text's length.  Every element of a written row
 *                  is written once; other rows are not touched.
 *   compose_sheets one workgroup per sample j of n: row j of codes int64 [n][ldx] drawn as black text on a white uint8 sheet
 *                  [height][width] in row r = out_rows ? out_rows[j] : j of out (64-bit addressing; every byte of a written row is
 *                  written once).  The text is the codes up to the first 0 (or ldx).  It is split at every code 32, empty words
 *                  included, and wrapped greedily: a word joins the current line (with one space) unless the line is non-empty and
 *                  the joined width exceeds wrap_width64, where width64(s) = sum of adv64[c] over s + sum of kern64[prev][c] over
 *                  adjacent pairs, spaces included; so a leading empty word vanishes and a word wider than the sheet keeps its own
 *                  line and is clipped.  On line i < n_lines (later lines are not drawn) the pen starts at 0; a character with a
 *                  predecessor on the line first adds kern64[prev][c], is drawn at px = (pen64 + 32) >> 6, then adds adv64[c].
 *                  Pixel (y, x) starts with coverage m = 0; every glyph whose cell covers it, in (line, character) order, adds
 *                  b = cells[c][y - baseline[i] + origin_y][x - px + origin_x] as m = m + b - (m * b + 127) / 255; the byte stored is
 *                  255 - m.  A code outside [0, n_codes) sets bit 0 of *err (device word, or NULL) and is skipped: no advance, no
 *                  kerning, no ink, as if the text did not hold it.
 * The atlas's cells are kept in LDS beside the layout's arrays and one glyph range per line and 8-pixel column block.
 * Errors, before anything is launched: a required pointer NULL or
 * misaligned (codes, the row vectors and out 8 bytes; cells, adv64, len, err 4; kern64 2), n < 1, min_len < 1, max_len < min_len,
 * max_len > ldx, n_lines outside 1..16, a non-positive size, an origin outside the cell -> AFR_EINVAL; ldx > 256, width not a multiple
 * of 8, a sheet of 2 GiB or more, cells + ranges + layout above the 64 KiB LDS budget -> AFR_EUNSUPPORTED. */
typedef struct afr_glyph_atlas { const uint8_t* cells;   /* device [n_codes][cell_h][cell_w], coverage 0..255 = 255 - pixel */
                                 const int32_t* adv64;   /* device [n_codes], advance in 1/64 px                          */
                                 const int16_t* kern64;  /* device [n_codes][n_codes] or NULL                             */
                                 int32_t n_codes, cell_h, cell_w, origin_x, origin_y; } afr_glyph_atlas;
typedef struct afr_sheet_geometry { int32_t height, width, wrap_width64, n_lines; int32_t baseline[16]; } afr_sheet_geometry;
int afr_op_dataset_text(int64_t first_seed, const int64_t* seed_rows, const int64_t* out_rows, int64_t n, int min_len, int max_len,
                        int64_t* codes, int ldx, int32_t* len /* or NULL */, void* stream);
int afr_op_compose_sheets(const afr_glyph_atlas* atlas, const afr_sheet_geometry* geo, const int64_t* codes, int ldx,
                          const int64_t* out_rows, int64_t n, uint8_t* out, uint32_t* err /* or NULL */, void* stream);

/* ---- the text source with any alphabet: dataset_text with the letter drawn from a table of integer weights over the codes 33..126,
 * and the launch that builds the table on the device from afr_op_sheet_char_errors' by-code counters.  Plain ops, integers only.
 *   dataset_text_w afr_op_dataset_text in every respect -- seed, row mapping, length draw, word-length draw, spaces, zero fill, len --
 *                  but the letter: with total = cum[93], after the same LCG update r = (state * total) >> 32 and the letter is
 *                  33 + (the smallest i with cum[i] > r).  cum: device uint32 [94], the inclusive cumulative weights, non-decreasing.
 *                  An entry of weight 0 (cum[i] == cum[i - 1]) is never drawn; the space and code 0 are outside the table.  With a
 *                  weight f on 65..90 alone the letter is 65 + ((state * 26 f) >> 32) / f = 65 + ((state * 26) >> 32): the texts are
 *                  afr_op_dataset_text's byte for byte, from the same draws.  total == 0 sets bit 0 of *err (device word, or NULL);
 *                  the rows are then zero-filled and len[r] = 0.  The table is read into LDS once per workgroup.
 *   text_weights   one workgroup.  members (HOST, three words): bit i of the 94-bit mask = code 33 + i belongs to the alphabet A.
 *                  by_code: device uint64 [n_codes + 1][5] as afr_op_sheet_char_errors leaves it, or NULL; only pixels (column 1)
 *                  and sumsq (column 2) of the member codes are read -- never a non-member or the background row.  In integers, with
 *                  P = sum over A of pixels and S = sum over A of sumsq (each must fit 64 bits):
 *                    by_code NULL, gain == 0 or S == 0:  w_c = floor_w for every member c;
 *                    otherwise  k = max(0, bit_length(S) - 47) and P, S and every pixels_c, sumsq_c are shifted right by k (so that
 *                               each << 16 below stays inside 64 bits for any table),
 *                               m_ref = max(1, (S << 16) / max(1, P)),
 *                               rel_c = 1 << 16 for a member with pixels_c == 0 (a character never seen counts as average), else
 *                               rel_c = min((((sumsq_c << 16) / pixels_c) << 16) / m_ref, 16 << 16)   (at most 16 times the mean),
 *                               w_c   = floor_w + ((gain * rel_c) >> 16);
 *                  non-members get w_c = 0.  cum (device uint32 [94]) = the inclusive sums of w, w (device uint32 [94], or NULL) the
 *                  weights themselves.  A weight is at most 65535 * 17, so the total is below 2^27.  No atomics: the words repeat.
 * Errors, before anything is launched: dataset_text_w -- everything afr_op_dataset_text refuses, cum NULL, cum or err not 4-byte
 * aligned; text_weights -- members or cum NULL, by_code given with n_codes < 127, an empty member set, member bits above bit 93,
 * floor_w outside 1..65535, gain above 65535, by_code not 8-byte or cum, w not 4-byte aligned -> AFR_EINVAL. */
#define AFR_TEXT_FIRST 33      /* first drawable code */
#define AFR_TEXT_CODES 94      /* codes 33..126 */
int afr_op_dataset_text_w(int64_t first_seed, const int64_t* seed_rows, const int64_t* out_rows, int64_t n, int min_len, int max_len,
                          const uint32_t* cum /* device [94], inclusive cumulative weights */,
                          int64_t* codes, int ldx, int32_t* len /* or NULL */, uint32_t* err /* or NULL */, void* stream);
int afr_op_text_weights(const uint64_t* by_code /* device [n_codes + 1][5] as afr_op_sheet_char_errors leaves it, or NULL */,
                        int n_codes, const uint32_t members[3] /* host: bit i = code 33 + i is in the alphabet */,
                        uint32_t floor_w /* 1..65535 */, uint32_t gain /* 0..65535 */,
                        uint32_t* cum /* device [94] */, uint32_t* w /* device [94] or NULL */, void* stream);

/* ---- the text source with context: a first-order Markov chain over the codes 33..126, an error table by (preceding character,
 * character), and the launch that builds the chain's table from the error table on the device.  Plain ops, integers only.  A CONTEXT
 * is one of 95 rows: row 0 = no letter before (the start of a word), row 1 + i = after letter i (code 33 + i).
 *   dataset_text_m afr_op_dataset_text_w in every respect -- seed, row mapping, length draw, word-length draw, single spaces, zero
 *                  fill, len, 64-bit row addressing -- but the letter.  cum2: device uint32 [95][94], per context the inclusive
 *                  cumulative weights, non-decreasing within a row.  Every word starts in context 0; after letter i is drawn the
 *                  context is row 1 + i.  A letter: the LCG update, r = (state * total) >> 32 with total = cum2[ctx][93], then the
 *                  smallest i with cum2[ctx][i] > r.  A sample that reaches a context whose total is 0 (row 0 included) is
 *                  zero-filled over its whole row, gets len[r] = 0 and sets bit 0 of *err (device word, or NULL); a zero row no
 *                  sample reaches sets nothing.  If every row of cum2 equals one cum the texts are afr_op_dataset_text_w's byte for
 *                  byte, from the same draws.  The table is read into LDS once per workgroup (95 rows padded to 128 entries).
 *   pair_errors    sample j of n reads row r = code_rows ? code_rows[j] : j of codes int64
 *                  [rows][ldx] and row j of per_pos uint32 [n][ldx + 1][4] = {pixels, sumsq, off2, wrong} as
 *                  afr_op_sheet_char_errors leaves it (slot ldx, the background, is not read).  Position i CONTRIBUTES when its code
 *                  c lies in 33..126 and its record's pixels > 0.  Its context is row 1 + (p - 33) if the code p at position i - 1
 *                  lies in 33..126, and row 0 otherwise: position 0, a preceding space, any other preceding code.  (A wrapped line
 *                  breaks at a space, so the text's predecessor is the line's; the layout is not run again.)
 *                  by_pair: device uint64 [95][94][4] = {chars, pixels, sumsq, wrong}, ADDED to, the caller zeroes it; a
 *                  contributing position adds {1, pixels, sumsq, wrong} to [context][c - 33].  Integer adds only: the table does
 *                  not depend on their order and repeats bit for bit.  A workgroup sums a band of 12 contexts over its chunk of
 *                  samples in LDS and issues one 64-bit global integer atomic per non-zero counter.
 *   pair_weights   one workgroup.  members (HOST, three words) as text_weights'.  A pair (p, c) is LIVE when c is a member and p is
 *                  row 0 or a member's row.  by_pair as pair_errors leaves it, or NULL; only the records of live pairs are read.
 *                  In integers, with P = the sum of pixels and S = the sum of sumsq over all live pairs (each must fit 64 bits):
 *                    by_pair NULL, gain == 0 or S == 0:  w = floor_w for every live pair;
 *                    otherwise  k = max(0, bit_length(S) - 47) and P, S and every pixels, sumsq are shifted right by k,
 *                               m_ref = max(1, (S << 16) / max(1, P))   -- one reference mean for the whole table,
 *                               rel   = 1 << 16 for a live pair with pixels == 0 (after the shift) or chars < min_chars (chars is
 *                                       not shifted): too little evidence counts as average, else
 *                               rel   = min((((sumsq << 16) / pixels) << 16) / m_ref, 16 << 16),
 *                               w     = floor_w + ((gain * rel) >> 16);
 *                  pairs that are not live get w = 0, so the rows of non-member contexts are all zero -- and never reached, since
 *                  only members are drawn.  cum2 (device uint32 [95][94]) = the inclusive sums of w along each row, w2 (device
 *                  uint32 [95][94], or NULL) the weights themselves.  A row's total is below 2^27.  No atomics: the words repeat.
 * Errors, before anything is launched: dataset_text_m -- everything afr_op_dataset_text_w refuses, with cum2 in the place of cum;
 * pair_errors -- codes, per_pos or by_pair NULL, codes, code_rows or by_pair not 8-byte aligned, per_pos not 16-byte aligned, n < 1,
 * ldx < 1 -> AFR_EINVAL, ldx > 256 -> AFR_EUNSUPPORTED; pair_weights -- members or cum2 NULL, an empty member set, member bits above
 * bit 93, floor_w outside 1..65535, gain above 65535, by_pair not 8-byte or cum2, w2 not 4-byte aligned -> AFR_EINVAL. */
#define AFR_TEXT_CONTEXTS 95   /* row 0 = word start, row 1 + i = after code 33 + i */
int afr_op_dataset_text_m(int64_t first_seed, const int64_t* seed_rows, const int64_t* out_rows, int64_t n, int min_len, int max_len,
                          const uint32_t* cum2 /* device [95][94], inclusive cumulative weights per context */,
                          int64_t* codes, int ldx, int32_t* len /* or NULL */, uint32_t* err /* or NULL */, void* stream);
int afr_op_pair_errors(const int64_t* codes, int ldx, const int64_t* code_rows /* or NULL */, int64_t n,
                       const uint32_t* per_pos /* device [n][ldx + 1][4] as afr_op_sheet_char_errors leaves it */,
                       uint64_t* by_pair /* device [95][94][4], ADDED to */, void* stream);
int afr_op_pair_weights(const uint64_t* by_pair /* device [95][94][4] as afr_op_pair_errors leaves it, or NULL */,
                        const uint32_t members[3] /* host: bit i = code 33 + i is in the alphabet */,
                        uint32_t floor_w /* 1..65535 */, uint32_t gain /* 0..65535 */, uint32_t min_chars,
                        uint32_t* cum2 /* device [95][94] */, uint32_t* w2 /* device [95][94] or NULL */, void* stream);

/* ---- rendering error attributed to characters: one launch that lays a text out exactly as compose_sheets does and measures a
 * prediction against the sheet compose_sheets would draw, pixel by pixel, charging every pixel to the character that owns it.  A
 * plain op: no plan, nothing allocated, one workgroup per sheet under compose's grid cap; integers only, so the result repeats
 * bit for bit.
 *   Sample j of n reads row r = code_rows ? code_rows[j] : j of codes int64 [rows][ldx] (text to the first 0, codes outside the
 *   atlas flagged in bit 0 of *err and skipped, wrap, pens and n_lines as compose_sheets) and the dense prediction
 *   pred uint8 [n][height][width] (afr_op_eval's q, for instance).  For pixel (y, x): m = the composed coverage, t = 255 - m the
 *   target level (recomputed, never read), p = pred[j][y][x], d = |p - t|.  Among the glyphs whose cell value b at the pixel is
 *   > 0, in (line, character) order, the OWNER is the one with the largest b, the earlier one on equal b; with none the pixel is
 *   background.  The owner's record gains pixels += 1, sumsq += d * d, off2 += (d >= 2), wrong += ((p >= 128) != (t >= 128)) --
 *   afr_op_eval's stats[1] and stats[3], split by owner.
 *   per_pos uint32 [n][ldx + 1][4] (or NULL), {pixels, sumsq, off2, wrong}: indexed by the character's position in its row of
 *                  codes (not in the packed text); slot ldx is the background.  Every element of row j is stored once; records
 *                  of characters that own nothing -- spaces, characters on lines from n_lines on, skipped codes, positions
 *                  behind the text -- are zero.
 *   by_code uint64 [n_codes + 1][5] (or NULL), {chars, pixels, sumsq, off2, wrong}: ADDED to, the caller zeroes it.  chars counts
 *                  the characters of the code that stand on a drawn line, whether or not they own a pixel; row n_codes is the
 *                  background and its chars counts sheets.  A workgroup sums its sheets in LDS and issues one global integer
 *                  atomic per non-zero field.
 * Errors, before anything is launched: everything compose_sheets refuses (pred in the place of out), both outputs NULL, by_code
 * not 8-byte or per_pos not 16-byte aligned -> AFR_EINVAL; compose_sheets' limits, the LDS budget with the records and counters
 * counted, a sheet of more than 66051 pixels (65025 * pixels must fit 32 bits) -> AFR_EUNSUPPORTED. */
int afr_op_sheet_char_errors(const afr_glyph_atlas* atlas, const afr_sheet_geometry* geo, const int64_t* codes, int ldx,
                             const int64_t* code_rows /* or NULL */, int64_t n, const uint8_t* pred, uint32_t* per_pos /* or NULL */,
                             uint64_t* by_code /* or NULL */, uint32_t* err /* or NULL */, void* stream);

/* ---- rendered sheets read back: one launch that lays a text out exactly as compose_sheets does and asks, for every drawn
 * character, which glyph of the atlas -- placed at this character's pen among its neighbours -- explains the predicted pixels
 * best.  A plain op: no plan, nothing allocated, one workgroup per sheet under compose's grid cap; integers only and no order
 * dependence, so all three outputs repeat bit for bit.
 *   Sample j of n reads row r = code_rows ? code_rows[j] : j of codes int64 [rows][ldx] (text to the first 0, codes outside the
 *   atlas flagged in bit 0 of *err and skipped, wrap, pens and n_lines as compose_sheets) and the dense prediction
 *   pred uint8 [n][height][width].  A character is SCORED if it stands on a drawn line, its code c is not 32, and its window --
 *   its cell box [baseline[i] - origin_y, + cell_h) x [px - origin_x, + cell_w) clipped to the sheet -- is not empty.  For every
 *   window pixel (y, x): a = 255 - pred[j][y][x]; ctx = compose_sheets' fold m = m + b - (m * b + 127) / 255 from 0 over every
 *   OTHER glyph whose cell covers the pixel, in (line, character) order, the scored glyph left out; for a candidate code k,
 *   hyp_k = ctx + b_k - (ctx * b_k + 127) / 255 with b_k = cells[k] at the pixel's place in the cell -- the candidate goes on
 *   last, at the true character's pen; candidates do not move with their own advance or kerning.  score_k = the sum of
 *   (a - hyp_k)^2 over the window.  The candidates are the member codes (members, HOST, three words: bit i = code 33 + i), 32
 *   (the blank: nothing was drawn here) and c itself, member or not.  The smallest score wins; among equal scores c wins if it
 *   is one of them, otherwise the smallest code (so the blank comes first).
 *   read      uint8  [n][ldx]    (or NULL): the winning code, indexed by the character's position in its row of codes (not in the
 *                  packed text).
 *   score     uint32 [n][ldx][2] (or NULL): {the winner's score, score_c}.
 *                  Every element of row j of both is stored once; positions that are not scored hold 0.
 *   confusion uint64 [n_codes][n_codes] (or NULL): confusion[c][read] += 1 per scored character: ADDED to, the caller zeroes it.
 *                  A workgroup counts its sheets in LDS and issues one global integer atomic per non-zero counter.
 * Errors, before anything is launched: everything compose_sheets refuses, as afr_op_sheet_char_errors does (pred in the place of
 * out; the sheet itself may be of any size compose_sheets takes: no sum here runs over more than a window), members NULL, member bits above bit 93, an atlas of fewer than 127 codes (the candidates' cells), all three outputs NULL,
 * score or confusion not 8-byte aligned -> AFR_EINVAL; compose_sheets' limits, a cell of more than 66051 pixels (65025 * pixels
 * must fit 32 bits), more than 256 codes (read is a byte), the LDS budget with the records, the waves' windows and the confusion
 * counters counted -> AFR_EUNSUPPORTED. */
int afr_op_sheet_read_back(const afr_glyph_atlas* atlas, const afr_sheet_geometry* geo, const int64_t* codes, int ldx,
                           const int64_t* code_rows /* or NULL */, int64_t n, const uint8_t* pred,
                           const uint32_t members[3] /* host: bit i = code 33 + i is a candidate */,
                           uint8_t* read /* [n][ldx] or NULL */, uint32_t* score /* [n][ldx][2] or NULL */,
                           uint64_t* confusion /* [n_codes][n_codes] or NULL, ADDED to */, uint32_t* err /* or NULL */, void* stream);

/* ---- the token-wise kernels of the per-pixel-token transformer (AFR_KIND_PIXEL), one launch each, exactly as the plan issues
 * them.  One wave per token row: rows >= 1, d = 64 * heads <= 512 (the widths a plan can reach; AFR_EUNSUPPORTED otherwise),
 * C = context tokens per glyph, 1 or 2; act_dtype AFR_F32 or AFR_BF16 is the type T of the GEMM operands (ctx, add, n, q, kv, o,
 * dO, dq, dy, dhT); the residual stream h / dh, the parameters and every partial slab are float32.  Pointers not marked
 * "or NULL" are required (AFR_EINVAL).  Rows are dense: row r starts at element r * d.
 *   pixel_ctx      ctx T [B][C][d]: ctx[b][0] = emb[x[b]], ctx[b][1] = femb[font[b]] (C = 2 iff n_fonts > 0; font, femb NULL
 *                  otherwise).  An index outside its table sets bit 0 of *err (device word) and is clamped.
 *   pixel_ctx_bwd  demb [vocab][d] (and dfont [n_fonts][d]): row v = sum of dctx[b][0] (dctx[b][1]) over the glyphs b with
 *                  x[b] == v (font[b] == v), in b order; a row no glyph uses is written 0.  dctx f32 [B][C][d].
 *   pixel_add_ln   h = (pos ? pos[r % tokens] : hin[r]) + (add ? add[r] : 0);  n = LayerNorm(h) * g + b.  Exactly one of pos / hin
 *                  is given; add and n may be NULL (n == NULL: g, b are not read).  hin == h is allowed.
 *   pixel_attn     o[r] = softmax_c(q[r]_head . k[b][c]_head / 8) . v[b][c]_head per head of 64 channels, b = r / tokens;
 *                  kv T [B][C][2 d] = [k | v].
 *   pixel_attn_bwd dq T [B * tokens][d]; dkv_part f32 [chunks][B][4 d] = [dk_0 | dv_0 | dk_1 | dv_1] summed over the
 *                  chunk's tokens (C == 1: the second half is written 0), chunks = ceil(tokens / afr_pixel_attn_chunk(tokens)):
 *                  the sum of the chunk slabs (afr_op_reduce) is dk | dv of every context token.
 *   pixel_head     h = hin + add;  u[r] = LayerNorm(h[r]) * g + b  .  w_out + b_out[0];  y = clamp(u, 0, 1), or sigmoid(u) with
 *                  AFR_LOSS_BCE.  u and y may each be NULL.
 *   pixel_head_bwd dh[r] = LayerNorm-backward(du[r] * w_out; x = hf[r]);  dhT (T copy of dh; AFR_BF16 only, or NULL; ignored in
 *                  AFR_F32);  part f32 [afr_pixel_bwd_blocks(rows)][4][d]: per-block sums of dgamma, dbeta, dw_out and (element
 *                  [3][0]) db_out, the rest of [3] zero.
 *   pixel_ln_bwd   dh[r] += LayerNorm-backward(dy[r]; x = hin[r]) in place;  dhT as above;  part f32 [blocks][2][d]: dgamma, dbeta.
 * Every block of the two slab kernels writes its whole slab (zeros where it had no row): no slab needs clearing. */
int afr_pixel_bwd_blocks(long long rows);     /* host-only: partial slabs of pixel_head_bwd / pixel_ln_bwd for a row count */
int afr_pixel_attn_chunk(int tokens);         /* host-only: tokens per attention-backward chunk */
int afr_op_pixel_ctx(int act_dtype, const float* emb, const float* femb, const int64_t* x, const int64_t* font, int B, int d,
                     int vocab, int n_fonts, void* ctx, uint32_t* err, void* stream);
int afr_op_pixel_ctx_bwd(const float* dctx, const int64_t* x, const int64_t* font, int B, int d, int vocab, int n_fonts,
                         float* demb, float* dfont, void* stream);
int afr_op_pixel_add_ln(int act_dtype, const float* hin, float* h, const float* pos, const void* add /* or NULL */, const float* g,
                        const float* b, void* n /* or NULL */, int64_t rows, int tokens, int d, float eps, void* stream);
int afr_op_pixel_attn(int act_dtype, const void* q, const void* kv, void* o, int64_t rows, int tokens, int d, int heads, int C,
                      void* stream);
int afr_op_pixel_attn_bwd(int act_dtype, const void* dO, const void* q, const void* kv, void* dq, float* dkv_part, int B, int tokens,
                          int d, int heads, int C, void* stream);
int afr_op_pixel_head(int act_dtype, int loss_kind, const float* hin, float* h, const void* add, const float* g, const float* b,
                      const float* w_out, const float* b_out, float* u /* or NULL */, float* y /* or NULL */, int64_t rows, int d,
                      float eps, void* stream);
int afr_op_pixel_head_bwd(int act_dtype, const float* du, const float* hf, const float* g, const float* b, const float* w_out,
                          float* dh, void* dhT /* or NULL */, float* part, int64_t rows, int d, float eps, void* stream);
int afr_op_pixel_ln_bwd(int act_dtype, const void* dy, const float* hin, const float* g, float* dh, void* dhT /* or NULL */,
                        float* part, int64_t rows, int d, float eps, void* stream);

/* ---- the sheet model's front end (AFR_KIND_SHEET), its two fused kernels one launch each, exactly as the plan issues them.
 * One 1024-thread block owns a string at a time and loops over the batch (afr_sheet_blocks(B) blocks).  The widths are the
 * reference's: embed_dim 32, 4 heads of 8, fc1 width 64.  act_dtype AFR_F32 or AFR_BF16 is the type T of z and dz (anything else
 * is AFR_EINVAL); parameters, the save area and the slabs are float32.  Pointers not marked "or NULL" are required.
 *   params     the ten small tensors in state_dict order: positional_encoding [max_length][32], embedding.weight [vocab][32],
 *              in_proj_weight [96][32], in_proj_bias [96], out_proj.weight [32][32], out_proj.bias [32], layer_norm.weight [32],
 *              layer_norm.bias [32], fc1.weight [64][32], fc1.bias [64].
 *   x, ldx     int64 codes [B][ldx]; the first L of every row are read (ldx >= L).  A code outside 0 .. vocab-1 sets bit 0 of
 *              *err (device word, or NULL) and is clamped into the table.
 *   drop       NULL: eval (no dropout).  Otherwise a training pass: the three keep masks come from the counter hash of
 *              (seed, step, rank), exactly as a plan with these afr_config fields derives them; every rate is in [0, 1).
 *   z          T [B][max_length*64]: fc1 + ReLU + dropout of the first L positions, then exact zeros.
 *   save       or NULL.  float32 [B][L*56] (afr_sheet_save_floats(B, L) floats; 56 = 32 + 4 + 4 + 16 per position): per string the attention
 *              output o [L][32], the softmax row maxima [4][L], 1/row-sum [4][L] and, in training only, the attention-dropout
 *              keep bits as uint32 [4][L][4]: row (h, i), key j is bit (j>>1)&31 of word (j&1)*2 + (j>>6).  The forward writes
 *              it; the backward reads it, or with save == NULL recomputes the attention from the same dropout stream.
 *   dz         T [B][max_length*64]: the gradient with respect to z (the part beyond L*64 is not read).
 *   slabs      float32 [afr_sheet_blocks(B)][layout->total], 16-byte aligned: every block writes its whole slab -- its partial
 *              gradient of each tensor at the tensor's offset, zeros everywhere else (rows of the positional gradient at or beyond
 *              L, embedding rows of codes it did not meet, the space between tensors) -- so no slab needs clearing and the sum of
 *              the slabs (afr_op_reduce) is the gradient.  layout: the ten offsets in floats (tensor order as in params) and
 *              total, a multiple of 4; the ranges lie inside total and do not overlap.
 * Refused with a message: B < 1, L < 1, L > max_length, ldx < L, vocab < 1, a rate outside [0, 1) (AFR_EINVAL); L > 120
 * (AFR_EUNSUPPORTED: a string's state must fit one compute unit's LDS). */
typedef struct afr_sheet_params { const float *pos, *emb, *w_in, *b_in, *w_o, *b_o, *ln_g, *ln_b, *w1, *b1; } afr_sheet_params;
typedef struct afr_sheet_dropout { uint64_t seed, step; int32_t rank; float p_embed, p_attn, p_fc; } afr_sheet_dropout;
typedef struct afr_sheet_slab_layout { int32_t pos, emb, w_in, b_in, w_o, b_o, ln_g, ln_b, w1, b1, total; } afr_sheet_slab_layout;
int afr_sheet_blocks(int B);                  /* host-only: blocks (= partial slabs) of both kernels for a batch of B strings */
size_t afr_sheet_save_floats(int B, int L);   /* host-only: floats of the save area */
int afr_op_sheet_fwd(int act_dtype, const afr_sheet_params* params, const int64_t* x, int ldx, int B, int L, int max_length, int vocab,
                     float ln_eps, const afr_sheet_dropout* drop /* or NULL */, void* z, float* save /* or NULL */,
                     uint32_t* err /* or NULL */, void* stream);
int afr_op_sheet_bwd(int act_dtype, const afr_sheet_params* params, const int64_t* x, int ldx, int B, int L, int max_length, int vocab,
                     float ln_eps, const afr_sheet_dropout* drop /* or NULL */, const void* dz, const float* save /* or NULL */,
                     float* slabs, const afr_sheet_slab_layout* layout, void* stream);

/* ---- the glyph nets' first layer (AFR_KIND_GLYPH), its kernels one call each, exactly as the plan issues them.  E = embed_dim,
 * N1 = width of fc1, both multiples of 8; K0 = afr_glyph_k0(E, vocab, n_fonts) = E + (vocab + n_fonts rounded up to 8), the columns
 * of the widened operand h0' = [h0 | one-hot of x | one-hot of vocab + font | zero pad].  act_dtype AFR_F32 or AFR_BF16 is the
 * type T of the activations (out, d); the tables emb [vocab][E], femb [n_fonts][E], W1 [N1][E], b1 [N1], every slab and
 * partial are float32; x, font are int64 [B].  n_fonts == 0: femb and font are not read.  font == NULL with n_fonts > 0 means
 * font 0 for every glyph.  The forward kernels set bit 0 of *err (device word) for an index outside its table and clamp it; the
 * backward kernels clamp without flagging.  Pointers not marked "or NULL" are required.
 *   glyph_embed        out T [B][E] = emb[x] + femb[font].
 *   glyph_combo        bf16, one launch: h1c [vocab * max(n_fonts, 1)][ld1] (ld1 >= N1; columns N1 .. ld1 are not written) = the h1
 *                      row of combination c = x * max(n_fonts, 1) + font: relu((T[x] + b1) + T[vocab + font]) with
 *                      T = [emb; femb] . W1^T in float32; h0c bf16 [..][E] = emb[x] + femb[font]; cidx int32 [B] = c of glyph b;
 *                      w1t (or NULL): bf16 [E][N1] = W1^T.  E <= 40 (48 KiB of staging).
 *   glyph_l1_bwd       the post-pass over the widened weight-gradient slabs [nslabs][N1][K0] (slab z at z * slab_stride floats, a
 *                      multiple of 4): dw1 [N1][E] = the slab sum's first E columns; dtab_part [afr_glyph_l1_bwd_blocks(N1)]
 *                      [vocab + n_fonts][E]: per block of 8 fc1 rows n, sum_n S[n][r] W1[n][k] with S = the one-hot columns.
 *   glyph_l1_bwd_fused bf16, E = 32: one kernel per (64 glyphs, column range).  d1 bf16 [B][N1] (row stride N1), h0 bf16 rows of
 *                      ldh elements whose first 32 are emb[x] + femb[font] (row b, or row h0_rowmap[b] with a row map), W1T bf16
 *                      [32][N1].  slabs f32 [afr_glyph_l1_bwd_fused_blocks(B, N1)][afr_glyph_l1_bwd_fused_slab_floats(..)]:
 *                      block (row block rb, range cs) = rb * split + cs holds [dW1 nc x 32 | db1 nc | dTab (vocab + n_fonts) x 32]
 *                      for its nc = N1 / split columns, dTab from ITS columns' share of dh0, rounded to bf16 per glyph.
 *                      Only where afr_glyph_l1_bwd_fused_eligible(AFR_BF16, 32, N1, vocab, n_fonts).
 *   glyph_embed_bwd    slabs f32 [afr_embed_bwd_blocks(B)][vocab + n_fonts][E]: per block of 32 glyphs the sum of d[b] by table
 *                      row, in b order.  The table's accumulator sits in LDS: ((vocab + n_fonts) E + 32 (E + 1)) floats + 256
 *                      bytes must fit 160 KiB (AFR_EUNSUPPORTED beyond; afr_plan_create refuses such a glyph config).
 *   glyph_l1_fwd       the folded forward, two launches: table f32 [vocab + n_fonts][N1] = [emb; femb] . W1^T (and w1t, or NULL: bf16
 *                      [E][N1] = W1^T), then h1 T [B][N1] = relu((table[x] + b1) + table[vocab + font]) and h0p T [B][K0] = h0'.
 *                      E <= 128 and K0 <= 512, the plan's own fold condition; emb, femb, W1, b1, table, h0p, h1 16-byte aligned.
 * Refused with a message before anything is launched: B < 1, vocab < 1, n_fonts < 0, a NULL required pointer (AFR_EINVAL); E or N1
 * not a multiple of 8, the limits above, a dynamic-LDS request above 160 KiB (AFR_EUNSUPPORTED). */
int afr_glyph_k0(int E, int vocab, int n_fonts);                 /* host-only getters, all of them */
int afr_glyph_l1_bwd_blocks(int N1);
int afr_embed_bwd_blocks(int B);
int afr_glyph_l1_bwd_fused_eligible(int dtype, int E, int N1, int vocab, int n_fonts);   /* 1 or 0 */
int afr_glyph_l1_bwd_fused_split(int B, int N1);                 /* column ranges per block of 64 glyphs */
int afr_glyph_l1_bwd_fused_blocks(int B, int N1);
long long afr_glyph_l1_bwd_fused_slab_floats(int B, int N1, int vocab, int n_fonts);
int afr_op_glyph_embed(int act_dtype, const float* emb, const float* femb, const int64_t* x, const int64_t* font /* or NULL */, int B,
                       int E, int vocab, int n_fonts, void* out, uint32_t* err, void* stream);
int afr_op_glyph_combo(const float* emb, const float* femb, const float* W1, const float* b1, const int64_t* x,
                       const int64_t* font /* or NULL */, int B, int E, int N1, int vocab, int n_fonts, void* h1c, int ld1, void* h0c,
                       int32_t* cidx, void* w1t /* or NULL */, uint32_t* err, void* stream);
int afr_op_glyph_l1_bwd(const float* slabs, int nslabs, long long slab_stride, const float* W1, int N1, int E, int vocab, int n_fonts,
                        float* dw1, float* dtab_part, void* stream);
int afr_op_glyph_l1_bwd_fused(const void* d1, const void* h0, int ldh, const int32_t* h0_rowmap /* or NULL */, const void* W1T,
                              const int64_t* x, const int64_t* font /* or NULL */, int B, int N1, int vocab, int n_fonts,
                              float* slabs, void* stream);
int afr_op_glyph_embed_bwd(int act_dtype, const void* d, const int64_t* x, const int64_t* font /* or NULL */, int B, int E, int vocab,
                           int n_fonts, float* slabs, void* stream);
int afr_op_glyph_l1_fwd(int act_dtype, const float* emb, const float* femb, const float* W1, const float* b1, const int64_t* x,
                        const int64_t* font /* or NULL */, int B, int E, int N1, int vocab, int n_fonts, float* table, void* h0p, void* h1,
                        void* w1t /* or NULL */, uint32_t* err, void* stream);

/* ---- the fused step of the small one-hidden-layer glyph nets (E -> N1 -> P), ONE launch: gather, fc1 + ReLU, fc_output, the loss head
 * (AFR_LOSS_MSE: clamp + MSE; AFR_LOSS_BCE: BCE with logits), all six gradient products and the one-hot scatter, exactly as the plan
 * issues it.  A block takes afr_glyph1_rows(dtype) glyphs (16 in AFR_F32, 64 in AFR_BF16) and one of the
 * cs = afr_glyph1_colsplit(dtype, B, P) ranges of P / cs output columns: block rb * cs + pc leaves in slab rb * cs + pc (layout->total
 * floats each, tensors at the layout's offsets) ITS rows [pc, pc + 1) * P / cs of dW2 [P][N1] and db2 [P], and -- from its columns'
 * share of dh1 -- partial dW1 [N1][E], db1 [N1], dEmb [vocab][E] and dFont [n_fonts][E] (table rows none of its glyphs used: +0).
 * Everything else of a slab is not written; the gradient is the sum over the slabs that own an element.
 *   dtype      AFR_F32: W1 [N1][E], W2 [P][N1] are the float32 masters; W1T, W2T are not read.  AFR_BF16: W1, W2 bf16, and their
 *              transposed copies W1T bf16 [E][N1], W2T bf16 [N1][P] (afr_op_transpose_bf16), all four required.
 *   target     uint8 (pixel / 255.0f) or float32 [..][P] by target_dtype; the targets of glyph b are row b, or row target_rows[b].
 *   layout     offsets in floats of emb, font, w1, b1, w2, b2 inside a slab and total, all multiples of 4; the ranges lie inside total
 *              and do not overlap (font is not read when n_fonts == 0).
 *   loss       *loss_accum += sum of the loss terms / mean_elems (mean_elems >= 1).  loss_scratch: 1040 + afr_glyph1_blocks(dtype, B, P)
 *              floats, zero before the first call; the kernel re-arms its counter.
 *   err        device word: bit 0 is set for an index outside its table, which is clamped.
 * Refused with a message before anything is launched: a shape outside afr_glyph1_eligible (E 32 or 64, N1 and P multiples of 64 up to
 * 256, vocab + n_fonts <= 264), a dynamic-LDS request above 160 KiB (AFR_EUNSUPPORTED); any other dtype, loss kind or target type, B < 1,
 * mean_elems < 1, a NULL required pointer, W1 / W2 / W1T / W2T / slabs not 16-byte aligned, a bad layout (AFR_EINVAL).
 * afr_op_transpose_bf16: WT bf16 [K][N] = the transpose of W f32 [N][K], rounded to nearest even. */
typedef struct afr_glyph1_layout { int32_t emb, font, w1, b1, w2, b2, total; } afr_glyph1_layout;
int afr_glyph1_rows(int dtype);                                  /* host-only getters */
int afr_glyph1_colsplit(int dtype, int B, int P);
int afr_glyph1_blocks(int dtype, int B, int P);                  /* row blocks x column split = slabs = loss partials */
int afr_glyph1_eligible(int E, int N1, int P, int vocab, int n_fonts);   /* 1 or 0 */
int afr_op_glyph1_step(int dtype, int loss_kind, const float* emb, const float* femb, const void* W1, const float* b1, const void* W2,
                       const float* b2, const void* W1T /* or NULL in AFR_F32 */, const void* W2T /* or NULL in AFR_F32 */, const int64_t* x,
                       const int64_t* font /* or NULL */, const void* target, int target_dtype, const int32_t* target_rows /* or NULL */,
                       int B, int E, int N1, int P, int vocab, int n_fonts, int64_t mean_elems, float* slabs,
                       const afr_glyph1_layout* layout, float* loss_accum, float* loss_scratch, uint32_t* err, void* stream);
int afr_op_transpose_bf16(const float* W, void* WT, int N, int K, void* stream);

/* ---- fp8 building blocks of BASELINE configs[4] ("fp8 MFMA weights on CDNA4"; no counterpart in the reference) ----
 * Operands are OCP e4m3fn bytes (gfx950's native fp8: exponent bias 7, largest finite 448, no infinities) with ONE float
 * scale per tensor: value = scale * e4m3.  afr_op_f32_to_fp8: dst[i] = e4m3(src[i] / scale) -- the quotient is the correctly
 * rounded float32 division (NOT src[i] * (1.f / scale), another float32 that rounds to another byte next to a tie), rounded to
 * the nearest e4m3 value, ties to the even code; saturating: every quotient beyond +-448, the infinities included, gives the
 * largest finite value of its sign (0x7E / 0xFE); a NaN stays a NaN (byte & 0x7F == 0x7F) and never becomes a finite operand;
 * a quotient that rounds to zero may keep either sign.  Byte-equal to torch's float8_e4m3fn cast of the clamped quotient.
 * Errors (checked before a device is touched): src or dst NULL, n < 0, scale not > 0 (0, negative, NaN) -> AFR_EINVAL.
 * afr_op_gemm_fp8: C[m][n] = scale_ab * sum_k A[m*lda+k] * B[n*ldb+k] (+bias[n]) (relu), f32 accumulation on
 * the MX-scaled matrix instruction (v_mfma_scale_f32_16x16x128_f8f6f4, unit block scales: fp8 at twice the bf16 rate),
 * C f32 or bf16 (AFR_GEMM_OUT_BF16); both operands k-contiguous (the forward form x . W^T), K, lda, ldb multiples of 16,
 * N and ldc multiples of 8.  flags: AFR_GEMM_BIAS | AFR_GEMM_RELU | AFR_GEMM_OUT_BF16.  A is read at [0, M) x [0, K) through lda,
 * B at [0, N) x [0, K) through ldb, C written at [0, M) x [0, N) through ldc and nowhere else; scale_ab multiplies the sum first,
 * then the bias is added, then the ReLU taken, then a bf16 output rounded to nearest even: the AFR_GEMM_OUT_BF16 launch leaves the
 * f32 launch's values rounded, the AFR_GEMM_RELU launch max(the launch without it, +0), bit for bit.  Integer-valued operands whose
 * partial sums stay below 2^11 give the exact sum.  Errors, in this order and before a device is touched: A, B or C NULL, an
 * extent <= 0 -> AFR_EINVAL; any other flag (AFR_GEMM_RELU_MASK, AFR_GEMM_A_KSTRIDED, AFR_GEMM_B_KSTRIDED) -> AFR_EUNSUPPORTED;
 * AFR_GEMM_BIAS with bias NULL -> AFR_EINVAL; K, lda, ldb not multiples of 16 or N, ldc not multiples of 8 -> AFR_EUNSUPPORTED; an
 * operand of 2 GiB or more (M * lda or N * ldb >= 2^31) -> AFR_EUNSUPPORTED. */
int afr_op_f32_to_fp8(const float* src, void* dst_e4m3, int64_t n, float scale, void* stream);
int afr_op_gemm_fp8(int flags, const void* A, const void* B, void* C, const float* bias, int M, int N, int K, int lda, int ldb,
                    int ldc, float scale_ab, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AFR_H */
