/*
 * astyle.h — C ABI of libastyle.so, the MI355X (gfx950) implementation of the
 * winlp4ever/audio_style_transfer optimisation loop's hot path.
 *
 * The reference has no FFI: its boundary is Python calling TensorFlow 1.x.  Each entry point
 * below replaces one reference interface (file:line into the reference):
 *
 *   ast_create / ast_destroy  <- GatysNet.build graph construction + tf.Session
 *                                (methods.py:44-77, 184-188)
 *   ast_set_weight            <- tf.train.Saver(...).restore(sess, ckpt)  (methods.py:79-84),
 *                                one variable per call, by TF name (masked.py:141-145)
 *   ast_forward /             <- cfg.build(...) + cfg.extracts (model.py:57-127) evaluated by
 *   ast_get_extract              sess.run on extracts[i]
 *   ast_embeds                <- GatysNet.get_embeds: sess.run(embeds_c | embeds_s)
 *                                (methods.py:86-95; taps and Gram methods.py:58-76)
 *   ast_set_targets           <- the phi_c / phi_s constants fed into define_loss
 *                                (methods.py:113-119, 207-213)
 *   ast_loss_grad             <- one ScipyOptimizerInterface evaluation: sess.run([loss, grad])
 *                                of define_loss + tf.gradients w.r.t. x (methods.py:113-137,167)
 *   ast_set_gamma             <- the --gamma constant of define_loss (methods.py:125)
 *   ast_lbfgs_*               <- scipy L-BFGS-B under ScipyOptimizerInterface.minimize
 *                                (methods.py:132-137,164-181), per clip on the device
 *   ast_set_anchor /          <- (no reference counterpart) an optional loss term of the long-form
 *   ast_anchor_loss              mode that pulls a window towards given audio where it overlaps
 *                                its neighbours
 *   ast_encoding /            <- the NSynth encoding: the bottleneck pooled over 512-sample hops
 *   ast_set_encoding_target /    (model.py:121-128 ae_pool; fastgen.py:86-113 encode), and an
 *   ast_encoding_loss            optional loss term on it (the term has no reference counterpart)
 *   ast_dec_*                 <- the NSynth WaveNet decoder, one sample step per call:
 *                                FastGenerationConfig.build (nsynth/wavenet/model.py:28-137),
 *                                causal_linear / linear (nsynth/utils.py:838-908) and the loop
 *                                body of fastgen.synthesize (fastgen.py:160-212)
 *   ast_dec_score             <- the decoder of Config.build teacher-forced on a given waveform
 *                                and its loss (nsynth/wavenet/model.py:264-320): log-likelihood
 *                                per sample and the mean negative log-likelihood per clip
 *   ast_stitch                <- (no reference counterpart) the join of overlapping optimised
 *                                windows; the reference writes one window (methods.py:176)
 *   ast_adam_step             <- (new) fused optimiser update on the audio buffer; the
 *                                reference's optimiser is host L-BFGS-B (methods.py:133-137)
 *
 * Conventions: every function returns 0 on success and a negative AST_E* code on failure;
 * ast_last_error() returns a thread-local message.  All buffers named *_dev are device
 * pointers owned by the caller; the context owns weights and the activation workspace
 * (sized at create).  No entry point allocates after ast_create, so ast_loss_grad and
 * ast_adam_step are hipGraph-capturable.  A context is bound to one device and is not
 * re-entrant; the stream is passed per call (NULL = legacy default stream).
 */
#ifndef ASTYLE_H
#define ASTYLE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AST_OK 0
#define AST_E_ARG (-1)      /* invalid argument / configuration */
#define AST_E_HIP (-2)      /* HIP runtime error */
#define AST_E_STATE (-3)    /* call order violated (e.g. loss before targets) */
#define AST_E_NAME (-4)     /* unknown weight name or wrong element count */

#define AST_MAX_TAPS 32

typedef struct ast_ctx ast_ctx;

typedef struct ast_cfg {
    int batch;                       /* clips per context (the reference: 1) */
    int T;                           /* samples per clip (--batch_size), multiple of 512 */
    int n_cont;                      /* --cont_lyrs count            (methods.py:254) */
    int cont_ids[AST_MAX_TAPS];      /* extract ids 0..31            (methods.py:58) */
    int cnt_channels;                /* --cnt_channels               (methods.py:259) */
    int n_style;                     /* resolved style layer count   (methods.py:60-66) */
    int style_ids[AST_MAX_TAPS];     /* extract ids 0..30 */
    int nb_channels;                 /* --channels                   (methods.py:75,258) */
    int gatys;                       /* --gatys                      (methods.py:68-71) */
    int precision;                   /* 0 = fp32 storage + fp32 MFMA; 1 = bf16 storage + bf16 MFMA;
                                        2 = fp32 storage, encoder GEMMs on split-fp16 MFMA (each
                                        fp32 operand as two fp16 halves, 3 products, fp32
                                        accumulation), Gram on bf16 MFMA */
    float lambd;                     /* --lambd                      (methods.py:125) */
    float gamma;                     /* --gamma, STFT regulariser    (methods.py:121-125) */
    int with_encoding;               /* 1: the context can form the NSynth encoding (model.py:121-128,
                                        fastgen.py:86-113) and carry the encoding term: all 30 blocks
                                        run, one more content-gradient buffer, the content tap is
                                        never fused into the Gram backward.  0: as without the field */
} ast_cfg;

/* Context lifetime. */
int ast_create(const ast_cfg* cfg, int hip_device, ast_ctx** out);
void ast_destroy(ast_ctx* ctx);
/* Device bytes ast_create(cfg) on the current device would allocate.  Where the Gram backward
 * puts the style-tapped tensors' direct loss gradients D: a buffer of their own (one more
 * activation set) when the workspace with it leaves max(16 GiB, 10 %) of the device free (this
 * query and ast_create decide so from the current device's free memory), else in place over the
 * activations.  Where both fit and D is >= 4 GiB, the context's first evaluation that is not
 * being captured into a graph (ast_loss_grad / _phase) times its Gram backward in both placements
 * on its own data and keeps the faster (releasing the buffer when in place wins; a capture before
 * it keeps out of place), so the query is the upper bound.  Env ASTYLE_DOOP=1 / 0 forces either.
 * Results are bit-identical in both. */
int ast_workspace_bytes(const ast_cfg* cfg, size_t* out_bytes);
/* *out = 1 when the context keeps D out of place (above), 0 when in place; tuned_ms (may be
 * NULL) [2] = the timed Gram backward in place / out of place (-1: not (yet) timed).  No
 * reference counterpart (a memory-placement report). */
int ast_d_out_of_place(const ast_ctx* ctx, int* out, float* tuned_ms);

/* Weights, HWIO float32 host arrays named as the TF variables ("ae_dilatedconv_7/W",
 * "ae_res_7/biases", "ae_startconv/W", "ae_bottleneck/W", ...). n = element count. */
int ast_set_weight(ast_ctx* ctx, const char* tf_name, const float* host, size_t n);

/* Encoder forward over x_dev [batch, T] (mu-law units, methods.py:49-54). */
int ast_forward(ast_ctx* ctx, const float* x_dev, void* stream);
/* Copy extracts[id] (after ast_forward) to out_dev as float32 [batch, T, C] (C = 16 for id 31). */
int ast_get_extract(ast_ctx* ctx, int extract_id, float* out_dev, void* stream);

/* Forward + taps: emb_c_dev [batch, T, n_cont_cols]; emb_s_dev [batch, nb, L, L] (ours) or
 * [batch, L, 128, 128] (Gatys), l2-normalised.  Either output may be NULL. */
int ast_embeds(ast_ctx* ctx, const float* x_dev, float* emb_c_dev, float* emb_s_dev, void* stream);
int ast_content_cols(ast_ctx* ctx);  /* n_cont_cols of emb_c */

/* Targets (device pointers, caller keeps them alive).  *_shared != 0: one target for all clips. */
int ast_set_targets(ast_ctx* ctx, const float* phi_c_dev, int phi_c_shared,
                    const float* phi_s_dev, int phi_s_shared);

/* One loss+grad evaluation of every clip: grad_dev [batch, T] = d loss / d x, parts_dev
 * [batch, 4] = (content + lambd*style + gamma*reg, content, style, reg).  reg is the STFT
 * regulariser of methods.py:121-123 (0 when T < 1024: no full frame); like TF it is evaluated
 * whatever gamma is, and enters the gradient only through gamma. */
int ast_loss_grad(ast_ctx* ctx, const float* x_dev, float* grad_dev, float* parts_dev, void* stream);
/* ast_loss_grad in two stream-ordered phases: phase 1 = the encoder forward, the content taps and
 * the Gram forward / style loss / Gram backward (grad_dev, parts_dev unused, may be NULL);
 * phase 2 = the backward chain through the blocks, d loss / d x, the loss parts, the STFT
 * regulariser and the range flags (needs phase 1 of the same x first: AST_E_STATE otherwise).
 * phase 0 = both (= ast_loss_grad).  Lets contexts of disjoint clip groups run phase-shifted on
 * separate streams (bench.py --groups): one group's HBM-bound Gram kernels overlap another's
 * MFMA-bound block kernels.  Graph-capturable. */
int ast_loss_grad_phase(ast_ctx* ctx, const float* x_dev, float* grad_dev, float* parts_dev,
                        int phase, void* stream);

/* Per-clip flags accumulated (OR) over every ast_loss_grad since the last reset, into flags_dev
 * (round 4 changed this from "the last call's flags" to sticky; ast_range_flags_last keeps the
 * old per-call meaning)
 * [batch] (int, device) -- sticky, so an out-of-range line-search trial inside a device
 * L-BFGS-B epoch stays visible after the epoch (the reference's ScipyOptimizerInterface sees
 * every evaluation, methods.py:164-181).  Reset: ast_range_flags_reset, ast_lbfgs_begin with
 * x0 or a continuation, and ast_create.  Bits:
 *   AST_RANGE_NONFINITE  the clip's loss parts or gradient hold a NaN / Inf (the reference
 *                        would hand them to the next L-BFGS-B step);
 *   AST_RANGE_ACT        precision 2: a per-clip max |e_l| or the forward intermediate bound
 *                        wdn max|e_l| + bdm (splitwave.h) is >= 2^74 or not finite, so the
 *                        power-of-two scale that keeps the split-fp16 halves in range clamps;
 *   AST_RANGE_GRAD       precision 2: the same for the backward chain max |d loss / d e_l| and
 *                        its bound wrn max|tot|;
 *   AST_RANGE_TINY       precision 2: some per-clip max is below 2^-60 (the halves of that
 *                        tensor lose significand bits; results stay finite).
 * 0 = the evaluation is within the split representation's range.  Graph-capturable. */
#define AST_RANGE_NONFINITE 1
#define AST_RANGE_ACT 2
#define AST_RANGE_GRAD 4
#define AST_RANGE_TINY 8
int ast_range_flags(ast_ctx* ctx, int* flags_dev, void* stream);
/* The same bits for the most recent ast_loss_grad alone (the per-call meaning ast_range_flags
 * had before round 4: a host that checks after every evaluation and never resets can use this
 * one).  Graph-capturable. */
int ast_range_flags_last(ast_ctx* ctx, int* flags_dev, void* stream);
/* Clear the accumulated range flags (stream-ordered; graph-capturable). */
int ast_range_flags_reset(ast_ctx* ctx, void* stream);

/* Workgroup budget of the persistent split block kernels (one workgroup per CU): at most cus
 * CUs (0 = every CU, the default).  Several contexts holding disjoint clip groups can then run
 * concurrently on one GPU, each on its own stream: while one group's HBM-bound Gram kernels run,
 * another's MFMA-bound block kernels use the other CUs (bench.py --groups).  A captured graph
 * bakes the grid in: recapture after a change.  No reference counterpart (a scheduling knob). */
int ast_set_cu_limit(ast_ctx* ctx, int cus);

/* Change gamma (methods.py:125) without rebuilding the context. */
int ast_set_gamma(ast_ctx* ctx, float gamma);

/* Seam anchor term (no reference counterpart; the long-form mode, longform.py).  Per clip b
 *   anchor_b = mu * sum_t w[b,t] (a(x[b,t]) - ref[b,t])^2 / sum_t w[b,t]   (0 when sum_t w[b,t] = 0)
 * with a the TF inv_mu_law of the STFT regulariser (utils.py:92-104).  While set, every
 * ast_loss_grad adds it to parts[b][0] (the [batch, 4] layout stays: the term's value is the
 * total minus the other three weighted parts, or ast_anchor_loss) and its gradient
 * 2 mu w (a - ref) a'(x) / sum w to grad_dev, in phase 2, before the range flags.  Computed in
 * fp32 whatever the precision, partial sums in a fixed order without atomics: a clip's value and
 * gradient are bit-identical in any slot of any batch and from run to run.
 * ref_dev [batch,T] audio units, w_dev [batch,T] >= 0, caller keeps both alive; the values are
 * read at every evaluation (sum w included), so they may be overwritten in place between
 * evaluations, also under a captured graph.  ref_dev == NULL or mu == 0 clears the term; unset,
 * no anchor kernel launches.  Setting or clearing changes the kernels ast_loss_grad launches:
 * recapture a captured graph. */
int ast_set_anchor(ast_ctx* ctx, const float* ref_dev, const float* w_dev, float mu);
/* the term's value (mu included) per clip at the most recent ast_loss_grad; 0 when unset */
int ast_anchor_loss(ast_ctx* ctx, float* out_dev /*[batch]*/, void* stream);

/* The NSynth encoding (model.py:121-128 `ae_pool`; fastgen.py:86-113 `encode`): the encoder
 * forward over x_dev [batch, T], then per clip and 512-sample hop r (R = T / 512)
 *   enc[b, r, j] = (1/512) sum_{t in hop r} (sum_c e_30[b, t, c] W_b[c, j] + b_b[j]),  j < 16
 * (ae_bottleneck 1x1, then pool1d window = stride = 512: no padding, a plain mean) to out_dev
 * [batch, T/512, 16].  The kernel averages the 128 channels over the hop first (rows in a fixed
 * order), then applies the 1x1 in channel order and adds the bias: the same linear map, and that
 * order defines the result.  fp32 whatever the precision; a clip's encoding is bit-identical in
 * any slot of any batch and from run to run.  AST_E_STATE on a context created without
 * with_encoding.  Graph-capturable. */
int ast_encoding(ast_ctx* ctx, const float* x_dev, float* out_dev /*[batch, T/512, 16]*/, void* stream);
/* Encoding term on the encoding above (model.py:121-128, fastgen.py:86-113; the term itself has no
 * reference counterpart).  Per clip b
 *   enc_term_b = omega * mean_{r, j} (enc(x)[b, r, j] - phi_e[b, r, j])^2     over all R x 16 entries.
 * While set, every ast_loss_grad adds it to parts[b][0] (the [batch, 4] layout stays: the term's
 * value is ast_encoding_loss) in phase 2 after the STFT regulariser and before the anchor term, and
 * its gradient 2 omega / (16 R 512) sum_j W_b[c, j] (enc - phi_e)[b, t / 512, j] to d loss / d e_30
 * in phase 1, next to the content taps.  fp32 whatever the precision, sums in a fixed order without
 * atomics: bit-identical per clip in any slot of any batch, from run to run and under graph replay.
 * phi_e_dev [batch, R, 16], or [R, 16] when shared != 0; caller keeps it alive; it is read at every
 * evaluation, so it may be overwritten in place between evaluations, also under a captured graph.
 * phi_e_dev == NULL or omega == 0 clears the term; unset, no encoding kernel launches and the
 * backward chain starts at the highest tapped tensor.  omega must be finite and >= 0.  Setting or
 * clearing changes the kernels ast_loss_grad launches: recapture a captured graph.  AST_E_STATE on
 * a context created without with_encoding. */
int ast_set_encoding_target(ast_ctx* ctx, const float* phi_e_dev, int shared, float omega);
/* the encoding term's value (omega included) per clip at the most recent ast_loss_grad; 0 when
 * unset (model.py:121-128, fastgen.py:86-113).  AST_E_STATE without with_encoding. */
int ast_encoding_loss(ast_ctx* ctx, float* out_dev /*[batch]*/, void* stream);

/* The NSynth WaveNet decoder (nsynth/wavenet/model.py:28-137 FastGenerationConfig; nsynth/utils.py:
 * 838-908 causal_linear / linear; fastgen.py:160-212 synthesize), one sample step per call.  A
 * context of its own: it shares nothing with an ast_ctx.  Per clip b and step t, with x the
 * previous step's sample (0 at t = 0) and en = enc[b, t / hop]:
 *   x_s = mu_law(x) / 128;  l = startconv(x_s(t-2), x_s(t-1), x_s(t));  s = skip_start(l)
 *   layer i, rate r = 2^(i mod n_stages):
 *     a = W_i[0] l(t-2r) + W_i[1] l(t-r) + W_i[2] l(t) + b_i + cond_map_i(en)     (l(t') = 0 for t' < 0)
 *     d = sigmoid(a[:width]) tanh(a[width:]);  l += res_i(d);  s += skip_i(d)
 *   s = relu(s);  s = relu(out1(s) + cond_map_out1(en));  pmf = softmax(logits(s))          256 bins
 *   cdf = running fp32 sum of pmf in bin order;  bin = min(first k with cdf[k] >= u, 255)
 *   audio = inv_mu_law_numpy(bin - 128)
 * The clamp to 255 is the one deviation: np.searchsorted returns 256 when rounding leaves
 * cdf[255] < u, and the reference then decodes a bin that does not exist.  bin -> audio and
 * bin -> the next x_s go through two 256-entry fp32 tables filled on the host at create
 * (ast_dec_tables): inv_mu_law_numpy (nsynth/utils.py:122-136) in float64 cast to float32, then
 * mu_law (nsynth/utils.py:70-85) with floor, / 128.  All products are fp32 MFMA with fp32
 * accumulation in a fixed order (csrc/decoder.hip), no atomics: a clip's pmf and bins are
 * bit-identical at batch 1 and in any slot of any batch, from run to run and under graph replay. */
typedef struct ast_dec ast_dec;
typedef struct ast_dec_cfg {
    int batch;        /* clips, 1..256 */
    int width;        /* residual channels (the reference: 512), a multiple of 64 */
    int skip_width;   /* skip channels (256), a multiple of 32, at most 352 */
    int n_layers;     /* 30; 1..64 */
    int n_stages;     /* 10: layer i has rate 2^(i mod n_stages); 1..16 */
    int n_z;          /* encoding channels: 16 */
    int hop;          /* samples per encoding row (512), >= 1 */
} ast_dec_cfg;
/* Device bytes ast_dec_create(cfg) allocates: weights, state and the per-layer rings
 * [2 rate][batch][width].  AST_E_ARG with a message for a configuration outside the ranges above. */
int ast_dec_workspace_bytes(const ast_dec_cfg* cfg, size_t* out_bytes);
/* The configuration is validated before the device is touched.  Nothing allocates after create. */
int ast_dec_create(const ast_dec_cfg* cfg, int hip_device, ast_dec** out);
void ast_dec_destroy(ast_dec* dec);
/* The two tables of the draw (above), host only: audio256[bin], xs256[bin] = the next step's x_s. */
int ast_dec_tables(float* audio256, float* xs256);
/* One variable by its TF name: startconv, skip_start, dilatedconv_k, cond_map_k, res_k, skip_k
 * (k = 1..n_layers), out1, cond_map_out1, logits; each with /W (HWIO float32) and /biases.
 * AST_E_NAME for an unknown name or a wrong element count. */
int ast_dec_set_weight(ast_dec* dec, const char* tf_name, const float* host, size_t n);
/* Saver.restore (fastgen.py:182-183): every decoder variable from a checkpoint-V2 prefix. */
int ast_dec_restore(ast_dec* dec, const char* prefix);
/* init_ops (fastgen.py:186): every queue reads as zero, position 0, input sample 0.  Graph-capturable. */
int ast_dec_reset(ast_dec* dec, void* stream);
/* One sample step at the position t kept in device memory: reads enc_dev [batch, R, n_z] row
 * t / hop and u_dev[b, t], writes bins_dev[b, t], audio_dev[b, t] and, when pmf_dev is not NULL,
 * pmf_dev[b, t, 0..255], then advances t.  At t >= total it does nothing, so a captured graph of
 * K calls replayed ceil(total / K) times is the whole synthesis.  With force_dev (int
 * [batch, total], values 0..255) the next step's input comes from force_dev[b, t] instead of the
 * drawn bin (teacher forcing); the bin is still drawn and written.  total must be in 1..R hop
 * (AST_E_ARG).  Launches only: graph-capturable with stable pointers. */
int ast_dec_step(ast_dec* dec, const float* enc_dev, int R, const float* u_dev, const int* force_dev,
                 int total, int* bins_dev, float* audio_dev, float* pmf_dev, void* stream);
/* *out_dev = t.  Graph-capturable. */
int ast_dec_position(ast_dec* dec, int* out_dev, void* stream);

/* Scoring: the decoder teacher-forced over whole sequences (Config.build, model.py:264-320), the
 * same network and weights as the step form above with time on the GEMMs' N side
 * (csrc/decoder_score.hip).  For clip b and t < T, with x_s(0) = 0 and x_s(t) = table[bins[b, t-1]]
 * (masked.shift_right), the step form's layers give logits[b, t]; then
 *   logp[b, t] = log_softmax(logits[b, t])[bins[b, t]] = (logit[label] - max) - logf(sum exp(. - max))
 *   nll[b]     = -(1/T) sum_t logp[b, t]                  (fp64 sum in a fixed order; nats per sample)
 * input_mode 0: table = xs256 of ast_dec_tables, the synthesis feedback, so a synthesised clip is
 * scored under exactly the distributions it was drawn from; input_mode 1: table[bin] =
 * (bin - 128) / 128, the training graph's input (model.py:213-214, 264), and nll is its `loss`.
 * fp32 MFMA with fp32 accumulation, one accumulation order per output element whatever batch, slot
 * or T: a clip's outputs are bit-identical at batch 1 and in any slot, and a run on a prefix equals
 * the first columns of the run on the whole sequence.  The label is clamped to 0..255 on the device
 * for memory safety only: callers pass bins in range.
 *
 * The work area (l, d [batch, T, width], s [batch, T, skip_width]) is the caller's; the score batch
 * is independent of cfg.batch.  Host only: its bytes.  AST_E_ARG for an invalid configuration,
 * batch outside 1..65535 or T < 1. */
int ast_dec_score_workspace_bytes(const ast_dec_cfg* cfg, int batch, int T, size_t* out_bytes);
/* bins_dev int [batch, T], enc_dev [batch, R, n_z] (row t / hop conditions sample t).  Writes
 * logp_dev [batch, T], nll_dev [batch] and, when not NULL, pmf_dev / logits_dev [batch, T, 256].
 * Reads the context's weights and writes none of its synthesis state (l, s, d, rings, position,
 * x queue).  AST_E_ARG with a message, before any launch, for batch < 1, T outside 1..R hop,
 * input_mode not 0 or 1, a NULL required pointer, or work_bytes below
 * ast_dec_score_workspace_bytes.  Launches only: graph-capturable with stable pointers. */
int ast_dec_score(ast_dec* dec, const int* bins_dev, const float* enc_dev, int batch, int R, int T,
                  int input_mode, void* work_dev, size_t work_bytes, float* logp_dev, float* nll_dev,
                  float* pmf_dev, float* logits_dev, void* stream);

/* Join n overlapping windows into one signal (no reference counterpart; no context).  Window k
 * [T] starts hop = T - 2 late - fade samples after window k - 1; the `late` guard samples at both
 * ends of a window are dropped (methods.py:39,176), neighbours crossfade over `fade` samples with
 * weights sin^2(pi/2 (j + 1/2) / fade) and one minus that, which sum to 1.  Every output sample
 * gathers the one or two windows covering it through inv_mu_law_numpy (utils.py:85-90, x == 0 ->
 * 0); no atomics, deterministic.  AST_E_ARG for T < 4096, fade < 0 or 2 fade > T - 2 late.  Peak
 * normalisation (methods.py:176) stays with the caller.  Graph-capturable. */
int ast_stitch(const float* x_dev /*[n,T] mu-law units*/, int n, int T, int late, int fade,
               float* out_dev /*[(n-1)*hop + T - 2*late] audio*/, void* stream);

/* Fused Adam on the audio buffer: m, v, x updated in place from grad_dev. step >= 1. */
int ast_adam_step(ast_ctx* ctx, float* x_dev, float* m_dev, float* v_dev, const float* grad_dev,
                  int step, float lr, float beta1, float beta2, float eps, void* stream);
/* Same, with the step counter in device memory: uses *step_dev + 1 and stores it back, so a
 * captured hipGraph of {ast_loss_grad, ast_adam_step_dev} replays as consecutive steps. */
int ast_adam_step_dev(ast_ctx* ctx, float* x_dev, float* m_dev, float* v_dev, const float* grad_dev,
                      int* step_dev, float lr, float beta1, float beta2, float eps, void* stream);

/* Device-resident batched L-BFGS-B: one scipy.optimize.minimize(method='L-BFGS-B') call per
 * clip (no bounds; history m, maxiter, maxls, ftol = factr*eps, gtol = pgtol as scipy's
 * options), all clips advancing together, one loss+grad evaluation per step:
 *   ast_lbfgs_begin(x0)                       x_dev <- fp32(x0): the first point to evaluate
 *   repeat { ast_loss_grad(x_dev -> grad, parts); ast_lbfgs_step(grad, parts) -> next x_dev }
 *   until every clip's phase (ast_lbfgs_state) is 0
 * ws_dev: caller-owned device workspace of ast_lbfgs_workspace_bytes(m); it records the m it
 * was started with (begin with x0), and step / state / a continuation use that m, so loops of
 * different m may share a context.  x0_dev [batch, T] float64 (NULL: continue from each clip's
 * current point with the workspace's own m, the next epoch of methods.py:164);
 * active_dev [batch] int (NULL = all) selects the clips that run.  info_dev [batch, 4] =
 * (phase, iterations, evaluations, reason: 0 running, 1 maxiter, 2 pgtol, 3 rel. reduction
 * of f, 4 abnormal line search, 5 the workspace header is not one begin wrote for this batch
 * and T); x64_dev [batch, T] (may be NULL) the current float64 point.  Both counts are
 * scipy.optimize.minimize's: iterations are its nit, accepted points only (an abnormal end of
 * the line search adds none); evaluations are its nfev, so a trial point bit-identical (the
 * whole float64 array) to the previous trial is not handed back for evaluation, as scipy
 * serves it from its cache -- the search goes on inside the same step with the f and grad at
 * hand, and neither the count nor the history (ast_lbfgs_history) moves.  step / state / a
 * continuation on a workspace this context never started with x0 fail with AST_E_STATE.
 * begin/step allocate nothing, so the step pair is hipGraph-capturable. */
int ast_lbfgs_workspace_bytes(ast_ctx* ctx, int m, size_t* out_bytes);
int ast_lbfgs_begin(ast_ctx* ctx, void* ws_dev, float* x_dev, const double* x0_dev,
                    const int* active_dev, int m, int maxiter, int maxls, double ftol,
                    double gtol, void* stream);
int ast_lbfgs_step(ast_ctx* ctx, void* ws_dev, float* x_dev, const float* grad_dev,
                   const float* parts_dev, void* stream);
int ast_lbfgs_state(ast_ctx* ctx, const void* ws_dev, int* info_dev, double* x64_dev,
                    void* stream);
/* The loss history of the current (or last) minimize call, every evaluation's
 * (total, content, style, regularizer) parts in evaluation order: what the reference's
 * loss_callback writes to its event file at every evaluation (methods.py:147-157, 167).
 * out_dev [batch, max_evals, 4] float; rows past a clip's evaluation count (info[2]) are NaN.
 * The workspace keeps the first AST_LBFGS_HISTORY evaluations of a call (scipy's maxiter 100
 * with maxls 20 makes at most 2001); max_evals in 1..AST_LBFGS_HISTORY. */
#define AST_LBFGS_HISTORY 4096
int ast_lbfgs_history(ast_ctx* ctx, const void* ws_dev, float* out_dev, int max_evals,
                      void* stream);

/* Per-kernel-family device timing (HIP events on the call's stream).  enable!=0 starts
 * recording; ast_timing_read fills out[0..n) with milliseconds summed since enable for
 * {block fwd, block bwd, gram fwd, gram bwd, other} and out[5] = number of ast_loss_grad
 * calls timed, out[6] = launches per family per call (blocks). */
int ast_timing(ast_ctx* ctx, int enable);
int ast_timing_read(ast_ctx* ctx, float* out, int n);

/* TensorFlow checkpoint-V2 reader (tf.train.NewCheckpointReader / Saver.restore, methods.py:
 * 79-84): <prefix>.index (SSTable of BundleEntryProto) + <prefix>.data-NNNNN-of-MMMMM.  Host
 * memory only, no device.  Entries are in name order; dtype is TF's DataType enum (1 float,
 * 2 double, 14 bfloat16, 19 half: read as float32; others refused). */
typedef struct ast_ckpt ast_ckpt;
int ast_ckpt_open(const char* prefix, ast_ckpt** out);
void ast_ckpt_close(ast_ckpt* ck);
int ast_ckpt_num_entries(const ast_ckpt* ck);
int ast_ckpt_entry(const ast_ckpt* ck, int i, char* name, size_t name_cap, int* dtype, int* ndim,
                   int64_t* dims, int max_dims);
int ast_ckpt_read_f32(const ast_ckpt* ck, const char* name, float* host, size_t n);
/* Saver.restore(sess, prefix) (methods.py:79-84): every encoder variable of the NSynth
 * checkpoint (ae_startconv, ae_dilatedconv_1..30, ae_res_1..30, ae_bottleneck; W and biases)
 * by its TF name into ctx, as ast_set_weight.  A missing variable fails with AST_E_NAME. */
int ast_restore(ast_ctx* ctx, const char* prefix);

/* Batched ADMM optimal transport between NMF palettes: OT_ADMM + transform_palette
 * (optimal_transport.py:77-162; compute_permutation = both).  For each of nprob problems,
 * p_mod_dev [n1, d] and p_ref_dev [n2, d] float64 -> plan_dev [n1, n2] (the transport plan),
 * palette_dev [n1, d] (p_ref moved onto p_mod's palette: plan p_ref / (row sums + 1e-10);
 * NULL = skip), iters_dev [nprob] int (ADMM iterations; NULL = skip).  eps, miter as OT_ADMM's
 * (1e-4, 1e5).  fp64, one workgroup per problem; no context.  n1 n2 <= 4096: iterates in
 * registers; larger (up to n1 n2 <= 2^16): iterates in a device workspace the call allocates
 * and frees stream-ordered (hipMallocAsync), so that form is not for capture in a graph that
 * outlives the call.  That kernel is one workgroup per problem streaming ~80 B per cell per
 * ADMM iteration (2^16 cells: ~0.1 ms per iteration); the NMF palettes of the reference are
 * 5..40 components per side. */
int ast_ot_admm(const double* p_mod_dev, const double* p_ref_dev, int nprob, int n1, int n2, int d,
                double eps, double miter, double* plan_dev, double* palette_dev, int* iters_dev,
                void* stream);

const char* ast_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* ASTYLE_H */
