/* glowk -- C ABI of the MI355X (gfx950) Glow forward / inverse / log-prob engine.
 *
 * The reference (SamArgt/AudioSourceSep) has no native boundary: its "operator API" for this path is
 * the Python duck type of tfd.TransformedDistribution / tfb.Bijector returned by
 * flow_models/flow_builder.py:60-146 (build_glow).  Each entry point below names the reference
 * interface it replaces; audiosourcesep_amd/flow_models/ binds them with ctypes and re-creates that
 * duck type (INTEGRATION.md shows the binding).
 *
 * Conventions
 *   - every tensor is NHWC, float32, contiguous; "dev" pointers are device (HBM) addresses owned by the
 *     caller (e.g. torch storages), "host" pointers are ordinary host memory;
 *   - every compute call is asynchronous on the hipStream_t passed as `stream` (void*, 0 = null stream);
 *   - return value: 0 = OK, non-zero = error (enum glowk_status); glowk_last_error() returns a thread-local message;
 *   - one handle per device; a handle is not thread safe; the engine owns packed weights + workspace;
 *   - every entry point that touches the GPU selects the handle's device for the duration of the call and restores the
 *     caller's current device before returning.
 *   - `level` counts blocks from 0 (glowBlock1 = 0); `step` is the creation index k of glowStep_k
 *     (flow_glow.py:44-49).  The forward pass applies steps K-1 ... 0 (tfb.Chain order, :51-52).
 */
#ifndef GLOWK_H
#define GLOWK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GLOWK_VERSION 559

/* Arguments of build_glow (flow_builder.py:60-61) + SpecPreprocessing kwargs (flow_tfp_bijectors.py:365). */
typedef struct glowk_config {
  int32_t H, W, C;     /* data_shape */
  int32_t L, K, F;     /* L in {2,3,4}; K steps per block; F = n_filters in {128, 256, 384, 512} (glowk_create rejects others) */
  int32_t learntop;    /* 1: learnable diagonal Gaussian prior (flow_builder.py:131-141), 0: N(0,1) (:142-144) */
  int32_t use_logit;   /* SpecPreprocessing(use_logit=...) */
  float minval, maxval, alpha;
  float bn_eps;        /* Keras BatchNormalization epsilon (1e-3) */
} glowk_config;

typedef struct glowk_handle glowk_handle;

/* Tensors of one flow step in the reference's own layouts (creation order of SURVEY appendix A.3). */
enum glowk_tensor_id {
  GLOWK_ACTNORM_LOG_SCALE = 0, /* [c]          ActNorm.log_scale   flow_tfp_bijectors.py:236 */
  GLOWK_ACTNORM_SHIFT = 1,     /* [c]          ActNorm.shift       :239 */
  GLOWK_INV1X1_P = 2,          /* [c,c]        Invertible1x1Conv.P :281 */
  GLOWK_INV1X1_SIGN_S = 3,     /* [c]          sign_S              :285 */
  GLOWK_INV1X1_L = 4,          /* [c,c]        L                   :289 */
  GLOWK_INV1X1_LOG_S = 5,      /* [c]          log_S               :291 */
  GLOWK_INV1X1_U = 6,          /* [c,c]        U                   :293 */
  GLOWK_CONV1_KERNEL = 7,      /* [3,3,c/2,F]  HWIO                flow_tfk_layers.py:56-60 */
  GLOWK_CONV1_BIAS = 8,        /* [F] */
  GLOWK_BN1_GAMMA = 9,         /* [F]          batch_norm_1        :61 */
  GLOWK_BN1_BETA = 10,
  GLOWK_BN1_MEAN = 11,
  GLOWK_BN1_VAR = 12,
  GLOWK_CONV2_KERNEL = 13,     /* [1,1,F,F]                        :63-65 */
  GLOWK_CONV2_BIAS = 14,       /* [F] */
  GLOWK_BN2_GAMMA = 15,        /* [F]          batch_norm_2        :66 */
  GLOWK_BN2_BETA = 16,
  GLOWK_BN2_MEAN = 17,
  GLOWK_BN2_VAR = 18,
  GLOWK_CONV3_KERNEL = 19,     /* [3,3,F,c]                        :68-70 */
  GLOWK_CONV3_BIAS = 20,       /* [c] */
  GLOWK_INV1X1_P_INV = 21,     /* [c,c]        P_inv, the stored inverse of P that _inverse multiplies by  :282-284,313.  Left unset
                                  (all zeros) the engine uses inv(P), which is what the reference initialises it to. */
  GLOWK_NUM_STEP_TENSORS = 22,
  /* prior (level = -1, step = 0), flow_builder.py:131-139 */
  GLOWK_PRIOR_LOC = 100,       /* [H/2^L, W/2^L, C*4^L] */
  GLOWK_PRIOR_LOG_SCALE = 101  /* same shape: log of scale_diag (TransformedVariable(.., Exp())) */
};

/* Arithmetic of the coupling-network contractions (the >95 % of the FLOPs), for every compute entry point of the handle
 * (forward, inverse, log_prob, log_prob_grad, param_grad, sample, the per-step calls).  Shapes without a split-kernel instance
 * run the exact kernels in every mode (at the supported widths: the 32-channel level of 4-level models at n_filters 128;
 * glowk_kernel_families tells which family every launch took). */
enum glowk_precision {
  GLOWK_PREC_F32 = 0,     /* v_mfma_f32_32x32x2_f32: exact fp32 products, fp32 accumulate (default) */
  GLOWK_PREC_F16X3 = 1,   /* error-compensated split: x = hi + lo in fp16, 3 fp16 MFMAs per product, fp32 accumulate:
                             fp32-class results (~5e-8 relative on log_prob) at ~3x the speed; assumes hidden activations
                             below 16 376 in magnitude (any normalised flow) */
  GLOWK_PREC_F16X2 = 2    /* throughput mode of the plain forward direction (forward, log_prob, inverse, sample): weights
                             hi + lo, activations rounded to fp16 once, 2 fp16 MFMAs per product -- log_prob ~1e-5 relative
                             (inside the 1e-4 bar, no longer fp32-class); log_prob_grad runs the F16X3 kernels in this mode,
                             and so do shapes without a two-term instance */
};

enum glowk_status {
  GLOWK_OK = 0,
  GLOWK_ERR = 1,         /* bad argument / unsupported shape / HIP error: see glowk_last_error() */
  GLOWK_ERR_RANGE = 2    /* a split-precision call left the fp16 range (see glowk_range_policy); outputs are not usable */
};

/* Range guard of the split arithmetics (F16X3 / F16X2).  Every value that is split into fp16 hi + lo must stay below
 * 65504 / 4 in magnitude; beyond that hi = inf, lo = -inf, the next contraction is NaN -- and the ReLU after it turns that NaN
 * into 0: a finite, WRONG result that no test of the outputs can see.  The guard is therefore STATIC: glowk_finalize_weights
 * (and the device-side refresh after glowk_apply_gradients) bounds every split value of a flow step by the L1 norms of its
 * BatchNorm-folded weights as a linear function of the largest coupling-network INPUT, and solves for the input magnitude
 * `xlim` up to which no split can overflow; the network kernels compare the inputs they gather against it (prologue, once per
 * pixel; nothing in the MFMA loops) and raise a sticky per-handle flag on the device.  It is a worst-case bound: it may send a
 * legitimate call to the exact kernels, it cannot miss an overflow.  Second, free source of the same flag: a non-finite network
 * output, coupling result or gradient seen by the coupling / gradient kernels (non-finite input tiles, a genuinely exploding
 * flow -- what the reference's callers assert on, run_basis_sep.py:183-191, train_glow.py:115-118).
 * What a compute call (forward, inverse, log_prob, log_prob_sum, log_prob_grad, param_grad, sample, step_*, coupling_net) does
 * with the flag:
 *   GLOWK_RANGE_ERROR (default)  after its launches the call waits for the stream, reads the flag and, if set, clears it and
 *                                returns GLOWK_ERR_RANGE: the outputs of the call are not usable;
 *   GLOWK_RANGE_FALLBACK         same check, but the call is re-run inside the engine on the exact fp32 kernels and returns
 *                                that result (0); glowk_range_status counts the re-runs;
 *   GLOWK_RANGE_IGNORE           no wait, no read: calls stay fully asynchronous (hipGraph capture); the caller polls
 *                                glowk_range_status.
 * Calls in GLOWK_PREC_F32 never check: there a non-finite result is the reference's own result. */
enum glowk_range_policy { GLOWK_RANGE_IGNORE = 0, GLOWK_RANGE_ERROR = 1, GLOWK_RANGE_FALLBACK = 2 };

int glowk_version(void);
const char* glowk_last_error(void);
/* Diagnostic switches (environment variables GLOWK_NO_FUSE, GLOWK_CO_OFF, GLOWK_CO_RING3, GLOWK_BWD_LIGHT_4, ...: one launch form forced for a
 * form-against-form parity test; none is needed for normal use) are read when the library is loaded, not per launch; a process
 * that changes its environment afterwards calls this to have them read again.  (No reference counterpart.) */
void glowk_reload_env(void);

/* --- construction: replaces build_glow (flow_builder.py:60-146) --------------------------------- */
int glowk_create(const glowk_config* cfg, int device, glowk_handle** out);
int glowk_destroy(glowk_handle* h);
/* number of elements tensor `id` of (level, step) holds, or 0 if the id/level is invalid */
size_t glowk_tensor_size(const glowk_handle* h, int level, int tensor_id);
/* copy one tensor host -> engine / engine -> host: replaces assigning / reading flow.variables
 * (train_utils.py:67-68 uses them as the checkpoint root) */
int glowk_set_tensor(glowk_handle* h, int level, int step, int tensor_id, const float* host, size_t n);
int glowk_get_tensor(const glowk_handle* h, int level, int step, int tensor_id, float* host, size_t n);
/* assemble W = P L U and W^-1 (flow_tfp_bijectors.py:300-303,309-315), fold ActNorm into the 1x1,
 * fold BN into per-channel affines, pack the conv kernels into MFMA operand order, upload. Must be
 * called after the last glowk_set_tensor and before any compute call. Synchronous. */
int glowk_finalize_weights(glowk_handle* h);
/* ActNorm data-dependent initialisation (flow_tfp_bijectors.py:222-234) as build_glow drives it: the
 * minibatch x [N,H,W,C] is preprocessed, squeezed and pushed through the steps one by one; before each
 * step its ActNorm log_scale/shift are set from the per-channel mean / population std (+1e-8) of the
 * tensor reaching it (GlowBlock.__init__, flow_glow.py:40-49).  All other tensors must be set and
 * glowk_finalize_weights called first; the new ActNorm tensors can be read back with glowk_get_tensor.
 *   runtime_order = 0: steps are visited in creation order 0..K-1 exactly like the reference constructor
 *                      (although tfb.Chain later applies them K-1..0);
 *   runtime_order = 1: steps are visited in the order the forward pass applies them (K-1..0), which keeps
 *                      every step's input normalised at run time (used for the synthetic benchmark weights);
 *   raw_minibatch_quirk = 1: blocks 2+ of the 3- and 4-level graphs are initialised from the RAW preprocessed
 *                      minibatch reinterpreted by Squeeze's reshape, as GlowBijector_3blocks/_4blocks do
 *                      (flow_glow.py:162-165,171-174); 0: from the propagated second half.
 * Synchronous (reads statistics back per step). */
int glowk_actnorm_data_init(glowk_handle* h, const float* x_dev, int N, int runtime_order, int raw_minibatch_quirk, void* stream);
int glowk_set_precision(glowk_handle* h, int precision);
int glowk_get_precision(const glowk_handle* h);
int glowk_set_range_policy(glowk_handle* h, int policy);
int glowk_get_range_policy(const glowk_handle* h);
/* waits for `stream`, reports whether the sticky range flag is set (and clears it) and how many calls were re-run on the
 * fp32 kernels so far; either output may be NULL */
int glowk_range_status(glowk_handle* h, int* tripped, int64_t* fallbacks, void* stream);
/* The margin of the static bound, measured: between glowk_range_probe_begin and glowk_range_probe_end every split-kernel launch
 * of the handle also records the largest coupling-network input it gathered (one atomic per wave, in the kernels' prologue);
 * glowk_range_probe_end waits for `stream` and returns, over all those launches, the largest  input / limit  of the forward
 * networks -- below 1 the guard did not fire, 0 means no split launch ran -- and, for the backward (gradient) networks, which
 * are linear and normalise every pixel's gradient vector by a power of two before the split (so that no gradient magnitude can
 * leave the range), the static ratio (smallest usable normalisation) / (what the weights' worst-case bound allows).  A
 * diagnostic (bench.py reports it for the trained BASIS priors); off by default. */
int glowk_range_probe_begin(glowk_handle* h);
int glowk_range_probe_end(glowk_handle* h, float* fwd_ratio, float* bwd_ratio, void* stream);
/* The split kernels' activation + fp16 hi/lo split on its own (handle-free; for tests): n fp32 values through the very device helpers
 * the network kernels inline, hi_dev / lo_dev = the two fp16 halves as bit patterns.  mode 0: max(x, 0) * sc, split (the hidden
 * activations); 1: the two-term mode, hi only and lo = 0 (f16x2); 2: x * sc, split, no activation (the gathered inputs).  sc must be a
 * power of two, as every scale the engine hands the kernels is (GLOWK_ERR otherwise).  New in version 551. */
int glowk_split_probe(const float* x_dev, int n, float sc, int mode, uint16_t* hi_dev, uint16_t* lo_dev, void* stream);
/* device memory (bytes) the engine allocates for batches up to N: the forward/inverse workspace, plus -- with_grad != 0 --
 * the per-step saves and gradient scratch of glowk_log_prob_grad in the handle's current precision.  glowk_reserve allocates
 * exactly that up front, so that no later compute call of that kind with that batch size (or a smaller one in the same
 * launch regime) allocates or synchronises the device (required before hipGraph capture).  Buffers only ever grow. */
size_t glowk_workspace_bytes(const glowk_handle* h, int N, int with_grad);
int glowk_reserve(glowk_handle* h, int N, int with_grad);
/* the largest batch ONE call accepts (2^28 elements / (H*W*C): indices within a call are 32-bit); every batch entry point
 * rejects a larger N with GLOWK_ERR.  Tiles are independent, so a caller with more tiles loops over chunks
 * (audiosourcesep_amd/engine.py does). */
int glowk_max_tiles(const glowk_handle* h);

/* --- the hot path ------------------------------------------------------------------------------- */
/* Chain([glow, prepro]).forward(x) and its forward_log_det_jacobian (flow_builder.py:127;
 * flow_glow.py:102-108,119-126 / 176-185,198-209 / 268-282,298-313): x [N,H,W,C] -> z [N,Hl,Wl,Cl],
 * logdet [N] (may be NULL). */
int glowk_forward(glowk_handle* h, const float* x_dev, int N, float* z_dev, float* logdet_dev, void* stream);
/* Chain.inverse(z): z -> x (flow_glow.py:110-117 / 187-196 / 284-296) */
int glowk_inverse(glowk_handle* h, const float* z_dev, int N, float* x_dev, void* stream);
/* TransformedDistribution.log_prob(x) (train_glow.py:30, run_basis_sep.py:77): logp [N];
 * z_dev may be NULL or receives the latent */
int glowk_log_prob(glowk_handle* h, const float* x_dev, int N, float* logp_dev, float* z_dev, void* stream);
/* glowk_log_prob that also leaves sum_n logp[n] on the device as ONE fp64 value (accumulate != 0: added to *sum_dev -- batches
 * evaluated in chunks): the summed log-likelihood of train_glow.py:29-31 / :52-54, which is what the ranks all-reduce (one
 * element, RCCL).  The sum is taken in a fixed order (k_sum_f64), so it is bitwise repeatable for a given shard. */
int glowk_log_prob_sum(glowk_handle* h, const float* x_dev, int N, float* logp_dev, float* z_dev, double* sum_dev, int accumulate,
                       void* stream);
/* the reduction alone: *out_dev = (accumulate ? *out_dev : 0) + scale * sum of n floats, fp64, fixed order; no handle needed
 * (scale = -1 / global batch gives the replica's share of tf.nn.compute_average_loss, train_glow.py:29-31) */
int glowk_sum_f64(const float* v_dev, size_t n, double* out_dev, int accumulate, double scale, void* stream);
/* compute_grad_logprob (run_basis_sep.py:73-79): logp [N] and d sum(logp) / dx [N,H,W,C] */
int glowk_log_prob_grad(glowk_handle* h, const float* x_dev, int N, float* logp_dev, float* dx_dev, void* stream);
/* TransformedDistribution.sample(n) (train_glow.py:74) with the standard-normal draw supplied by the
 * caller: eps [N,Hl,Wl,Cl] -> x = chain.inverse(loc + exp(log_scale) * eps) */
int glowk_sample(glowk_handle* h, const float* eps_dev, int N, float* x_dev, void* stream);
/* prior.log_prob(z) alone: [N] */
int glowk_prior_log_prob(glowk_handle* h, const float* z_dev, int N, float* logp_dev, void* stream);

/* --- measurement ---------------------------------------------------------------------------------- */
/* Per-kernel HIP-event timing of the coupling-network kernel (k_net), recorded on the stream each launch
 * goes to.  glowk_profile_begin arms it, every later compute call brackets its k_net launches with
 * events, glowk_profile_end synchronises, sums the elapsed times per level and disarms.  Used by bench.py
 * for the roofline object; off by default (no events, no overhead). */
typedef struct glowk_profile {
  double net_ms[4];          /* summed k_net duration per level */
  int64_t net_launches[4];
} glowk_profile;
int glowk_profile_begin(glowk_handle* h);
/* number of flow steps so far that ran as ONE kernel -- coupling network + affine coupling + next step's ActNorm / 1x1 fused
 * (flow_glow.py:21-22 as a single launch) -- rather than as network kernel + coupling kernel */
int64_t glowk_fused_steps(const glowk_handle* h);
/* coupling-network launches of the handle so far, by kernel family: out7[0] the exact fp32 kernel (k_net_f32), [1] the split
 * kernel on v_mfma_f32_32x32x16_f16 (k_net_h3), [2] on 16x16x32 (k_net_h3s), [3] its 128-pixel half-wave form, [4] the fused
 * network + coupling kernel, [5] of these ([2] or [4]) the launches that took the co-resident form (k_net_h3c: four-wave / 128-pixel
 * workgroups, two to a CU), [6] of [3] the launches that took the small-grid form with all conv1 blocks first (k_net_h3q).  A handle
 * in a split arithmetic whose out7[0] stays put ran no level on the exact kernels. */
int glowk_kernel_families(const glowk_handle* h, int64_t* out7);
int glowk_profile_end(glowk_handle* h, glowk_profile* out);
/* Launch trace of the coupling-network kernels (since version 510; no reference counterpart).  Which of the ~100 kernel instances a
 * launch takes is decided at run time from the level shape, the direction and arithmetic, the pixel count against the device's
 * compute units and the host's flags; the seven counters above cannot tell two or four passes, passes as workgroups of their own
 * or not, merged or pre-summed outputs apart.  Between glowk_net_trace_begin and glowk_net_trace_end the handle keeps one record
 * per coupling-network launch of its compute calls, in launch order -- the recompute launch of a training sweep that does not keep
 * its hiddens included, dry queries of the policy not.  Every field but the request is what the launch function itself reports it
 * took.  Host memory only: no device call, no synchronisation, the kernels and their arguments are untouched; off by default, and an
 * unarmed handle pays one untaken branch per launch. */
typedef struct glowk_net_record {
  int32_t level;      /* block of the flow, from 0 */
  int32_t dir;        /* the request: 0 plain forward network, 1 the gradient path's saving forward network, 2 backward network */
  int32_t arith;      /* ... 0 exact fp32, 1 the three-term fp16 split, 2 the two-term split */
  int32_t store;      /* ... 1: a training launch that also stores its hidden tensors */
  int32_t Q;          /* pixels of the launch: N * h * w of the level */
  int32_t family;     /* index into glowk_kernel_families' out7: 0 k_net_f32, 1 k_net_h3, 2 k_net_h3s, 3 its half-wave form, 4 fused */
  int32_t passes;     /* passes over the hidden width of the instance: 2 or 4; 0 for the exact kernel */
  int32_t split;      /* 1: every pass ran as workgroups of its own (grid.y = passes), 0: all passes in one workgroup */
  int32_t np;         /* partial output buffers written (1: the passes' sums were merged in the kernel; 0: the coupling was fused) */
  int32_t co;         /* 1: the co-resident form (k_net_h3c) */
  int32_t q;          /* 1: the small-grid form with all conv1 blocks first (k_net_h3q) */
  int32_t fused_px;   /* > 0: the coupling ran inside the kernel, in workgroups of this many pixels */
  int32_t presum;     /* 1: conv3's horizontal taps were added in registers */
} glowk_net_record;
/* arms the trace and drops what an earlier one left */
int glowk_net_trace_begin(glowk_handle* h);
/* disarms it; *count = the number of launches since glowk_net_trace_begin, whatever cap is; out[0 .. min(cap, *count)) receive the
 * first records (out may be NULL when cap is 0).  When *count <= cap the records are dropped; otherwise they are kept until a
 * second call with room for them (or the next glowk_net_trace_begin). */
int glowk_net_trace_end(glowk_handle* h, glowk_net_record* out, int cap, int* count);

/* --- sub-bijectors, as exercised one by one by unittest_flow_models.py:124-186 --------------------- */
/* Squeeze._forward / _inverse (flow_tfp_bijectors.py:170-180); no handle needed */
int glowk_squeeze(const float* x_dev, int N, int H, int W, int C, float* y_dev, void* stream);
int glowk_unsqueeze(const float* y_dev, int N, int h, int w, int c4, float* x_dev, void* stream);
/* SpecPreprocessing forward / inverse / fldj (flow_tfp_bijectors.py:372-396) */
int glowk_preprocess_forward(glowk_handle* h, const float* x_dev, int N, float* y_dev, float* logdet_dev, void* stream);
int glowk_preprocess_inverse(glowk_handle* h, const float* y_dev, int N, float* x_dev, void* stream);
/* GlowStep forward (+fldj) / inverse (flow_glow.py:24-31) of step `step` of block `level`:
 * u, y are [N,h,w,c] of that level; logdet [N] may be NULL */
int glowk_step_forward(glowk_handle* h, int level, int step, const float* u_dev, int N, float* y_dev, float* logdet_dev, void* stream);
int glowk_step_inverse(glowk_handle* h, int level, int step, const float* y_dev, int N, float* u_dev, void* stream);
/* ShiftAndLogScaleConvNet.call (flow_tfk_layers.py:73-84) of one step: xb [N,h,w,c/2] -> log_s, t [N,h,w,c/2] */
int glowk_coupling_net(glowk_handle* h, int level, int step, const float* xb_dev, int N, float* log_s_dev, float* t_dev, void* stream);

/* --- training step (train_glow.py:29-44, train_noisy_glow.py:31-44) -------------------------------------------------------
 * The reference's train_step is  loss = sum(-flow.log_prob(X)) / global_batch;  gradients = tape.gradient(loss,
 * flow.trainable_variables);  optimizer.apply_gradients(...)  under MirroredStrategy (per-replica gradients summed by an
 * all-reduce).  Here: glowk_param_grad fills ONE flat fp32 vector with  scale * d sum_n log_prob(x_n) / d theta  for this rank's
 * tiles (scale = -1 / global batch), the caller all-reduces that vector across ranks (RCCL; torch.distributed in the mirror),
 * glowk_apply_gradients takes the optimizer step on the engine's device-resident master copy of the parameters and refreshes
 * the packed kernel images on the device.  The sweep runs in the handle's arithmetic: with GLOWK_PREC_F16X3 / F16X2 on the split
 * kernels (hidden tensors stored in their scaled units, undone in the gradient assembly; weight-gradient GEMMs in the same
 * three-product fp16 split; fp32-class gradients, ~3x the exact sweep) wherever every level has training instances, under the range guard (a tripped sweep is repeated on the exact kernels
 * unless the policy is GLOWK_RANGE_ERROR); otherwise, and with GLOWK_PREC_F32, on the exact fp32 kernels.  glowk_apply_gradients
 * refreshes the exact images always and the fp16 hi/lo images (BatchNorm folds, power-of-two scales, epilogue constants,
 * range-guard limits; bit for bit the host packer's) when the handle is in a split arithmetic.
 * Layout of the vector: glowk_param_offset.  It holds every tf.Variable of the flow except the frozen P, P_inv, sign_S; the
 * BatchNorm moving mean / variance (non-trainable, never updated by the reference: the layers are called without training=)
 * are carried with zero gradient.
 * Memory: the sweep keeps, per pixel and flow step, the two hidden activations of the coupling network (4 KB at n_filters 512:
 * 5.6 GB for 32 tiles of 64x64, K = 32, L = 3) and, a level at a time, their two gradients (as much again for the largest
 * level) when a quarter / a third of the free device memory holds them; otherwise it re-runs each step's forward network and
 * works step by step -- slower, same results to fp32 rounding. */
size_t glowk_param_vector_size(glowk_handle* h);
/* where tensor `tensor_id` of (level, step) -- or a prior tensor (level, step ignored) -- sits in the vector */
int glowk_param_offset(glowk_handle* h, int level, int step, int tensor_id, size_t* offset, size_t* count);
/* x [N,H,W,C] -> grad_dev [glowk_param_vector_size] (overwritten) and, if logp_dev != NULL, log_prob [N].  The results are
 * ordered on `stream` like those of every other call.  The call returns once the data-gradient sweep has finished on the device (the
 * host's share -- the c x c fp64 chain rule of ActNorm / 1x1 -- then runs beside the last weight-gradient GEMMs; its results go up on
 * an internal stream that `stream` waits for by event); since version 400 it does NOT join `stream`: synchronise it before reading
 * grad_dev from the host. */
int glowk_param_grad(glowk_handle* h, const float* x_dev, int N, float scale, float* logp_dev, float* grad_dev, void* stream);
/* one optimizer step: optimizer 0 = Adam, 1 = Adamax (train_utils.py:23-41; Keras defaults beta_1 0.9, beta_2 0.999, epsilon 1e-7).
 * glowk_get_tensor / flow.variables see the new values. */
int glowk_apply_gradients(glowk_handle* h, const float* grad_dev, int optimizer, float lr, void* stream);

/* --- BASIS: the annealed-Langevin update around the log_prob_grad calls of a step (run_basis_sep.py:152-181) --------------- */
/* One kernel, two argument lists: glowk_basis_update_n (further down) takes 2..16 sources and either mixing process of the
 * reference (:106-149); glowk_basis_update is its call for two sources and the dB mixture under the argument list the package
 * started with.  Its results are pinned bit for bit (tests/golden/basis_two_source.npz). */
/* One step of basis_inner_loop for two sources, in place, as ONE kernel:
 *     mix = g(x1, x2) (:133-141),  (m1, m2) = grad_g(x1, x2) (:143-147),
 *     x_k <- x_k + eta (g_k + lambda_recon m_k (mixed - mix)) + sqrt(2 eta) N(0, I)        (:163-164, :180-181)
 * with g_k = compute_grad_logprob(x_k, model_k) supplied by the caller (glowk_log_prob_grad).  All tensors hold n floats.
 * The normal draws come from the engine's counter-based device RNG (Philox4x32-10 keyed by `seed`, counter = element, `step`,
 * source) unless eps1_dev / eps2_dev supply them (tests replay the oracle's draws; the reference draws unseeded).
 * `offset` (a multiple of 4) is the position of element 0 in that stream: a rank that holds tiles [a, b) of the mixture passes
 * a * H * W * C and draws exactly what one process would have drawn for those tiles, so a sharded run is the unsharded one.
 * nonfinite_dev (optional, one int on the device): set to 1 when a gradient, the mixture or an updated value is not finite --
 * the reference's debug asserts (:183-191).
 * The conditions of glowk_basis_update_n hold here too: step < 2^48, and x1, x2 are distinct buffers that do not overlap
 * `mixed` (a state updated in place under an alias never had a meaning: each element's update reads both states). */
int glowk_basis_update(float* x1_dev, float* x2_dev, const float* g1_dev, const float* g2_dev, const float* mixed_dev, size_t n,
                       float eta, float lambda_recon, const float* eps1_dev, const float* eps2_dev, uint64_t seed, uint64_t step,
                       uint64_t offset, int* nonfinite_dev, void* stream);
/* g(x1, x2) alone: the mixture of two sources in dB, sum in power (:133-141); glowk_basis_mix_n for two sources */
int glowk_basis_mix(const float* x1_dev, const float* x2_dev, float* out_dev, size_t n, void* stream);
/* The mixing processes g(*sources) / grad_g(*sources) of run_basis_sep.py for S = len(sources).  (Its scale == 'power' branch is
 * not offered: its grad_g is not the derivative of its g, and nothing here lives in power scale.) */
enum glowk_mixing {
  GLOWK_MIX_DB = 0,   /* :131-147  g = 10/ln10 (logsumexp_k(x_k ln10/10) - ln S),  grad_g = softmax_k(x_k ln10/10) */
  GLOWK_MIX_MEAN = 1  /* :108-116  g = mean_k x_k,                                 grad_g = 1/S */
};
/* One step of basis_inner_loop for nsrc sources, in place, as ONE kernel (since version 470):
 *     mix = g(x_0 .. x_{S-1}),  (m_k) = grad_g(x_0 .. x_{S-1}),
 *     x_k <- x_k + eta (g_k + lambda_recon m_k (mixed - mix)) + sqrt(2 eta) N(0, I)         for k = 0 .. S-1
 * x, g, eps: HOST arrays of nsrc DEVICE pointers, each to n floats (the pointers travel in the kernel arguments; the arrays are
 * not read after the call returns).  eps may be NULL, and so may any entry of it: that source draws from the device RNG, stream
 * `which` = k & 1 with source pair k >> 1 (glowk_random_source), so sources 0 and 1 draw what glowk_basis_update draws and no two
 * sources share a draw.  nsrc in [2, 16]; the x buffers must not overlap each other or `mixed`; `offset` a multiple of 4, as
 * for glowk_basis_update; step < 2^48 (the pair shares the counter word of step >> 32); mixing: enum glowk_mixing.  A thread
 * moves four consecutive elements of every source as 16-byte accesses when every pointer is 16-byte aligned; the last partial
 * quad and unaligned pointers go element by element.  GLOWK_ERR on any violated condition, before anything is launched. */
int glowk_basis_update_n(float* const* x, const float* const* g, const float* const* eps, int nsrc, const float* mixed_dev, size_t n,
                         int mixing, float eta, float lambda_recon, uint64_t seed, uint64_t step, uint64_t offset,
                         int* nonfinite_dev, void* stream);
/* g(x_0 .. x_{nsrc-1}) alone; x as above, nsrc in [2, 16] */
int glowk_basis_mix_n(const float* const* x, int nsrc, float* out_dev, size_t n, int mixing, void* stream);
/* the device RNG itself: out[e] = the draw glowk_basis_update makes for element e of (seed, step, which); uniform != 0 gives
 * U(0, 1) from the same stream instead of N(0, 1) (the chain's initial state, run_basis_sep.py:360-361); `offset` (a multiple
 * of 4): out[0] is element `offset` of the stream, as for glowk_basis_update.
 * The mapping, exactly (tests/rng_ref.py restates it; the U(0, 1) draws are bit for bit a function of it).  Element e of the
 * stream (seed, step, which, pair) sits in the quad q = (offset + e) / 4 and takes word (offset + e) % 4 of the output of
 * Philox4x32-10 (Salmon et al., SC'11: multipliers 0xD2511F53 and 0xCD9E8D57, Weyl increments 0x9E3779B9 and 0xBB67AE85, ten
 * rounds, the key bumped after each round) for
 *     c0 = lo32(q)
 *     c1 = hi32(q) ^ (which << 28)
 *     c2 = lo32(step)
 *     c3 = hi32(step) ^ (pair << 16)
 *     key = (lo32(seed), hi32(seed))
 * with pair = 0 for glowk_random and glowk_add_noise.  A word w becomes u = (top 24 bits of w + 0.5) / 2^24 in float32,
 * ((float)(w >> 8) + 0.5f) * 2^-24: the sum rounds to even from 2^23 on and to 2^24 at the largest word, so the U(0, 1) draws
 * are clamped to the largest float below 1 (since version 490; the draw was 1.0 there before) and lie in [2^-25, 1 - 2^-24].
 * The N(0, 1) draws are Box-Muller on the unclamped u: words (0, 1) of a quad give elements (0, 1) and words (2, 3) elements
 * (2, 3) as (u1, u2) -> sqrt(-2 ln u1) (cos, sin)(fl32(2 pi) u2) in float32; u1 = 1 gives the pair (0, 0).
 * Elements at or beyond 2^62 would carry hi32(q) into the bits of `which`: offset + n above 2^62 is GLOWK_ERR, before anything
 * is launched, here and in glowk_random_source, glowk_add_noise, glowk_basis_update_n and glowk_basis_update (since version
 * 490). */
int glowk_random(float* out_dev, size_t n, uint64_t seed, uint64_t step, int which, int uniform, uint64_t offset, void* stream);
/* the draw source k of glowk_basis_update_n makes: glowk_random with the source pair k >> 1 folded into the counter (XORed as
 * pair << 16 into the word that holds step >> 32) and which = k & 1; pair = 0 is glowk_random itself.  pair in [0, 65535]; a
 * non-zero pair needs step < 2^48. */
int glowk_random_source(float* out_dev, size_t n, uint64_t seed, uint64_t step, int which, int pair, int uniform, uint64_t offset,
                        void* stream);
/* out = x + sigma * N(0, I), the draws being those of glowk_random(seed, step, which, offset): the input noise of the
 * noise-conditioned training step (train_noisy_glow.py:31, X + tf.random.normal(X.shape) * noise).  out_dev may equal x_dev. */
int glowk_add_noise(const float* x_dev, float* out_dev, size_t n, float sigma, uint64_t seed, uint64_t step, int which, uint64_t offset,
                    void* stream);

/* --- audio: mel front end and mel-to-audio inversion (datasets/data_loader.py:146-164, melspec_inversion_basis.py:21-93) ----- */
/* Handle-free; the constants of the reference's front end are compiled in: 16 kHz, n_fft 2048, hop 512, periodic Hann, 96 Slaney
 * mels over 125..7600 Hz (librosa.filters.mel defaults), dB clipped to [-100, 20].  Spectra are [.., 1025, F] with the frame
 * fastest; a complex spectrum is re/im interleaved (torch.complex64).  The first call on a device uploads its constants there.
 * Every tensor must be device memory on one device (a host pointer is refused); the caller owns the shapes.
 */
/* the front end's mel filterbank W [96][1025] (float32, row-major) as the kernels use it, into a host buffer; no device call */
int glowk_mel_filterbank(float* host_out);
/* audio [N, n_samples] 16 kHz -> mel_db [N, 96, F], F = 1 + n_samples/512 (librosa.stft center=True, reflect padding,
 * |X|^2, mel, power_to_db, np.clip); stft_dev (nullable) [N, 1025, F] complex, re/im interleaved; top_db <= 0: no per-extract
 * floor, else L = max(L, max over the extract of L - top_db) before the clip.  1024 < n_samples < 65536 (F <= 128).  Without
 * stft_dev the call takes an [N, 1025, F] float scratch from the stream-ordered allocator for |X|^2. */
int glowk_mel_frontend(const float* audio_dev, int N, int n_samples, float top_db, float* mel_db_dev, float* stft_dev, void* stream);
/* mel_db [N, 96, F] -> linear power [N, 1025, F]: 10^(L/10), then per frame the NNLS of librosa.feature.inverse.mel_to_stft
 * by FISTA (projected gradient with Nesterov momentum, step 1/|W|_2^2) from max(0, W+ b), `iters` iterations (0..100000);
 * F in [1, 128]. */
int glowk_mel_to_power(const float* mel_db_dev, int N, int frames, int iters, float* power_dev, void* stream);
/* power [S, N, 1025, F] + mixture STFT [N, 1025, F] -> audio [S, N, (F-1)*512] (librosa.istft, center=True): wiener == 0 reuses
 * the mixture's phase, sqrt(x) X / |X| (phase 1 where X == 0); wiener != 0 needs S >= 2 and filters x_i / (sum_j x_j + 1e-10) X.
 * S in [1, 16], F in [2, 128]. */
int glowk_masked_istft(const float* power_dev, int S, const float* stft_mix_dev, int N, int frames, int wiener, float* audio_dev,
                       void* stream);
/* Griffin-Lim (librosa.griffinlim: n_iter iterations, momentum, then one last iSTFT): magnitudes mag [N, 1025, F] -> audio
 * [N, (F-1)*512].  angles0_dev (nullable: all ones) [N, 1025, F] complex holds iteration 0's phases as given; each iteration is
 * an STFT of the latest signal, then an iSTFT of mag a / (|a| + 1e-16), a = rebuilt - momentum / (1 + momentum) * previous
 * rebuilt (previous = 0 at the first update).  2n_iter + 1 launches on `stream`, no host synchronisation; for n_iter >= 1 the
 * call takes two complex [N, 1025, F] spectra from the stream-ordered allocator (one when n_iter == 1), and audio_dev holds the
 * signal between launches.  N in [0, 2^20], F in [4, 2^20], n_iter in [0, 100000], momentum finite and >= 0; bitwise
 * reproducible. */
int glowk_griffinlim(const float* mag_dev, const float* angles0_dev, int N, int frames, int n_iter, float momentum, float* audio_dev,
                     void* stream);

/* --- sample-rate conversion: the resampling of librosa.core.load (datasets/preprocessing.py:21) ---------------------------- */
/* Handle-free.  The filter is librosa 0.7's default design (resampy's kaiser_best: Kaiser-windowed sinc, 64 zero crossings, 512
 * table points per zero crossing, beta = 14.769656459379492, roll-off 0.9475937167399596), evaluated at the exact position of every
 * tap: same design, not bit-compatible with resampy (whose samples cannot be observed here; derived, not observed).  With a, b =
 * sr_in, sr_out over their gcd, s = min(1, b / a) and t a = q b + r in 64-bit integers:
 *   y[t] = s sum_m x[m] h(s ((q - m) + r / b)),  h(u) = T[k] + (p - k) (T[k + 1] - T[k]) with p = |u| 512, k = floor(p), 0 for p > 32768,
 *   T[k] = rho sinc(rho k / 512) I0(beta sqrt(1 - (k / 32768)^2)) / I0(beta);  x is zero outside [0, n_in).
 * Ranges: sr_in, sr_out in [1000, 768000] with 1/64 <= sr_out / sr_in <= 64, nsig in [0, 2^20], n_in in [0, 2^32]; anything else
 * is GLOWK_ERR. */
/* ceil(n_in * sr_out / sr_in), or -1 for arguments the conversion would refuse; no device call */
int64_t glowk_resample_length(int64_t n_in, int sr_in, int sr_out);
/* the table T [32769] (double) as the kernel's host builder makes it, into a host buffer; no device call */
int glowk_resample_filter(double* host_out);
/* x [nsig][n_in] -> y [nsig][n_out], n_out as above; float32 device memory on one device (a host pointer is refused), one launch
 * on `stream`, no allocation beyond the first call's table upload on a device, no host synchronisation.  fp32 accumulation in an
 * order fixed relative to each output's centre q: bitwise reproducible, and independent of nsig, of n_in and of the position in
 * the signal (x delayed by a samples gives y delayed by b).  nsig == 0 or n_in == 0 is a successful no-op.  sr_in == sr_out runs
 * the filter (a low-pass at 0.9476 of Nyquist, not the identity): audio.resample returns its input for equal rates instead.  One
 * launch holds at most 2^31 - 1 workgroups of 256 outputs (fewer per workgroup when sr_in / sr_out exceeds 40). */
int glowk_resample(const float* x_dev, int nsig, int64_t n_in, int sr_in, int sr_out, float* y_dev, void* stream);

/* --- BSS Eval v4: SDR / ISR / SIR / SAR (bsseval_v4.py, sigsep's v4 with the v3 wrappers) ----------------------------------- */
/* Handle-free, fp64 throughout.  sig_dev [nsig][nsampl] holds the reference channels p = j * nchan + c (P = nsrc * nchan of
 * them) followed by the estimate channels P + jest * nchan + c.  A window is a half-open sample range [start, stop); a window's
 * slice of a signal is zero outside it.  Tensors and descriptor arrays are device memory on one device (a host pointer is
 * refused); out-of-range descriptors give empty windows or status 2, never an access outside the tensors.  Each call enqueues on
 * `stream` and takes its scratch from the stream-ordered allocator.  audiosourcesep_amd/bsseval.py drives the three calls.
 */
/* the correlations of _compute_reference_correlations (:465-498) and _compute_projection_filters (:520-534), linear:
 * corr[w][k][d] = sum_m s_u[m] s_v[m + d] over window w's slices, (u, v) = pairs[k], d in [0, filters_len); win [nwin][2]
 * (int64), max_len >= every window's length.  filters_len in [1, 512].  Partial sums are added in a fixed order: bitwise
 * reproducible. */
int glowk_bss_xcorr(const double* sig_dev, int nsig, int64_t nsampl, const int64_t* win_dev, int nwin, int64_t max_len, const int* pairs_dev,
                    int npairs, int filters_len, double* corr_dev, void* stream);
/* the distortion filters of _compute_projection_filters (:536-548): per system k, (G + eps I) C = D with eps = DBL_EPSILON, by
 * Cholesky.  sys [nsys][2] = (window w of corr, first reference channel p0); G[(p,a),(q,b)] over the nchan_sys channels from p0
 * is corr[w][p nref + q][a - b] (or corr[w][q nref + p][b - a]), D[(p,a), e] = corr[w][nref^2 + p nref + e][a] for the nref
 * estimate channels e; so corr needs npairs >= 2 nref^2 in that order.  coef [nsys][nref][nchan_sys * filters_len] (column e
 * of C, row p * filters_len + a).  status [nsys]: 0 solved, 1 a pivot was not positive and finite (the caller redoes the
 * system by least squares, as the reference does on LinAlgError), 2 bad descriptor.  nchan_sys * filters_len <= 2048; the
 * Cholesky workspaces in flight are capped at 2 GiB (systems run in chunks). */
int glowk_bss_solve(const double* corr_dev, int nwin, int npairs, int nref, int filters_len, int nchan_sys, const int* sys_dev, int nsys,
                    double* coef_dev, int* status_dev, void* stream);
/* _bss_decomp_mtifilt (:421-437) with _project (:557-581) and the sums of _bss_crit (:584-608): items [nitems][6] (int64) =
 * (start, stop, jtrue, jest, C system, Cj system); C = coef_c[C system] (nref = nsrc * nchan, all reference channels), Cj =
 * coef_j[Cj system] (nchan_sys = nchan, the channels of jtrue).  energy [nitems][8]: |s_true|^2, |est - s_true|^2, |e_spat|^2,
 * |s_true + e_spat|^2, |e_interf|^2, |s_true + e_spat + e_interf|^2, |e_artif|^2, |e_interf + e_artif|^2 over the window's
 * len + filters_len - 1 samples and every channel.  nsrc * nchan * filters_len <= 2048. */
int glowk_bss_project(const double* sig_dev, int64_t nsampl, int nsrc, int nchan, int filters_len, const int64_t* items_dev, int nitems,
                      int64_t max_len, const double* coef_c_dev, int nsys_c, const double* coef_j_dev, int nsys_j, double* energy_dev,
                      void* stream);

/* --- oracle separation systems: IBM, IRM, MWF and the mel-domain masks (oracle_systems.py, from sigsep-mus-oracle) ---------- */
/* Handle-free.  STFT / iSTFT in scipy.signal's conventions for nperseg 2048: periodic Hann, hop 1024, 1024 zeros on each side,
 * zero-padded to whole frames, scaled by 1/sum(win) = 1/1024, one-sided; T = ceil(n / 1024) + 1 frames.  Spectra are
 * [nsig][1025][T] complex (re/im interleaved, frame fastest), fp32 on the exact-fp32 MFMA.  The mask and MWF calls take the spectra
 * of one separation: rows 0 .. nchan-1 the mixture's channels, then source j's channel c at row nchan + j * nchan + c, and
 * overwrite the source rows with the estimates' spectra.  eps = DBL_EPSILON.  Every tensor must be device memory on one device (a
 * host pointer is refused); each call enqueues on `stream`; scratch comes from the stream-ordered allocator.
 * audiosourcesep_amd/oracle_systems.py drives the calls.
 */
/* x [nsig][n] (float) -> spec [nsig][1025][T] (scipy.signal.stft(x, nperseg=2048)).  1 <= n <= 2^40. */
int glowk_sp_stft(const float* x_dev, int nsig, int64_t n, float* spec_dev, void* stream);
/* spec [nsig][1025][frames] -> out [nsig][length] (scipy.signal.istft defaults, then [:length]): irfft (the imaginary parts of DC
 * and Nyquist dropped) times sum(win), overlap-add of the 2 frames of each sample, divided by the overlap-added win^2, 1024
 * samples trimmed at each end.  frames >= 2, 0 <= length <= (frames - 1) * 1024. */
int glowk_sp_istft(const float* spec_dev, int nsig, int frames, int64_t length, float* out_dev, void* stream);
/* in place on the source rows, per channel, fp64: irm == 0: Y_j = X * [|Y_j|^alpha / (eps + |X|^alpha) >= theta] (the reference's
 * two assignments in order: >= theta -> 1, then < theta -> 0), the bits optionally to mask [nsrc][nchan][1025][frames] (uint8,
 * nullable); irm != 0: Y_j = X * |Y_j|^alpha / (eps + sum_k |Y_k|^alpha), mask must be null.  nsrc, nchan in [1, 1024]. */
int glowk_oracle_mask(float* spec_dev, int nsrc, int nchan, int frames, int irm, double alpha, double theta, uint8_t* mask_dev,
                      void* stream);
/* the multichannel Wiener filter, stereo (nchan = 2), in place on the source rows, fp64: R_j(f) = mean_t Y Y^H / (eps + P_j),
 * normalised as the reference's np.trace of the [F, 2, 2] array does (column k of every R_j(f) times 2 / (R_j(0)[0][k] +
 * R_j(1)[1][k])), + eps I; P_j = Re tr(R_j^-1 Y Y^H) / 2; Y_j = P_j R_j (sum_k P_k R_k)^-1 X, 2 x 2 inverses with eps added to the
 * determinant.  nsrc in [1, 16]; the time means are fixed-order reductions (bitwise reproducible). */
int glowk_mwf(float* spec_dev, int nsrc, int frames, void* stream);
/* IBM_melspec (irm == 0) / IRM_melspec (irm != 0), elementwise: mix [n] (double), src [nsrc][n] and out [nsrc][n] in float
 * (src_f64 == 0) or double; the IRM's source sum in the sources' type, in source order; + eps, the ratio, the threshold and the
 * product in double; one rounding to the output type.  0 <= n <= 2^40. */
int glowk_oracle_mel(const double* mix_dev, const void* src_dev, int nsrc, int64_t n, int src_f64, int irm, double theta, void* out_dev,
                     void* stream);

/* --- stereo separation: the multichannel Wiener filter with EM-fitted spatial covariances (Duong, Vincent, Gribonval 2010) --- */
/* Handle-free, in the front end's STFT convention (hop 512, [.., 1025, T], frame fastest, complex re/im interleaved), batched over
 * nprob problems (extracts).  A problem has the stereo mixture STFT x(f,t) in C^2, nsrc source PSDs v_j(f,t) >= 0 and the 2 x 2
 * Hermitian spatial covariances R_j(f), R_j = I at the start.  With eps = 1e-10, one iteration (the old v, R on every right-hand
 * side):
 *   Cx = sum_k v_k R_k + eps I,  W_j = v_j R_j Cx^-1,  y_j = W_j x,  C_j = y_j y_j^H + (I - W_j) v_j R_j,
 *   v_j' = max(0, Re tr(R_j^-1 C_j) / 2),  R_j'(f) = (1/T) sum_t C_j / (v_j' + eps) + eps I,
 * and after n_iter iterations Y_j = v_j R_j Cx^-1 x with the final v, R; n_iter = 0 is v_j / (sum_k v_k + eps) x per channel, the
 * single-channel Wiener mask of glowk_masked_istft on each channel.  (Unlike glowk_mwf, the reference's oracle: no true source
 * spectra, no np.trace normalisation.)
 *   x [nprob][2][1025][T] complex, v [nsrc][nprob][1025][T] float (in: the PSDs; out: the fitted ones, untouched when n_iter = 0),
 *   y [nsrc][nprob][2][1025][T] complex, r (nullable) [nsrc][nprob][1025][4] double = (r00, r11, Re r01, Im r01) of the final R_j(f).
 * One launch on `stream` for the whole call, all iterations included: one workgroup owns one (problem, bin) and runs the loop; no
 * host synchronisation, no atomics, no allocation.  fp64 arithmetic in registers, v held in fp32 between iterations; 2 x 2
 * determinants as det M + eps tr M + eps^2 with det M clamped at 0, so they stay >= 1e-20.  The time sums are added in one fixed
 * order that depends on T alone: bitwise reproducible, and a (problem, bin)'s results depend on nothing outside it.  nsrc in
 * [1, 16], nprob in [0, 2^20] (0 is a successful no-op), frames in [1, 2^20], n_iter in [0, 1000]; anything else is GLOWK_ERR;
 * a host pointer is refused.  v_dev is the only input written. */
int glowk_mwf_em(const float* x_dev, float* v_dev, int nsrc, int nprob, int frames, int n_iter, float* y_dev, double* r_dev,
                 void* stream);

/* --- whole-signal separation: mel frames of a signal of any length, overlapping tiles out and back --------------------------- */
/* Handle-free, the project's own (the reference only cuts disjoint 2.04 s extracts): one STFT of the whole signal, overlapping
 * tiles of its dB frames for the priors, the separated tiles cross-faded back into frames.  The front end's constants are
 * compiled in (see the audio section).  Every tensor is float32 device memory on one device (a host pointer is refused); each
 * call enqueues on `stream`, synchronises nothing with the host and uses no atomics; every sum runs in a fixed order: bitwise
 * reproducible.  nsig in [0, 2^20], nsig == 0 is a successful no-op; anything outside the stated ranges is GLOWK_ERR.  Added to
 * version 480 without a new number: nothing that existed changed; a library without them lacks the symbols.
 */
/* audio [nsig][n_samples] 16 kHz -> mel_db [nsig][96][F], F = 1 + n_samples / 512, and (nullable) the complex STFT stft
 * [nsig][1025][F]: glowk_mel_frontend's convention (center, reflect padding, periodic Hann, |X|^2, Slaney mel,
 * 10 log10(max(1e-10, .)), clip to [-100, 20]) and arithmetic, without its per-extract top_db floor and without its bound on F.
 * n_samples: a multiple of 512 in [1536, (2^20 - 1) * 512].  Two launches; without stft_dev the call takes an [nsig][1025][F]
 * float scratch from the stream-ordered allocator for |X|^2. */
int glowk_mel_frames(const float* audio_dev, int nsig, int64_t n_samples, float* mel_db_dev, float* stft_dev, void* stream);
/* frames [nsig][96][F] (dB) -> tiles [nsig][N][96][width], N = 1 if F <= width, else 1 + ceil((F - width) / hop): tile k holds
 * frames [k hop, k hop + width), -100 dB (silence) at and beyond F.  top_db > 0: each cell becomes max(cell, tile_max - top_db),
 * the maximum taken over the padded tile (glowk_mel_frontend's floor, per tile); then every cell is clipped to [-100, 20].
 * width in [2, 128], hop in [1, width], frames = F in [1, 2^20], top_db finite.  One launch, one workgroup per tile. */
int glowk_tile_cut(const float* frames_dev, int nsig, int frames, int width, int hop, float top_db, float* tiles_dev, void* stream);
/* tiles [nsig][N][96][width] -> frames [nsig][96][F], F <= (N - 1) hop + width: the weighted mean, in dB, of the tiles that
 * cover a frame,  out[f] = sum_k w[f - k hop] t_k[f - k hop] / sum_k w[f - k hop],  w[j] = sin^2(pi (j + 1/2) / width)
 * (strictly positive; w[j] + w[j + width / 2] = 1, so the denominator is 1 at hop = width / 2), built in fp64 and rounded once;
 * k ascends, fp32 fused multiply-adds.  A frame that exactly one tile covers is that tile's value, bit for bit.  The tiles are
 * not clipped (BASIS states may leave [-100, 20]).  width in [2, 128], hop in [1, width], N in [1, 2^20], frames = F in
 * [1, 2^20].  One launch, one thread per output cell, no allocation. */
int glowk_tile_stitch(const float* tiles_dev, int nsig, int N, int width, int hop, int frames, float* frames_dev, void* stream);

/* --- BASIS as one chain over a whole signal: the state is its frames, the priors see its overlapping tiles -------------------- */
/* The project's own (glowk_tile_stitch above cross-fades finished estimates of chains that never hear of each other; here the
 * tiles are coupled inside the Langevin loop).  For source k the state is x_k [rows][F]; tile t of it, c_t(x_k), holds frames
 * [t hop, t hop + width) and `pad` at and beyond F, t = 0 .. N - 1, N = 1 if F <= width, else 1 + ceil((F - width) / hop).  The
 * prior score of a frame is the mean of the scores the tiles that cover it give it, weighted by glowk_tile_stitch's window,
 *     s_k[b][f] = sum_t w[f - t hop] grad log p_k(c_t(x_k))[b][f - t hop] / sum_t w[f - t hop],   w[j] = sin^2(pi (j + 1/2) / width),
 * over the t with 0 <= f - t hop < width: glowk_tile_stitch's arithmetic on gradient tiles (the same table, t ascending, fp32
 * fused multiply-adds; a frame under exactly one tile takes that tile's gradient, bit for bit).  The weights of a frame sum to
 * one, so the prior pulls on every frame as hard as in a per-tile chain; at hop = width this is the per-tile chain.  Gradients
 * with respect to pad cells are dropped.  Every tensor is float32 device memory on one device (a host pointer is refused); each
 * call is one launch on `stream`, synchronises nothing with the host, uses no atomics and no allocation, and sums in a fixed
 * order: bitwise reproducible.  rows in [1, 65536], frames = F in [1, 2^20], width in [2, 128], hop in [1, width], pad finite;
 * anything else is GLOWK_ERR before anything is launched.  Added to version 480 without a new number: nothing that existed
 * changed; a library without them lacks the symbols. */
/* x [nsig][rows][F] -> tiles [nsig][N][rows][width]: a raw gather, `pad` at and beyond F, no floor and no clip (BASIS states
 * leave [-100, 20]; glowk_tile_cut is the front end's cut, with both).  The first tiles of a noise level.  nsig in [0, 2^20],
 * nsig == 0 is a successful no-op; the tiles must not overlap x. */
int glowk_frames_to_tiles(const float* x_dev, int nsig, int rows, int frames, int width, int hop, float pad, float* tiles_dev,
                          void* stream);
/* One Langevin step of all nsrc sources on the frames, in place, as ONE kernel:
 *     x_k <- x_k + eta (s_k + lambda_recon m_k (mixed - mix)) + sqrt(2 eta) N(0, I)              for k = 0 .. nsrc - 1
 * with mix, m_k and every rounding of glowk_basis_update_n (the device code is shared) and s_k stitched from the gradient tiles
 * as above.  x_dev: [nsrc][rows][F].  g: HOST array of nsrc DEVICE pointers, each [N][rows][width], the gradient of prior k at
 * the tiles of x_k (glowk_log_prob_grad's output as it is).  mixed: [rows][F].  eps: NULL, or a HOST array of nsrc entries, each
 * NULL or [rows][F] standard-normal draws; a source without draws takes the device RNG's, stream k & 1 of pair k >> 1 at
 * (seed, step): element e = b F + f of the frame layout takes element e of that stream (glowk_random_source at offset 0).
 * tiles_out (nullable): [nsrc][N][rows][width], receives the tiles of the updated states for the next step's gradient calls --
 * every cell of it is written, the pad cells with `pad` -- so a step is nsrc gradient evaluations and this launch.
 * nonfinite_dev as for glowk_basis_update: set to 1 on a non-finite stitched gradient, mixture or result.  nsrc in [2, 16],
 * step < 2^48, eta >= 0, mixing: enum glowk_mixing; x, mixed, the gradient tiles, the noise and tiles_out must not overlap
 * (gradient and noise tensors are only read and may repeat).  A thread moves four consecutive elements of the frame layout
 * (one Philox call per source), as 16-byte accesses of x, mixed and eps when rows F is a multiple of 4 and they are 16-byte
 * aligned; the tiles are read and written cell by cell, neighbouring threads at neighbouring frames. */
int glowk_basis_update_frames(float* x_dev, const float* const* g, const float* const* eps, int nsrc, const float* mixed_dev, int rows,
                              int frames, int width, int hop, int mixing, float eta, float lambda_recon, uint64_t seed, uint64_t step,
                              float pad, float* tiles_out_dev, int* nonfinite_dev, void* stream);

/* --- harmonic / percussive separation by median filtering (Fitzgerald 2010; librosa.decompose.hpss) ------------------------- */
/* Handle-free, the prior-free baseline: no trained flows, no true sources.  s [nsig][rows][frames] float32, frames contiguous --
 * |STFT| with rows = 1025 or the 96 mel rows; no geometry is compiled in.  Every tensor is float32 device memory on one device (a
 * host pointer is refused); each call is one launch on `stream`, with no atomics, no allocation and no host synchronisation:
 * bitwise reproducible.  Anything outside the stated ranges is GLOWK_ERR with a glowk_last_error message before anything is
 * launched.  Inputs are finite; what a NaN does is unspecified.  audiosourcesep_amd/hpss.py drives the calls.  Since version 500.
 */
/* The running median of odd length `size` along the frame axis (axis = 0: the harmonic filter) or the row axis (axis = 1: the
 * percussive filter), out [nsig][rows][frames].  Edges as scipy.ndimage.median_filter(mode='reflect'), the half-sample symmetric
 * extension d c b a | a b c d | d c b a: sample j of an axis of length n (j in [-size / 2, n + size / 2), so j may be negative)
 * reads index r = j mod 2 n (mathematical mod), then r if r < n, else 2 n - 1 - r; right for windows many times longer than the
 * axis.  The output is the window element v with #(w < v) <= size / 2 < #(w <= v): a selection by compares, no arithmetic on the
 * values, so ties, runs of equal values and zeros give the same bits as sorting the window (of elements that compare equal but
 * differ in bits, -0 and +0, the first in window order).  A (signal, row) or (signal, frame) line depends on nothing outside its
 * signal: a batch gives what its signals give alone.  nsig in [0, 65535] (0 is a successful no-op), rows in [1, 4096], frames in
 * [1, 2^20], nsig * rows * frames <= 2^31 - 1, size odd in [1, 127] (1 is the identity), axis in {0, 1}, out_dev != s_dev (the two
 * must not overlap). */
int glowk_median_filter(const float* s_dev, int nsig, int rows, int frames, int size, int axis, float* out_dev, void* stream);
/* The two soft masks of librosa.util.softmask from the two filtered spectra, elementwise over n floats, in fp32.  For (X, R):
 *   Z = max(X, R), bad = Z < FLT_MIN (1.17549435e-38), Z = 1 where bad; m = (X / Z)^power, r = (R / Z)^power; mask = m / (m + r),
 *   and where bad mask = 0.5 if both margins are exactly 1 (split_zeros), else 0;  power = +inf: the hard mask X > R (1.0 / 0.0).
 * out_h uses X = harm, R = perc * margin_h; out_p uses X = perc, R = harm * margin_p.  With a non-null s the outputs are s * mask
 * instead of the masks (one more fp32 product).  power > 0 (+inf allowed, NaN not), both margins finite and >= 1, n <= 2^40 (0 is
 * a successful no-op); the two outputs must not overlap each other. */
int glowk_hpss_mask(const float* harm_dev, const float* perc_dev, const float* s_dev, size_t n, float power, float margin_h,
                    float margin_p, float* out_h_dev, float* out_p_dev, void* stream);

/* --- REPET-SIM: nearest-neighbour median filtering (Rafii & Pardo 2012; librosa.decompose.nn_filter) ------------------------- */
/* Handle-free, the prior-free baseline for a foreground over a repeating accompaniment: every frame is replaced by the per-row
 * median of its most similar frames elsewhere in the signal; what repeats survives.  s [nsig][rows][frames] float32, frames
 * contiguous, real and non-negative.  Every tensor is device memory on one device (a host pointer is refused); the calls launch on
 * `stream` with no atomics, no allocation and no host synchronisation, the number of launches depends on the shapes alone, and
 * the results are bitwise reproducible; a batch gives what its signals give alone.  Anything outside the stated ranges is
 * GLOWK_ERR with a glowk_last_error message before anything is launched.  Inputs are finite.  Ranges of all three: nsig in
 * [0, 65535] (0 is a successful no-op of valid arguments), rows in [1, 4096], frames in [1, 32768], k in [1, 512], nsig * rows *
 * frames and nsig * frames * k at most 2^31 - 1.  audiosourcesep_amd/repet.py drives the calls; the two masks of REPET-SIM are
 * glowk_hpss_mask(harm = min(s, filt), perc = s - min(s, filt)).  Since version 520. */
/* The bytes of work_dev that glowk_nn_neighbors and glowk_nn_median need for these shapes: the frame norms and a frame-major copy
 * of s, 4 nsig frames (rows + 1) rounded up to a multiple of 8 (as every size query here is) -- linear in frames; there is no
 * frames x frames matrix anywhere.  0 for arguments out of range. */
size_t glowk_nn_workspace_bytes(int nsig, int rows, int frames, int k);
/* The neighbours of every frame.  sim(i, j) = <s[:, i], s[:, j]> / max(|s[:, i]| |s[:, j]|, FLT_MIN), so a silent frame has
 * similarity 0 to everything; the dot product is an fp32 fma chain over the rows in row order on the fp32 matrix cores, the same
 * bits for (i, j) and (j, i).  The candidates of frame i are the frames j with |i - j| >= width; with k_i = min(k, #candidates),
 * idx[i][:k_i] holds the k_i candidates of largest similarity in decreasing similarity, equal similarities to the lower index,
 * and idx[i][k_i:] = -1 (librosa's recurrence_matrix rule: the k + 2 width nearest, the band removed, the top k kept).  sim_dev
 * (nullable) receives the similarities, 0 where idx is -1.  width in [1, 2^20]; work_bytes at least glowk_nn_workspace_bytes;
 * s, idx, sim and work must not overlap.  Two launches. */
int glowk_nn_neighbors(const float* s_dev, int nsig, int rows, int frames, int k, int width,
                       int32_t* idx_dev /* [nsig][frames][k] */, float* sim_dev /* same shape, may be null; 0 where idx is -1 */,
                       void* work_dev, size_t work_bytes, void* stream);
/* The filter: out[r][i] = the median over the neighbours j = idx[i][t] of s[r][j], gathered from a frame-major copy of s in
 * work_dev.  The neighbours of a frame are its entries in [0, frames); any other entry (-1, or a caller's error) is skipped and
 * never read through.  With n of them: n odd, the middle element -- a selection by compares, the bits a sort gives; n even,
 * (a + b) * 0.5f of the two middle elements in fp32, the only arithmetic on the values; n = 0, out[r][i] = s[r][i].  out_dev must
 * not overlap s_dev; work_bytes at least glowk_nn_workspace_bytes.  Two launches. */
int glowk_nn_median(const float* s_dev, const int32_t* idx_dev, int nsig, int rows, int frames, int k,
                    float* out_dev /* [nsig][rows][frames], not s_dev */, void* work_dev, size_t work_bytes, void* stream);

/* --- REPET and adaptive REPET: beat spectrum, period, periodic neighbours (Rafii & Pardo 2013; Liutkus et al. 2012) ----------- */
/* The front end of the original REPET: the repeating period from the beat spectrum (or one period per window from the beat
 * spectrogram), and per frame the list of the frames whole periods away, which glowk_nn_median then filters over -- the segment
 * median of REPET with a long list, the adaptive REPET's filter of a given order with a short one; the ratio mask of the
 * publication is glowk_hpss_mask(harm = min(s, filt), perc = s - min(s, filt), power = 1, both margins 1).  The conventions are
 * those of the REPET-SIM section: handle-free, every tensor device memory on one device (a host pointer is refused), launches on
 * `stream` with no atomics, no allocation and no host synchronisation, a launch count that depends on the shapes alone, bitwise
 * reproducible results, a batch gives what its signals give alone.  Anything outside the stated ranges is GLOWK_ERR with a
 * glowk_last_error message before anything is launched; nsig = 0 (nseg = 0) is a successful no-op of otherwise valid arguments.
 * Inputs are finite.  audiosourcesep_amd/repet.py drives the calls.  Since version 530. */
/* The bytes of work_dev that glowk_beat_spectrum needs: 768 nsig nwin nu nch, the fp64 partial sums of 96 lags per workgroup, with
 * nwin as below, nmax = frames (win = 0) or win, nu = (min(nlags, nmax) + 30) / 64 + 1, units = sum over u < nu of
 * ceil(max(nmax - 64 u, 0) / 32), tpw = min(16, max(1, ceil(units / 4096))), nch = ceil(ceil(nmax / 32) / (4 tpw)) (integer
 * divisions) -- about 12 nlags nmax / tpw bytes per window against the 4 nmax^2 of a Gram matrix, which exists nowhere.  0 for
 * arguments out of range (and for nsig = 0). */
size_t glowk_beat_workspace_bytes(int nsig, int rows, int frames, int nlags, int win, int step);
/* The beat spectrum (win = 0: one window, the whole signal, nwin = 1) or the beat spectrogram (win in [2, frames], step in
 * [1, win], nwin = ceil(frames / step); window t covers the frames [t step - win / 2, t step - win / 2 + win) that lie in
 * [0, frames), n_t >= 1 of them from frame a on).  With P = s * s in fp32, for l < n_t
 *   acf[l] = sum_r sum_{j = a .. a + n_t - 1 - l} P[r][j] P[r][j + l],   raw[l] = acf[l] / (rows (n_t - l)),
 *   beat[t][l] = raw[l] / raw[0]
 * (both frames of a pair inside the window), beat[t][l] = 0 for l >= n_t, and all zeros where raw[0] = 0.  sum_r P[r][i] P[r][j]
 * is one element of the frame Gram matrix of P: an fp32 fma chain over the rows in row order on the fp32 matrix cores, as in
 * glowk_nn_neighbors, and only the band 0 <= j - i < nlags of the upper triangle is computed.  Everything after it -- the sums
 * along the diagonals, across tiles and workgroups in a fixed order, the divisions -- is fp64, rounded to float32 once.  Every term
 * is non-negative, so the error is relative per lag: at most 2 (rows + 2) 2^-24 of the value.  nlags in [1, frames]; beside the
 * ranges of glowk_nn_* (nsig in [0, 65535], rows in [1, 4096], frames in [1, 32768], nsig * rows * frames <= 2^31 - 1)
 * nsig * nwin * nlags and the workgroup count nsig * nwin * nu * nch are at most 2^31 - 1.  work_bytes at least
 * glowk_beat_workspace_bytes, work_dev aligned to 8 bytes; s, beat and work must not overlap.  Nothing is read outside s.  Two
 * launches. */
int glowk_beat_spectrum(const float* s_dev, int nsig, int rows, int frames, int nlags, int win, int step,
                        float* beat_dev /* [nsig][nwin][nlags] */, void* work_dev, size_t work_bytes, void* stream);
/* period[g] = the lag in [pmin, pmax] of largest beat[g][lag] for each of the nseg segments of nlags values, equal values to the
 * lower lag (all zeros give pmin): the maximum of one key, the value's bits as an ordered integer above and ~lag below.
 * 1 <= pmin <= pmax <= nlags - 1, nlags <= 32768, nseg * nlags <= 2^31 - 1.  One launch. */
int glowk_beat_period(const float* beat_dev /* [nseg][nlags] */, int nseg, int nlags, int pmin, int pmax,
                      int32_t* period_dev /* [nseg] */, void* stream);
/* The periodic neighbours.  Frame j uses p = max(1, period[sig][min((j + step / 2) / step, nper - 1)]) (integer division; nper = 1
 * for one period per signal), and idx[j] lists the frames j + i p for i = 0, -1, +1, -2, +2, .. in that order: those in
 * [0, frames) are kept until k are kept, the remaining entries are -1.  With k >= ceil(frames / p) that is every frame congruent
 * to j mod p (REPET's segment median, since a median ignores the order); with a small k the k nearest repetitions (the adaptive
 * REPET's filter order).  nsig in [0, 65535], frames, nper and step in [1, 32768], k in [1, 512], nsig * frames * k <= 2^31 - 1;
 * period and idx must not overlap.  One launch. */
int glowk_period_neighbors(const int32_t* period_dev /* [nsig][nper] */, int nsig, int frames, int nper, int step, int k,
                           int32_t* idx_dev /* [nsig][frames][k] */, void* stream);

/* --- 2DFT separation: real 2-D DFT and inverse, plane std, peak mask (Seetharaman, Pishdadian & Pardo 2017) ------------------ */
/* Repetition as peaks of the 2-D Fourier transform of the magnitude spectrogram: no period, no window.  With R = rows,
 * T = frames, fc = T / 2 + 1: F = rfft2(s) (numpy's layout, [R][fc]), mag the full Hermitian plane of |F|, std its population
 * standard deviation, M the peaks of mag (below), B = irfft2(F M) the background, |s - B| the foreground's model, and the masks
 * are glowk_hpss_mask(harm = |B|, perc = |s - B|).  The conventions are those of the REPET sections: handle-free, every tensor
 * device memory on one device (a host pointer is refused), launches on `stream` with no atomics, no allocation and no host
 * synchronisation, a launch count that depends on the shapes (and on which optional tensors are given) alone, bitwise
 * reproducible results, a batch gives what its signals give alone.  Anything outside the stated ranges is GLOWK_ERR with a
 * glowk_last_error message before anything is launched; nsig = 0 is a successful no-op of otherwise valid arguments.  Ranges:
 * nsig in [0, 65535], rows in [1, 4096], frames (cols) in [1, 32768], nsig * rows * frames <= 2^31 - 1.  Inputs are finite.
 * audiosourcesep_amd/ft2d.py drives the calls.  Since version 540. */
/* The bytes of work_dev of both transforms: 8 (frames + rows + nsig rows fc) -- the two tables (cos, sin)(2 pi m / N), evaluated in
 * fp64 and rounded once, and the [nsig][rows][fc] complex plane between the two stages.  0 out of range and for nsig = 0. */
size_t glowk_dft2_workspace_bytes(int nsig, int rows, int frames);
/* spec[u][v] = sum_r sum_t s[r][t] exp(-2 pi i (u r / R + v t / T)), u in [0, R), v in [0, fc): two GEMMs on the fp32 matrix
 * cores, along frames (an fp32 fma chain of T terms in t order per component) then along rows (a chain of 2 R terms in r order),
 * the twiddles from the tables at the exact integer index (v t) mod T.  Per component |error| <= (2 R + 2 T + 8) 2^-24 sum |s| of
 * the signal.  mag_dev (nullable) receives the full plane: (float) sqrt((double) re re + (double) im im) for v < fc, and the
 * bitwise copies mag[u][v] = mag[(R - u) % R][(T - v) % T] for v >= fc and, inside the self-conjugate columns (v = 0, and v = T / 2
 * for even T), for the rows 2 u > R -- so the plane is Hermitian in its bits everywhere.  spec and work aligned to 8 bytes; s,
 * spec, mag and work must not overlap.  Nothing is read outside s.  Four launches, five with mag_dev. */
int glowk_rdft2(const float* s_dev, int nsig, int rows, int frames, float* spec_dev /* [nsig][rows][fc] interleaved complex64 */,
                float* mag_dev /* [nsig][rows][frames], may be null */, void* work_dev, size_t work_bytes, void* stream);
/* out = numpy.fft.irfft2(spec * mask[:, :fc], s = (R, T)): the complex inverse along rows, then complex-to-real along frames, where
 * the imaginary parts of column 0 and (T even) column T / 2 are dropped.  mask_dev (nullable: all ones) is a full plane of which
 * only the columns < fc are read, multiplied in as spec is loaded (one fp32 product; exact for a 0 / 1 mask); the masked spectrum
 * is never written.  The scaling 1 / (R T) and the column weights 1 or 2 are folded into the last stage.  Per element
 * |error| <= (2 R + 2 T + 8) 2^-24 sum |F| / (R T) over the full Hermitian plane.  out must not overlap spec, mask or work.  Four
 * launches. */
int glowk_irdft2(const float* spec_dev, const float* mask_dev /* [nsig][rows][frames], may be null */, int nsig, int rows, int frames,
                 float* out_dev /* [nsig][rows][frames] */, void* work_dev, size_t work_bytes, void* stream);
/* out[sig] = (mean, population standard deviation) of the n floats of plane[sig], in fp64: per-workgroup partial sums in
 * work_dev added in index order, two passes (the sum, then the squared deviations from the mean).  The workgroups per signal
 * depend on n alone.  n in [1, 2^31 - 1], nsig * n <= 2^31 - 1; work_bytes at least glowk_plane_std_workspace_bytes (16 nsig
 * min(256, ceil(n / 4096)); 0 out of range); out and work aligned to 8 bytes.  Three launches. */
size_t glowk_plane_std_workspace_bytes(int nsig, int64_t n);
int glowk_plane_std(const float* plane_dev /* [nsig][n] */, int nsig, int64_t n, double* out_dev /* [nsig][2] */, void* work_dev,
                    size_t work_bytes, void* stream);
/* The peak rule.  mx and mn are the largest and smallest value of the periodic nb_r x nb_c neighbourhood of (u, v) (both sizes odd
 * in [1, 127]; indices wrap modulo rows and cols, as often as a long neighbourhood needs: scipy.ndimage.maximum_filter /
 * minimum_filter(size = (nb_r, nb_c), mode = 'wrap')); mask = 1.0f where plane == mx and (mx - mn) > thr[sig] (one fp32
 * subtraction, strict), else 0.0f; with thr_dev null there is no threshold test.  Compares select and nothing else computes, so
 * max_dev / min_dev (nullable) carry input elements' bits; which of -0 and +0 is returned is unspecified.  A separable running
 * max / min: along the columns into work_dev (glowk_peak_workspace_bytes = 8 nsig rows cols), then along the rows.  The tensors
 * must not overlap.  Two launches. */
size_t glowk_peak_workspace_bytes(int nsig, int rows, int cols);
int glowk_peak_mask(const float* plane_dev, int nsig, int rows, int cols, int nb_r, int nb_c, const float* thr_dev /* [nsig], may be null */,
                    float* mask_dev, float* max_dev /* may be null */, float* min_dev /* may be null */, void* work_dev, size_t work_bytes,
                    void* stream);

/* --- DUET: blind separation of a two-channel STFT from its attenuation-delay histogram (glowk_duet.h) ------------------------------
 * Handle-free; every call enqueues on `stream`, synchronises with nothing, refuses host pointers and overlapping buffers before it
 * launches anything, and returns GLOWK_OK at once for nsig == 0.  x: [nsig][2][rows][frames] complex64 (re, im interleaved), the
 * STFT of two channels; rows in [1, 4096], frames in [1, 32768], nsig * 2 * rows * frames <= 2^31 - 1.  n_fft = 2 (rows - 1),
 * omega_r = 2 pi r / n_fft.  All arithmetic after the load is fp64.
 *
 * Features, rows r >= 1, m1 = |X1|, m2 = |X2|: a cell with m1 == 0 or m2 == 0, and every cell of row 0, has alpha = delta = w = 0;
 * otherwise alpha = (m2^2 - m1^2) / (m1 m2) (the symmetric attenuation a - 1/a), delta = -arg(X2 conj X1) / omega_r (samples),
 * w = (m1 m2)^p omega_r^q (p == 1 and q == 0 skip their pow). */
int glowk_duet_features(const float* x_dev, int nsig, int rows, int frames, double p, double q, double* alpha_dev /* [nsig][rows][frames] */,
                        double* delta_dev, double* w_dev, void* stream);
/* The weighted histogram.  A cell counts when its weight is finite and > 0 and i = floor((alpha - a_lo) n_a / (a_hi - a_lo)),
 * j = floor((delta - d_lo) n_d / (d_hi - d_lo)) (fp64) satisfy 0 <= i < n_a, 0 <= j < n_d (half-open; a non-finite coordinate never
 * does).  wmax: the largest counted weight of the signal; e: wmax < 2^e <= 2 wmax; s = min(40, 62 - ceil_log2(max(cells, 2)) -
 * 4 smooth).  hist[sig][i][j] = the int64 sum of rint(w 2^(s - e)) over the cells counted there; es[sig] = (e, s), e = 0 and an
 * all-zero plane for a signal without a counted weight.  Integer sums: the same bits every run, and in a batch what the signal
 * gives alone.  n_a, n_d >= 1, n_a n_d <= 16384; finite ranges with lo < hi; smooth in [0, 3] is the number of smoothing passes
 * glowk_duet_peaks will make, for which s leaves headroom (every smoothed sum stays at or below 2^62).  work_bytes at least
 * glowk_duet_hist_workspace_bytes (0 out of range); 8-byte alignment.  A memset and two launches: the maximum, then the plane
 * (per-workgroup LDS planes of 64-bit cells, integer LDS adds, flushed with 64-bit integer global adds).
 * glowk_duet_histogram reads three fp64 planes of `cells` elements per signal (nsig * cells <= 2^31 - 1); glowk_duet_histogram_stft
 * reads x and computes the features in registers (cells = rows * frames): bit for bit the plane of glowk_duet_features followed by
 * glowk_duet_histogram. */
size_t glowk_duet_hist_workspace_bytes(int nsig, int64_t cells, int n_a, int n_d);
int glowk_duet_histogram(const double* alpha_dev, const double* delta_dev, const double* w_dev, int nsig, int64_t cells, double a_lo, double a_hi,
                         int n_a, double d_lo, double d_hi, int n_d, int smooth, int64_t* hist_dev /* [nsig][n_a][n_d] */,
                         int32_t* es_dev /* [nsig][2] */, void* work_dev, size_t work_bytes, void* stream);
int glowk_duet_histogram_stft(const float* x_dev, int nsig, int rows, int frames, double p, double q, double a_lo, double a_hi, int n_a, double d_lo,
                              double d_hi, int n_d, int smooth, int64_t* hist_dev, int32_t* es_dev, void* work_dev, size_t work_bytes, void* stream);
/* Peaks of non-negative int64 planes.  `smooth` passes of the separable binomial kernel [1 2 1] x [1 2 1] in int64, zero beyond the
 * edges, no division (the caller keeps 16^smooth times the plane's sum below 2^63); then num_sources (1..16) times: the largest
 * value among the cells not yet excluded, ties to the lowest row-major index; stop if it is <= 0; record the cell; exclude every
 * cell with |di| <= dist_a and |dj| <= dist_d.  peaks[sig][k] = (i, j), (-1, -1) from n_found[sig] on; smooth_dev (nullable) gets
 * the smoothed plane.  One workgroup per signal, one launch; work_bytes at least glowk_duet_peaks_workspace_bytes
 * (16 nsig n_a n_d). */
size_t glowk_duet_peaks_workspace_bytes(int nsig, int n_a, int n_d);
int glowk_duet_peaks(const int64_t* hist_dev, int nsig, int n_a, int n_d, int smooth, int num_sources, int dist_a, int dist_d,
                     int64_t* smooth_dev /* may be null */, int32_t* peaks_dev /* [nsig][num_sources][2] */, int32_t* nfound_dev /* [nsig] */,
                     void* work_dev, size_t work_bytes, void* stream);
/* Assignment, every row including 0.  Source j < n_found has alpha_j, delta_j = the centres lo + (i + 1/2)(hi - lo) / n of its
 * peak's bins and a_j = (alpha_j + sqrt(alpha_j^2 + 4)) / 2; J_j = |a_j e^{-i delta_j omega_r} X1 - X2|^2 / (1 + a_j^2) in fp64,
 * the rotation and 1 / (1 + a_j^2) read from a table per (signal, source, row) that the first launch fills in work_dev
 * (glowk_duet_assign_workspace_bytes = 32 nsig num_sources rows).  mask[sig][j] = 1.0f where j is the lowest found index that
 * attains the minimum, else 0.0f (all 0 when n_found == 0); spec[sig][j][ch] = X_ch where the mask is 1, +0 elsewhere.  Two
 * launches. */
size_t glowk_duet_assign_workspace_bytes(int nsig, int rows, int num_sources);
int glowk_duet_assign(const float* x_dev, int nsig, int rows, int frames, const int32_t* peaks_dev, const int32_t* nfound_dev, int num_sources,
                      double a_lo, double a_hi, int n_a, double d_lo, double d_hi, int n_d, float* mask_dev /* [nsig][S][rows][frames] */,
                      float* spec_dev /* [nsig][S][2][rows][frames] complex64 */, void* work_dev, size_t work_bytes, void* stream);

/* --- NMF: multiplicative updates for the beta divergences, ratio masks of component ranges (Lee & Seung 2001; Fevotte & Idier 2011) -- */
/* V [nsig][rows][frames] float32, finite and >= 0, frames contiguous; W [nw][rows][K], K contiguous, nw = nsig or 1 (one dictionary
 * shared by every signal, allowed only where W is not updated); H [nsig][K][frames]; W and H float32, finite and >= 0.
 * FLOOR = 2^-40.  beta = 0 (Itakura-Saito), 1 (Kullback-Leibler) or 2 (Euclidean); there is no general power.
 *   L = W H, an fp32 fma chain over K (padded with exact zeros) on v_mfma_f32_32x32x2_f32;  Le = max(L, FLOOR);
 *   beta 2: Q = V, P = Le;   beta 1: Q = V / Le, P = 1;   beta 0: Q = V / (Le Le), P = 1 / Le;
 *   H update: H' = H g(W^T Q / max(W^T P, FLOOR));   W update: W' = W g(Q H^T / max(P H^T, FLOOR));
 *   g(x) = sqrt(x) for beta 0, x otherwise (the majorise-minimise exponent 1 / (2 - beta) of scikit-learn: no update increases D).
 * The outer sums (over the rows for H, over the frames for W) are fp32 fma chains on the same instruction, in an order that the
 * shapes fix; the division, the square root and the last product are one fp32 operation each.  Every term is non-negative, so the
 * error of one update is relative per element: at most (3 K + 2 n + 16) 2^-24 of the value, n = rows for H and frames for W, and an
 * exact 0 where the exact result is 0.  L, Q and P exist in registers alone.  The conventions are those of the REPET section:
 * handle-free, every tensor device memory on one device (a host pointer is refused), launches on `stream` with no atomics, no
 * allocation and no host synchronisation, a launch count that depends on the shapes and n_iter alone, bitwise reproducible
 * results, a batch gives what its signals give alone.  nsig in [0, 65535] (0: a successful no-op), rows in [1, 4096], frames in
 * [1, 32768], K in [1, 128], every tensor at most 2^31 - 1 elements; anything else is GLOWK_ERR with a glowk_last_error message
 * before anything is launched.  audiosourcesep_amd/nmf.py drives the calls.  Since version 550. */
/* The bytes of work_dev that glowk_nmf_fit and glowk_nmf_divergence need.  With rtiles = ceil(rows / 32), ftiles =
 * ceil(frames / 32), want = min(max(1, 256 / rtiles), max(1, ftiles / 4)) (integer divisions), tpc = ceil(ftiles / want), nch = ceil(ftiles / tpc)
 * (the frames are cut into nch chunks of 32 tpc; a function of rows and frames alone, never of nsig):
 * nsig max(8 nch rows K, 8 rtiles nch).  0 for arguments out of range (and for nsig = 0). */
size_t glowk_nmf_workspace_bytes(int nsig, int rows, int frames, int K);
/* n_iter iterations in place.  update_w = 1: the W update (with the old H), then the H update (with the new W), scikit-learn's
 * order; 0: H alone moves (W may be shared, nw = 1); 2: W alone moves.  n_iter in [0, 100000]; 0 is a successful no-op.  The W
 * update writes partial numerators and denominators per chunk of frames to work_dev and a second launch adds them in chunk order:
 * 3 n_iter launches with update_w = 1, 2 n_iter with 2, n_iter with 0 (then work_dev may be null).  V, W, H and work must not
 * overlap; work_dev aligned to 8 bytes. */
int glowk_nmf_fit(const float* v_dev, int nsig, int rows, int frames, float* w_dev, int nw, float* h_dev, int K, int beta, int n_iter,
                  int update_w, void* work_dev, size_t work_bytes, void* stream);
/* out[sig] = D_beta(V | W H), float64: the terms in fp64 from the fp32 Le, added in an order the shapes fix.
 *   beta 2: (V - Le)^2 / 2;   beta 1: V ln(V / Le) - V + Le with 0 ln 0 = 0;   beta 0: q - ln q - 1, q = max(V, FLOOR) / Le.
 * At most (K + 4) 2^-24 sum(w) from the exact value, w = (V + L)^2, V + L, q + 1.  Two launches. */
int glowk_nmf_divergence(const float* v_dev, int nsig, int rows, int frames, const float* w_dev, int nw, const float* h_dev, int K, int beta,
                         double* out_dev /* [nsig] */, void* work_dev, size_t work_bytes, void* stream);
/* Ratio masks of num_sources <= 16 sources that own the component ranges [bounds[s], bounds[s + 1]), bounds_host[0] = 0 < .. <
 * bounds_host[num_sources] = K (host memory, read before the call returns): L_s = the fp32 chain over the range of source s,
 * m_s = L_s^power (power 1 or 2), mask_s = m_s / sum_s m_s (the sum in source order), and 1 / num_sources where the sum is below
 * FLOOR.  With x_dev, a complex64 spectrum of `channels` in {1, 2} planes per signal, also spec[sig][s][ch] = mask_s X_ch (one fp32
 * product per component); x_dev and spec_dev are both given or both null (then channels is ignored).  nsig * S * C * rows *
 * frames <= 2^31 - 1.  The outputs must not overlap the inputs or each other.  One launch. */
int glowk_nmf_masks(const float* w_dev, int nw, const float* h_dev, int nsig, int rows, int frames, int K, const int32_t* bounds_host,
                    int num_sources, int power, const float* x_dev /* [nsig][C][rows][frames] complex64, or null */, int channels,
                    float* mask_dev /* [nsig][S][rows][frames] */, float* spec_dev /* [nsig][S][C][rows][frames] complex64, or null */,
                    void* stream);

/* --- AuxIVA and ILRMA: blind separation of M channels by one demixing matrix per row (Ono 2011; Kitamura et al. 2016; glowk_iva.h) -- */
/* X [nsig][M][rows][frames] complex64 (re, im interleaved), the STFT of M channels; W [nsig][rows][M][M] complex128, row k of W_f is
 * w_{k,f}^H; y_k(f, t) = sum_m W_f[k][m] X[m][f][t], m ascending.  M in [2, 4], frames in [M, 32768] (fewer frames than channels make
 * every weighted covariance rank-deficient), rows in [1, 4096], nsig in [0, 65535] (0: a successful no-op), nsig M rows frames <=
 * 2^31 - 1.  FLOOR = 2^-40.  Everything after the load of X is fp64 without contraction; every sum has an order that the shapes fix
 * (the rows in at most 32 blocks of ceil(rows / min(ceil(rows / 32), 32)) rows, block after block; the frames t = i, i + 256, .. per
 * thread i, the 64 lanes of a wave by halving, the four waves in order; the sums behind r_k(t) and lambda_k Neumaier-compensated per
 * thread); no atomics, no allocation, no host synchronisation: bitwise
 * reproducible, and a batch gives what its signals give alone.  The conventions are those of the NMF section: handle-free, device
 * memory on one device, GLOWK_ERR with a glowk_last_error message before anything is launched; tensors the call writes must not
 * overlap its other tensors; 8-byte alignment (float32 tensors 4).  audiosourcesep_amd/iva.py drives the calls.  Since version 552.
 *
 * Weights (model 0 = laplace, 1 = gauss): r_k(t) = sum_f |y_k(f, t)|^2; phi_k(t) = 1 / max(sqrt(r_k(t)), FLOOR) for laplace and
 * 1 / max(r_k(t) / rows, FLOOR) for gauss.  ILRMA's weights are phi_k(f, t) = 1 / max(rho_k(f, t), FLOOR), rho_k(f, t) = sum_l
 * basis[k][f][l] act[k][l][t] in fp64 from the float32 factors, l ascending.
 * Covariances: V_k(f) = (1 / frames) sum_t phi_k x(f, t) x(f, t)^H, Hermitian, stored as full matrices [nsig][rows][M(k)][M][M].
 * Iterative projection, per row, k = 0 .. M - 1 in order with rows < k already replaced: u = (W_f V_k(f))^-1 e_k by Gaussian
 * elimination with partial pivoting, d = Re(u^H V_k(f) u); where every component of u and d is finite and d > 0, row k of W_f becomes
 * (u / sqrt(d))^H, else it stays.  All V_k of one iteration come from the weights at the iteration's start.
 * Error of one iteration fed the same W, per row: max |dW_f| <= 2^-53 (frames + 64 M) (1 + c_f) max |W_f|, c_f the largest 2-norm
 * condition number of W_f V_k(f) over k (the frame sum, then the M x M solve). */
/* work_dev of glowk_iva_weights, glowk_auxiva_fit and glowk_iva_normalize: 8 (nsig nrb M frames + nsig M frames + nsig M) bytes, nrb the
 * number of row blocks above.  0 for arguments out of range. */
size_t glowk_iva_workspace_bytes(int nsig, int M, int rows, int frames);
/* phi [nsig][M][frames] float64 from X and W.  Two launches: the partial norms per row block, then their sum and the model. */
int glowk_iva_weights(const float* x_dev, const double* w_dev, int nsig, int M, int rows, int frames, int model, double* phi_dev, void* work_dev,
                      size_t work_bytes, void* stream);
/* V [nsig][rows][M][M][M] complex128 from X and either phi_dev [nsig][M][frames] (basis_dev and act_dev null, K ignored) or the factors
 * basis_dev [nsig][M][rows][K] and act_dev [nsig][M][K][frames], float32, K in [1, 128] (phi_dev null).  One launch, one workgroup
 * per row. */
int glowk_iva_covariances(const float* x_dev, int nsig, int M, int rows, int frames, const double* phi_dev, const float* basis_dev,
                          const float* act_dev, int K, double* v_dev, void* stream);
/* The M sequential row updates of every W_f, in place, from stored covariances.  One launch. */
int glowk_iva_ip_update(double* w_dev, const double* v_dev, int nsig, int M, int rows, void* stream);
/* n_iter AuxIVA iterations in place on W: weights, covariances and iterative projection, the covariances never stored.  Three launches
 * per iteration; n_iter in [0, 100000].  Bit for bit n_iter times glowk_iva_weights, glowk_iva_covariances, glowk_iva_ip_update. */
int glowk_auxiva_fit(const float* x_dev, double* w_dev, int nsig, int M, int rows, int frames, int model, int n_iter, void* work_dev,
                     size_t work_bytes, void* stream);
/* ILRMA.  One iteration: (1) P_k = |y_k|^2, rounded once to float32 (glowk_iva_power); (2) one Itakura-Saito iteration of
 * glowk_nmf_fit (beta 0, update_w 1) on P as a batch of nsig M spectrograms, bit for bit; (3, 4) the covariances with the factors'
 * weights and the iterative projection; (5) with y refreshed, lambda_k = sqrt(mean_{f,t} |y_k|^2) (the sum in the orders above);
 * where lambda_k is finite and positive, row k of every W_f is divided by lambda_k and basis_k by lambda_k^2 (in fp64, rounded once
 * to float32) (glowk_iva_normalize: four launches).  nsig M <= 65535.  Nine launches per iteration.
 * glowk_ilrma_workspace_bytes: glowk_iva_workspace_bytes + 4 nsig M rows frames + glowk_nmf_workspace_bytes(nsig M, rows, frames, K),
 * each rounded up to 8 bytes; 0 out of range. */
size_t glowk_ilrma_workspace_bytes(int nsig, int M, int rows, int frames, int K);
int glowk_iva_power(const float* x_dev, const double* w_dev, int nsig, int M, int rows, int frames, float* p_dev /* [nsig][M][rows][frames] */,
                    void* stream);
int glowk_iva_normalize(const float* x_dev, double* w_dev, float* basis_dev, int nsig, int M, int rows, int frames, int K, void* work_dev,
                        size_t work_bytes, void* stream);
int glowk_ilrma_fit(const float* x_dev, double* w_dev, float* basis_dev, float* act_dev, int nsig, int M, int rows, int frames, int K, int n_iter,
                    void* work_dev, size_t work_bytes, void* stream);
/* Output.  glowk_iva_inverse: W_f^-1 by Gauss-Jordan elimination with partial pivoting, [nsig][rows][M][M] complex128; a row whose
 * inverse has a non-finite entry gets an all-zero matrix.  glowk_iva_demix: Y = W X, complex64 [nsig][M][rows][frames], each
 * component rounded once.  glowk_iva_images: img[sig][k][m][f][t] = W_f^-1[m][k] y_k(f, t) with y_k the complex64 value demix stores,
 * the product in fp64, rounded once; complex64 [nsig][M][M][rows][frames] (source, then channel; nsig M M rows frames <= 2^31 - 1), the
 * minimal-distortion projection: the images of one cell add up to X, and are all zero in a row without a finite inverse.  y_dev may
 * be null; one pass over X, one launch each. */
int glowk_iva_inverse(const double* w_dev, int nsig, int M, int rows, double* winv_dev, void* stream);
int glowk_iva_demix(const float* x_dev, const double* w_dev, int nsig, int M, int rows, int frames, float* y_dev, void* stream);
int glowk_iva_images(const float* x_dev, const double* w_dev, const double* winv_dev, int nsig, int M, int rows, int frames,
                     float* y_dev /* may be null */, float* img_dev, void* stream);

/* --- melody: harmonic salience, a Viterbi f0 track, a harmonic comb mask (Salamon & Gomez 2012; Hsu & Jang 2010; glowk_melody.h) ---- */
/* s [nsig][rows][frames] float32 magnitudes, frames contiguous; f0 [B] float64, the grid of candidate fundamentals, strictly ascending
 * and positive; everything is per signal.  nsig in [0, 65535] (0: a successful no-op), rows in [2, 4096], frames in [1, 32768], B in
 * [1, 1024], H in [1, 32]; nsig rows frames and nsig (B + 1) frames <= 2^31 - 1.  The library takes tables, not formulas: the grid, the
 * harmonic weights w [H], the jump penalties pen [J + 1] and the interpolation positions are float64 (int32) device tables that all the
 * signals of a call share.  fp64 without contraction after the loads, every order fixed by the shapes, no atomics, no allocation, no
 * host synchronisation: bitwise reproducible, and a batch gives what its signals give alone.  The conventions are those of the NMF and
 * IVA sections: handle-free, device memory on one device, GLOWK_ERR with a glowk_last_error message before anything is launched;
 * tensors a call writes must not overlap its other tensors; float64 tensors and workspaces 8-byte aligned, the others 4.  Inputs are
 * finite and non-negative.  audiosourcesep_amd/melody.py drives the calls.  Since version 553.
 *
 * Positions (host): for h = 1 .. H, p = h f0_b / bin_hz in IEEE fp64, i = floor(p), a = p - i; term (b, h) is live iff i + 1 <= rows - 1.
 * glowk_melody_positions fills idx_host [B][H] (i, or -1 for a dead term) and frac_host [B][H] (a); it refuses a grid that is not finite,
 * positive and strictly ascending and a bin_hz that is not finite and positive.  The caller copies both to the device.
 * Salience: sal[b][t] = sum_h w_h ((1 - a) s[i][t] + a s[i + 1][t]) over the live terms, h ascending, rounded once to float32.
 * Emission: m = the maximum of the signal's salience plane (exact), e = (double) sal / max((double) m, 2^-40).
 * Track: states 0 .. B - 1 are the bins, state B is "unvoiced"; only fp64 add, subtract and compare.  D_0[b] = e[b][0], D_0[B] = theta.
 * For t >= 1 a candidate replaces the best only if strictly greater, in this order: voiced b: state B with D[B] - nu, then b' = max(0,
 * b - J) .. min(B - 1, b + J) ascending with D[b'] - pen[|b - b'|]; D_t[b] = e[b][t] + best.  Unvoiced: state B with D[B], then b' = 0 ..
 * B - 1 ascending with D[b'] - nu; D_t[B] = theta + best.  The path ends in the first maximum of D_{T-1}[0 .. B] and follows the back
 * pointers.  J in [0, 1023]; theta and nu finite.
 * Mask: 0 where path[t] is not in [0, B); else with x = f bin_hz and g = f0[path[t]], max(0, 1 - min_{h = 1 .. Hm} |x - h g| / width),
 * rounded once.  Hm in [1, 1024], width and bin_hz finite and positive. */
int glowk_melody_positions(const double* f0_host, int B, int H, double bin_hz, int rows, int32_t* idx_host, double* frac_host);
/* Workspaces: emission 4 nsig groups bytes (groups = min(256, ceil(B frames / 4096)) partial maxima), track nsig frames (B + 1) uint16
 * back pointers, the fused call both and the salience and emission planes (12 nsig B frames bytes); each part rounded up to 8 bytes.
 * 0 for arguments out of range. */
size_t glowk_melody_emission_workspace_bytes(int nsig, int B, int frames);
size_t glowk_melody_track_workspace_bytes(int nsig, int B, int frames);
size_t glowk_melody_workspace_bytes(int nsig, int B, int frames);
/* sal [nsig][B][frames] float32.  One launch: a thread per (bin, frame), the frame fastest. */
int glowk_melody_salience(const float* s_dev, int nsig, int rows, int frames, const int32_t* idx_dev, const double* frac_dev, const double* w_dev,
                          int B, int H, float* sal_dev, void* stream);
/* e [nsig][B][frames] float64 and m [nsig] float32.  Two launches. */
int glowk_melody_emission(const float* sal_dev, int nsig, int B, int frames, double* e_dev, float* m_dev, void* work_dev, size_t work_bytes,
                          void* stream);
/* path [nsig][frames] int32 in [0, B].  One launch, one workgroup per signal, one barrier per frame.  ticks_dev (may be null): [nsig][2]
 * int64, the ticks of the constant 100 MHz clock the recursion and the back-trace took. */
int glowk_melody_track(const double* e_dev, int nsig, int B, int frames, const double* pen_dev, int J, double theta, double nu, int32_t* path_dev,
                       int64_t* ticks_dev, void* work_dev, size_t work_bytes, void* stream);
/* mask [nsig][rows][frames] float32.  One launch. */
int glowk_melody_mask(const int32_t* path_dev, int nsig, int frames, const double* f0_dev, int B, int rows, int Hm, double width, double bin_hz,
                      float* mask_dev, void* stream);
/* Salience, emission, track and mask in one call (five launches): bit for bit the four calls above. */
int glowk_melody_fit(const float* s_dev, int nsig, int rows, int frames, const int32_t* idx_dev, const double* frac_dev, const double* w_dev,
                     const double* f0_dev, int B, int H, const double* pen_dev, int J, double theta, double nu, int Hm, double width, double bin_hz,
                     int32_t* path_dev, float* mask_dev, float* m_dev, void* work_dev, size_t work_bytes, void* stream);

/* --- RPCA: low-rank plus sparse by inexact ALM (Lin et al. 2010; Huang et al. 2012; glowk_rpca.h) ------------------------------------- */
/* m [nsig][rows][frames] float32 magnitudes, frames contiguous; everything is per signal.  nsig in [0, 65535] (0: a successful no-op),
 * rows in [1, 2049], frames in [1, 65535]; nsig rows frames and nsig rows rows <= 2^31 - 1.  All state and arithmetic after the load of
 * m are fp64 without contraction; every order is fixed by the shapes, there are no atomics, no spin waits and no allocation: bitwise
 * reproducible, and a batch gives what its signals give alone.  The eigensolver reads its sweep flags (4 nsig bytes) on the host once
 * per sweep and glowk_rpca_fit its stop flags once per iteration; these calls synchronise the stream, the others do not.  Conventions
 * as in the NMF, IVA and melody sections: handle-free, device memory on one device, GLOWK_ERR with a glowk_last_error message before
 * anything is launched; tensors a call writes must not overlap its other tensors; float64 tensors and workspaces 8-byte aligned, the
 * others 4.  Inputs are finite.  audiosourcesep_amd/rpca.py drives the calls.  Since version 554.
 *
 * GEMM (v_mfma_f64_16x16x4_f64, 64 x 64 tiles): form 0, c [M][M] = a a^T with a [M][K]; form 1, c [M][M] = a diag(scale) a^T with scale
 * [K], each term a_ik (scale_k a_jk); form 2, c [M][N] = a b with b [K][N].  N == M for forms 0 and 1, whose elements i <= j are computed
 * once and mirrored: c is exactly symmetric.  The sum over k is one fused multiply-add chain in ascending k from 0; form 0 splits K into
 * min(8, ceil(K / 1024)) parts of ceil(K / parts) rounded up to 16, a chain each, added in ascending order from part 0 by a second
 * launch (work_dev: 8 nsig parts M M bytes when parts > 1, else none; the other forms need none).  M in [1, 2049], N and K in [1, 65535].
 * Error per element: at most (K + 4) 2^-53 sum_k |a_ik| |b_kj|.
 * Eigensolver: cyclic Jacobi on g [nsig][n][n] (symmetric, overwritten; its diagonal ends as l) in round-robin order: m = n rounded up
 * to even, position 0 holds index 0 and position j >= 1 holds 1 + (j - 1 - r) mod (m - 1) in round r = 0 .. m - 2; round r pairs
 * positions i and m - 1 - i, i < m / 2; the pair with index n (odd n) rests.  A pair p < q is rotated when |g_pq| > 2^-52 sqrt(|g_pp
 * g_qq|) and |g_pq| > 2^-51 max |g| (of g as given; without it the null space of a rank-deficient matrix rotates rounding noise against
 * a diagonal of rounding noise until the cap): theta = (g_qq - g_pp) / (2 g_pq), t = sign(theta) / (|theta| + sqrt(theta^2 + 1)) (1 for theta = 0), c = 1 / sqrt(t^2 + 1),
 * s = t c.  All rotations of a round come from g at the round's start; then rows p and q of g become c g_p - s g_q and s g_p + c g_q
 * (one launch), then columns p and q of g and of v likewise (a second launch).  v starts as the identity: g_in = v diag(l) v^T.  A
 * sweep is the m - 1 rounds; the solve ends after the first sweep that rotated nothing, or after 30 sweeps, and then bit 0 of
 * status_dev is set.  sweeps_dev [nsig]: the sweeps run, that last one included (1 for a diagonal matrix).  l is in the solver's
 * order, not sorted.  work_dev: 16 nsig ceil(n / 2) + 8 nsig + 120 nsig bytes, rounded up to 8.
 * Shrink: out = sign(t) max(|t| - thr, 0); out_dev may be t_dev.
 * SVT: G = a a^T (form 0), G = v diag(l) v^T, sigma_i = sqrt(max(l_i, 0)), g_i = sigma_i > tau ? 1 - tau / sigma_i : 0, P = v diag(g)
 * v^T (form 1), l_dev = P a (form 2); tau_dev [nsig] float64.
 * Fit: lam = gain / sqrt(max(rows, frames)); n2 = sqrt of the largest eigenvalue of m m^T from the solver; ninf = max |m|; a signal
 * with n2 == 0 gets L = S = 0 and 0 iterations.  Else Y = m / max(n2, ninf / lam), mu = 1.25 / n2, mu_bar = 1e7 mu, L = S = 0, and per
 * iteration: S = shrink((m - L) + Y / mu, lam / mu); L = SVT((m - S) + Y / mu, 1 / mu); Z = (m - L) - S; Y = Y + mu Z; mu = min(1.5 mu,
 * mu_bar); the signal stops when sqrt(sum Z^2) / sqrt(sum m^2) < tol (the sums over chunks of the cells, 256 strided threads each in
 * ascending order, a pairwise tree, the chunks in order).  A stopped signal's L, S and count are frozen.  gain > 0, tol >= 0, n_iter in
 * [0, 100000].  iters_dev [nsig] int32; status_dev [nsig] int32, the OR of the solves' status.
 * Binary mask: mask = |S| > gain_mask |L| ? 1 : 0; with x_dev (complex64) also bg = (1 - mask) x and fg = mask x. */
size_t glowk_rpca_gemm_workspace_bytes(int nsig, int M, int N, int K, int form);
int glowk_rpca_gemm(const double* a_dev, const double* b_dev, const double* scale_dev, int nsig, int M, int N, int K, int form, double* c_dev, void* work_dev,
                    size_t work_bytes, void* stream);
size_t glowk_rpca_eigh_workspace_bytes(int nsig, int n);
int glowk_rpca_eigh(double* g_dev, int nsig, int n, double* l_dev, double* v_dev, int32_t* sweeps_dev, int32_t* status_dev, void* work_dev, size_t work_bytes,
                    void* stream);
int glowk_rpca_shrink(const double* t_dev, size_t count, double thr, double* out_dev, void* stream);
/* svt workspace: three n x n matrices, two n vectors and the flags per signal, the form 0 partials, the solver's.  fit workspace: two
 * rows x frames float64 planes per signal, the state, the partial sums, and the svt workspace.  0 for arguments out of range. */
size_t glowk_rpca_svt_workspace_bytes(int nsig, int rows, int frames);
int glowk_rpca_svt(const double* a_dev, int nsig, int rows, int frames, const double* tau_dev, double* l_dev, int32_t* sweeps_dev, int32_t* status_dev,
                   void* work_dev, size_t work_bytes, void* stream);
size_t glowk_rpca_workspace_bytes(int nsig, int rows, int frames);
int glowk_rpca_fit(const float* m_dev, int nsig, int rows, int frames, double gain, double tol, int n_iter, double* l_dev, double* s_dev, int32_t* iters_dev,
                   int32_t* status_dev, void* work_dev, size_t work_bytes, void* stream);
int glowk_rpca_binary_mask(const double* l_dev, const double* s_dev, const float* x_dev, size_t count, double gain_mask, float* mask_dev, float* bg_dev,
                           float* fg_dev, void* stream);

/* --- PROJET: panned sources from two channels by projections (Fitzgerald, Liutkus & Badeau 2016; glowk_projet.h) --------------------- */
/* X [nsig][2][rows][frames] complex64 (re, im interleaved, frames fastest), the STFT of two channels.  nsig in [0, 65535] (0: a
 * successful no-op), rows in [1, 4096], frames in [1, 32768], M in [2, 32] projections, L in [1, 128] pan positions, J in [1, 8] sources,
 * alpha in [1, 2], beta in {0, 1, 2}, n_iter in [0, 100000]; nsig J rows frames <= 2^31 - 1 (and nsig M rows frames for the stored
 * projections).  FLOOR = 2^-40.  Everything after the load of X is fp64 without contraction; every sum has an order that the shapes
 * alone fix, never nsig or the data; no atomics, no spin waits, no allocation, no host synchronisation: bitwise reproducible, and a
 * batch gives what its signals give alone.  Conventions as in the IVA section: handle-free, device memory on one device, enqueued on
 * `stream`, GLOWK_ERR with a glowk_last_error message before anything is launched; tensors a call writes must not overlap its other
 * tensors; everything 8-byte aligned.  Inputs are finite, P and Q non-negative.  audiosourcesep_amd/projet.py drives the calls and builds
 * the tables: the library takes tables, not formulas.  Since version 555.
 *
 * Tables (float64, shared by the signals of a call): u [M][2], the projection directions; k [M][L], the gain of pan position l seen
 * through projection m; up [2][M], the pseudo-inverse of u.  State: p [nsig][J][rows][frames] and q [nsig][L][J], float64; g [nsig][M][J]
 * = k q (l ascending).
 * Per cell: c_m = u[m][0] X_1 + u[m][1] X_2 (two products and an add per component); V_m = |c_m|^alpha: sqrt(re^2 + im^2) for alpha 1,
 * re^2 + im^2 for alpha 2, else pow(re^2 + im^2, alpha / 2); sigma_m = max(sum_j p_j g[m][j], FLOOR), j ascending.
 * With wn_m = V_m sigma_m^(beta - 2) and wd_m = sigma_m^(beta - 1) -- (V, sigma), (V / sigma, 1), (V / (sigma sigma), 1 / sigma) for beta
 * 2, 1, 0 -- and g(x) = sqrt(x) for beta 0, x otherwise:
 *   P update: p_j' = p_j g(sum_m g[m][j] wn_m / max(sum_m g[m][j] wd_m, FLOOR)), m ascending.
 *   Outer sums, with sigma' from p' of the same cell: An[m][j] = sum_cells p_j' wn_m', Ad[m][j] = sum_cells p_j' wd_m', accumulated by
 *   v_mfma_f64_16x16x4_f64.  A signal's cells are cut into G = ceil(cells / chunk) chunks, chunk = ceil(ceil(cells / min(1024,
 *   ceil(cells / 256))) / 256) 256 cells, a workgroup each; a wave adds 64 consecutive cells with 16 instructions of four cells, step
 *   after step of 256 cells; the workgroup adds its four waves in ascending order; the Q kernel adds the G partials in ascending order
 *   from 0.0.  Longest chain of additions: 64 chunk / 256 + 4 + G.
 *   Q update: q[l][j]' = q[l][j] g(sum_m k[m][l] An[m][j] / max(sum_m k[m][l] Ad[m][j], FLOOR)), m ascending; then g = k q'.
 * Divergence: d[sig] = sum_{m, cells} d_beta(V_m | sigma_m) with (V - s)^2 / 2; V ln(V / s) - V + s (0 ln 0 = 0); q - ln q - 1 with q =
 * max(V, FLOOR) / s.  A thread adds its cells' terms in order (m ascending), a halving tree adds the workgroup, the partials in
 * ascending order from 0.0.
 * Separation: w_mj = p_j g[m][j] / sigma_m where sum_j p_j g[m][j] >= FLOOR, else 1 / J; Y_j[ch] = sum_m (up[ch][m] w_mj) c_m, m
 * ascending, rounded once to complex64; y [nsig][J][2][rows][frames].  up u = I and sum_j w_mj = 1: the stems of a cell add up to X. */
/* work_dev of update_q, fit and divergence: 16 nsig G M J bytes (the partial outer sums).  0 for arguments out of range. */
size_t glowk_projet_workspace_bytes(int nsig, int M, int J, int rows, int frames);
/* v [nsig][M][rows][frames] float64, the same bits as the V the other calls hold in registers.  One launch. */
int glowk_projet_projections(const float* x_dev, int nsig, int rows, int frames, const double* u_dev, int M, double alpha, double* v_dev, void* stream);
/* g = k q.  One launch, one workgroup per signal. */
int glowk_projet_gains(const double* k_dev, const double* q_dev, int nsig, int M, int L, int J, double* g_dev, void* stream);
/* The P update alone, in place.  One launch. */
int glowk_projet_update_p(const float* x_dev, int nsig, int rows, int frames, const double* u_dev, const double* g_dev, int M, int J, double alpha, int beta,
                          double* p_dev, void* stream);
/* The outer sums from p as given (sigma from g as given), then the Q update in place and g = k q'.  Two launches. */
int glowk_projet_update_q(const float* x_dev, const double* p_dev, int nsig, int rows, int frames, const double* u_dev, const double* k_dev, int M, int L, int J,
                          double alpha, int beta, double* q_dev, double* g_dev, void* work_dev, size_t work_bytes, void* stream);
/* g = k q, then n_iter iterations in place on p, q and g: one fused pass over X and p (the P update and the outer sums of the new p),
 * then the Q kernel.  2 n_iter + 1 launches.  Bit for bit glowk_projet_gains, then n_iter times glowk_projet_update_p,
 * glowk_projet_update_q. */
int glowk_projet_fit(const float* x_dev, int nsig, int rows, int frames, const double* u_dev, const double* k_dev, int M, int L, int J, double alpha, int beta,
                     int n_iter, double* p_dev, double* q_dev, double* g_dev, void* work_dev, size_t work_bytes, void* stream);
/* d [nsig] float64.  Two launches. */
int glowk_projet_divergence(const float* x_dev, const double* p_dev, int nsig, int rows, int frames, const double* u_dev, const double* g_dev, int M, int J,
                            double alpha, int beta, double* d_dev, void* work_dev, size_t work_bytes, void* stream);
/* y [nsig][J][2][rows][frames] complex64.  One launch. */
int glowk_projet_separate(const float* x_dev, const double* p_dev, int nsig, int rows, int frames, const double* u_dev, const double* up_dev, const double* g_dev,
                          int M, int J, float* y_dev, void* stream);

/* --- Clustering: a weighted Gaussian mixture over time-frequency cells (nussl's PrimitiveClustering, Seetharaman et al. 2019, and ----- */
/* --- SpatialClustering; glowk_cluster.h) ---------------------------------------------------------------------------------------------- */
/* f [nsig][D][rows][frames] float32 features (planes, frames fastest; cell c = r frames + t), w [nsig][rows][frames] float32 weights,
 * non-negative and finite.  nsig in [0, 65535] (0: a successful no-op), rows in [1, 4096], frames in [1, 32768], D in [1, 8] features,
 * J in [1, 8] clusters, nsig max(D, J) rows frames <= 2^31 - 1, reg_covar finite and >= 2^-40, tol finite and >= 0, n_iter in [0, 100000].
 * Only full covariances.  A batch is independent signals.  Everything after the float32 loads is fp64 without contraction (the
 * matrix-core instruction is the one fused operation); every sum has an order that the shapes alone fix, never nsig or the data; no
 * atomics, no spin waits, no allocation, no host synchronisation: bitwise reproducible, and a batch gives what its signals give alone.
 * Conventions as in the PROJET section: handle-free, device memory on one device, enqueued on `stream`, GLOWK_ERR with a
 * glowk_last_error message before anything is launched; tensors a call writes must not overlap its other tensors; float64 tensors and
 * workspaces 8-byte aligned, the others 4.  audiosourcesep_amd/cluster.py drives the calls.  Since version 556.
 *
 * State (float64): pi [nsig][J], mu [nsig][J][D], sigma [nsig][J][D][D], origin o [nsig][D], total W [nsig].
 * Pass 0: W = sum w, o = sum w x / W.  All later moments are of u = x - o, so that B / N - (a / N)(a / N)^T does not cancel against the
 * features' offset.
 * Per cluster: Cholesky sigma_j = L L^T (row by row, the sums in ascending order), Linv = L^-1 by forward substitution, k_j = (log pi_j
 * - sum_d log L[d][d]) - D log(2 pi) / 2.
 * Per cell: y = Linv (x - mu_j) (columns ascending), l_j = k_j - |y|^2 / 2, m = max_j l_j, e_j = exp(l_j - m), s = sum_j e_j in ascending
 * j, lse = m + log s, r_j = e_j / s.
 * Statistics: N_j = sum w r_j, a_j = sum w r_j u, B_j = sum w r_j u u^T (the upper triangle; the update mirrors it, so sigma is bitwise
 * symmetric), LL = sum w lse.  stats [nsig][J (1 + D + D (D + 1) / 2) + 1]: per cluster N, a [D], B[a][b] for a <= b (a ascending, then
 * b); then LL.  They are R^T Phi with R [cells][J] = w r_j (and a row of w for LL) and Phi [cells][P] = (1, u, u u^T upper, lse),
 * accumulated by v_mfma_f64_16x16x4_f64.  A signal's cells are cut into G = ceil(cells / chunk) chunks, chunk = ceil(ceil(cells /
 * min(1024, ceil(cells / 256))) / 256) 256 cells, a workgroup each; a wave adds 64 consecutive cells with 16 instructions of four
 * cells, step after step of 256 cells; the workgroup adds its four waves in ascending order; the per-signal kernel adds the G partials
 * in ascending order from 0.0.  Longest chain of additions: chain = 64 chunk / 256 + 4 + G.
 * Update: pi_j = N_j / W, mu_j = o + a_j / N_j, sigma_j = B_j / N_j - (a_j / N_j)(a_j / N_j)^T + reg_covar I.  A cluster with N_j <
 * 2^-40 W is dead: its mu and sigma stay, its pi is 0, so its r_j is an exact 0 from then on.  A non-positive (or NaN) Cholesky pivot in
 * any cluster leaves the signal's whole state as it was and, in a fit, freezes the signal.  W == 0 leaves the state alone.
 * Status bits (int32 per signal): 1, all weights are zero (posteriors 1 / J); 2, a cluster is dead; 4, a Cholesky factorisation failed
 * (in glowk_cluster_stats and glowk_cluster_posteriors, of the state as given: posteriors 1 / J).
 * Stop: ll_k = LL / W is the likelihood of the state before update k = 0, 1, ..  With tol > 0 a signal stops after update k >= 1 when
 * ll_k - ll_{k-1} <= tol |ll_k|; update k is applied, then the signal is frozen: iters = k + 1, and ll of later k is NaN.  tol == 0
 * runs all n_iter.
 * Start (z_dev [J], the standard-normal quantiles of (j + 1/2) / J: the library takes tables, not formulas): Sigma0 = B / W - (a / W)(a
 * / W)^T + reg_covar I from a second pass about o; v = 64 power-iteration steps on Sigma0 from all ones, divided by its Euclidean norm
 * each step, the sign such that the earliest component of largest magnitude is positive; lambda = v^T Sigma0 v; mu_j = (o + a / W) +
 * (z_j sqrt(lambda)) v, sigma_j = Sigma0, pi_j = 1 / J.  W == 0: pi = 1 / J, mu = 0, sigma = I.
 * Posteriors: mask [nsig][J][rows][frames] float32 = r_j rounded; with x [nsig][C][rows][frames] complex64, C in {1, 2}, also y
 * [nsig][J][C][rows][frames] = mask_j x, each component one float32 product.
 * Spatial features of x [nsig][2][rows][frames] complex64: pan = atan2(|X2|, |X1|) - pi / 4; with delay, delta = -arg(X2 conj X1) /
 * omega_r clipped to +-max_delay (omega_r = 2 pi r / (2 (rows - 1)); 0 in row 0 and where a channel is exactly 0); w = (|X1|^2 +
 * |X2|^2)^(p / 2) (sqrt for p 1, itself for p 2, else pow), 0 in row 0 and where both channels are exactly 0.  fp64, rounded to float32;
 * feat [nsig][1 + delay][rows][frames].
 *
 * Error bound of the statistics against exact arithmetic on the same float32 inputs and float64 constants, with eps = 2^-53.  The
 * quadratic form q_j = |Linv (x - mu_j)|^2 is D (D + 1) / 2 products and as many additions of terms whose absolute values sum to at
 * most q~_j = | |Linv| |x - mu_j| |^2; each y_a carries at most (D + 1) eps relative to its absolute sum and the squares and their sum
 * another D + 1, so |dq_j| <= 2 (D + 2) eps q~_j (1 + O(eps)); l_j = k_j - q_j / 2 adds one rounding of |l_j| <= |k_j| + q~_j / 2.  exp and
 * log are within 1 ulp (2 eps): |dl_j| <= eps e_j with e_j = 4 (D + 2)^2 (q~_j + |k_j| + 1) is a generous cover of all of it.  With
 * r_j = exp(l_j) / sum_i exp(l_i): |dr_j| / r_j <= |dl_j| + sum_i r_i |dl_i| + 4 eps (two exp, the sum's ratio, the division), so |dr_j|
 * <= eps r_j (e_j + sum_i r_i e_i + 4).  A statistic sum_c w r_j phi then differs by at most
 *   eps [ chain sum_c w r_j |phi| + sum_c w |phi| r_j (e_j + sum_i r_i e_i + 4) ]
 * (the first term is the summation in the order above, the products w r_j and u_a u_b included in the 4), and LL by at most
 *   eps [ chain sum_c w |lse| + sum_c w (|lse| + max_j e_j) ].
 * Update: Cholesky and the triangular solves are backward stable; every element of the new state is within eps 64 D^2 (1 + cond(sigma_j))
 * of the exact update of the same statistics, relative to the element's scale (max |sigma_j| for sigma, max(|mu_j|, sqrt(max |sigma_j|))
 * for mu, 1 for pi). */
/* work_dev: 8 (nsig G (J (P - 1) + 1) + nsig (J (P - 1) + 1) + nsig (D + J (1 + D + D D)) + 2 nsig) bytes, P = 2 + D + D (D + 1) / 2.  0
 * for arguments out of range. */
size_t glowk_cluster_work_bytes(int nsig, int D, int J, int rows, int frames);
/* Pass 0 and the start.  status is written.  Four launches. */
int glowk_cluster_init(const float* f_dev, const float* w_dev, int nsig, int D, int J, int rows, int frames, const double* z_dev, double reg_covar, double* pi_dev,
                       double* mu_dev, double* sigma_dev, double* origin_dev, double* total_dev, int32_t* status_dev, void* work_dev, size_t work_bytes,
                       void* stream);
/* The statistics of the state as given.  status is written (bits 1 and 4).  Three launches. */
int glowk_cluster_stats(const float* f_dev, const float* w_dev, int nsig, int D, int J, int rows, int frames, const double* pi_dev, const double* mu_dev,
                        const double* sigma_dev, const double* origin_dev, const double* total_dev, double* stats_dev, int32_t* status_dev, void* work_dev,
                        size_t work_bytes, void* stream);
/* The update from statistics, in place on pi, mu, sigma; ll [nsig] = LL / W (NaN for W == 0); bits are ORed into status.  work_dev: 8
 * nsig (D + J (1 + D + D D)) bytes.  One launch. */
int glowk_cluster_update(const double* stats_dev, int nsig, int D, int J, double reg_covar, double* pi_dev, double* mu_dev, double* sigma_dev,
                         const double* origin_dev, const double* total_dev, double* ll_dev, int32_t* status_dev, void* work_dev, size_t work_bytes, void* stream);
/* The whole loop: pass 0 (origin, total), the start (z_dev) or, with z_dev null, the state as given in pi, mu, sigma; then n_iter times
 * the statistics pass and the per-signal kernel.  ll [nsig][n_iter], iters and status [nsig] int32.  Four or five launches and two per
 * iteration.  Bit for bit glowk_cluster_init, then n_iter times glowk_cluster_stats, glowk_cluster_update. */
int glowk_cluster_fit(const float* f_dev, const float* w_dev, int nsig, int D, int J, int rows, int frames, const double* z_dev, double reg_covar, int n_iter,
                      double tol, double* pi_dev, double* mu_dev, double* sigma_dev, double* origin_dev, double* total_dev, double* ll_dev, int32_t* iters_dev,
                      int32_t* status_dev, void* work_dev, size_t work_bytes, void* stream);
/* The masks and, with x_dev (then y_dev too), the masked spectra.  status is written (bits 1 and 4).  work_dev as for the update.  Two
 * launches. */
int glowk_cluster_posteriors(const float* f_dev, int nsig, int D, int J, int rows, int frames, const double* pi_dev, const double* mu_dev, const double* sigma_dev,
                             const double* origin_dev, const double* total_dev, const float* x_dev, int C, float* mask_dev, float* y_dev, int32_t* status_dev,
                             void* work_dev, size_t work_bytes, void* stream);
/* One launch. */
int glowk_cluster_spatial_features(const float* x_dev, int nsig, int rows, int frames, int delay, double max_delay, double p, float* feat_dev, float* w_dev,
                                   void* stream);

/* --- Kernel additive modelling: sparse-kernel medians with back-fitting (Liutkus, FitzGerald, Rafii, Pardo & Daudet 2014; KAML 2015; ---- */
/* --- glowk_kam.h) ---------------------------------------------------------------------------------------------------------------------- */
/* Every source j has a proximity kernel, the set of time-frequency neighbours it is locally constant over; the sources are estimated
 * together by back-fitting: median-filter each source's estimate over its own kernel, share the mixture out by the ratio of the results,
 * repeat.  With J = 2, a horizontal and a vertical kernel and one iteration that is HPSS; with a periodic kernel, the adaptive REPET.
 * s, v [nsig][rows][frames] float32, frames contiguous.  nsig in [0, 65535] (0: a successful no-op of valid arguments), rows in [1, 4096],
 * frames in [1, 32768], J in [1, 8] sources, nsig J rows frames <= 2^31 - 1.  Conventions as in the sections above: handle-free, every
 * tensor device memory on one device, enqueued on `stream`, no atomics, no allocation, no host synchronisation, a launch count that the
 * shapes and models alone fix, GLOWK_ERR with a glowk_last_error message before anything is launched; tensors a call writes must not
 * overlap its other tensors; bitwise reproducible, and a batch gives what its signals give alone.  Inputs are finite.
 * audiosourcesep_amd/kam.py drives the calls.  Since version 557.
 *
 * The median over a sparse kernel.  `offsets` is a HOST table of n pairs (d_row, d_frame), int32 [n][2]: a parameter like a filter's
 * size, checked on the host and passed to the kernel by value in its launch arguments (as int16 pairs).  1 <= n <= 127, |d_row| <= 4095,
 * |d_frame| <= 32767; duplicates are allowed and count twice; (0, 0) need not be present.  The neighbours of cell (r, t) are the cells
 * (r + d_row, t + d_frame) that lie inside the plane; the others are skipped and never read (no reflection).  With m of them: m odd, the
 * middle element -- a selection by compares, the bits a sort gives; m even, (a + b) * 0.5f of the two middle elements in fp32, the only
 * arithmetic on the values; m = 0, the cell itself (glowk_nn_median's rules).  Of elements that compare equal (they differ in bits only
 * as -0 and +0 do) the first in table order is taken (glowk_median_filter's rule).  out_dev must not overlap s_dev.  One launch: a wave
 * owns 64 consecutive frames of one row; a workgroup is four waves for n <= 64 and one above, a function of n alone. */
int glowk_kam_median(const float* s_dev, int nsig, int rows, int frames, const int32_t* offsets, int n, float* out_dev, void* stream);
/* The back-fitting step, elementwise in fp32 over n cells per signal: a [nsig][J][n] (the filtered estimates, >= 0), v [nsig][n] (the
 * mixture magnitude), p and mask [nsig][J][n]; mask_dev may be null.  glowk_hpss_mask's arithmetic (both margins 1) from 2 to J sources:
 *   Z = max_j a_j, bad = Z < FLT_MIN (1.17549435e-38), Z = 1 where bad; r_j = (a_j / Z)^power (powers 1 and 2 without powf);
 *   mask_j = r_j / (r_0 + r_1 + .. + r_{J-1}), the sum in ascending j, and 1 / J where bad; p_j = v mask_j.
 * Every operation rounds once (no contraction).  power finite and > 0; nsig J n <= 2^31 - 1 (n = 0 is a no-op).  One launch. */
int glowk_kam_backfit(const float* v_dev, const float* a_dev, int nsig, int J, size_t n, float power, float* p_dev, float* mask_dev, void* stream);
/* The bytes of work_dev that glowk_kam_fit needs: the filtered estimates, 4 nsig J rows frames rounded up to a multiple of 8 (as every
 * size query here is), plus, when some model_k[j] > 0, glowk_nn_workspace_bytes(1, rows, frames, k).  model_k: host [J], as below.  0 for
 * arguments out of range (and for nsig = 0). */
size_t glowk_kam_work_bytes(int nsig, int rows, int frames, int J, const int32_t* model_k);
/* The loop.  The model of source j is one of two kinds, told by two HOST arrays [J] of which exactly one is non-zero at j:
 *   model_n[j] = n_j >= 1: an offset table of n_j pairs, filtered as glowk_kam_median does; the tables of these sources follow each other
 *     in `offsets` (host, int32 [sum n_j][2]) in source order;
 *   model_k[j] = k_j >= 1: a frame-neighbour tensor idx_dev[j] (idx_dev: a host array [J] of device pointers, null entries for the other
 *     kind) int32 [nsig][frames][k_j], what glowk_nn_neighbors and glowk_period_neighbors write, filtered by glowk_nn_median, one signal
 *     at a time.
 * P_j = V for every j; each of the n_iter iterations (1 <= n_iter <= 100) computes A_j = filter_j(P_j) for every j, then P, mask =
 * backfit(V, A).  p [nsig][J][rows][frames]; mask_dev (nullable) receives the last iteration's masks.  Bit for bit n_iter staged rounds of
 * glowk_kam_median / glowk_nn_median and glowk_kam_backfit.  Per iteration one launch per offset model, 2 nsig per frame-neighbour model,
 * and one for the back-fit.  work_bytes at least glowk_kam_work_bytes; work_dev 8-byte aligned is enough. */
int glowk_kam_fit(const float* v_dev, int nsig, int rows, int frames, int J, const int32_t* model_n, const int32_t* offsets, const int32_t* model_k,
                  const int32_t* const* idx_dev, int n_iter, float power, float* p_dev, float* mask_dev, void* work_dev, size_t work_bytes, void* stream);

/* --- Convolutive NMF (NMFD): time-varying templates (Smaragdis 2004; Schmidt & Morup 2006; Smaragdis 2007; glowk_nmfd.h) --------------- */
/* Every component is a patch of Tw spectra instead of one spectrum; the activations say where the patches start.
 * V [nsig][rows][frames] float32, finite and >= 0, frames contiguous; W [nw][rows][K][Tw], Tw contiguous, nw = nsig or 1 (one
 * dictionary shared by every signal, allowed only where W is not updated); H [nsig][K][frames]; W and H float32, finite and >= 0.
 * FLOOR = 2^-40, beta = 0, 1 or 2 and g as in the NMF section.
 * The stacked view, s = k Tw + tau (k-major): Ws [rows][K Tw] is W's own memory read as an NMF dictionary; Hs[s][t] = H[k][t - tau],
 * and an exact 0 for t < tau.  L = Ws Hs, an fp32 fma chain over s (padded with exact zeros) on v_mfma_f32_32x32x2_f32; Le, Q, P and g
 * exactly as in the NMF section.  Hs is never in memory: the shift is applied where H is loaded.
 *   W update: W' = W g(Q Hs^T / max(P Hs^T, FLOOR)): the NMF W update on (V, Ws, Hs), bit for bit what glowk_nmf_fit (update_w 2)
 *     gives on a materialised Hs (the same chain order over s, the same chunk plan at K Tw components).
 *   H update, the joint one (the majorise-minimise argument holds for it: no update increases D):
 *     N[k][t] = sum_tau sum_f W[f][k][tau] Q[f][t + tau] over t + tau < frames, D the same sum with P, H' = H g(N / max(D, FLOOR)).
 *     The sums over f are the NMF H update's chains Ws^T Q and Ws^T P; the Tw shifted rows are then added in ascending tau in fp32.
 *     At Tw = 1 this is glowk_nmf_fit's H update bit for bit.
 * One iteration is the W update with the old H, then the H update with the new W.  frames < Tw is allowed: the slices tau >= frames
 * meet no data, and a W update makes them exact zeros.  A source that owns the components [k0, k1) owns the stacked range
 * [k0 Tw, k1 Tw).  Every term is non-negative, so the error of one update is relative per element: at most (3 K Tw + 2 rows Tw + 16)
 * 2^-24 of the value for H, (3 K Tw + 2 frames + 16) 2^-24 for W, and an exact 0 where the exact result is 0.  L, Q and P exist in
 * registers alone.  Conventions as in the NMF section: handle-free, every tensor device memory on one device, launches on `stream`
 * with no atomics, no allocation and no host synchronisation, a launch count that depends on the shapes and n_iter alone, bitwise
 * reproducible results, a batch gives what its signals give alone.  K in [1, 128], Tw in [1, 32], K Tw <= 128 (more needs several
 * passes over the accumulators); nsig, rows, frames and the element counts as in the NMF section with K Tw for K; anything else is
 * GLOWK_ERR with a glowk_last_error message before anything is launched.  audiosourcesep_amd/nmfd.py drives the calls.
 * Since version 558. */
/* The bytes of work_dev that glowk_nmfd_fit and glowk_nmfd_divergence need: with nch and rtiles of glowk_nmf_workspace_bytes at K Tw
 * components, nsig max(8 nch rows K Tw, 8 rtiles nch, 8 K Tw frames) -- the W update's partial sums, the divergence's, and the H
 * update's stacked numerators and denominators.  0 for arguments out of range (and for nsig = 0). */
size_t glowk_nmfd_workspace_bytes(int nsig, int rows, int frames, int K, int Tw);
/* n_iter iterations in place; update_w = 1: W, then H; 0: H alone (W may be shared, nw = 1); 2: W alone, as in glowk_nmf_fit.  The W
 * update is two launches as there.  The H update is two launches: the stacked numerators and denominators [2][K Tw][frames] go to
 * work_dev (a workgroup owns 32 frames of them), and a second launch adds the shifts and takes the step, so work_dev is needed in
 * every mode.  4 n_iter launches with update_w = 1, 2 n_iter with 0 or 2.  V, W, H and work must not overlap; work_dev aligned to 8
 * bytes. */
int glowk_nmfd_fit(const float* v_dev, int nsig, int rows, int frames, float* w_dev, int nw, float* h_dev, int K, int Tw, int beta, int n_iter,
                   int update_w, void* work_dev, size_t work_bytes, void* stream);
/* out[sig] = D_beta(V | Ws Hs), float64: glowk_nmf_divergence on (V, Ws, Hs), bit for bit.  At most (K Tw + 4) 2^-24 sum(w) from the
 * exact value.  Two launches. */
int glowk_nmfd_divergence(const float* v_dev, int nsig, int rows, int frames, const float* w_dev, int nw, const float* h_dev, int K, int Tw, int beta,
                          double* out_dev /* [nsig] */, void* work_dev, size_t work_bytes, void* stream);
/* Ratio masks of num_sources <= 16 sources that own the component ranges [bounds[s], bounds[s + 1]), bounds_host[0] = 0 < .. <
 * bounds_host[num_sources] = K, in components: glowk_nmf_masks on (Ws, Hs) with the bounds scaled by Tw, bit for bit; power, x_dev,
 * channels, mask_dev and spec_dev as there.  One launch. */
int glowk_nmfd_masks(const float* w_dev, int nw, const float* h_dev, int nsig, int rows, int frames, int K, int Tw, const int32_t* bounds_host,
                     int num_sources, int power, const float* x_dev /* [nsig][C][rows][frames] complex64, or null */, int channels,
                     float* mask_dev /* [nsig][S][rows][frames] */, float* spec_dev /* [nsig][S][C][rows][frames] complex64, or null */,
                     void* stream);

/* --- WPE dereverberation: delayed linear prediction (Nakatani et al. 2010; Yoshioka & Nakatani 2012; nara_wpe; glowk_wpe.h) ----------- */
/* Per signal and frequency row, independently.  X [nsig][M][rows][frames] complex64, K taps, delay, D = M K.  The stacked past
 * x~(t) in C^D has x~[k M + m](t) = x_m(t - delay - k), zero where t - delay - k < 0.  One iteration:
 *   power         q(t) = (sum_m |y_m(t)|^2) / M (m ascending); p(t) = q(t), or with context c > 0 the sum of q over the frames of
 *                 [t - c, t + c] that exist (ascending) divided by their count; w(t) = 1 / max(p(t), eps max_t p(t)).  A row whose
 *                 maximum is zero or not finite gets w = 0 everywhere: its correlations are zero, its solve fails its first pivot, so
 *                 it is flagged, G = 0, and the filter passes it through.
 *   correlations  R = sum_t w(t) x~ x~^H [D][D] (both triangles, R[j][i] the bitwise conjugate of R[i][j], the diagonal's imaginary
 *                 part exactly 0) and P = sum_t w(t) x~ x^H [D][M], on v_mfma_f64_16x16x4_f64: with x~ = a + i b an element is
 *                 (Gaa + Gbb) + i (Gba - Gab) with the four real Gram sums Gpq[i][j] = sum_t (w p_i) q_j, frames ascending, four to an
 *                 instruction, each in its own accumulator from 0.0 and combined once at the end.
 *   solve         tr = sum_i Re R[i][i] (ascending); R[i][i] += loading (tr / D); R = L L^H by columns; a pivot that is not finite
 *                 or not > 0 gives G = 0 and status GLOWK_WPE_PIVOT (1); else status 0 and G = R^-1 P [D][M] by the two triangular
 *                 solves.
 *   filter        y_m(t) = x_m(t) - sum_e conj(G[e][m]) x~_e(t), e ascending, each component rounded once to float32.  A row whose G
 *                 is all zeros is copied.
 * From the second iteration on the power is taken from the complex64 y the previous iteration stored, so glowk_wpe_fit gives the bits
 * of the four staged calls iterated by hand.  Error bounds, with u = 2^-53 and T = frames:
 *   w             relative (M + 2 c + 6) u per element; the row maximum is exact where the q are.
 *   R, P          with the stacked real vector v = [a; b], a real Gram sum is within (T + 8) u sum_t w |v_i| |v_j| of its exact value;
 *                 so |Re error[i][j]| <= (T + 8) u sum_t w (|a_i| |a_j| + |b_i| |b_j|) and |Im error[i][j]| <= (T + 8) u sum_t w
 *                 (|b_i| |a_j| + |a_i| |b_j|).
 *   G             backward: (R' + E) G = P with R' the loaded matrix as stored in fp64 and |E| <= 12 (D + 1) u |L| |L^H|
 *                 elementwise (Cholesky plus two triangular solves, 3 D + 1 roundings of complex arithmetic at 2 sqrt 2 u each), so
 *                 |R' G - P| <= 12 (D + 1) u |L| |L^H| |G|.
 *   y             one float32 rounding of the fp64 value, whose error is at most (4 D + 2) u (|x_m| + sum_e |G[e][m]| |x~_e|_1).
 *   one iteration given its weights: the bound of y plus 2 cond(R') ((T + 8) + 12 (D + 1)) u ||G||_F ||x~(t)||_2, normwise: the
 *                 operation counts of the correlations and of the solve are part of the bound, not u cond alone.  Over several
 *                 iterations it holds as long as the complex64 estimates between them round alike; in practice the float32
 *                 rounding term dominates.
 * Everything after the float32 load is fp64 without contraction; every order is fixed by the shapes; results are bitwise
 * reproducible and a batch gives what its signals give alone.  Handle-free, every tensor device memory on one device, launches on
 * `stream`, no atomics, no allocation, no host synchronisation.  M in [1, 4], K in [1, 32], M K <= 64, delay in [1, 16], context in
 * [0, 8], eps in (0, 1], loading in [0, 1], iterations in [0, 1000], nsig in [0, 65535], rows in [1, 4096], frames in [1, 32768], nsig M
 * rows frames <= 2^31 - 1; anything else is GLOWK_ERR with a glowk_last_error message before anything is launched.  Tensors aligned
 * to 8 bytes (status 4); a tensor a call writes must not overlap another of its tensors.  audiosourcesep_amd/wpe.py drives the
 * calls.  Since version 559. */
#define GLOWK_WPE_OK 0
#define GLOWK_WPE_PIVOT 1
/* The bytes of glowk_wpe_fit's work_dev: w [nsig][rows][frames] float64, R [nsig][rows][D][D] and P [nsig][rows][D][M] complex128.
 * 0 for arguments out of range (and for nsig = 0). */
size_t glowk_wpe_workspace_bytes(int nsig, int M, int K, int rows, int frames);
/* w [nsig][rows][frames] float64 from y [nsig][M][rows][frames] complex64; max_dev [nsig][rows] float64, or null, receives max_t p.
 * One launch, one workgroup per (signal, row). */
int glowk_wpe_power(const float* y_dev, int nsig, int M, int rows, int frames, int context, double eps, double* w_dev, double* max_dev, void* stream);
/* r_dev [nsig][rows][D][D] and p_dev [nsig][rows][D][M] complex128.  One launch, one workgroup per (signal, row). */
int glowk_wpe_correlations(const float* x_dev, const double* w_dev, int nsig, int M, int rows, int frames, int K, int delay, double* r_dev, double* p_dev,
                           void* stream);
/* g_dev [nsig][rows][D][M] complex128 and status_dev [nsig][rows] int32 for any D in [1, 64].  One launch, one wave per (signal, row). */
int glowk_wpe_solve(const double* r_dev, const double* p_dev, int nsig, int rows, int D, int M, double loading, double* g_dev, int32_t* status_dev, void* stream);
/* y_dev like x_dev.  One launch, one workgroup per (signal, row, 256 frames). */
int glowk_wpe_filter(const float* x_dev, const double* g_dev, int nsig, int M, int rows, int frames, int K, int delay, float* y_dev, void* stream);
/* `iterations` iterations (power of x, then of y; correlations; solve; filter): 4 launches each, all in one call.  y_dev, g_dev and
 * status_dev receive the last iteration's; with iterations = 0 nothing is written. */
int glowk_wpe_fit(const float* x_dev, int nsig, int M, int rows, int frames, int K, int delay, int iterations, int context, double eps, double loading,
                  float* y_dev, double* g_dev, int32_t* status_dev, void* work_dev, size_t work_bytes, void* stream);

/* --- host utility ----------------------------------------------------------------------------------------------------------- */
/* CRC-32C (Castagnoli) of a host buffer: the checksum of TFRecord frames (datasets/preprocessing.py:197-271) and of TensorFlow
 * checkpoint bundles (train_utils.py:62-75), whose tensors are too large for an interpreted byte loop */
uint32_t glowk_crc32c(const void* host_data, size_t n);

#ifdef __cplusplus
}
#endif
#endif /* GLOWK_H */
