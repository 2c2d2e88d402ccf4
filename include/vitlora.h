/*
 * vitlora.h -- C ABI of libvitlora_hip.so: the MI355X (gfx950) implementation of the
 * ViT + LoRA + FGSM/PGD hot path of
 *   rneddojr/Adapting-Pretrained-Vision-Transformers-with-LoRA-against-Attack-Vectors.
 *
 * The reference has no FFI: the path is reached through Python callables.  Each
 * entry point below names the reference callable (file:line in /root/reference) it
 * stands in for; INTEGRATION.md shows the ctypes binding a maintainer would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller unless marked "host";
 *   - every launch function takes a hipStream_t (as void*) and only enqueues work:
 *     no allocation, no host synchronisation after vl_plan()/vl_set_workspace();
 *   - return value 0 = OK, negative = error; vl_last_error() gives the message;
 *   - one handle per device, driven by one host thread (the reference's model:
 *     a single Python thread drives one device, whitebox_attacks.py:67).
 */
#ifndef VITLORA_H
#define VITLORA_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VL_OK 0
#define VL_ERR_ARG (-1)
#define VL_ERR_HIP (-2)
#define VL_ERR_STATE (-3)
#define VL_ERR_UNSUPPORTED (-4)
#define VL_ERR_NONFINITE (-5)   /* an EARLIER call produced a non-finite gradient (fp16 range exceeded): that step must be skipped / redone in f32 */

/* LoRA target bits.  peft matches module-name suffixes: the reference's
 * ["query","key","value","output.dense"] (train_loras.py:81) = Q|K|V|O|FC2. */
#define VL_T_Q 1u
#define VL_T_K 2u
#define VL_T_V 4u
#define VL_T_O 8u      /* attention.output.dense */
#define VL_T_FC1 16u   /* intermediate.dense     */
#define VL_T_FC2 32u   /* output.dense           */

#define VL_PREC_F16 0
#define VL_PREC_F32 1
#define VL_PREC_BF16 2     /* bf16 operands, fp32 accumulation: the same kernels as VL_PREC_F16 instantiated on __bf16 (no gradient-range
                              cliff, 8 mantissa bits); BASELINE config 5 / north_star name this type.
                              DOCUMENTED DEVIATION from north_star's "1e-2 bf16": against the fp32 reference this mode is held to
                              logits 1.5e-2, dLoss/dx 2.2e-2, LoRA gradients 3.5e-2 on ViT-B/16 (measured 7.9e-3 / 1.5e-2 / 2.5e-2;
                              tests/test_hip_bf16.py) and 2e-2 / 3e-2 on the 24-layer ViT-L/16 (tests/test_hip_patch.py).  Cause, priced on
                              the CPU oracle with no kernel involved (tools/error_budget_mixed.py, profiles/r05_bf16_mixed_mode_cpu.txt):
                              the bf16 MFMA OPERANDS alone (weights, LayerNorm output, q/k/v, probabilities, context, gelu, dz) cost
                              8.9e-3 of the ViT-B and 1.02e-2 of the ViT-L input gradient with EVERY other site in fp32 -- no storage
                              choice brings ViT-L under 1e-2 with bf16 products.  VL_PREC_F16 meets 1e-2 at both depths (1.8e-3 / 2.4e-3)
                              at the same speed and is the default everywhere, including patch_attack.py (config 5); bf16 is for range:
                              it cannot raise VL_ERR_NONFINITE. */

typedef struct vl_config {
    /* architecture: HF ViTConfig as built by create_vit_model, Utils.py:84-90 */
    int32_t image_size;   /* 224 */
    int32_t patch_size;   /* 16  */
    int32_t hidden;       /* 768  (multiple of 128; head_dim must be 64) */
    int32_t layers;       /* 12  */
    int32_t heads;        /* 12  */
    int32_t mlp;          /* 3072 (multiple of 128) */
    int32_t num_labels;   /* #lines of class_mappings.txt, whitebox_attacks.py:88-90 */
    float   ln_eps;       /* 1e-12 */
    /* LoRA: LoraConfig(r, lora_alpha, lora_dropout, target_modules), train_loras.py:83-90 */
    int32_t lora_r;       /* 0 = no adapters */
    float   lora_alpha;
    float   lora_dropout; /* applied to the LoRA branch input in train mode only */
    uint32_t lora_targets;/* VL_T_* bits */
    int32_t lora_merged;  /* 0: rank-r update fused into the GEMMs as extra K tiles;
                             1: W' = W + s*B*A folded at vl_lora_commit (merge_and_unload,
                                eval_compose.py:110) */
    int32_t precision;    /* VL_PREC_F16 (default): fp16 operands and 16-bit residual streams, fp32 accumulation (MFMA rate);
                             VL_PREC_BF16: the same kernels on bf16 operands (fp32's range: no VL_ERR_NONFINITE; 8 mantissa bits);
                             VL_PREC_F32: every operand and activation fp32 (v_mfma_f32_16x16x4_f32), the
                             parity mode held to 1e-3 against the reference's fp32 CPU path */
    int32_t reserved[3];
} vl_config;

typedef struct vl_model vl_model;

const char* vl_version(void);
const char* vl_last_error(void);

/* create_vit_model(num_classes) + setup_peft_lora(model, rank, alpha, dropout, targets)
 * (Utils.py:84-90, train_loras.py:79-95).  Allocates the packed frozen weights. */
int vl_create(const vl_config* cfg, vl_model** out);
int vl_destroy(vl_model* m);

/* model.load_state_dict(torch.load(path)) (whitebox_attacks.py:94): one call per
 * state-dict entry, HF-4.55.2 key names ("vit.encoder.layer.3.attention.attention.query.weight",
 * "classifier.bias", ...).  src = device fp32, contiguous, numel elements. */
int vl_load_tensor(vl_model* m, const char* name, const float* src, int64_t numel, void* stream);

/* LoRA / classifier master parameters live in ONE flat fp32 buffer (so that the
 * gradient all-reduce and Adam are single flat operations).
 * which: 0 = lora_A [r,in], 1 = lora_B [out,r].  target = one VL_T_* bit.
 * Classifier: layer = -1, which 0 = weight [C,D], 1 = bias [C]. */
int vl_param_tensor(vl_model* m, int layer, uint32_t target, int which, float** ptr, int64_t* numel);
int vl_param_flat(vl_model* m, float** ptr, int64_t* numel);
/* Re-derive the 16-bit GEMM operands from the flat master buffer (after loading an
 * adapter, after an optimiser step, or to merge).  PeftModel.from_pretrained /
 * merge_and_unload (train_loras.py:419, eval_compose.py:108-110). */
int vl_lora_commit(vl_model* m, void* stream);
/* The library tracks whether the flat parameters changed since the last commit: vl_param_tensor /
 * vl_param_flat hand out writable pointers and mark the handle dirty, vl_adam_step marks the model
 * whose flat buffer it updates, and a caller that writes through a pointer it kept calls
 * vl_params_changed.  vl_forward / vl_pgd_attack commit by themselves when the handle is dirty.  The contract is
 * therefore: writes the library can see (its own entry points) are never stale; a write through a KEPT pointer is the
 * caller's to announce (vl_params_changed).  The Python facade announces in-place torch operations on the flat
 * Parameter itself (it compares the Parameter's version counter before each forward / attack), so the reference's
 * unmodified torch.optim.Adam and parameter.copy_ are covered; writes through parameter.data or through a tensor obtained
 * from vl_param_tensor / vl_param_flat do not move that counter and are the caller's to announce (mark_dirty()). */
int vl_params_changed(vl_model* m);

/* merge_and_unload for one adapted module (eval_compose.py:102-114): W_out = W_in + (alpha/r) B A,
 * fp32 [out,in] device buffers of the caller (may alias); A, B are the module's current adapters. */
int vl_merge_weight(vl_model* m, int layer, uint32_t target, const float* W_in, float* W_out, void* stream);

/* mean/std used when normalise != 0 (default: ImageNet constants of get_normalization,
 * Utils.py:92-93; torchattacks' set_normalization_used(mean, std), whitebox_attacks.py:169). */
int vl_set_normalization(vl_model* m, const float mean[3], const float std[3]);

/* Workspace: vl_plan returns the bytes needed for batches up to max_batch;
 * train != 0 additionally keeps what the LoRA weight-gradient needs (per-layer activations, and the per-chunk copies of the LoRA
 * gradient that make it bit-reproducible: at most 32 x the LoRA parameters x 4 B, 123 MB at r = 8).  The bytes handed to
 * vl_set_workspace are the ONLY scratch memory the library touches (guard-band tested) and belong to it until the next
 * vl_set_workspace / vl_destroy; results do not depend on what they held before (tested with 0x00 against 0xFF fills).
 * What the bytes contain on the 16-bit path: the main activation workspace for max_batch images PLUS two half-batch eval
 * workspaces of ceil(min(max_batch, 191) / 2) images each for the two-chain forms of vl_pgd_attack / vl_forward(train = 0)
 * ("pgd_chains", "api_chains" below) -- for every plan, train-mode ones included (config 3's step attacks, then trains, through one
 * handle).  At max_batch = 256 that is about +75 % (ViT-B/16: 12 GB + 9 GB; the chains serve calls with 2 .. 191 images of that
 * plan); vl_debug_set_option(m, "pgd_chains", 1) BEFORE vl_plan leaves them out (round-4 ADVICE). */
int vl_plan(vl_model* m, int max_batch, int train, size_t* bytes);
int vl_set_workspace(vl_model* m, void* ws, size_t bytes);

/* model(x) -> logits [B, C] fp32  (LogitsModel.forward / get_model_output,
 * whitebox_attacks.py:13-19,41-48; peft_model.base_model(pixel_values=x).logits,
 * train_loras.py:310-311).  x = [B,3,S,S] fp32 NCHW.  normalise != 0 applies
 * (x-mean)/std with the ImageNet constants of get_normalization (Utils.py:92-93)
 * inside the patch gather (whitebox_attacks.py:26).  train != 0: LoRA dropout on,
 * activations for vl_backward_lora kept. */
int vl_forward(vl_model* m, const float* x, int batch, int normalise, int train,
               float* logits_out, void* stream);

/* F.cross_entropy(logits, labels) mean reduction (whitebox_attacks.py:29,
 * train_loras.py:313) on the logits of the last vl_forward.  labels int64 [B].
 * loss_out: 1 float (device). Also stages dLoss/dlogits for the backward calls. */
int vl_loss_ce(vl_model* m, const int64_t* labels, float* loss_out, void* stream);

/* Supply dLoss/dlogits [B,C] fp32 computed by the caller instead of vl_loss_ce (lets
 * `criterion(logits, labels).backward()` of train_loras.py:313-314 drive the chain). */
int vl_set_dlogits(vl_model* m, const float* dlogits, void* stream);

/* One backward pass producing both gradients; either output may be NULL. */
int vl_backward(vl_model* m, float* grad_x_out, float* flat_grad_out, void* stream);

/* LoRA dropout (LoraConfig.lora_dropout, train_loras.py:88; active only in vl_forward(train=1)):
 * the keep-mask of a LoRA branch input is a pure function of (seed, layer, projection, element),
 * regenerated by the dgrad and wgrad kernels instead of being stored; q, k, v share the mask of
 * the fused QKV projection's input.  The seed advances by one per train-mode forward.
 * vl_dropout_mask writes the mask (0 or 1/(1-p)) the LAST train-mode forward used for projection
 * proj (0 fused qkv, 1 attention out, 2 fc1, 3 fc2) of `layer`: [B*T, in] fp32 -- parity tests
 * feed it to the oracle. */
int vl_set_dropout_seed(vl_model* m, uint64_t seed);
int vl_dropout_mask(vl_model* m, int layer, int proj, float* out, void* stream);

/* loss.backward() restricted to the input: dLoss/dx [B,3,S,S] fp32 in the space of
 * the x given to vl_forward (perturbed.grad, whitebox_attacks.py:30-32). */
int vl_backward_input(vl_model* m, float* grad_x_out, void* stream);

/* loss.backward() restricted to the trainable parameters (train_loras.py:314):
 * flat_grad_out has the layout of vl_param_flat.  Requires vl_forward(train=1). */
int vl_backward_lora(vl_model* m, float* flat_grad_out, void* stream);

/* Fused FGSM/PGD update (K10): adv <- clamp(x0 + clamp(adv + alpha*sign(g) - x0, -eps, eps), lo, hi)
 * FGSM (whitebox_attacks.py:32-36) = one call with x0 == adv, alpha = eps. n elements. */
int vl_pgd_step(float* adv, const float* x0, const float* grad, float eps, float alpha,
                float lo, float hi, int64_t n, void* stream);
/* PGD random start (K11): adv = clamp(x0 + U(-eps,eps), lo, hi), counter-based RNG. */
int vl_pgd_init(float* adv, const float* x0, float eps, float lo, float hi, uint64_t seed,
                int64_t n, void* stream);

/* torchattacks.PGD(model, eps, alpha, steps, random_start)(images, labels)
 * (whitebox_attacks.py:112-113,170).  One iteration (forward, CE, backward-to-input,
 * fused step) is captured once into a hipGraph and replayed `steps` times (batches of 2 .. 191 images: one graph per
 * half batch, replayed on `stream` and on an internal stream that is joined before the result is copied out).
 * x0, adv_out: [B,3,S,S] fp32 in [0,1]; adv_out may not alias x0. */
int vl_pgd_attack(vl_model* m, const float* x0, const int64_t* labels, int batch,
                  float eps, float alpha, int steps, int random_start, uint64_t seed,
                  float* adv_out, void* stream);

/* ---- Auto-PGD on cross-entropy, L-inf (APGD-CE): the first component of AutoAttack(model, norm='Linf', eps, version='standard'),
 * which auto_attack.py:98-108 runs.  The algorithm is the restatement in DESIGN.md section 3.9 and tests/apgd_ref.py, written from
 * memory of the autoattack package's autopgd_base.py (not installed here): PARITY WITH THE PACKAGE IS UNPINNED.
 * One iteration (forward, CE, backward to the input, apgd_track_kernel, apgd_step_kernel) is captured once and replayed steps + 1
 * times (replay 0 evaluates the start point).  Step size, best loss, best point, momentum point and the checkpoint bookkeeping
 * live per image on the device, the iteration index in a device-side counter: no device-to-host copy, no stream synchronisation.
 * One chain only.  The model is fed normalised pixels as in vl_pgd_attack.
 * ALL image state lives in `scratch` (vl_apgd_scratch_bytes; 256-byte aligned, the only memory besides the workspace that the call
 * writes; results do not depend on what it held): x_adv, x_old, x_best, x_best_adv, grad_best, the staged x0 and labels, the
 * per-image scalars, the schedule table and the trace -- about 6 image batches.  vl_plan and the workspace are unchanged. */
typedef struct vl_apgd_args {
    const float* x0;          /* [B,3,S,S] fp32 in [0,1] */
    const int64_t* labels;    /* [B] */
    int32_t batch;
    int32_t steps;            /* n_iter >= 1 */
    float eps;
    float rho;                /* .75 */
    const float* x_init;      /* NULL, or the start point [B,3,S,S] (clamped to [0,1], NOT projected; random_start is ignored) */
    int32_t random_start;     /* x_init == NULL: 0 = start at x0, else x0 + eps t / max|t|, t ~ U(-1,1) (counter-based, per-image max) */
    int32_t reserved0;
    uint64_t seed;
    void* scratch;
    size_t scratch_bytes;
    /* outputs, each may be NULL */
    float* x_best;            /* [B,3,S,S] the maximum-loss point (adversarial training) */
    float* x_best_adv;        /* [B,3,S,S] the latest misclassified point; the start point for an image that was never fooled */
    float* loss_best;         /* [B] per-image CE at x_best */
    int32_t* robust;          /* [B] 1 = classified as its label at the start point and after every iteration */
    /* optional trace */
    float* trace_loss;        /* [steps + 1][B] row 0 = the start point, row i + 1 = the point of iteration i */
    float* trace_step;        /* [steps][B] the step size iteration i's update used */
    int32_t* trace_pred;      /* [steps + 1][B] argmax == label */
    void* stream;
    int32_t reserved[4];
} vl_apgd_args;
int vl_apgd_scratch_bytes(vl_model* m, int batch, int steps, size_t* bytes);
int vl_apgd_attack(vl_model* m, const vl_apgd_args* args);

/* One launch of apgd_step_kernel on CALLER-OWNED buffers (tests): per image b of `image_elems` floats (a multiple of 4; every
 * pointer 16-byte aligned), with flags[b] = 1 improved | 2 fooled | 4 restart and the step size step[b]:
 *   improved: x_best, grad_best <- x_adv, grad;  fooled: x_best_adv <- x_adv;  restart (and not improved): x_adv, grad <- x_best, grad_best;
 *   last == 0:  g2 = x_adv - x_old;  x_old <- x_adv;  z = P(x_adv + step sign(grad));  x_adv <- P((x_adv + (z - x_adv) a) + g2 (1 - a)),
 *   P(v) = clamp(min(max(v, x0 - eps), x0 + eps), 0, 1), every operation rounded to fp32 on its own;  last != 0: copies only. */
int vl_apgd_step(float* x_adv, float* x_old, float* x_best, float* x_best_adv, float* grad_best, const float* x0,
                 const float* grad, const uint32_t* flags, const float* step, int batch, int64_t image_elems, float eps,
                 float a, int last, void* stream);

/* One launch of apgd_track_kernel (tests): the state lives in `scratch` as in vl_apgd_attack (sized for batch, steps).  reset != 0
 * first builds the schedule table and zeroes the iteration counter; each call then consumes one iteration index (call j = replay j:
 * 0 = the start point, j = the point of iteration j - 1) from loss_img [B], logits [B][num_labels] and labels [B], and copies out
 * what the kernel left: step_out [B], flags_out [B] (1 improved | 2 fooled | 4 restart), loss_best_out [B], robust_out [B]
 * (each may be NULL). */
typedef struct vl_apgd_track_case {
    void* scratch; size_t scratch_bytes;
    int32_t batch, steps, reset, reserved0;
    float eps, rho;
    const float* loss_img; const float* logits; const int64_t* labels;
    float* step_out; uint32_t* flags_out; float* loss_best_out; int32_t* robust_out;
} vl_apgd_track_case;
int vl_debug_apgd_track(vl_model* m, const vl_apgd_track_case* c, void* stream);

/* ---- Targeted Auto-PGD on the DLR loss, L-inf (APGD-T): the second component of AutoAttack(model, norm='Linf', eps,
 * version='standard').  The algorithm is the restatement in DESIGN.md section 3.11 and tests/apgdt_ref.py, written from memory of
 * the autoattack package's autopgd_base.py (APGDAttack_targeted; not installed here): PARITY WITH THE PACKAGE IS UNPINNED.
 *   1. one eval-mode forward of x0: clean_correct[b] = (argmax == labels[b]);
 *   2. target k = 0 .. n_target_classes - 1 of image b = the class with the (k + 1)-th largest clean logit among the classes
 *      != labels[b], ties broken by the lower class index (or row k of targets_in).  DEVIATION: the package takes
 *      sort(logits)[:, -(k + 2)], which is the same class for every clean-correct image -- the only images whose result is used;
 *   3. for each target k, for each restart r: one APGD run of `steps` iterations -- the schedule, step rule, momentum,
 *      checkpoints and rho of vl_apgd_attack, started as its random_start = 1 does with the seed `seed + k * n_restarts + r` --
 *      that MAXIMISES the DLR-targeted loss  -(z_y - z_t) / (z_pi1 - (z_pi3 + z_pi4) / 2 + 1e-12), pi = the descending order of
 *      the logits row (value descending, index ascending); num_labels >= 4;
 *   4. an image counts as fooled when argmax != label, as in the package: hitting the target is not required;
 *   5. after each run, an image that was still robust and that the run fooled takes the run's x_best_adv; robust &= the run's.
 *      Clean-wrong images and images no run fooled keep x0 bit for bit.
 * What is back-propagated is D * dloss/dlogits, D = the loss's denominator > 0 (only the sign of the input gradient is used and
 * the backward rescales each image anyway; dloss/dlogits itself carries 1 / D^2).
 * One iteration (forward, DLR loss, backward to the input, apgd_track_kernel, apgd_step_kernel) is captured once per (batch, steps,
 * eps, rho, scratch) and replayed runs * (steps + 1) times, runs = n_target_classes * n_restarts: the loss kernel reads the
 * current target row from a fixed place in the scratch, refreshed between runs.  No device-to-host copy, no stream synchronisation.
 * ALL state lives in `scratch` (vl_apgdt_scratch_bytes; 256-byte aligned): the APGD state, the target table, x_adv and the fold's
 * flags.  The per-run rows (loss_best, robust_run) go straight to the caller's buffers after each run, so the scratch does not grow
 * with n_restarts.  vl_plan and the workspace are unchanged.
 * Refused (nothing is launched): num_labels < 4 (VL_ERR_UNSUPPORTED); n_target_classes outside 1 .. num_labels - 1,
 * n_restarts < 1, eps not finite or < 0, rho outside [0, 1], batch, steps and scratch as vl_apgd_attack.  A label outside
 * [0, num_labels), or a target in targets_in that is outside it or equals the label, gives that image NaN losses and makes a
 * LATER call return an error. */
typedef struct vl_apgdt_args {
    const float* x0;          /* [B,3,S,S] fp32 in [0,1] */
    const int64_t* labels;    /* [B] */
    int32_t batch;
    int32_t steps;            /* n_iter >= 1 */
    float eps;
    float rho;                /* .75 */
    int32_t n_target_classes; /* 1 .. num_labels - 1 (the package: 9) */
    int32_t n_restarts;       /* >= 1 */
    uint64_t seed;
    const int32_t* targets_in;/* NULL = pick from the clean logits, or [n_target_classes][B] */
    void* scratch;
    size_t scratch_bytes;
    /* outputs, each may be NULL; runs = n_target_classes * n_restarts, run = k * n_restarts + r */
    float* x_adv;             /* [B,3,S,S] */
    int32_t* robust;          /* [B] clean_correct and robust in every run */
    int32_t* clean_correct;   /* [B] */
    int32_t* targets;         /* [n_target_classes][B] */
    int32_t* fooled_by;       /* [B] the first run that fooled the image (and gave x_adv), -1 if none or clean-wrong */
    float* loss_best;         /* [runs][B] */
    int32_t* robust_run;      /* [runs][B] */
    /* optional trace of the LAST run, shapes as vl_apgd_args */
    float* trace_loss;
    float* trace_step;
    int32_t* trace_pred;
    void* stream;
    int32_t reserved[4];
} vl_apgdt_args;
int vl_apgdt_scratch_bytes(vl_model* m, int batch, int steps, int n_target_classes, size_t* bytes);
int vl_apgdt_attack(vl_model* m, const vl_apgdt_args* args);

/* One launch of dlr_targeted_loss_kernel on CALLER-OWNED buffers (tests): logits [B][C] fp32, labels [B] int64, targets [B] int32,
 * C >= 4; loss_img [B] and dlogits [B][C] (= D * dloss/dlogits, see above) are written.  err_flag: NULL, or one device-visible int
 * that is set to 1 for a label outside [0, C) and to 6 for a target outside it or equal to the label (that row: NaN). */
int vl_dlr_targeted_loss(const float* logits, const int64_t* labels, const int32_t* targets, int B, int C, float* loss_img,
                         float* dlogits, int* err_flag, void* stream);
/* One launch of apgd_targets_kernel on CALLER-OWNED buffers (tests): targets [n_target][B] int32, clean_correct [B] int32;
 * 1 <= n_target <= C - 1. */
int vl_apgd_targets(const float* logits, const int64_t* labels, int B, int C, int n_target, int32_t* targets,
                    int32_t* clean_correct, void* stream);

/* ---- Square attack, L-inf (Andriushchenko et al. 2020): the LAST component of AutoAttack(model, norm='Linf', eps,
 * version='standard'), which auto_attack.py:98-108 runs -- a score-based random search that reads only the logits, the suite's
 * gradient-free cross-check.  The algorithm is the restatement in DESIGN.md section 3.10 and tests/square_ref.py, written from
 * memory of the autoattack package's square.py and the paper (neither installed here): PARITY WITH THE PACKAGE IS UNPINNED.
 * Two DELIBERATE DEVIATIONS from the package: the window and its signs are drawn PER IMAGE from a counter-based generator keyed
 * by the image's global index image_offset + b (the package draws one window per batch; here an image's random stream depends
 * neither on its neighbours nor on how a dataset is cut into batches), and the window is written as clamp(x0 +- eps, 0, 1)
 * directly (the package adds 2 eps to the best point and projects).
 * Loss: the untargeted margin m = z_y - max_{j != y} z_j on the fp32 logits.  Schedule: proposal j = 1 .. n_queries has the
 * side s_j = min(S, max(1, round_half_even(sqrt(p S S)))), p = p_init / 2^k, k = how many of {10, 50, 200, 500, 1000, 2000,
 * 4000, 6000, 8000} the value int((j - 1) / n_queries * 10000) exceeds.  Replay 0 evaluates the start point (vertical stripes
 * x0 +- eps, one sign per image, channel and column); replay j evaluates proposal j: x_best with one s_j x s_j window, at a
 * uniform position, set to x0 + eps or x0 - eps per channel; it is accepted iff its margin is below margin_min.  An image with
 * margin_min <= 0 is frozen: no proposal, no query counted, x_best final; it is still forwarded (the batch shape is fixed).
 * A margin that is not finite is never accepted and makes a LATER call return VL_ERR_NONFINITE.
 * One iteration (eval-mode forward of x_cur with normalised pixels, square_track_kernel, square_step_kernel) is captured once
 * and replayed; the replay index is a device-side counter; the step kernel touches only the union of the previous and the next
 * window.  No device-to-host copy, no stream synchronisation.  One chain only.
 * RESUMABLE: a call runs replays first .. first + count - 1 of the n_queries + 1 the schedule has.  first == 0 stages x0 and
 * labels, builds the schedule and initialises the state; first > 0 continues from the state `scratch` holds (x0, labels,
 * p_init, seed and image_offset of THAT call are ignored; eps must be what it was) -- the caller guarantees that the scratch is untouched since the
 * previous chunk and that first is where that chunk ended; this cannot be checked without a synchronisation.  The outputs are
 * copied out after every call, so a caller may run a few hundred queries, look at `robust` and stop early.
 * ALL state lives in `scratch` (vl_square_scratch_bytes; 256-byte aligned, the only memory besides the workspace that the call
 * writes; results do not depend on what it held at first == 0): x0, x_cur, x_best (three image batches), labels, the counter,
 * the side table, the per-image scalars and the trace.  vl_plan and the workspace are unchanged.
 * Refused (nothing is launched): num_labels < 2, batch > 65535, n_queries outside 1 .. 65535, first < 0, count < 1,
 * first + count > n_queries + 1, eps not finite or < 0, p_init outside (0, 1], an unaligned or too small scratch. */
typedef struct vl_square_args {
    const float* x0;          /* [B,3,S,S] fp32 in [0,1] (read when first == 0) */
    const int64_t* labels;    /* [B] (read when first == 0) */
    int32_t batch;
    int32_t n_queries;        /* N >= 1: the forwards an active image gets besides the start point */
    int32_t first;            /* first replay of this call, 0 .. N */
    int32_t count;            /* replays of this call, >= 1 */
    float eps;
    float p_init;             /* .8 */
    uint64_t seed;
    uint64_t image_offset;    /* global index of image 0 of this batch */
    void* scratch;
    size_t scratch_bytes;
    /* outputs, each may be NULL; the state after replay first + count - 1 */
    float* x_best;            /* [B,3,S,S] */
    float* margin_min;        /* [B] the margin at x_best */
    int32_t* queries;         /* [B] forwards spent on this image while it was active (the start point included) */
    int32_t* robust;          /* [B] margin_min > 0 */
    /* optional trace; rows of replays that have not run yet are not written */
    float* trace_margin;      /* [N + 1][B] the margin seen at replay j (a frozen image's rows equal its margin_min) */
    int32_t* trace_win;       /* [N][B][4] row j - 1 = proposal j: h, w, s, signs | active << 3 | accepted << 4 (signs bit c: channel c
                                 is +eps); all zero for an image that was frozen */
    void* stream;
    int32_t reserved[4];
} vl_square_args;
int vl_square_scratch_bytes(vl_model* m, int batch, int n_queries, size_t* bytes);
int vl_square_attack(vl_model* m, const vl_square_args* args);

/* One launch of square_step_kernel on CALLER-OWNED buffers (tests): [batch,3,S,S] fp32 images, per image b the flag word flags[b] =
 * 1 a previous window to resolve | 2 it was accepted | 4 a next window, and the windows win_prev[b] / win_next[b] = {h, w, s,
 * signs}.  Only pixels of the union of the two windows are touched, each by one thread, which does in order:
 *   in the previous window:  accepted: x_best <- x_cur;  else: x_cur <- x_best;
 *   in the next window:      x_cur <- clamp(x0 + eps, 0, 1) where bit c of signs is set for the pixel's channel c, else x0 - eps.
 * A window that does not lie inside the image is ignored.  x0 is not written. */
int vl_square_step(float* x_cur, float* x_best, const float* x0, const uint32_t* flags, const int32_t* win_prev,
                   const int32_t* win_next, int batch, int image_size, float eps, void* stream);

/* One launch of square_track_kernel (tests): the state lives in `scratch` as in vl_square_attack (sized for batch, n_queries).
 * reset != 0 first builds the side table from p_init, stores seed / image_offset and zeroes the replay counter; each call then
 * consumes one replay index (call j = replay j) from logits [B][num_labels] and labels [B] and copies out what the kernel left:
 * flags_out [B], win_prev_out / win_next_out [B][4], margin_min_out [B], queries_out [B] (each may be NULL).  A margin that is
 * not finite does not raise the error word here. */
typedef struct vl_square_track_case {
    void* scratch; size_t scratch_bytes;
    int32_t batch, n_queries, reset, reserved0;
    float p_init, reserved1;
    uint64_t seed, image_offset;
    const float* logits; const int64_t* labels;
    uint32_t* flags_out; int32_t* win_prev_out; int32_t* win_next_out; float* margin_min_out; int32_t* queries_out;
} vl_square_track_case;
int vl_debug_square_track(vl_model* m, const vl_square_track_case* c, void* stream);

/* optimizer.step() of torch.optim.Adam(lr, betas, eps) (train_loras.py:284,315) on a
 * flat buffer; t = 1-based step count. */
int vl_adam_step(float* param, const float* grad, float* m1, float* m2, float lr, float b1,
                 float b2, float eps, int t, int64_t n, void* stream);

/* save_images quantisation (Utils.py:108-112): clamp(0,1)*255 -> uint8 truncation,
 * CHW float -> HWC bytes. */
int vl_quantize_u8(const float* images, uint8_t* out_hwc, int batch, int channels, int height,
                   int width, void* stream);

/* dst[b,c,:,:] = src[b,c,:,:] * scale[c] + shift[c]  (torchattacks' normalize /
 * inverse_normalize around the attack when set_normalization_used was called). dst may alias src. */
int vl_channel_affine(float* dst, const float* src, const float scale[3], const float shift[3],
                      int batch, int64_t hw, void* stream);

/* Adversarial patch with expectation over transformations: the overlay ART's AdversarialPatchPyTorch._random_overlay
 * computes for patch_attack.py:47-75,193-208 (generate / apply_patch).  patch [3,ps,ps] fp32 in [0,1]; inv_affine [B,6]
 * fp32 device = per-image INVERSE affine matrix of torchvision's affine(angle, translate, scale) (the host samples scale /
 * rotation / location and builds it: patch.py); patch_type 0 = square, 1 = circle.  out may not alias images.
 *   out = clamp(images * (1 - M') + P' * M', 0, 1),  P' / M' = the resized (bilinear, ps -> S) patch / mask warped by the affine
 *   (bilinear / nearest, zero fill).
 * vl_patch_grad: d(loss)/d(patch) [3,ps,ps] from d(loss)/d(out) of the same overlay (the input gradient of vl_backward_input). */
int vl_patch_apply(const float* images, const float* patch, const float* inv_affine, int batch, int image_size,
                   int patch_size, int patch_type, float* out, void* stream);
int vl_patch_grad(const float* grad_out, const float* inv_affine, int batch, int image_size, int patch_size, int patch_type,
                  float* patch_grad, void* stream);
/* The same overlay with ART's perspective distortion (patch_attack.py:95 --distortion_scale_max > 0): both canvases go through
 * torchvision's perspective(startpoints, endpoints; bilinear, zero fill) BEFORE the affine.  persp [B,8] fp32 device = the
 * per-image coefficients (a..h) of torchvision's _get_perspective_coeffs: canvas pixel (x, y) of the warped canvas reads the
 * unwarped one at ((a X + b Y + c) / (g X + h Y + 1) - .5, (d X + e Y + f) / (g X + h Y + 1) - .5), X = x + .5, Y = y + .5
 * (the host draws the corner displacements and solves for the coefficients: patch.py).  persp == NULL: no distortion,
 * bit-identical to vl_patch_apply / vl_patch_grad. */
int vl_patch_apply_persp(const float* images, const float* patch, const float* inv_affine, const float* persp, int batch,
                         int image_size, int patch_size, int patch_type, float* out, void* stream);
int vl_patch_grad_persp(const float* grad_out, const float* inv_affine, const float* persp, int batch, int image_size,
                        int patch_size, int patch_type, float* patch_grad, void* stream);
/* x <- clamp(x, lo, hi): the patch is clipped to the classifier's clip_values after every optimiser step. */
int vl_clamp(float* x, float lo, float hi, int64_t n, void* stream);

/* ---- Swin Transformer + LoRA (BASELINE config 4: Swin-T + LoRA r = 16, PGD-40) -----------------------------------------
 * The reference lists Swin-T (README.md:53) without code; the model is HF's SwinForImageClassification (modeling_swin.py):
 * 4x4 patch embedding + LayerNorm, four stages of shifted-window attention blocks (window 7, relative position bias,
 * -100 shift mask), patch merging between stages, final LayerNorm + mean pool + classifier.  fp32 on the exact-f32 MFMA.
 * State-dict keys are HF-4.55.2 names ("swin.encoder.layers.S.blocks.B.attention.self.query.weight", ...).  LoRA adapters
 * (eval mode: no dropout, no weight gradients on this path) on the VL_T_* targets; A / B live in one flat fp32 buffer. */
typedef struct vl_swin_config {
    int32_t image_size;   /* 224 */
    int32_t patch_size;   /* 4   */
    int32_t embed_dim;    /* 96  (stage i has embed_dim << i channels and heads[i] heads of dimension 32) */
    int32_t depths[4];    /* 2, 2, 6, 2 */
    int32_t heads[4];     /* 3, 6, 12, 24 */
    int32_t window;       /* 7 */
    int32_t num_labels;
    float   ln_eps;       /* 1e-5 */
    int32_t lora_r;       /* 0, 4, 8, 12 or 16 */
    float   lora_alpha;
    uint32_t lora_targets;
    int32_t reserved[4];
} vl_swin_config;
typedef struct vl_swin vl_swin;
int vl_swin_create(const vl_swin_config* cfg, vl_swin** out);
int vl_swin_destroy(vl_swin* m);
int vl_swin_load_tensor(vl_swin* m, const char* name, const float* src, int64_t numel, void* stream);
int vl_swin_param_flat(vl_swin* m, float** ptr, int64_t* numel);
/* which: 0 = lora_A [r, in], 1 = lora_B [out, r] of `target` in block `block` of stage `stage` */
int vl_swin_param_tensor(vl_swin* m, int stage, int block, uint32_t target, int which, float** ptr, int64_t* numel);
int vl_swin_set_normalization(vl_swin* m, const float mean[3], const float std[3]);
int vl_swin_plan(vl_swin* m, int max_batch, size_t* bytes);
/* as vl_set_workspace (the planned bytes are zeroed once, synchronously).  Since round 5 the results do NOT depend on what the
 * bytes hold between calls (round 4 required them to stay zero where the channel-padding columns were): the 16-bit activations of
 * stages 1-2 are dense (no pad columns), pad columns that remain are written by the kernel that owns the row, and the K-tail heads
 * a GEMM reads past the last valid row are zeroed at the start of every forward (csrc/swin.hip: zero_tails_kernel); tested by
 * filling every planned byte with 0xFF between two runs (tests/test_hip_swin.py). */
int vl_swin_set_workspace(vl_swin* m, void* ws, size_t bytes);
int vl_swin_forward(vl_swin* m, const float* x, int batch, int normalise, float* logits_out, void* stream);
int vl_swin_loss_ce(vl_swin* m, const int64_t* labels, float* loss_out, void* stream);
int vl_swin_backward_input(vl_swin* m, float* grad_x_out, void* stream);
/* Batches of >= 32 images run as TWO half-batch chains on two streams (the caller's and an internal one that forks after the staging
 * copies and joins before the result is copied out); the chains' workspaces share the planned bytes with the main workspace, so a
 * forward held for vl_swin_backward_input does not survive an attack (the handle then reports "backward before loss").  Bit-identical
 * to one chain; VITLORA_SWIN_CHAINS=0 (environment, read at vl_swin_create) restores the single chain. */
int vl_swin_pgd_attack(vl_swin* m, const float* x0, const int64_t* labels, int batch, float eps, float alpha, int steps,
                       int random_start, uint64_t seed, float* adv_out, void* stream);
/* vl_check_errors for a Swin handle (same codes: VL_ERR_ARG bad label, VL_ERR_NONFINITE fp16 gradient out of range). */
int vl_swin_check_errors(vl_swin* m, void* stream);

/* Per-launch timing with HIP events on the launch stream, for bench.py's roofline object.
 * Between begin and report every kernel launch of this library is bracketed by an event
 * pair (PGD runs eagerly, not as a graph, while active).  report synchronises the device and
 * writes a JSON object {"<kernel>": {"n": launches, "ms": total, "flops": algorithmic,
 * "bytes": algorithmic}, ...} into buf. */
/* Synchronises `stream` and returns the error kernels have flagged since the last check: VL_ERR_ARG (label outside
 * [0, num_labels)), VL_ERR_NONFINITE (fp16 mode: a gradient left the fp16 range or is NaN; the caller skips that step or
 * redoes the batch with precision = f32 -- what an AMP skip-step does; torch autograd in the reference is fp32 and has no
 * counterpart).  Every other entry point reports the same condition at its next call, without synchronising. */
int vl_check_errors(vl_model* m, void* stream);

int vl_profile_begin(void);
int vl_profile_report(char* buf, size_t cap);

/* GEMM micro-benchmark (tools/gemm_sweep.py): random bf16 operands allocated internally, `iters`
 * launches timed with HIP events; epi = GemmEpilogue of csrc/gemm.h (+100: all rows stored to row 0). */
int vl_bench_gemm(int M, int N, int K1, int K2, int epi, int bn, int iters, float* ms_out);

/* GEMM self-check: one random GEMM (M % 128 == 0, N % 256 == 0) through the 128-row kernel and through the kernel
 * selected with pp_mode (0 = 256-row persistent kernel, 1 = ping-pong kernel, 2 / 3 = ping-pong kernel with the LoRA down
 * projection of 16 / 32 columns computed inside it, checked against the separate skinny GEMM); *max_diff = largest |difference|. */
int vl_check_gemm(int M, int N, int K1, int K2, int epi, int pp_mode, float* max_diff);
/* A/B switch of the ping-pong GEMM (same values as the environment variable VITLORA_GEMM_PP); returns the old mode. */
int vl_debug_set_gemm_pp(int mode);
/* A/B switch of the streaming GEMM (tall, shallow products: the Swin stages 1-2; csrc/gemm_stream.hip): bit 0 = kernel on,
 * bit 1 = LoRA down projections computed inside it (same values as VITLORA_GEMM_STREAM / VITLORA_GEMM_STREAM_DOWN);
 * returns the old mode. */
int vl_debug_set_gemm_stream(int mode);
/* Diagnostic switches of one handle: "dead_rows" (1: eval-mode forwards compute the last encoder layer on the CLS rows only,
 * exact; 0: every row) "fuse_pgd" (1: vl_pgd_attack applies K10 in the patch-gradient epilogue; 0: separate launch) and "pgd_chains" (0, default:
 * vl_pgd_attack runs batches of 2 .. 191 images as two half-batch chains -- one captured iteration each, own activation workspaces
 * carved behind the main one by vl_plan, two streams that meet at the start and the end of the attack; 1: one chain always, set
 * BEFORE vl_plan to save those workspaces; 2: two chains whenever the halves fit) and "api_chains" (0, default; 1: vl_forward(train = 0)
 * and the backward after it run such batches as the same two chains -- the adversarial-patch EoT step goes through these calls;
 * vl_debug_tensor then does not see the activations).  Results are bit-identical either way.  "square_bare" (0, default; 1: a replay
 * of vl_square_attack is the eval-mode forward alone, with no bookkeeping -- the baseline tools/square_bench.py times a query
 * against; the attack's outputs are then meaningless). */
int vl_debug_set_option(vl_model* m, const char* name, int value);
int vl_debug_set_cus(vl_model* m, int cus);   /* grid size of the persistent GEMM kernels -- 256-row, ping-pong, streaming (diagnostic; default = the device's CU count) */

/* Introspection for tests / profiling.  vl_debug_counter: "graph_captures" = PGD graphs captured so far,
 * "commits" = vl_lora_commit executions, "dirty" = 1 if parameters changed since the last commit, "lds_poisons" = launches of the
 * "poison_lds" test hook (vl_debug_set_option: 1 = every profiled kernel launch is preceded by a kernel that fills every CU's
 * LDS with NaN patterns; results must not change -- process-wide, attacks then run without the graph). */
int vl_debug_counter(vl_model* m, const char* what, int64_t* value);
int vl_debug_tensor(vl_model* m, const char* what, int layer, void** ptr, int64_t* numel, int* dtype);

/* One GEMM on CALLER-OWNED device buffers through one chosen kernel with one chosen epilogue (tests/test_hip_gemm_ref.py compares
 * the result element by element with a float64 reference; vl_check_gemm above only compares kernels with each other).
 * The handle's precision selects the operand type: VL_PREC_F16 / VL_PREC_BF16 run the 16-bit kernels of csrc/gemm.h
 *   C[M,N] = A1[M,K1] W1[N,K1]^T + A2[M,K2] W2[N,K2]^T + bias, then the epilogue `epi` (GemmEpilogue of csrc/gemm.h),
 * VL_PREC_F32 runs k_gemm_f32:  C = alpha * op(A1) op(W1) + bias + R  (K = K1; the fields marked "f32").
 * The entry VALIDATES AND REFUSES: null required pointers, base pointers or row pitches that are not 16-byte aligned, pitches below
 * the row width, sizes that are not the multiples the kernels need (M % 128, N % bn, K % 64, n_store % 16; fp32: K % 4, N % 4,
 * M % 4 when transA) give VL_ERR_ARG; a forced route whose kernel cannot run the shape / epilogue / argument set gives
 * VL_ERR_UNSUPPORTED.  Nothing is launched then.  Buffer SIZES are the caller's: every operand holds M (W: N) rows of its pitch.
 * A forced route bypasses the thresholds that only pick the faster kernel (the streaming kernel's minimum row counts, the
 * ping-pong kernel's depth limit) and nothing else.  Only enqueues on `stream`: no allocation, no synchronisation. */
typedef struct vl_gemm_case {
    int32_t M, N, K1, K2;
    int32_t epi;          /* GemmEpilogue value (not EPI_NONE) */
    int32_t bn;           /* column tile: 128, or 64 (skinny form, EPI_STORE_H16 only) */
    int32_t Mvalid;       /* rows the patch epilogues may store / gather (0 = M) */
    int32_t n_store;      /* 0, or leading columns stored (multiple of 16, < N; row-layout epilogues; routes 0, 1, 4) */
    int32_t k2_used;      /* nonzero columns of the LoRA K tile (0 = unknown: all of them) */
    int32_t route;        /* 0 = what launch_gemm picks, 1 = 128-row kernel, 2 = 256-row persistent, 3 = ping-pong, 4 = streaming */
    const void* A1; const void* W1; const void* A2; const void* W2;     /* 16-bit operands (f32 handle: fp32 A1, W1) */
    int32_t lda1, ldw1, lda2, ldw2;                                     /* pitches in elements */
    const float* bias;    /* [N] or NULL */
    void* C; void* C2;    /* C2: gelu'(z) of EPI_GELU */
    const void* R;        /* residual / saved gelu'(z) / x0 of EPI_PATCH_PGD (may alias C for EPI_RESID_F32 and on an f32 handle) */
    const void* G;        /* EPI_DROP_ACC: optional extra factor */
    int32_t ldc, ldc2, ldr, ldg;
    const float* pos;     /* EPI_PATCH_FWD: position embedding [tokens][ldc] */
    const float* row_scale;   /* EPI_PATCH_BWD / EPI_PATCH_PGD: per-image factor or NULL */
    int32_t tokens, patches, grid, psize, img;      /* patch geometry: tokens = patches + 1, patches = grid^2, img = grid * psize */
    int32_t a_gather;     /* A row m reads row m + m / patches + 1 (the non-CLS token rows); f32 handle too */
    float inv_std[3];
    float pgd_eps, pgd_alpha, pgd_lo, pgd_hi;
    float drop_p;         /* EPI_DROP_ACC: mask = drop_scale(drop_seed, drop_stream, m * N + n) of csrc/common.h */
    uint32_t drop_stream;
    uint64_t drop_seed;
    /* LoRA down projection inside the GEMM (routes 0, 3, 4): t = A1 down_W^T, down_W = [64 rows][K1] zero padded, K2 = 64, A2 unused */
    const void* down_W; void* down_out;     /* down_out: receives t [M][64] (ping-pong kernel; must be NULL for the streaming kernel) */
    int32_t down_ldw, down_ld, down_groups; /* 16-column groups of t in use: 1 or 2 */
    int32_t ones_col;     /* EPI_RESID_H16 with the down projection inside: column 63 of W2 holds the bias, `bias` NULL */
    /* f32 handle (GemmF32 of csrc/f32_kernels.h) */
    int32_t f32_big;      /* 0: the 64 x 64 kernel, 1: the 128 x 128 kernel */
    int32_t transA, transW;
    int32_t Mstore;       /* rows >= Mstore are computed, not stored (0 = M) */
    float alpha;
    int32_t reserved[3];
} vl_gemm_case;
/* The patch-gradient epilogues flag a non-finite gradient in the handle's error word: vl_check_errors reports it. */
int vl_debug_gemm(vl_model* m, const vl_gemm_case* c, void* stream);

/* One ATTENTION kernel on CALLER-OWNED device buffers, named explicitly (tests/test_hip_attn_ref.py compares every output element
 * with a float64 softmax attention and its textbook backward; the model-level tests only see these kernels through several layers).
 * `kernel` picks the kernel itself, not a route: no process-wide switch (attn_ring, VITLORA_ATTN_RING, VITLORA_F32_ATTN,
 * VITLORA_ATTN_IMG) is read.  The template instantiation follows T as in the product: <1> for T <= 32, else <7>.
 * Head dimension 64, D = 64 H, softmax scale 1/8.  Layouts (16-bit elements of the handle's type; fp32 on an fp32 handle):
 *   qkv, dqkv [B*T][3D]  (q | k | v column groups of D, head hd at columns 64 hd .. 64 hd + 63 of its group)
 *   ctx, dctx [B*T][D]   (CLS kernels: compact [B][D], the row of token 0)
 *   lse       [B][H][T] fp32  (CLS kernels: [B][H]).  UNIT: the 16-bit kernels keep the BASE-2 log-sum-exp of the scaled scores,
 *             lse2 = log2(sum_k exp(q.k / 8)); the fp32 kernels keep the NATURAL log-sum-exp.
 *   down_W    forward: Ad [>= r rows][D]; backward: Bd [3r rows][3D], rows 0 / r / 2r .. = the query / key / value adapter, each
 *             read at its own column group (rows of a module that `mods` leaves out are not read)
 *   down_out  t / u [B*T][64]
 * What each kernel writes (rows = tokens 0 .. B*T - 1; nothing outside these is touched, padding rows included):
 *   VL_ATTN_FWD, VL_ATTN_IMG_FWD, VL_ATTN_F32_*_FWD   every element of ctx and of lse.
 *   VL_ATTN_IMG_FWD with down_W                        additionally t = ctx Ad^T summed over heads in fp32 from the 16-bit ctx: ALL 64
 *                                                      columns of every row are written -- the rows are zeroed first, then columns
 *                                                      0 .. r - 1 (r <= 4) or 0 .. 7 (r > 4) receive the sums; columns >= r end as zero.
 *   VL_ATTN_BWD, VL_ATTN_IMG_BWD, VL_ATTN_RING_BWD,    every element of dqkv (dq | dk | dv).
 *   VL_ATTN_F32_*_BWD
 *   VL_ATTN_IMG_BWD / VL_ATTN_RING_BWD with down_W     additionally u = dqkv Bd^T: all 64 columns of every row are zeroed, then the
 *                                                      module md (0 q, 1 k, 2 v) of every bit set in `mods` receives its r sums at
 *                                                      columns md r .. md r + r - 1; the column groups of the other modules stay zero.
 *   VL_ATTN_CLS_FWD                                    ctx row and lse of token 0 only (compact buffers).
 *   VL_ATTN_CLS_BWD                                    every element of dqkv: dk, dv of every token, dq of token 0, and ZEROS in
 *                                                      the dq columns of every other token.
 * The backward kernels read ctx only for delta = rowsum(dctx * ctx).
 * VALIDATES AND REFUSES, nothing is launched then: VL_ERR_ARG for a null required pointer (qkv always; ctx, lse; dctx and dqkv for a
 * backward kernel; down_out with down_W), a pointer that is not 16-byte aligned, T < 2, B < 1, H < 1, an unknown `kernel` or one of
 * the other precision, r outside 1 .. 8 or mods outside 1 .. 7 when down_W is given; VL_ERR_UNSUPPORTED for T above the kernel's
 * limit (224; CLS kernels 256; ring kernel 200) and for down_W on a kernel without a fused down projection.
 * Only enqueues ONE kernel on `stream`: no allocation, no synchronisation, the handle's workspace is not touched. */
#define VL_ATTN_FWD 0             /* attn_fwd32_kernel: one workgroup per (image, head) */
#define VL_ATTN_BWD 1             /* attn_bwd32_kernel */
#define VL_ATTN_IMG_FWD 2         /* attn_fwd_img_kernel: one workgroup per image, optional t */
#define VL_ATTN_IMG_BWD 3         /* attn_bwd_img_kernel: two-phase per-image backward, optional u */
#define VL_ATTN_RING_BWD 4        /* attn_bwd_ring_kernel: single-pass per-image backward, optional u, T <= 200 */
#define VL_ATTN_CLS_FWD 5         /* attn_cls_fwd_kernel */
#define VL_ATTN_CLS_BWD 6         /* attn_cls_bwd_kernel */
#define VL_ATTN_F32_MFMA_FWD 7    /* fp32 handle: attn_fwd_f32_mfma_kernel */
#define VL_ATTN_F32_MFMA_BWD 8    /* attn_bwd_f32_mfma_kernel */
#define VL_ATTN_F32_SCALAR_FWD 9  /* attn_fwd_f32_kernel */
#define VL_ATTN_F32_SCALAR_BWD 10 /* attn_bwd_f32_kernel */
typedef struct vl_attn_case {
    int32_t B, T, H;      /* images, tokens per image, heads (D = 64 H) */
    int32_t kernel;       /* VL_ATTN_* */
    const void* qkv;
    void* ctx;            /* written by a forward kernel, read by a backward kernel */
    float* lse;           /* likewise */
    const void* dctx;     /* backward kernels */
    void* dqkv;           /* backward kernels */
    const void* down_W;   /* NULL: no down projection */
    void* down_out;
    int32_t r;            /* LoRA rank of the down projection, 1 .. 8 */
    uint32_t mods;        /* backward: bit 0 / 1 / 2 = query / key / value adapted (forward: ignored) */
    int32_t reserved[4];
} vl_attn_case;
int vl_debug_attention(vl_model* m, const vl_attn_case* c, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VITLORA_H */
