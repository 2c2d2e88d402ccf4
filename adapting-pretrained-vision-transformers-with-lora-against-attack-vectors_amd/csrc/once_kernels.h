// Launchers, host helpers and argument types of the kernels that are compiled ONCE (once_kernels.hip): fp32 / integer data only,
// nothing typed on the 16-bit operand.  kernels.h includes this header and makes the names visible inside each build's
// namespace, so callers spell them as they spell every other launcher.  All launchers enqueue on the given stream, no sync.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vl_once {

// blocks of t threads that cover n items: at least 1, at most cap
static inline int nblk(int64_t n, int t, int cap = 1 << 20) {
    int64_t b = (n + t - 1) / t;
    return (int)(b < 1 ? 1 : (b > cap ? cap : b));
}

// err: mapped host word; set to 1 when a label is outside [0, C) (that image's loss / dlogits become NaN)
void k_ce_loss(const float* logits, const int64_t* labels, int B, int C, float* dlogits, float* loss_img, float* loss,
               int* err, hipStream_t s);
// per-image power-of-two gradient scale of the fp16 backward: gscale[b] = 2^(10 - e), max|dlogits[b]| = f * 2^e with
// f in [0.5, 1); uniform != 0: one scale for the whole batch (parameter gradients sum over images)
void k_grad_scale(const float* dlogits, int B, int C, int uniform, float* gscale, float* inv_gscale, hipStream_t s);
void k_classifier_grad(const float* dlogits, const float* xf, int B, int D, int C, float* dW, float* db, hipStream_t s);
// err (optional): mapped host word, set to 2 when a gradient element is not finite
void k_pgd_step(float* adv, const float* x0, const float* grad, float eps, float alpha, float lo, float hi, int64_t n,
                hipStream_t s, int* err = nullptr);
void k_zero(void* p, size_t bytes, hipStream_t s);   // bytes % 16 == 0; a kernel node, not a memset node, under capture
void k_pgd_init(float* adv, const float* x0, float eps, float lo, float hi, uint64_t seed, int64_t n, hipStream_t s);
// ---- Auto-PGD (APGD-CE, L-inf) ----
// Schedule entry j: replay j of the captured iteration evaluates the point of iteration j - 1 and makes the point of iteration j.
struct ApgdSched {
    float a;            // momentum of iteration j's update (1 at j = 0, else .75)
    int32_t k;          // > 0: iteration j - 1 ends a checkpoint window of k iterations
    int32_t flags;      // APGD_FIRST: the evaluation of the start point; APGD_LAST: no further point is made
    int32_t pad;
};
enum { APGD_FIRST = 1, APGD_LAST = 2 };
enum { APGD_IMPROVED = 1u, APGD_FOOLED = 2u, APGD_RESTART = 4u };     // per-image flag word of one iteration
struct ApgdState {      // per-image scalars, the schedule and the trace rows, all inside the caller's scratch
    int32_t* ctr;       // [4]: ctr[0] read by the track kernel, ctr[1] by the step kernel
    ApgdSched* sched;   // [N + 1]
    float *step, *loss_best, *loss_best_last;     // [B]
    int32_t *reduced_last, *robust;               // [B]
    uint32_t* flags;                              // [B]
    float* tr_loss;     // [N + 1][B]: row j = loss at replay j (row 0 the start point; loss_steps[i] = row i + 1)
    float* tr_step;     // [N][B]: the step size iteration j's update used
    int32_t* tr_pred;   // [N + 1][B]
};
void apgd_schedule_constants(int N, int* k0, int* kmin, int* dec);
void k_apgd_sched(ApgdSched* sched, int32_t* ctr, int N, hipStream_t s);     // fills the table, zeroes the counter
void k_apgd_rand_init(float* x_adv, const float* x0, float eps, uint64_t seed, int B, int64_t n_img, hipStream_t s);
void k_apgd_start(float* x_adv, const float* src, int64_t n, hipStream_t s);     // x_adv = clamp(src, 0, 1)
void k_apgd_track(const ApgdState& st, const float* loss_img, const float* logits, const int64_t* labels, int B, int C, int N,
                  float eps, float rho, hipStream_t s);
// sched != nullptr: a / last are read from sched[ctr[1] - 1] and ctr[0] is advanced; nullptr: the arguments.  n_img % 4 == 0.
void k_apgd_step(float* x_adv, float* x_old, float* x_best, float* x_best_adv, float* grad_best, const float* x0,
                 const float* grad, const uint32_t* flags, const float* step, int B, int64_t n_img, float eps,
                 const ApgdSched* sched, int32_t* ctr, int N, float a, int last, hipStream_t s, int* err = nullptr);
// ---- APGD-T (targeted Auto-PGD on the DLR loss) ----
// DLR-targeted loss of one row: pi = the row's descending order (value descending, index ascending), N = z_y - z_t,
// D = z_pi1 - (z_pi3 + z_pi4) / 2 + 1e-12, loss = -N / D (maximised).  dlogits = D * dloss/dz, NOT dloss/dz: only the sign of the
// input gradient is used and the backward rescales every image anyway (k_grad_scale), while dloss/dz itself carries 1 / D^2 --
// about 1e24 at a near-tie among the top four classes.  C >= 4.  err (optional): set to 1 for a label outside [0, C), to 6 for a
// target outside [0, C) or equal to the label; that image's loss and dlogits row become NaN.  loss (optional): the batch mean.
void k_dlr_targeted_loss(const float* logits, const int64_t* labels, const int32_t* targets, int B, int C, float* dlogits,
                         float* loss_img, float* loss, int* err, hipStream_t s);
// targets[k * B + b] = the class with the (k + 1)-th largest logit among the classes != labels[b] (ties: the lower index first),
// k < n_target <= C - 1; clean_correct[b] = (argmax == labels[b], the first maximum)
void k_apgd_targets(const float* logits, const int64_t* labels, int B, int C, int n_target, int32_t* targets,
                    int32_t* clean_correct, hipStream_t s);
// The fold over runs: for an image with still_in[b] && !run_robust[b], x_out[b] <- x_best_adv[b] and fooled_by[b] = run;
// still_out[b] = still_in[b] & run_robust[b].  still_in and still_out are two arrays (no block reads a word another one writes).
// n_img % 4 == 0.
void k_apgdt_fold(float* x_out, const float* x_best_adv, const int32_t* still_in, int32_t* still_out, const int32_t* run_robust,
                  int32_t* fooled_by, int run, int B, int64_t n_img, hipStream_t s);
// ---- Square attack (score-based random search, L-inf) ----
// Replay j of the captured iteration evaluates proposal j (replay 0: the stripes) and draws proposal j + 1.
enum { SQ_PREV = 1u, SQ_ACCEPT = 2u, SQ_NEXT = 4u };      // per-image flag word of one replay: a pending window to resolve
                                                          // (accepted or not), a next window to write
struct SquareSched {    // the at most ten distinct sides of a schedule: proposal j >= from[i] uses side[i] (from[0] = 1)
    int32_t from[10];
    int32_t side[10];
};
struct SquareParams {   // what would otherwise be kernel arguments baked into the captured iteration
    uint64_t key;       // seed * 0xD1342543DE82EF95
    uint64_t offset;    // global index of image 0
};
struct SquareState {    // counter, table, per-image scalars and the trace rows, all inside the caller's scratch
    int32_t* ctr;       // [4]: ctr[0] read by the track kernel, ctr[1] by the step kernel
    SquareParams* par;
    int32_t* side;      // [N + 1]: side[j] of proposal j (entry 0 unused)
    float* margin_min;  // [B]
    int32_t *queries, *robust;     // [B]
    uint32_t* flags;    // [B]
    int32_t *win_prev, *win_next;  // [B][4]: h, w, s, sign bits (bit c = channel c is +eps)
    float* tr_margin;   // [N + 1][B]: the margin seen at replay j
    int32_t* tr_win;    // [N][B][4]: h, w, s, signs | active << 3 | accepted << 4 of proposal j + 1 (all zero: no proposal)
};
void square_schedule(int S, int N, float p_init, SquareSched* out);      // host, in double
void k_square_sched(const SquareState& st, const SquareSched& sc, int N, uint64_t seed, uint64_t image_offset, hipStream_t s);
void k_square_init(float* x_cur, float* x_best, const float* x0, const SquareParams* par, int B, int S, float eps, hipStream_t s);
// err (optional): set to 1 for a label outside [0, C), to 5 for a margin that is not finite
void k_square_track(const SquareState& st, const float* logits, const int64_t* labels, int B, int C, int S, int N, hipStream_t s,
                    int* err = nullptr);
// ctr != nullptr: ctr[0] = ctr[1], nothing past replay N (the attack); nullptr: one launch on caller-owned buffers (vl_square_step)
void k_square_step(float* x_cur, float* x_best, const float* x0, const uint32_t* flags, const int32_t* win_prev,
                   const int32_t* win_next, int B, int S, float eps, int32_t* ctr, int N, hipStream_t s);
// err (optional): set to 3 when a gradient element is not finite (that element is skipped)
void k_adam(float* p, const float* g, float* m, float* v, float lr, float b1, float b2, float eps, int t, int64_t n,
            hipStream_t s, int* err = nullptr);
void k_channel_affine(float* dst, const float* src, const float* scale, const float* shift, int B, int64_t hw,
                      hipStream_t s);
void k_quantize(const float* img, uint8_t* out, int B, int C, int H, int W, hipStream_t s);
// fp32 form of k_merge_lora's fold (adapter composition: the merged weight becomes the next base)
void k_merge_f32(const float* W, const float* A, const float* B, int out, int in, int r, float sc, float* dst,
                 hipStream_t s);
// keep-mask (0 or 1 / (1 - p)) of the LoRA dropout of module `stream`, as fp32
void k_dropout_mask(float* out, int64_t n, uint64_t seed, uint32_t stream, float p, hipStream_t s);

}  // namespace vl_once
